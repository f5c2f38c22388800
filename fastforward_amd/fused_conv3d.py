"""The 3-D convolution — ``conv3d`` — registered in this package's dispatcher.

The reference registers no kernel for it: ``ff.nn.functional.conv3d`` runs the generated fallback
(src/fastforward/_gen/fallback.py:218-265) — A2 of input and weight into data-dtype tensors, ``F.conv3d``, the output quantizer. The
predicate below accepts what the int8 implicit GEMM of csrc/ffq_conv3d.hip covers (include/ffq_3d.h) and returns False for
everything else, so the fallback in :mod:`fastforward_amd.nn.functional` runs unchanged there. The rules are ``ConvKernels``'
(fused_conv.py) with one more spatial axis:

* input and weight static-affine codes on the HIP device, the device library loaded AND exporting ``ffq_conv3d_w8a8`` (a library
  without the symbol — the C oracle — declines): <= 8 bits, an int8 container or a float one, fp32 parameters; the input per
  tensor, the weight per tensor or per output channel; data dtype bf16 / fp16 / fp32, the same for both;
* ``groups == 1``, a batched input [B, C, D, H, W], ``C * KD * KH * KW < 131072``, int or triple stride / dilation / padding,
  ``padding='valid'``, and ``padding='same'`` where the padding it implies is symmetric;
* bias: none, a plain tensor of the data dtype, or static-affine codes that dequantize to it;
* no operand or parameter that needs a gradient while grad mode is on (the launch has no autograd formula).

A ``torch.channels_last_3d`` input with ``C % 16 == 0`` reaches the GEMM as it is (one launch fewer). The output quantizer runs
inside the launch under the int8 GEMM's rules (``DispatcherKernels._requant``). Nothing here reads device memory on the host: the
route is capturable in a ``torch.cuda.graph``.
"""

from __future__ import annotations

from typing import Any

from fastforward_amd import _native, ops
from fastforward_amd.dispatcher import Predicate, register
from fastforward_amd.fused_conv import ConvKernels, geometry
from fastforward_amd.fused_modules import KERNELS as _MODULES
from fastforward_amd.fused_modules import _settle


class Conv3dKernels(ConvKernels):
    """Predicate and kernel of ``conv3d``."""

    def supported_conv3d(self, **kwargs: Any) -> bool:
        # (`supported` first: it is what establishes that the device library is loaded)
        return self.supported(3, **kwargs) and getattr(_native.library(), "ffq_conv3d_w8a8", None) is not None

    def conv3d(self, input: Any, weight: Any, bias: Any = None, stride: Any = 1, padding: Any = 0, dilation: Any = 1, groups: int = 1, *,
               output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        k = self._k
        deq = k._deq_dtype(input)
        stride3, padding3, dilation3 = geometry(3, input.shape[2:], weight.shape[2:], stride, padding, dilation)
        if isinstance(bias, k.surface.quantized_tensor):
            bias = bias.dequantize()
        _settle(input)
        _settle(weight)
        (xs, xo), (ws, wo) = k._scale_offset(input), k._scale_offset(weight)
        x, w = k._int8_codes(input), k._int8_codes(weight)
        fused = self._m._output(output_quantizer, deq)
        if fused is not None:
            args = dict(out_scale=fused["out_scale"], out_offset=fused["out_offset"], out_num_bits=fused["out_num_bits"], requant_from=deq)
        else:
            args = dict(out_dtype=deq)
        out = ops.conv3d_w8a8(x, w, xs, xo, ws, wo, bias, stride3, padding3, dilation3, **args)
        return self._m._finish(out, [out], fused, output_quantizer, deq)


KERNELS = Conv3dKernels(_MODULES)
conv3d_predicate = Predicate(KERNELS.supported_conv3d)
_registrations = {"conv3d": register("conv3d", conv3d_predicate, KERNELS.conv3d)}
