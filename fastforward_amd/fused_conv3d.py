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

from fastforward_amd.dispatcher import Predicate, register
from fastforward_amd.fused_conv import MAX_REDUCTION, ConvKernels, ConvSet, any_operands, geometry, ungrouped
from fastforward_amd.fused_modules import KERNELS as _MODULES


class Conv3dKernels(ConvKernels):
    """Predicate and kernel of ``conv3d``: ``ConvKernels``' rules and run body under the operator's names."""

    def supported_conv3d(self, **kwargs: Any) -> bool:
        return self._accepts(3, **kwargs)

    def conv3d(self, input: Any, weight: Any, bias: Any = None, stride: Any = 1, padding: Any = 0, dilation: Any = 1, groups: int = 1, *,
               output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        return self._run(3, input, weight, bias, output_quantizer, stride, padding, dilation)


KERNELS = Conv3dKernels(_MODULES, ConvSet(in_axis=1, oc_axis=0, groups_rule=ungrouped, grouping_rule=any_operands, bound=MAX_REDUCTION, geometry=geometry,
                                          geometry_operands=("stride", "padding", "dilation"), op="conv3d_w8a8",
                                          symbol="ffq_conv3d_w8a8"))
conv3d_predicate = Predicate(KERNELS.supported_conv3d)
_registrations = {"conv3d": register("conv3d", conv3d_predicate, KERNELS.conv3d)}
