"""The depthwise convolutions — ``conv1d`` / ``conv2d`` with ``groups == C`` — registered in this package's dispatcher as a second
kernel next to the implicit GEMM of fused_conv.py (whose predicate declines every ``groups != 1``).

The reference registers no kernel for them: the generated fallbacks (src/fastforward/_gen/fallback.py:116-214) run A2 of input and
weight, the float grouped convolution and the output quantizer. The predicate below accepts exactly what the direct int8 stencil of
csrc/ffq_depthwise.hip covers (include/ffq_depthwise.h) and returns False for everything else, so the reference chain runs unchanged
there — general grouped convolutions (``1 < groups < C``) included:

* ``groups == input.shape[1] > 1``, ``weight.shape[1] == 1``, ``weight.shape[0] % groups == 0`` (a channel multiplier M >= 1);
* ``prod(kernel) <= 1024`` (31 x 31 fits): one channel's taps stay on chip;
* every other rule of ``ConvKernels.supported`` (fused_conv.py): static-affine codes of <= 8 bits in an int8 or float container with
  fp32 parameters, the input per tensor and the weight per tensor or per output channel, one data dtype (bf16 / fp16 / fp32) for both,
  a batched input, ``geometry()`` (integer stride / dilation / padding, ``'valid'``, ``'same'`` where it is symmetric), the bias
  forms, everything on the HIP device, no gradient needed, and under strict quantization an output quantizer with quantized operands;
* the device library exports ``ffq_depthwise_conv2d_w8a8`` (a library without the symbol — the C oracle — declines).

Conv1d runs as H = KH = 1. The output quantizer runs inside the launch (``DispatcherKernels._requant``'s rules). Nothing here reads
device memory on the host: the route is capturable in a ``torch.cuda.graph``. ``QuantizedConv1d`` / ``QuantizedConv2d`` pass
``groups`` through, so a converted model's depthwise layers take this route with no class of their own.
"""

from __future__ import annotations

import math

from typing import Any

import torch

from fastforward_amd import _native, fused_conv, ops
from fastforward_amd.dispatcher import Predicate, register
from fastforward_amd.fused_conv import geometry
from fastforward_amd.fused_linear import _FLOATS
from fastforward_amd.fused_modules import KERNELS as _MODULES
from fastforward_amd.fused_modules import _needs_grad, _settle

MAX_TAPS = 1024  # KH * KW (include/ffq_depthwise.h)


class DepthwiseKernels(fused_conv.ConvKernels):
    """Predicates and kernels of the depthwise ``conv1d`` / ``conv2d`` (``_codes_ok`` is ConvKernels'; ``supported`` is not)."""

    def supported(self, dims: int, input: Any = None, weight: Any = None, bias: Any = None, stride: Any = 1, padding: Any = 0,
                  dilation: Any = 1, groups: int = 1, output_quantizer: Any = None, strict_quantization: bool | None = None, **_: Any) -> bool:
        k = self._k
        if not self._m._strict_ok(strict_quantization, output_quantizer, input, weight):
            return False
        if not (self._codes_ok(input) and self._codes_ok(weight)) or input.dim() != dims + 2 or weight.dim() != dims + 2:
            return False
        if not isinstance(groups, int) or isinstance(groups, bool) or not groups == input.shape[1] > 1:
            return False
        if weight.shape[1] != 1 or weight.shape[0] % groups != 0 or math.prod(weight.shape[2:]) > MAX_TAPS:
            return False
        if not fused_conv._on_device(input, weight) or input.numel() == 0 or weight.numel() == 0:
            return False
        deq = k._deq_dtype(input)
        if deq not in _FLOATS or k._deq_dtype(weight) != deq:
            return False
        if k._tile(input) != tuple(input.shape) or k._tile(weight) not in (tuple(weight.shape), (1, *weight.shape[1:])):
            return False  # per-tensor activations; per-tensor or per-output-channel weights
        if getattr(k._params(weight).granularity, "channel_dims", (0,)) != (0,):
            return False  # PerChannel(1): one "input channel" per group, so its tile IS the tensor; still not a per-tensor quantizer
        if geometry(dims, input.shape[2:], weight.shape[2:], stride, padding, dilation) is None:
            return False
        if bias is not None:
            if isinstance(bias, k.surface.quantized_tensor):
                if not k.static_affine(bias) or k._deq_dtype(bias) != deq:
                    return False
            elif not isinstance(bias, torch.Tensor) or bias.dtype != deq:
                return False
            if bias.numel() != weight.shape[0] or not fused_conv._on_device(bias):
                return False
        return not _needs_grad(input, weight, bias)

    def _exported(self) -> bool:
        # (`supported` first: it is what establishes that the device library is loaded)
        return getattr(_native.library(), "ffq_depthwise_conv2d_w8a8", None) is not None

    def supported_conv1d(self, **kwargs: Any) -> bool:
        return self.supported(1, **kwargs) and self._exported()

    def supported_conv2d(self, **kwargs: Any) -> bool:
        return self.supported(2, **kwargs) and self._exported()

    def _conv(self, dims: int, input: Any, weight: Any, bias: Any, stride: Any, padding: Any, dilation: Any, output_quantizer: Any) -> Any:
        k = self._k
        deq = k._deq_dtype(input)
        stride2, padding2, dilation2 = geometry(dims, input.shape[2:], weight.shape[2:], stride, padding, dilation)
        if isinstance(bias, k.surface.quantized_tensor):
            bias = bias.dequantize()
        _settle(input)
        _settle(weight)
        (xs, xo), (ws, wo) = k._scale_offset(input), k._scale_offset(weight)
        x, w = k._int8_codes(input), k._int8_codes(weight)
        if dims == 1:
            x, w = x.unsqueeze(2), w.unsqueeze(2)
        fused = self._m._output(output_quantizer, deq)
        if fused is not None:
            args = dict(out_scale=fused["out_scale"], out_offset=fused["out_offset"], out_num_bits=fused["out_num_bits"], requant_from=deq)
        else:
            args = dict(out_dtype=deq)
        out = ops.depthwise_conv2d_w8a8(x, w, xs, xo, ws, wo, bias, stride2, padding2, dilation2, **args)
        if dims == 1:
            out = out.squeeze(2)
        return self._m._finish(out, [out], fused, output_quantizer, deq)


KERNELS = DepthwiseKernels(_MODULES)
conv1d_predicate = Predicate(KERNELS.supported_conv1d)
conv2d_predicate = Predicate(KERNELS.supported_conv2d)
_registrations = {
    "conv1d": register("conv1d", conv1d_predicate, KERNELS.conv1d),
    "conv2d": register("conv2d", conv2d_predicate, KERNELS.conv2d),
}
