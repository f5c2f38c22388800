"""The convolutions — ``conv1d``, ``conv2d`` — registered in this package's dispatcher.

The reference registers no kernel for them: QuantizedConv1d / QuantizedConv2d run the generated fallbacks
(src/fastforward/_gen/fallback.py:116-214) — A2 of input and weight into data-dtype tensors, the float convolution, the output
quantizer. The predicates below accept what the int8 implicit GEMM of csrc/ffq_conv.hip covers and return False for everything
else, so the reference chain (the fallbacks in :mod:`fastforward_amd.nn.functional`) runs unchanged there:

* input and weight static-affine codes on the HIP device with the device library loaded (the C oracle declines): <= 8 bits, an
  int8 container or a float one (converted exactly, as ``DispatcherKernels._int8_codes``), fp32 parameters; the input per tensor,
  the weight per tensor or per output channel; data dtype bf16 / fp16 / fp32, the same for both;
* ``groups == 1``, a batched input ([B, C, L] / [B, C, H, W]), ``C * prod(kernel) < 131072``, integer stride / dilation / padding,
  ``padding='valid'``, and ``padding='same'`` where the padding it implies is symmetric;
* bias: none, a plain tensor of the data dtype, or static-affine codes that dequantize to it;
* no operand or parameter that needs a gradient while grad mode is on (the launch has no autograd formula).

``groups == C`` (depthwise) is not this module's: :mod:`fastforward_amd.fused_depthwise` registers a second kernel on both operators for
it, and any other ``groups != 1`` stays on the fallback. Conv1d runs as a conv2d with H = KH = 1. The output quantizer runs inside the launch under the int8 GEMM's rules
(``DispatcherKernels._requant``, int8 containers only), so range estimation still sees the real-valued output. Nothing here reads
device memory on the host: the route is capturable in a ``torch.cuda.graph``.
"""

from __future__ import annotations

import math

from typing import Any

import torch

from fastforward_amd import ops
from fastforward_amd.dispatcher import Predicate, register
from fastforward_amd.fused_linear import _FLOATS
from fastforward_amd.fused_modules import KERNELS as _MODULES
from fastforward_amd.fused_modules import _fp32_param, _needs_grad, _on_device, _settle

MAX_REDUCTION = 131071  # C * KH * KW: the int32 accumulator's bound, 2^14 * taps < 2^31 (include/ffq.h, ffq_conv2d_w8a8)


def _ints(v: Any, n: int) -> tuple[int, ...] | None:
    """`v` as n ints (an int repeats), or None."""
    if isinstance(v, int) and not isinstance(v, bool):
        return (v,) * n
    if isinstance(v, (tuple, list, torch.Size)) and len(v) == n and all(isinstance(e, int) and not isinstance(e, bool) for e in v):
        return tuple(v)
    return None


def geometry(dims: int, input_shape: Any, kernel: Any, stride: Any, padding: Any, dilation: Any) -> tuple[tuple[int, ...], ...] | None:
    """((stride_h, stride_w), (pad_h, pad_w), (dil_h, dil_w)) of the 2-D launch (one triple each for the 3-D launch of
    fused_conv3d.py), or None where the kernel does not take the call (then F.conv raises or computes it on the fallback)."""
    s, d = _ints(stride, dims), _ints(dilation, dims)
    if s is None or d is None or min(s) < 1 or min(d) < 1:
        return None
    if isinstance(padding, str):
        if padding == "valid":
            p: tuple[int, ...] | None = (0,) * dims
        elif padding == "same" and max(s) == 1 and all(di * (k - 1) % 2 == 0 for di, k in zip(d, kernel)):
            p = tuple(di * (k - 1) // 2 for di, k in zip(d, kernel))
        else:
            return None
    else:
        p = _ints(padding, dims)
    if p is None or min(p) < 0:
        return None
    if any(n + 2 * pi < di * (k - 1) + 1 for n, pi, di, k in zip(input_shape, p, d, kernel)):
        return None
    if dims == 1:
        return (1, s[0]), (0, p[0]), (1, d[0])
    return tuple(s), tuple(p), tuple(d)


class ConvKernels:
    """Predicates and kernels of ``conv1d`` / ``conv2d`` (on the int8 GEMM's Surface, through the generic modules' helpers)."""

    def __init__(self, modules: Any) -> None:
        self._m = modules
        self._k = modules._k

    def _codes_ok(self, t: Any) -> bool:
        k = self._k
        if not k.static_affine(t) or not k._bits_ok(t):
            return False
        p = k._params(t)
        return t.raw_data.dtype in (torch.int8, *_FLOATS) and _fp32_param(p.scale) and _fp32_param(p.offset)

    def supported(self, dims: int, input: Any = None, weight: Any = None, bias: Any = None, stride: Any = 1, padding: Any = 0,
                  dilation: Any = 1, groups: int = 1, output_quantizer: Any = None, strict_quantization: bool | None = None, **_: Any) -> bool:
        k = self._k
        if not self._m._strict_ok(strict_quantization, output_quantizer, input, weight) or groups != 1:
            return False
        if not (self._codes_ok(input) and self._codes_ok(weight)) or input.dim() != dims + 2 or weight.dim() != dims + 2:
            return False
        if not _on_device(input, weight) or input.numel() == 0 or weight.numel() == 0 or input.shape[1] != weight.shape[1]:
            return False
        deq = k._deq_dtype(input)
        if deq not in _FLOATS or k._deq_dtype(weight) != deq:
            return False
        if k._tile(input) != tuple(input.shape) or k._tile(weight) not in (tuple(weight.shape), (1, *weight.shape[1:])):
            return False  # per-tensor activations; per-tensor or per-output-channel weights
        if math.prod(weight.shape[1:]) > MAX_REDUCTION:
            return False
        if geometry(dims, input.shape[2:], weight.shape[2:], stride, padding, dilation) is None:
            return False
        if bias is not None:
            if isinstance(bias, k.surface.quantized_tensor):
                if not k.static_affine(bias) or k._deq_dtype(bias) != deq:
                    return False
            elif not isinstance(bias, torch.Tensor) or bias.dtype != deq:
                return False
            if bias.numel() != weight.shape[0] or not _on_device(bias):
                return False
        return not _needs_grad(input, weight, bias)

    def supported_conv1d(self, **kwargs: Any) -> bool:
        return self.supported(1, **kwargs)

    def supported_conv2d(self, **kwargs: Any) -> bool:
        return self.supported(2, **kwargs)

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
        out = ops.conv2d_w8a8(x, w, xs, xo, ws, wo, bias, stride2, padding2, dilation2, **args)
        if dims == 1:
            out = out.squeeze(2)
        return self._m._finish(out, [out], fused, output_quantizer, deq)

    def conv1d(self, input: Any, weight: Any, bias: Any = None, stride: Any = 1, padding: Any = 0, dilation: Any = 1, groups: int = 1, *,
               output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        return self._conv(1, input, weight, bias, stride, padding, dilation, output_quantizer)

    def conv2d(self, input: Any, weight: Any, bias: Any = None, stride: Any = 1, padding: Any = 0, dilation: Any = 1, groups: int = 1, *,
               output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        return self._conv(2, input, weight, bias, stride, padding, dilation, output_quantizer)


KERNELS = ConvKernels(_MODULES)
conv1d_predicate = Predicate(KERNELS.supported_conv1d)
conv2d_predicate = Predicate(KERNELS.supported_conv2d)
_registrations = {
    "conv1d": register("conv1d", conv1d_predicate, KERNELS.conv1d),
    "conv2d": register("conv2d", conv2d_predicate, KERNELS.conv2d),
}
