"""The transposed convolutions — ``conv_transpose1d``, ``conv_transpose2d`` — registered in this package's dispatcher.

The reference registers no kernel for them: the generated fallbacks run (src/fastforward/_gen/fallback.py:346-449) — A2 of input
and weight into data-dtype tensors, the float transposed convolution, the output quantizer. The predicates below accept what the
phase-split int8 implicit GEMM of csrc/ffq_conv_transpose.hip covers and return False for everything else, so the reference chain
(the fallbacks in :mod:`fastforward_amd.nn.functional`) runs unchanged there. They accept what ``ConvKernels.supported`` accepts
(:mod:`fastforward_amd.fused_conv`), with the transposed layout's differences:

* the weight is [C, OC, *kernel]: ``input.shape[1] == weight.shape[0]``, and its tile is the whole tensor or ``(C, 1, *kernel)`` —
  ``PerChannel(1)``, one parameter pair per OUTPUT channel. ``PerChannel(0)`` weights (per input channel) take the chain;
* ``groups == 1``, a batched input, ``C * prod(kernel) < 131072``, integer stride / padding / output_padding / dilation with
  ``0 <= output_padding < max(stride, dilation)`` (torch's rule), an output of at least one element per axis, and
  ``stride_h * stride_w <= 64`` (the kernel's phase table);
* bias, gradient and device rules as for the forward convolution.

conv_transpose1d runs as a conv_transpose2d with H = KH = 1. The output quantizer runs inside the launch under the int8 GEMM's
rules (int8 containers only). Nothing here reads device memory on the host: the route is capturable in a ``torch.cuda.graph``.
"""

from __future__ import annotations

import math

from typing import Any

import torch

from fastforward_amd import ops
from fastforward_amd.dispatcher import Predicate, register
from fastforward_amd.fused_conv import KERNELS as _CONV
from fastforward_amd.fused_conv import MAX_REDUCTION, _ints
from fastforward_amd.fused_linear import _FLOATS
from fastforward_amd.fused_modules import _needs_grad, _on_device, _settle
from fastforward_amd.ops.conv import MAX_PHASES


def transposed_geometry(dims: int, input_shape: Any, kernel: Any, stride: Any, padding: Any, output_padding: Any,
                        dilation: Any) -> tuple[tuple[int, int], ...] | None:
    """((stride_h, stride_w), (pad_h, pad_w), (out_pad_h, out_pad_w), (dil_h, dil_w)) of the 2-D launch, or None where torch
    would raise or the kernel does not take the call (then F.conv_transpose raises or computes it on the fallback)."""
    s, p, op, d = _ints(stride, dims), _ints(padding, dims), _ints(output_padding, dims), _ints(dilation, dims)
    if s is None or p is None or op is None or d is None or min(s) < 1 or min(d) < 1 or min(p) < 0:
        return None
    if any(not 0 <= o < max(si, di) for o, si, di in zip(op, s, d)):
        return None  # torch: output padding must be smaller than either stride or dilation
    if any((n - 1) * si - 2 * pi + di * (k - 1) + o + 1 < 1 for n, si, pi, di, k, o in zip(input_shape, s, p, d, kernel, op)):
        return None
    if math.prod(s) > MAX_PHASES:
        return None
    if dims == 1:
        return (1, s[0]), (0, p[0]), (0, op[0]), (1, d[0])
    return (s[0], s[1]), (p[0], p[1]), (op[0], op[1]), (d[0], d[1])


class ConvTransposeKernels:
    """Predicates and kernels of ``conv_transpose1d`` / ``conv_transpose2d`` (through ``ConvKernels``' helpers)."""

    def __init__(self, conv: Any) -> None:
        self._c = conv
        self._m = conv._m
        self._k = conv._k

    def supported(self, dims: int, input: Any = None, weight: Any = None, bias: Any = None, stride: Any = 1, padding: Any = 0,
                  output_padding: Any = 0, groups: int = 1, dilation: Any = 1, output_quantizer: Any = None,
                  strict_quantization: bool | None = None, **_: Any) -> bool:
        k, codes_ok = self._k, self._c._codes_ok
        if not self._m._strict_ok(strict_quantization, output_quantizer, input, weight) or groups != 1:
            return False
        if not (codes_ok(input) and codes_ok(weight)) or input.dim() != dims + 2 or weight.dim() != dims + 2:
            return False
        if not _on_device(input, weight) or input.numel() == 0 or weight.numel() == 0 or input.shape[1] != weight.shape[0]:
            return False
        deq = k._deq_dtype(input)
        if deq not in _FLOATS or k._deq_dtype(weight) != deq:
            return False
        if k._tile(input) != tuple(input.shape) or k._tile(weight) not in (tuple(weight.shape), (weight.shape[0], 1, *weight.shape[2:])):
            return False  # per-tensor activations; per-tensor or per-output-channel (dim 1) weights
        if weight.shape[0] * math.prod(weight.shape[2:]) > MAX_REDUCTION:
            return False
        if transposed_geometry(dims, input.shape[2:], weight.shape[2:], stride, padding, output_padding, dilation) is None:
            return False
        if bias is not None:
            if isinstance(bias, k.surface.quantized_tensor):
                if not k.static_affine(bias) or k._deq_dtype(bias) != deq:
                    return False
            elif not isinstance(bias, torch.Tensor) or bias.dtype != deq:
                return False
            if bias.numel() != weight.shape[1] or not _on_device(bias):
                return False
        return not _needs_grad(input, weight, bias)

    def supported_conv_transpose1d(self, **kwargs: Any) -> bool:
        return self.supported(1, **kwargs)

    def supported_conv_transpose2d(self, **kwargs: Any) -> bool:
        return self.supported(2, **kwargs)

    def _conv_transpose(self, dims: int, input: Any, weight: Any, bias: Any, stride: Any, padding: Any, output_padding: Any,
                        dilation: Any, output_quantizer: Any) -> Any:
        k = self._k
        deq = k._deq_dtype(input)
        stride2, padding2, out_padding2, dilation2 = transposed_geometry(dims, input.shape[2:], weight.shape[2:], stride, padding,
                                                                         output_padding, dilation)
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
        out = ops.conv_transpose2d_w8a8(x, w, xs, xo, ws, wo, bias, stride2, padding2, out_padding2, dilation2, **args)
        if dims == 1:
            out = out.squeeze(2)
        return self._m._finish(out, [out], fused, output_quantizer, deq)

    def conv_transpose1d(self, input: Any, weight: Any, bias: Any = None, stride: Any = 1, padding: Any = 0, output_padding: Any = 0,
                         groups: int = 1, dilation: Any = 1, *, output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        return self._conv_transpose(1, input, weight, bias, stride, padding, output_padding, dilation, output_quantizer)

    def conv_transpose2d(self, input: Any, weight: Any, bias: Any = None, stride: Any = 1, padding: Any = 0, output_padding: Any = 0,
                         groups: int = 1, dilation: Any = 1, *, output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        return self._conv_transpose(2, input, weight, bias, stride, padding, output_padding, dilation, output_quantizer)


KERNELS = ConvTransposeKernels(_CONV)
conv_transpose1d_predicate = Predicate(KERNELS.supported_conv_transpose1d)
conv_transpose2d_predicate = Predicate(KERNELS.supported_conv_transpose2d)
_registrations = {
    "conv_transpose1d": register("conv_transpose1d", conv_transpose1d_predicate, KERNELS.conv_transpose1d),
    "conv_transpose2d": register("conv_transpose2d", conv_transpose2d_predicate, KERNELS.conv_transpose2d),
}
