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

from fastforward_amd.dispatcher import Predicate, register
from fastforward_amd.fused_conv import MAX_REDUCTION, ConvKernels, ConvSet, _ints, any_operands, ungrouped
from fastforward_amd.fused_modules import KERNELS as _MODULES
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


class ConvTransposeKernels(ConvKernels):
    """Predicates and kernels of ``conv_transpose1d`` / ``conv_transpose2d``: ``ConvKernels``' rules and run body under the
    operators' names and argument order."""

    def supported_conv_transpose1d(self, **kwargs: Any) -> bool:
        return self._accepts(1, **kwargs)

    def supported_conv_transpose2d(self, **kwargs: Any) -> bool:
        return self._accepts(2, **kwargs)

    def conv_transpose1d(self, input: Any, weight: Any, bias: Any = None, stride: Any = 1, padding: Any = 0, output_padding: Any = 0,
                         groups: int = 1, dilation: Any = 1, *, output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        return self._run(1, input, weight, bias, output_quantizer, stride, padding, output_padding, dilation)

    def conv_transpose2d(self, input: Any, weight: Any, bias: Any = None, stride: Any = 1, padding: Any = 0, output_padding: Any = 0,
                         groups: int = 1, dilation: Any = 1, *, output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        return self._run(2, input, weight, bias, output_quantizer, stride, padding, output_padding, dilation)


KERNELS = ConvTransposeKernels(_MODULES, ConvSet(in_axis=0, oc_axis=1, groups_rule=ungrouped, grouping_rule=any_operands, bound=MAX_REDUCTION,
                                                 geometry=transposed_geometry,
                                                 geometry_operands=("stride", "padding", "output_padding", "dilation"),
                                                 op="conv_transpose2d_w8a8"))
conv_transpose1d_predicate = Predicate(KERNELS.supported_conv_transpose1d)
conv_transpose2d_predicate = Predicate(KERNELS.supported_conv_transpose2d)
_registrations = {
    "conv_transpose1d": register("conv_transpose1d", conv_transpose1d_predicate, KERNELS.conv_transpose1d),
    "conv_transpose2d": register("conv_transpose2d", conv_transpose2d_predicate, KERNELS.conv_transpose2d),
}
