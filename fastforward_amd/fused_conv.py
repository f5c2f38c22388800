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

import dataclasses
import math

from typing import Any, Callable

import torch

from fastforward_amd import _native, ops
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


@dataclasses.dataclass(frozen=True)
class ConvSet:
    """What one set of convolution kernels tells ``ConvKernels`` — the one predicate and the one run body — about itself."""

    in_axis: int  # the weight axis with one group's input channels: input.shape[1] == weight.shape[in_axis] * groups
    oc_axis: int  # the weight axis with the output channels: the bias's length, and the 1 of a per-output-channel tile
    groups_rule: Callable[[Any], bool]  # the `groups` the kernel is built for, on the argument alone: the cheap first decline
    grouping_rule: Callable[[Any, Any, Any, Any], bool]  # (groups, input shape, weight shape, weight codes): what that grouping asks of the operands
    bound: int  # on weight.shape[in_axis] * prod(kernel): the int32 accumulator's reduction, or the taps one channel keeps on chip
    geometry: Callable[..., Any]  # (dims, input size, kernel, *operands) -> the launch's geometry, None where the kernel declines
    geometry_operands: tuple[str, ...]  # the operator's arguments `geometry` takes as operands, in its order
    op: str  # the wrapper's name in fastforward_amd.ops, looked up per call: op(x, w, x_scale, x_offset, w_scale, w_offset, bias, *geometry's result, **output arguments)
    symbol: str | None = None  # the entry point the loaded library has to export (None: every device library has it)


_DEFAULTS = {"stride": 1, "padding": 0, "output_padding": 0, "dilation": 1}  # torch's, for a predicate called without them


class ConvKernels:
    """Predicates and kernels of one ``ConvSet`` (on the int8 GEMM's Surface, through the generic modules' helpers): ``conv1d`` /
    ``conv2d`` here and in fused_depthwise.py; fused_conv3d.py and fused_conv_transpose.py add their operators' signatures."""

    def __init__(self, modules: Any, kernel_set: ConvSet) -> None:
        self._m = modules
        self._k = modules._k
        self._set = kernel_set

    def _codes_ok(self, t: Any) -> bool:
        k = self._k
        if not k.static_affine(t) or not k._bits_ok(t):
            return False
        p = k._params(t)
        return t.raw_data.dtype in (torch.int8, *_FLOATS) and _fp32_param(p.scale) and _fp32_param(p.offset)

    def supported(self, dims: int, input: Any = None, weight: Any = None, bias: Any = None, groups: int = 1, output_quantizer: Any = None,
                  strict_quantization: bool | None = None, **operands: Any) -> bool:
        k, s = self._k, self._set
        if not self._m._strict_ok(strict_quantization, output_quantizer, input, weight) or not s.groups_rule(groups):
            return False
        if not (self._codes_ok(input) and self._codes_ok(weight)) or input.dim() != dims + 2 or weight.dim() != dims + 2:
            return False
        x_shape, w_shape = tuple(input.shape), tuple(weight.shape)  # (once: an attribute of a quantized tensor is a dispatched call)
        if x_shape[1] != w_shape[s.in_axis] * groups or not s.grouping_rule(groups, x_shape, w_shape, weight):
            return False
        if not _on_device(input, weight) or input.numel() == 0 or weight.numel() == 0:
            return False
        deq = k._deq_dtype(input)
        if deq not in _FLOATS or k._deq_dtype(weight) != deq:
            return False
        per_channel = tuple(1 if axis == s.oc_axis else n for axis, n in enumerate(w_shape))
        if k._tile(input) != x_shape or k._tile(weight) not in (w_shape, per_channel):
            return False  # per-tensor activations; per-tensor or per-output-channel weights
        if w_shape[s.in_axis] * math.prod(w_shape[2:]) > s.bound:
            return False
        if s.geometry(dims, x_shape[2:], w_shape[2:], *(operands.get(n, _DEFAULTS[n]) for n in s.geometry_operands)) is None:
            return False
        if bias is not None:
            if isinstance(bias, k.surface.quantized_tensor):
                if not k.static_affine(bias) or k._deq_dtype(bias) != deq:
                    return False
            elif not isinstance(bias, torch.Tensor) or bias.dtype != deq:
                return False
            if bias.numel() != w_shape[s.oc_axis] or not _on_device(bias):
                return False
        return not _needs_grad(input, weight, bias)

    def _accepts(self, dims: int, **kwargs: Any) -> bool:
        # (`supported` first: it is what establishes that the device library is loaded)
        return self.supported(dims, **kwargs) and (self._set.symbol is None or getattr(_native.library(), self._set.symbol, None) is not None)

    def supported_conv1d(self, **kwargs: Any) -> bool:
        return self._accepts(1, **kwargs)

    def supported_conv2d(self, **kwargs: Any) -> bool:
        return self._accepts(2, **kwargs)

    def _run(self, dims: int, input: Any, weight: Any, bias: Any, output_quantizer: Any, *operands: Any) -> Any:
        """The launch of a call `supported` took; `operands` are the set's ``geometry_operands``. A 1-D call runs as the 2-D one with
        H = KH = 1 (that is what `geometry` answers for it)."""
        k = self._k
        deq = k._deq_dtype(input)
        launch_geometry = self._set.geometry(dims, input.shape[2:], weight.shape[2:], *operands)
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
        out = getattr(ops, self._set.op)(x, w, xs, xo, ws, wo, bias, *launch_geometry, **args)
        if dims == 1:
            out = out.squeeze(2)
        return self._m._finish(out, [out], fused, output_quantizer, deq)

    def conv1d(self, input: Any, weight: Any, bias: Any = None, stride: Any = 1, padding: Any = 0, dilation: Any = 1, groups: int = 1, *,
               output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        return self._run(1, input, weight, bias, output_quantizer, stride, padding, dilation)

    def conv2d(self, input: Any, weight: Any, bias: Any = None, stride: Any = 1, padding: Any = 0, dilation: Any = 1, groups: int = 1, *,
               output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        return self._run(2, input, weight, bias, output_quantizer, stride, padding, dilation)


def ungrouped(groups: Any) -> bool:
    """The groups rule of the implicit GEMMs: they are built for ``groups == 1``."""
    return groups == 1


def any_operands(groups: Any, x_shape: Any, w_shape: Any, weight: Any) -> bool:
    """... which asks nothing more of the operands."""
    return True


KERNELS = ConvKernels(_MODULES, ConvSet(in_axis=1, oc_axis=0, groups_rule=ungrouped, grouping_rule=any_operands, bound=MAX_REDUCTION, geometry=geometry,
                                        geometry_operands=("stride", "padding", "dilation"), op="conv2d_w8a8"))
conv1d_predicate = Predicate(KERNELS.supported_conv1d)
conv2d_predicate = Predicate(KERNELS.supported_conv2d)
_registrations = {
    "conv1d": register("conv1d", conv1d_predicate, KERNELS.conv1d),
    "conv2d": register("conv2d", conv2d_predicate, KERNELS.conv2d),
}
