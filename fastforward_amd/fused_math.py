"""The math operators — ``rms_norm``, ``pow``, ``exp``, ``sin``, ``cos``, ``sum``, ``cumsum`` — registered in this package's dispatcher.

The reference registers no kernel for them: ff.nn.functional runs the generated fallbacks (src/fastforward/_gen/fallback.py: pow :955,
sum :993, cumsum :1520, exp :1831, sin :1856, cos :1881, rms_norm :1906) — A2 of the quantized input, the ATen op, the output
quantizer: three launches with a temporary between each. The predicates below accept what the one-pass kernels of
csrc/ffq_math.hip cover and return False for everything else, so the reference chain (the fallbacks in
:mod:`fastforward_amd.nn.functional`) runs unchanged there. They follow the rules of ``ElementwiseKernels``
(fused_elementwise.py):

* calls of ``ff.nn.functional`` only: a call without the ``strict_quantization`` keyword (``torch.exp(qx)`` through
  ``QuantizedTensor.__torch_function__``) is declined;
* the input on the HIP device and the device library loaded (the C oracle declines);
* bf16 / fp16 values: a plain tensor, or static-affine codes (int8 or value-dtype container, <= 8 bits, fp32 parameters) with
  per-tensor or per-row parameters, 8 | numel (and 8 | the row of per-row parameters);
* ``rms_norm`` over the last dimension only, 8 | cols <= 16384, ``eps`` None (the fp32 epsilon, as F.rms_norm for bf16 / fp16) or
  a number; ``weight`` None, plain of the value dtype, or static-affine (dequantized on its own, as ``layer_norm``'s);
* ``pow`` by a Python number only (finite, |exponent| <= 65504): a tensor exponent takes the fallback;
* ``sum`` / ``cumsum`` over the last ``dim`` (dims of size 1 after it aside) of a multiple of 8 elements, and ``sum(dim=None)``
  (the whole tensor, a 0-dim result). A dim before the last is declined: the column kernels behind it (``ops.sum_quantize`` /
  ``ops.cumsum_quantize`` still take it) measured slower than the route (docs/kernels.md);
* any layout: a strided or misaligned view reaches the kernel as an aligned copy (``ops._base._dense``);
* no operand that needs a gradient while grad mode is on (the launches have no autograd formula);
* under strict quantization, only calls the fallback would accept (an output quantizer, a quantized input and weight).

The output quantizer runs inside the launch under the int8 GEMM's ``_requant`` rules (fused_modules.py); otherwise the launch
writes the value and the quantizer is called on it, so range estimation still sees the value.
"""

from __future__ import annotations

import math

from typing import Any

import torch

from fastforward_amd import ops
from fastforward_amd.dispatcher import Predicate, register
from fastforward_amd.fused_elementwise import ElementwiseKernels, _number
from fastforward_amd.fused_linear import KERNELS as _LINEAR
from fastforward_amd.fused_modules import _needs_grad, _on_device

_FP32_EPS = torch.finfo(torch.float32).eps


def _dim(dim: Any, ndim: int) -> int | None:
    """`dim` as a non-negative axis of an `ndim`-dim tensor, or None when it is not one."""
    if isinstance(dim, bool) or not isinstance(dim, int) or not -ndim <= dim < ndim:
        return None
    return dim + ndim if dim < 0 else dim


class MathKernels(ElementwiseKernels):
    """Predicates and kernels of ``rms_norm`` / ``pow`` / ``exp`` / ``sin`` / ``cos`` / ``sum`` / ``cumsum``."""

    def _call_ok(self, kwargs: dict[str, Any], output_quantizer: Any, *required: Any) -> bool:
        if "strict_quantization" not in kwargs or "out" in kwargs:
            return False
        return self._strict_ok(kwargs["strict_quantization"], output_quantizer, *required)

    # ---- rms_norm -----------------------------------------------------------------------------------------------------
    def supported_rms_norm(self, input: Any = None, normalized_shape: Any = None, weight: Any = None, eps: Any = None, *_args: Any,
                           output_quantizer: Any = None, **kwargs: Any) -> bool:
        if _args or not self._call_ok(kwargs, output_quantizer, input, *([] if weight is None else [weight])):
            return False
        dt = self._streamed(input)
        if dt is None:
            return False
        shape = tuple(normalized_shape) if isinstance(normalized_shape, (tuple, list, torch.Size)) else (normalized_shape,)
        cols = input.shape[-1]
        if shape != (cols,) or cols % 8 or cols > 16384 or not (eps is None or _number(eps)):
            return False
        if weight is not None:
            if isinstance(weight, self._k.surface.quantized_tensor):
                if not self.static_or_dequantizable(weight, dt):
                    return False
            elif not isinstance(weight, torch.Tensor) or weight.dtype != dt:  # (module parameters: nn.Parameter)
                return False
            if tuple(weight.shape) != shape or not _on_device(weight):
                return False
        return not _needs_grad(input, weight)

    def rms_norm(self, input: Any, normalized_shape: Any, weight: Any = None, eps: Any = None, *, output_quantizer: Any = None,
                 strict_quantization: bool | None = None) -> Any:
        dt = self._value_dtype(input)
        weight = weight.dequantize() if isinstance(weight, self._k.surface.quantized_tensor) else weight
        x, dequant = self._dequant(input)
        fused = self._output(output_quantizer, dt)
        value, codes = ops.rms_norm_quantize(x, weight, _FP32_EPS if eps is None else eps, dtype=dt, dequant=dequant, **self._launch_args(fused))
        return self._finish(value, codes, fused, output_quantizer, dt)

    # ---- pow / exp / sin / cos ----------------------------------------------------------------------------------------
    def supported_unary(self, input: Any = None, *_args: Any, output_quantizer: Any = None, **kwargs: Any) -> bool:
        if _args or not self._call_ok(kwargs, output_quantizer, input):
            return False
        return self._streamed(input) is not None and not _needs_grad(input)

    def supported_pow(self, input: Any = None, exponent: Any = None, *_args: Any, output_quantizer: Any = None, **kwargs: Any) -> bool:
        if not _number(exponent) or not math.isfinite(exponent) or abs(exponent) > 65504:
            return False
        return self.supported_unary(input, *_args, output_quantizer=output_quantizer, **kwargs)

    def _unary(self, op: str, input: Any, output_quantizer: Any, exponent: float = 0.0) -> Any:
        dt = self._value_dtype(input)
        x, dequant = self._dequant(input)
        fused = self._output(output_quantizer, dt)
        value, codes = ops.unary_quantize(op, x, exponent, dtype=dt, dequant=dequant, **self._launch_args(fused))
        return self._finish(value, codes, fused, output_quantizer, dt)

    def pow(self, input: Any, exponent: Any, *, output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        return self._unary("pow", input, output_quantizer, float(exponent))

    def exp(self, input: Any, *, output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        return self._unary("exp", input, output_quantizer)

    def sin(self, input: Any, *, output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        return self._unary("sin", input, output_quantizer)

    def cos(self, input: Any, *, output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        return self._unary("cos", input, output_quantizer)

    # ---- sum / cumsum -------------------------------------------------------------------------------------------------
    def _axes_ok(self, input: Any, dim: Any, whole: bool) -> bool:
        if whole and dim is None:
            return True
        d = _dim(dim, input.dim())
        if d is None:
            return False
        return math.prod(input.shape[d + 1:]) == 1 and input.shape[d] % 8 == 0

    def supported_sum(self, input: Any = None, dim: Any = None, *_args: Any, output_quantizer: Any = None, **kwargs: Any) -> bool:
        if not self.supported_unary(input, *_args, output_quantizer=output_quantizer, **kwargs):
            return False
        return self._axes_ok(input, dim, whole=True)

    def supported_cumsum(self, input: Any = None, dim: Any = None, *_args: Any, output_quantizer: Any = None, **kwargs: Any) -> bool:
        if not self.supported_unary(input, *_args, output_quantizer=output_quantizer, **kwargs):
            return False
        return self._axes_ok(input, dim, whole=False)

    def sum(self, input: Any, dim: int | None = None, *, output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        dt = self._value_dtype(input)
        x, dequant = self._dequant(input)
        fused = self._output(output_quantizer, dt)
        value, codes = ops.sum_quantize(x, dim, dtype=dt, dequant=dequant, **self._launch_args(fused))
        return self._finish(value, codes, fused, output_quantizer, dt)

    def cumsum(self, input: Any, dim: int, *, output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        dt = self._value_dtype(input)
        x, dequant = self._dequant(input)
        fused = self._output(output_quantizer, dt)
        value, codes = ops.cumsum_quantize(x, dim, dtype=dt, dequant=dequant, **self._launch_args(fused))
        return self._finish(value, codes, fused, output_quantizer, dt)


KERNELS = MathKernels(_LINEAR)
rms_norm_predicate = Predicate(KERNELS.supported_rms_norm)
pow_predicate = Predicate(KERNELS.supported_pow)
unary_predicate = Predicate(KERNELS.supported_unary)
sum_predicate = Predicate(KERNELS.supported_sum)
cumsum_predicate = Predicate(KERNELS.supported_cumsum)
_registrations = {
    "rms_norm": register("rms_norm", rms_norm_predicate, KERNELS.rms_norm),
    "pow": register("pow", pow_predicate, KERNELS.pow),
    "exp": register("exp", unary_predicate, KERNELS.exp),
    "sin": register("sin", unary_predicate, KERNELS.sin),
    "cos": register("cos", unary_predicate, KERNELS.cos),
    "sum": register("sum", sum_predicate, KERNELS.sum),
    "cumsum": register("cumsum", cumsum_predicate, KERNELS.cumsum),
}
