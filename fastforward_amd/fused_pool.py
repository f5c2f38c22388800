"""The spatial operators — ``avg_pool1d``, ``avg_pool2d``, ``avg_pool3d``, ``max_pool2d``, ``interpolate`` — registered in this package's
dispatcher.

The reference registers no kernel for them: ff.nn.functional runs the generated fallbacks (src/fastforward/_gen/fallback.py:
avg_pool1d :505, avg_pool2d :542, avg_pool3d :579, max_pool2d :1574, interpolate :1611) — A2 of the quantized input, the ATen op, the output
quantizer: three launches with a temporary between each. The predicates below accept what the one-pass kernels of
csrc/ffq_pool.hip (and csrc/ffq_pool3d.hip) cover and return False for everything else, so the reference chain (the fallbacks in
:mod:`fastforward_amd.nn.functional`) runs unchanged there. They follow the rules of ``MathKernels`` (fused_math.py):

* calls of ``ff.nn.functional`` only: a call without the ``strict_quantization`` keyword is declined;
* the input on the HIP device and the device library loaded (the C oracle declines);
* bf16 / fp16 values: a plain tensor, or static-affine codes (int8 or value-dtype container, <= 8 bits, fp32 parameters) with
  per-tensor or per-channel (``PerChannel(1)``) parameters;
* a batched input: ``[B, C, H, W]`` for the 2-D pools, ``[B, C, L]`` for ``avg_pool1d``, ``[B, C, D, H, W]`` for ``avg_pool3d`` (whose
  entry point, include/ffq_3d.h, the loaded library must export), 3-D or 4-D for ``interpolate``; fewer than 2^31
  input and output elements. Planes of any size: nothing here asks for a multiple of 8;
* any layout but one: a strided or misaligned view reaches the kernel as an aligned copy (``ops._base._dense``); an input whose
  strides are channels-last is declined, because ATen answers it with a channels-last result (``avg_pool3d`` declines a
  ``channels_last_3d`` input likewise);
* the pools: int or tuple ``kernel_size`` / ``stride`` / ``padding`` (/ ``dilation``), ``ceil_mode`` and ``count_include_pad``
  either way; geometry ATen refuses (padding beyond half the kernel, an empty output) is declined, so the fallback raises ATen's error;
* ``interpolate``: ``mode`` "nearest" or "nearest-exact", exactly one of ``size`` / ``scale_factor``, ``align_corners`` None,
  ``antialias`` False, ``recompute_scale_factor`` None or False; an output of the input's size is declined (ATen copies it);
* no operand that needs a gradient while grad mode is on (the launches have no autograd formula);
* under strict quantization, only calls the fallback would accept (an output quantizer, a quantized input).

The output quantizer runs inside the launch under the int8 GEMM's ``_requant`` rules (fused_modules.py); otherwise the launch
writes the value and the quantizer is called on it, so range estimation still sees the value.
"""

from __future__ import annotations

import math

from typing import Any

import torch

from fastforward_amd import _native, ops
from fastforward_amd.dispatcher import Predicate, register
from fastforward_amd.fused_elementwise import _number
from fastforward_amd.fused_linear import KERNELS as _LINEAR
from fastforward_amd.fused_math import MathKernels
from fastforward_amd.fused_modules import _needs_grad, _on_device
from fastforward_amd.ops.pool import pooled_size

_LIMIT = 2**31


def _ints(v: Any, n: int) -> tuple[int, ...] | None:
    """`v` as `n` ints the way ATen's int lists take it (one int for every dim), or None."""
    if isinstance(v, (tuple, list, torch.Size)) and len(v) in (1, n):
        v = tuple(v) * (n // len(v))
    elif not isinstance(v, (tuple, list)):
        v = (v,) * n
    else:
        return None
    if any(isinstance(i, bool) or not isinstance(i, int) for i in v):
        return None
    return v


def _channels_last_strides(t: torch.Tensor) -> bool:
    """ATen's ``is_channels_last_strides_2d`` of a 4-D tensor: what makes its pooling and upsampling answer in channels-last."""
    least = 0
    for d in (1, 3, 2, 0):
        if t.shape[d] == 0 or t.stride(d) < least or (d == 0 and least == t.stride(1)):
            return False
        least = t.stride(d) * max(t.shape[d], 1)
    return True


class PoolKernels(MathKernels):
    """Predicates and kernels of ``avg_pool1d`` / ``avg_pool2d`` / ``max_pool2d`` / ``interpolate`` (an ``ElementwiseKernels`` through
    ``MathKernels``, whose ``_call_ok`` holds the rule for the ``strict_quantization`` keyword)."""

    # ---- what an input is ---------------------------------------------------------------------------------------------
    def _planes(self, x: Any, dims: tuple[int, ...]) -> torch.dtype | None:
        """The value dtype of a batched [B, C, *spatial] input on the device in a form the kernels take, else None."""
        dt = self._value_dtype(x)
        if dt is None or x.dim() not in dims or x.numel() == 0 or x.numel() >= _LIMIT or not _on_device(x):
            return None
        data = x
        if isinstance(x, self._k.surface.quantized_tensor):
            tile, shape = self._k._tile(x), tuple(x.shape)
            if tile != shape and tile != (shape[0], 1, *shape[2:]):
                return None
            data = x.raw_data
        if data.dim() == 5:
            if not data.is_contiguous() and data.is_contiguous(memory_format=torch.channels_last_3d):
                return None
        elif not data.is_contiguous() and _channels_last_strides(data if data.dim() == 4 else data.unsqueeze(-2)):
            return None
        return dt

    # ---- avg_pool1d / avg_pool2d / max_pool2d --------------------------------------------------------------------------
    def _geometry(self, input: Any, n: int, kernel_size: Any, stride: Any, padding: Any, dilation: Any, ceil_mode: Any) -> bool:
        k, s, p, d = _ints(kernel_size, n), _ints(stride, n), _ints(padding, n), _ints(dilation, n)
        if None in (k, s, p, d) or not isinstance(ceil_mode, bool):
            return False
        total = math.prod(input.shape[:2])
        for size, ki, si, pi, di in zip(input.shape[2:], k, s, p, d):
            if min(ki, si, di) < 1 or not 0 <= pi <= ki // 2 or max(ki, si, di) > 2**20:
                return False
            out = pooled_size(size, ki, pi, si, di, ceil_mode)
            if out < 1:
                return False
            total *= out
        return total < _LIMIT

    def _supported_pool(self, n: int, input: Any, kernel_size: Any, stride: Any, padding: Any, dilation: Any, ceil_mode: Any,
                        output_quantizer: Any, kwargs: dict[str, Any]) -> bool:
        if not self._call_ok(kwargs, output_quantizer, input) or self._planes(input, (n + 2,)) is None:
            return False
        return self._geometry(input, n, kernel_size, stride, padding, dilation, ceil_mode) and not _needs_grad(input)

    def supported_avg_pool1d(self, input: Any = None, kernel_size: Any = None, stride: Any = None, padding: Any = 0, ceil_mode: Any = False,
                             count_include_pad: Any = True, *_args: Any, output_quantizer: Any = None, **kwargs: Any) -> bool:
        if _args or not isinstance(count_include_pad, bool):
            return False
        return self._supported_pool(1, input, kernel_size, stride, padding, 1, ceil_mode, output_quantizer, kwargs)

    def supported_avg_pool2d(self, input: Any = None, kernel_size: Any = None, stride: Any = None, padding: Any = 0, ceil_mode: Any = False,
                             count_include_pad: Any = True, *_args: Any, output_quantizer: Any = None, **kwargs: Any) -> bool:
        if _args or not isinstance(count_include_pad, bool):
            return False
        return self._supported_pool(2, input, kernel_size, stride, padding, 1, ceil_mode, output_quantizer, kwargs)

    def supported_avg_pool3d(self, input: Any = None, kernel_size: Any = None, stride: Any = None, padding: Any = 0, ceil_mode: Any = False,
                             count_include_pad: Any = True, *_args: Any, output_quantizer: Any = None, **kwargs: Any) -> bool:
        if _args or not isinstance(count_include_pad, bool):
            return False
        if not self._supported_pool(3, input, kernel_size, stride, padding, 1, ceil_mode, output_quantizer, kwargs):
            return False
        return getattr(_native.library(), "ffq_pool3d_quantize", None) is not None

    def supported_max_pool2d(self, input: Any = None, kernel_size: Any = None, stride: Any = None, padding: Any = 0, dilation: Any = 1,
                             ceil_mode: Any = False, *_args: Any, output_quantizer: Any = None, **kwargs: Any) -> bool:
        if _args:
            return False
        stride = kernel_size if stride is None else stride
        return self._supported_pool(2, input, kernel_size, stride, padding, dilation, ceil_mode, output_quantizer, kwargs)

    def _pool(self, mode: str, n: int, input: Any, kernel_size: Any, stride: Any, padding: Any, dilation: Any, ceil_mode: bool,
              output_quantizer: Any) -> Any:
        dt = self._value_dtype(input)
        x, dequant = self._dequant(input)
        fused = self._output(output_quantizer, dt)
        k, s, p, d = ((1,) * (2 - n) + _ints(v, n) for v in (kernel_size, stride, padding, dilation))
        if n == 1:  # avg_pool1d is avg_pool2d with H = KH = 1, as in ATen
            x, p = x.unsqueeze(-2), (0, p[1])
        value, codes = ops.pool2d_quantize(mode, x, k, s, p, d, ceil_mode, dtype=dt, dequant=dequant, **self._launch_args(fused))
        if n == 1:
            value, codes = None if value is None else value.squeeze(-2), [c.squeeze(-2) for c in codes]
        return self._finish(value, codes, fused, output_quantizer, dt)

    def avg_pool1d(self, input: Any, kernel_size: Any, stride: Any, padding: Any = 0, ceil_mode: bool = False, count_include_pad: bool = True, *,
                   output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        return self._pool("avg" if count_include_pad else "avg_exclude_pad", 1, input, kernel_size, stride, padding, 1, ceil_mode, output_quantizer)

    def avg_pool2d(self, input: Any, kernel_size: Any, stride: Any, padding: Any = 0, ceil_mode: bool = False, count_include_pad: bool = True, *,
                   output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        return self._pool("avg" if count_include_pad else "avg_exclude_pad", 2, input, kernel_size, stride, padding, 1, ceil_mode, output_quantizer)

    def avg_pool3d(self, input: Any, kernel_size: Any, stride: Any, padding: Any = 0, ceil_mode: bool = False, count_include_pad: bool = True, *,
                   output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        dt = self._value_dtype(input)
        x, dequant = self._dequant(input)
        fused = self._output(output_quantizer, dt)
        k, s, p = (_ints(v, 3) for v in (kernel_size, stride, padding))
        value, codes = ops.pool3d_quantize("avg" if count_include_pad else "avg_exclude_pad", x, k, s, p, ceil_mode, dtype=dt, dequant=dequant,
                                           **self._launch_args(fused))
        return self._finish(value, codes, fused, output_quantizer, dt)

    def max_pool2d(self, input: Any, kernel_size: Any, stride: Any = None, padding: Any = 0, dilation: Any = 1, ceil_mode: bool = False, *,
                   output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        return self._pool("max", 2, input, kernel_size, kernel_size if stride is None else stride, padding, dilation, ceil_mode, output_quantizer)

    # ---- interpolate --------------------------------------------------------------------------------------------------
    @staticmethod
    def _target(input: Any, size: Any, scale_factor: Any) -> tuple[tuple[int, ...], tuple[float, ...] | None] | None:
        """(output size, the scale factors ATen maps indices by or None) of a nearest ``F.interpolate``, or None when the
        arguments are not ones it takes: exactly one of `size` / `scale_factor`, an int / number or one per spatial dim."""
        n = input.dim() - 2
        if (size is None) == (scale_factor is None):
            return None
        if size is not None:
            if isinstance(size, (tuple, list)) and len(size) != n:
                return None
            out = _ints(size, n)
            return None if out is None or min(out) < 1 else (out, None)
        factors = tuple(scale_factor) if isinstance(scale_factor, (tuple, list)) else (scale_factor,) * n
        if len(factors) != n or not all(_number(f) and math.isfinite(f) and f > 0 for f in factors):
            return None
        out = tuple(int(extent * float(f)) for extent, f in zip(input.shape[2:], factors))  # ATen: the double product, truncated
        return None if min(out) < 1 else (out, tuple(float(f) for f in factors))

    def supported_interpolate(self, input: Any = None, size: Any = None, scale_factor: Any = None, mode: Any = "nearest", align_corners: Any = None,
                              recompute_scale_factor: Any = None, antialias: Any = False, *_args: Any, output_quantizer: Any = None,
                              **kwargs: Any) -> bool:
        if _args or not self._call_ok(kwargs, output_quantizer, input):
            return False
        if mode not in ("nearest", "nearest-exact") or align_corners is not None or antialias is not False:
            return False
        if recompute_scale_factor not in (None, False) or self._planes(input, (3, 4)) is None:
            return False
        target = self._target(input, size, scale_factor)
        if target is None or target[0] == tuple(input.shape[2:]) or math.prod(input.shape[:2]) * math.prod(target[0]) >= _LIMIT:
            return False
        return not _needs_grad(input)

    def interpolate(self, input: Any, size: Any = None, scale_factor: Any = None, mode: str = "nearest", align_corners: Any = None,
                    recompute_scale_factor: Any = None, antialias: bool = False, *, output_quantizer: Any = None,
                    strict_quantization: bool | None = None) -> Any:
        dt = self._value_dtype(input)
        out, factors = self._target(input, size, scale_factor)
        x, dequant = self._dequant(input)
        fused = self._output(output_quantizer, dt)
        flat = input.dim() == 3  # [B, C, L] is [B, C, 1, L]
        if flat:
            x, out, factors = x.unsqueeze(-2), (1, *out), None if factors is None else (0.0, *factors)
        value, codes = ops.upsample_nearest_quantize(x, out, factors, mode, dtype=dt, dequant=dequant, **self._launch_args(fused))
        if flat:
            value, codes = None if value is None else value.squeeze(-2), [c.squeeze(-2) for c in codes]
        return self._finish(value, codes, fused, output_quantizer, dt)


KERNELS = PoolKernels(_LINEAR)
avg_pool1d_predicate = Predicate(KERNELS.supported_avg_pool1d)
avg_pool2d_predicate = Predicate(KERNELS.supported_avg_pool2d)
avg_pool3d_predicate = Predicate(KERNELS.supported_avg_pool3d)
max_pool2d_predicate = Predicate(KERNELS.supported_max_pool2d)
interpolate_predicate = Predicate(KERNELS.supported_interpolate)
_registrations = {
    "avg_pool1d": register("avg_pool1d", avg_pool1d_predicate, KERNELS.avg_pool1d),
    "avg_pool2d": register("avg_pool2d", avg_pool2d_predicate, KERNELS.avg_pool2d),
    "avg_pool3d": register("avg_pool3d", avg_pool3d_predicate, KERNELS.avg_pool3d),
    "max_pool2d": register("max_pool2d", max_pool2d_predicate, KERNELS.max_pool2d),
    "interpolate": register("interpolate", interpolate_predicate, KERNELS.interpolate),
}
