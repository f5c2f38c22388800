"""The reference's quantized rms_norm, pow by a number, exp, sin, cos, sum and cumsum as one-pass kernels with A1 fused in
(csrc/ffq_math.hip), each with its quantized input dequantized in registers (A2) and up to three static per-tensor output
quantizers (reference ff.nn.functional through _gen/fallback.py: pow :955, sum :993, cumsum :1520, exp :1831, sin :1856, cos :1881,
rms_norm :1906).

An input given as codes comes with ``dequant=(scale, offset)``: int8 or value-dtype codes with fp32 parameters, one pair for the
tensor or one per row of the last dimension. Each function returns ``(value or None, [codes per quantizer])``; the value has the
data dtype and the shape the ATen op gives."""

from __future__ import annotations

import ctypes
import math

import torch

from fastforward_amd.ops import _base
from fastforward_amd.ops._base import _ptr, _tag
from fastforward_amd.ops.elementwise import _rows
from fastforward_amd.ops.modules import Quantizers, _entry, _operand
from fastforward_amd.ops.producers import _fan

UNARY_OPS = {"exp": 0, "sin": 1, "cos": 2, "pow": 3}


def _axes(x: torch.Tensor, dim: int | None) -> tuple[int, int, int]:
    """[outer, len, inner] of a reduction or scan of `x` over `dim` (None: the whole tensor)."""
    if dim is None:
        return 1, x.numel(), 1
    d = dim + x.dim() if dim < 0 else dim
    if not 0 <= d < max(x.dim(), 1):
        raise IndexError(f"Dimension out of range (expected to be in range of [{-x.dim()}, {x.dim() - 1}], but got {dim})")
    if x.dim() == 0:
        return 1, 1, 1
    return math.prod(x.shape[:d]), x.shape[d], math.prod(x.shape[d + 1:])


def rms_norm_quantize(
    x: torch.Tensor,
    weight: torch.Tensor | None,
    eps: float,
    quantizers: Quantizers = (),
    num_bits: float = 8.0,
    dtype: torch.dtype | None = None,
    dequant: tuple[torch.Tensor, torch.Tensor | None] | None = None,
    want_value: bool = True,
) -> tuple[torch.Tensor | None, list[torch.Tensor]]:
    """``F.rms_norm(x, (x.shape[-1],), weight, eps)`` + A1, one pass; `x` plain or codes with per-tensor or per-row parameters.
    `eps` is a number (F.rms_norm's ``eps=None`` is ``torch.finfo(torch.float32).eps`` for bf16 / fp16)."""
    dtype = dtype or x.dtype
    cols, rows = _rows(x)
    xc, s, o, per_row = _operand(x, dtype, rows, dequant, "rms_norm_quantize")
    wc = None if weight is None else _base._dense(weight.detach())
    if wc is not None and (wc.numel() != cols or wc.dtype != dtype):
        raise RuntimeError(f"rms_norm_quantize: weight must hold {cols} elements of {dtype}")
    lib, stream = _base._prepare(xc, s, o, wc, *[t for q in quantizers for t in q])
    value = torch.empty(xc.shape, dtype=dtype, device=xc.device) if want_value else None
    fan, codes, keep = _fan(quantizers, num_bits, xc.shape, xc.device)
    lib.check(
        _entry(lib, "ffq_rms_norm_quantize")(
            _ptr(xc), _tag(xc.dtype), _ptr(s), _ptr(o), int(per_row), _ptr(wc), _tag(dtype), rows, cols, float(eps), _ptr(value),
            ctypes.byref(fan), stream,
        )
    )
    del keep
    return value, codes


def unary_quantize(
    op: str,
    x: torch.Tensor,
    exponent: float = 0.0,
    quantizers: Quantizers = (),
    num_bits: float = 8.0,
    dtype: torch.dtype | None = None,
    dequant: tuple[torch.Tensor, torch.Tensor | None] | None = None,
    want_value: bool = True,
) -> tuple[torch.Tensor | None, list[torch.Tensor]]:
    """``torch.exp / sin / cos`` (op="exp" / "sin" / "cos") or ``torch.pow(x, exponent)`` for a Python number (op="pow") + A1, one
    pass; `x` plain or codes as in :func:`rms_norm_quantize`."""
    if op not in UNARY_OPS:
        raise RuntimeError(f"unary_quantize: op is one of {sorted(UNARY_OPS)}, got {op!r}")
    dtype = dtype or x.dtype
    run, rows = _rows(x)
    xc, s, o, per_row = _operand(x, dtype, rows, dequant, "unary_quantize")
    lib, stream = _base._prepare(xc, s, o, *[t for q in quantizers for t in q])
    value = torch.empty(xc.shape, dtype=dtype, device=xc.device) if want_value else None
    fan, codes, keep = _fan(quantizers, num_bits, xc.shape, xc.device)
    lib.check(
        _entry(lib, "ffq_unary_quantize")(
            UNARY_OPS[op], _ptr(xc), _tag(xc.dtype), _ptr(s), _ptr(o), run if per_row else 0, float(exponent) if op == "pow" else 0.0,
            _tag(dtype), xc.numel(), _ptr(value), ctypes.byref(fan), stream,
        )
    )
    del keep
    return value, codes


def sum_quantize(
    x: torch.Tensor,
    dim: int | None = None,
    quantizers: Quantizers = (),
    num_bits: float = 8.0,
    dtype: torch.dtype | None = None,
    dequant: tuple[torch.Tensor, torch.Tensor | None] | None = None,
    want_value: bool = True,
) -> tuple[torch.Tensor | None, list[torch.Tensor]]:
    """``torch.sum(x, dim)`` + A1 with an fp32 accumulator; ``dim=None`` sums the whole tensor into a 0-dim result. `x` plain or
    codes as in :func:`rms_norm_quantize`."""
    dtype = dtype or x.dtype
    run, rows = _rows(x)
    outer, length, inner = _axes(x, dim)
    shape = () if dim is None else tuple(n for i, n in enumerate(x.shape) if i != (dim + x.dim() if dim < 0 else dim))
    xc, s, o, per_row = _operand(x, dtype, rows, dequant, "sum_quantize")
    lib, stream = _base._prepare(xc, s, o, *[t for q in quantizers for t in q])
    value = torch.empty(shape, dtype=dtype, device=xc.device) if want_value else None
    fan, codes, keep = _fan(quantizers, num_bits, shape, xc.device)
    nbytes = int(_entry(lib, "ffq_sum_quantize_workspace_bytes")(outer, length, inner))
    ws = _base._workspace(nbytes, xc.device)
    lib.check(
        _entry(lib, "ffq_sum_quantize")(
            _ptr(xc), _tag(xc.dtype), _ptr(s), _ptr(o), run if per_row else 0, _tag(dtype), outer, length, inner, _ptr(value),
            ctypes.byref(fan), _ptr(ws), nbytes, stream,
        )
    )
    del keep
    return value, codes


def cumsum_quantize(
    x: torch.Tensor,
    dim: int,
    quantizers: Quantizers = (),
    num_bits: float = 8.0,
    dtype: torch.dtype | None = None,
    dequant: tuple[torch.Tensor, torch.Tensor | None] | None = None,
    want_value: bool = True,
) -> tuple[torch.Tensor | None, list[torch.Tensor]]:
    """``torch.cumsum(x, dim)`` + A1 with an fp32 running sum, each prefix rounded once. `x` plain or codes as in
    :func:`rms_norm_quantize`."""
    dtype = dtype or x.dtype
    run, rows = _rows(x)
    outer, length, inner = _axes(x, dim)
    xc, s, o, per_row = _operand(x, dtype, rows, dequant, "cumsum_quantize")
    lib, stream = _base._prepare(xc, s, o, *[t for q in quantizers for t in q])
    value = torch.empty(xc.shape, dtype=dtype, device=xc.device) if want_value else None
    fan, codes, keep = _fan(quantizers, num_bits, xc.shape, xc.device)
    lib.check(
        _entry(lib, "ffq_cumsum_quantize")(
            _ptr(xc), _tag(xc.dtype), _ptr(s), _ptr(o), run if per_row else 0, _tag(dtype), outer, length, inner, _ptr(value),
            ctypes.byref(fan), stream,
        )
    )
    del keep
    return value, codes
