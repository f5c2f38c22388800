"""The reference's quantized elementwise operators as one-pass kernels with A1 fused in (csrc/ffq_elementwise.hip): add / sub /
mul / div, softmax over the last dimension, sigmoid and GELU, each with its quantized operands dequantized in registers (A2) and up
to three static per-tensor output quantizers (reference ff.nn.functional through _gen/fallback.py: softmax :269, sigmoid :321,
add :801, sub :840, mul :879, div :917, gelu :1373).

Operands given as codes come with ``dequant=(scale, offset)``: int8 or value-dtype codes with fp32 parameters, one pair for the
tensor or one per row of the last dimension. Each function returns ``(value or None, [codes per quantizer])``; the value has the
data dtype and the shape of the (first) input."""

from __future__ import annotations

import ctypes

import torch

from fastforward_amd.ops import _base
from fastforward_amd.ops._base import _ptr, _tag
from fastforward_amd.ops.modules import Quantizers, _entry, _operand
from fastforward_amd.ops.producers import _fan

BINARY_OPS = {"add": 0, "sub": 1, "mul": 2, "div": 3}
ACTIVATION_OPS = {"sigmoid": 0, "gelu": 1, "gelu_tanh": 2}


def _rows(x: torch.Tensor) -> tuple[int, int]:
    """(row length, rows) of the last dimension: the run of per-row parameters."""
    run = x.shape[-1] if x.dim() else 1
    return run, (x.numel() // run if run else 0)


def _suffix(b: torch.Tensor, a: torch.Tensor) -> bool:
    """b's shape, leading ones dropped, is a suffix of a's: element i of a meets b[i % b.numel()]."""
    shape = list(b.shape)
    while shape and shape[0] == 1:
        shape.pop(0)
    return b.dim() <= a.dim() and tuple(a.shape[a.dim() - len(shape):]) == tuple(shape)


def binary_quantize(
    op: str,
    a: torch.Tensor,
    b: torch.Tensor | float | int,
    quantizers: Quantizers = (),
    num_bits: float = 8.0,
    dtype: torch.dtype | None = None,
    a_dequant: tuple[torch.Tensor, torch.Tensor | None] | None = None,
    b_dequant: tuple[torch.Tensor, torch.Tensor | None] | None = None,
    alpha: float = 1,
    want_value: bool = True,
) -> tuple[torch.Tensor | None, list[torch.Tensor]]:
    """``torch.add / sub`` (with `alpha`), ``torch.mul / div`` of `a` and `b` + A1, one pass. `a` plain or codes as in
    :func:`~fastforward_amd.ops.modules.layer_norm_quantize`; `b` the same, of `a`'s shape or of a suffix of it (a bias), or a
    Python number."""
    if op not in BINARY_OPS:
        raise RuntimeError(f"binary_quantize: op is one of {sorted(BINARY_OPS)}, got {op!r}")
    dtype = dtype or a.dtype
    run, rows = _rows(a)
    ac, sa, oa, per_row_a = _operand(a, dtype, rows, a_dequant, "binary_quantize")
    if isinstance(b, torch.Tensor):
        if not _suffix(b, a):
            raise RuntimeError(f"binary_quantize: other's shape {tuple(b.shape)} must equal input's {tuple(a.shape)} or a suffix of it")
        b_run, b_rows = _rows(b)
        bc, sb, ob, per_row_b = _operand(b, dtype, b_rows, b_dequant, "binary_quantize")
        scalar = 0.0
    else:
        if b_dequant is not None:
            raise RuntimeError("binary_quantize: a scalar other has no parameters")
        bc, sb, ob, per_row_b, b_run, scalar = None, None, None, False, 0, float(b)
    lib, stream = _base._prepare(ac, sa, oa, bc, sb, ob, *[t for q in quantizers for t in q])
    value = torch.empty(ac.shape, dtype=dtype, device=ac.device) if want_value else None
    fan, codes, keep = _fan(quantizers, num_bits, ac.shape, ac.device)
    lib.check(
        _entry(lib, "ffq_binary_quantize")(
            BINARY_OPS[op], _ptr(ac), _tag(ac.dtype), _ptr(sa), _ptr(oa), run if per_row_a else 0,
            _ptr(bc), _tag(bc.dtype) if bc is not None else _tag(dtype), _ptr(sb), _ptr(ob), b_run if per_row_b else 0,
            bc.numel() if bc is not None else 0, scalar, float(alpha), _tag(dtype), ac.numel(), _ptr(value), ctypes.byref(fan), stream,
        )
    )
    del keep
    return value, codes


def softmax_quantize(
    x: torch.Tensor,
    quantizers: Quantizers = (),
    num_bits: float = 8.0,
    dtype: torch.dtype | None = None,
    dequant: tuple[torch.Tensor, torch.Tensor | None] | None = None,
    want_value: bool = True,
) -> tuple[torch.Tensor | None, list[torch.Tensor]]:
    """``F.softmax(x, -1)`` + A1, one pass; `x` plain or codes with per-tensor or per-row parameters."""
    dtype = dtype or x.dtype
    cols, rows = _rows(x)
    xc, s, o, per_row = _operand(x, dtype, rows, dequant, "softmax_quantize")
    lib, stream = _base._prepare(xc, s, o, *[t for q in quantizers for t in q])
    value = torch.empty(xc.shape, dtype=dtype, device=xc.device) if want_value else None
    fan, codes, keep = _fan(quantizers, num_bits, xc.shape, xc.device)
    lib.check(
        _entry(lib, "ffq_softmax_quantize")(
            _ptr(xc), _tag(xc.dtype), _ptr(s), _ptr(o), int(per_row), _tag(dtype), rows, cols, _ptr(value), ctypes.byref(fan), stream,
        )
    )
    del keep
    return value, codes


def activation_quantize(
    op: str,
    x: torch.Tensor,
    quantizers: Quantizers = (),
    num_bits: float = 8.0,
    dtype: torch.dtype | None = None,
    dequant: tuple[torch.Tensor, torch.Tensor | None] | None = None,
    want_value: bool = True,
) -> tuple[torch.Tensor | None, list[torch.Tensor]]:
    """``torch.sigmoid`` (op="sigmoid"), ``F.gelu`` (op="gelu") or ``F.gelu(approximate="tanh")`` (op="gelu_tanh") + A1, one pass;
    `x` plain or codes as in :func:`softmax_quantize`."""
    if op not in ACTIVATION_OPS:
        raise RuntimeError(f"activation_quantize: op is one of {sorted(ACTIVATION_OPS)}, got {op!r}")
    dtype = dtype or x.dtype
    run, rows = _rows(x)
    xc, s, o, per_row = _operand(x, dtype, rows, dequant, "activation_quantize")
    lib, stream = _base._prepare(xc, s, o, *[t for q in quantizers for t in q])
    value = torch.empty(xc.shape, dtype=dtype, device=xc.device) if want_value else None
    fan, codes, keep = _fan(quantizers, num_bits, xc.shape, xc.device)
    lib.check(
        _entry(lib, "ffq_activation_quantize")(
            ACTIVATION_OPS[op], _ptr(xc), _tag(xc.dtype), _ptr(s), _ptr(o), run if per_row else 0, _tag(dtype), xc.numel(),
            _ptr(value), ctypes.byref(fan), stream,
        )
    )
    del keep
    return value, codes
