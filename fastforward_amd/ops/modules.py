"""The reference's generic quantized modules as one-pass kernels with A1 fused in (csrc/ffq_modules.hip): LayerNorm, Embedding,
ReLU and SiLU, each with its quantized operand dequantized in registers (A2) and up to three static per-tensor output quantizers
(reference nn/normalization.py, nn/embedding.py, nn/activations.py through _gen/fallback.py: layer_norm :655, embedding :616,
relu :296, silu :1348).

Operands given as codes are ``(codes, scale, offset)`` triples: int8 or value-dtype codes with fp32 parameters, one pair for the
tensor or one per row. Each function returns ``(value or None, [codes per quantizer])``; the value has the data dtype."""

from __future__ import annotations

import ctypes

from typing import Sequence

import torch

from fastforward_amd.exceptions import BackendError
from fastforward_amd.ops import _base
from fastforward_amd.ops._base import _dense, _ptr, _tag
from fastforward_amd.ops.producers import _fan

Quantizers = Sequence[tuple[torch.Tensor, torch.Tensor | None]]
VALUE_DTYPES = (torch.bfloat16, torch.float16)
POINTWISE_OPS = {"relu": 0, "silu": 1}


def _entry(lib, name: str):
    fn = getattr(lib, name, None)
    if fn is None:
        raise BackendError(f"the loaded library does not export {name} (a host library has no fused module kernels)")
    return fn


def _params(scale: torch.Tensor, offset: torch.Tensor | None, count: int, what: str) -> tuple[torch.Tensor, torch.Tensor | None, bool]:
    """fp32 (scale, offset) flattened; per-row when there are `count` pairs (count > 1), per-tensor when there is one."""
    s = scale.detach().reshape(-1).to(torch.float32).contiguous()
    o = None if offset is None else offset.detach().reshape(-1).to(torch.float32).contiguous()
    if s.numel() not in (1, count) or (o is not None and o.numel() != s.numel()):
        raise RuntimeError(f"{what}: parameters are one pair for the tensor or one per row ({count} rows), got {s.numel()}")
    return s, o, s.numel() != 1


def _operand(x: torch.Tensor, dtype: torch.dtype, rows: int, dequant: tuple[torch.Tensor, torch.Tensor | None] | None, what: str):
    """(contiguous, 16-byte aligned data, scale, offset, per_row) of a plain or quantized operand."""
    xc = _dense(x.detach())
    if dequant is None:
        if xc.dtype != dtype:
            raise RuntimeError(f"{what}: a plain input must have the value dtype {dtype}, got {xc.dtype}")
        return xc, None, None, False
    if xc.dtype not in (torch.int8, dtype):
        raise RuntimeError(f"{what}: codes are int8 or {dtype}, got {xc.dtype}")
    s, o, per_row = _params(dequant[0], dequant[1], rows, what)
    return xc, s, o, per_row


def layer_norm_quantize(
    x: torch.Tensor,
    normalized_numel: int,
    weight: torch.Tensor | None,
    bias: torch.Tensor | None,
    eps: float,
    quantizers: Quantizers = (),
    num_bits: float = 8.0,
    dtype: torch.dtype | None = None,
    dequant: tuple[torch.Tensor, torch.Tensor | None] | None = None,
    want_value: bool = True,
) -> tuple[torch.Tensor | None, list[torch.Tensor]]:
    """``F.layer_norm`` over the last `normalized_numel` elements + A1, one pass. `x` is the plain input (bf16 / fp16) or, with
    ``dequant=(scale, offset)``, its codes (int8 or `dtype`) with per-tensor or per-row (per-token) parameters."""
    dtype = dtype or x.dtype
    cols = int(normalized_numel)
    rows = x.numel() // cols if cols else 0
    xc, s, o, per_row = _operand(x, dtype, rows, dequant, "layer_norm_quantize")
    wc = None if weight is None else _dense(weight.detach())
    bc = None if bias is None else _dense(bias.detach())
    for name, t in (("weight", wc), ("bias", bc)):
        if t is not None and (t.numel() != cols or t.dtype != dtype):
            raise RuntimeError(f"layer_norm_quantize: {name} must hold {cols} elements of {dtype}")
    lib, stream = _base._prepare(xc, s, o, wc, bc, *[t for q in quantizers for t in q])
    value = torch.empty(xc.shape, dtype=dtype, device=xc.device) if want_value else None
    fan, codes, keep = _fan(quantizers, num_bits, xc.shape, xc.device)
    lib.check(
        _entry(lib, "ffq_layer_norm_quantize")(
            _ptr(xc), _tag(xc.dtype), _ptr(s), _ptr(o), int(per_row), _ptr(wc), _ptr(bc), _tag(dtype), rows, cols, float(eps),
            _ptr(value), ctypes.byref(fan), stream,
        )
    )
    del keep
    return value, codes


def embedding_quantize(
    ids: torch.Tensor,
    table: torch.Tensor,
    scale: torch.Tensor,
    offset: torch.Tensor | None,
    per_row: bool,
    group: int,
    dtype: torch.dtype,
    quantizers: Quantizers = (),
    num_bits: float = 8.0,
    want_value: bool = True,
) -> tuple[torch.Tensor | None, list[torch.Tensor], torch.Tensor]:
    """Gather rows of a quantized [V, D] table, A2 in registers, A1: ``F.embedding(ids, A2(table))`` + the output quantizers,
    one pass. Parameters on the grid ``[per_row ? V : 1, D / group]`` (per tensor: (False, D); PerChannel(0): (True, D);
    PerBlock (1, G): (True, G); PerChannel(1): (False, 1)). Returns ``(value [*ids.shape, D] or None, codes, bad)``: `bad` is a
    one-element int32 device tensor holding the first position of an id outside [0, V), or 2^31 - 1 if there is none (ids out
    of range give rows of zeros; reading `bad` is the caller's choice, and synchronises)."""
    if ids.dtype not in (torch.int64, torch.int32):
        raise RuntimeError(f"embedding_quantize: ids must be int64 or int32, got {ids.dtype}")
    if table.dim() != 2:
        raise RuntimeError("embedding_quantize: the table is [V, D]")
    ic, tc = ids.detach().contiguous(), _dense(table.detach())
    V, D = tc.shape
    s = scale.detach().reshape(-1).to(torch.float32).contiguous()
    o = None if offset is None else offset.detach().reshape(-1).to(torch.float32).contiguous()
    want = (V if per_row else 1) * (D // group if group and D % group == 0 else 0)
    if s.numel() != want or (o is not None and o.numel() != want):
        raise RuntimeError(f"embedding_quantize: {want} parameter pairs expected, got {s.numel()}")
    lib, stream = _base._prepare(ic, tc, s, o, *[t for q in quantizers for t in q])
    shape = (*ic.shape, D)
    value = torch.empty(shape, dtype=dtype, device=tc.device) if want_value else None
    bad = torch.full((1,), 2**31 - 1, dtype=torch.int32, device=tc.device)
    fan, codes, keep = _fan(quantizers, num_bits, shape, tc.device)
    lib.check(
        _entry(lib, "ffq_embedding_quantize")(
            _ptr(ic), _tag(ic.dtype), ic.numel(), _ptr(tc), _tag(tc.dtype), V, D, _ptr(s), _ptr(o), int(bool(per_row)), int(group),
            _tag(dtype), _ptr(value), ctypes.byref(fan), _ptr(bad), stream,
        )
    )
    del keep
    return value, codes, bad


def pointwise_quantize(
    op: str,
    x: torch.Tensor,
    quantizers: Quantizers = (),
    num_bits: float = 8.0,
    dtype: torch.dtype | None = None,
    dequant: tuple[torch.Tensor, torch.Tensor | None] | None = None,
    want_value: bool = True,
) -> tuple[torch.Tensor | None, list[torch.Tensor]]:
    """``F.relu`` (op="relu") or ``F.silu`` (op="silu") + A1, one pass; `x` plain or codes as in :func:`layer_norm_quantize`
    (per-row parameters: one pair per row of the last dimension)."""
    if op not in POINTWISE_OPS:
        raise RuntimeError(f"pointwise_quantize: op is one of {sorted(POINTWISE_OPS)}, got {op!r}")
    dtype = dtype or x.dtype
    run = x.shape[-1] if x.dim() else 1
    rows = x.numel() // run if run else 0
    xc, s, o, per_row = _operand(x, dtype, rows, dequant, "pointwise_quantize")
    lib, stream = _base._prepare(xc, s, o, *[t for q in quantizers for t in q])
    value = torch.empty(xc.shape, dtype=dtype, device=xc.device) if want_value else None
    fan, codes, keep = _fan(quantizers, num_bits, xc.shape, xc.device)
    lib.check(
        _entry(lib, "ffq_pointwise_quantize")(
            POINTWISE_OPS[op], _ptr(xc), _tag(xc.dtype), _ptr(s), _ptr(o), run if per_row else 0, _tag(dtype), xc.numel(),
            _ptr(value), ctypes.byref(fan), stream,
        )
    )
    del keep
    return value, codes
