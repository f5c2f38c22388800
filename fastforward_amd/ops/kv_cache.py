"""A preallocated int8 KV cache on the kernels of csrc/ffq_kv_cache.hip and csrc/ffq_sdpa_decode.hip (include/ffq_kv_cache.h).

``kv_append`` is one launch: the new K / V rows quantized (A1, per-tensor static quantizers) and written into the two cache buffers at
every sequence's own position, K optionally rotated on the way. ``kv_decode`` is ``sdpa_decode`` with the key count of every
sequence read on the device: the split count stays a host integer (so the call is the same under graph capture whatever the lengths
become), each batch cuts its own keys over it, and ``causal`` is bottom-right. `lens` (int32 ``[B]``) is read by both and written by
neither: the caller advances it with ``lens.add_(L)`` on the stream ahead of ``kv_append``.

``kv_paged_append`` / ``kv_paged_decode`` (include/ffq_kv_paged.h) are the same two calls over K / V held in fixed-size pages: two
pools ``[num_pages, H, P, E]`` shared by every sequence and an int32 block table ``[B, max_pages]`` on the device, read by the kernels
and never on the host. The codes and the attention's bits are those of the dense calls.

``kv_token_append`` / ``kv_token_decode`` (include/ffq_kv_token.h) are the dense calls with one DYNAMIC ``(scale, offset)`` per
(sequence, kv head, position) for K and for V, kept in an fp32 store ``[B, H, S_max, 4]`` beside the codes: the append computes them on
the device from every new row's own min / max (the codes and parameters of ``quantize_dynamic_by_tile`` with the tile ``(1, 1, 1, E)``),
the decode reads them back per key row.

``kv_paged_token_append`` / ``kv_paged_token_decode`` (include/ffq_kv_paged_token.h) are both at once: the codes in pages behind a block
table and the per-position parameters in a third pool ``[num_pages, H, P, 4]`` of the same pages, so a shared page shares them."""

from __future__ import annotations

import ctypes

from typing import Sequence

import torch

from fastforward_amd.ops import _base
from fastforward_amd.ops._base import _ptr, _tag
from fastforward_amd.ops.decode import Dequant, _check_decode, _rows_ok, _run_decode
from fastforward_amd.ops.modules import _entry
from fastforward_amd.ops.sdpa import _scalar, _strides

Quantizer = tuple[torch.Tensor, "torch.Tensor | None", float]
Spec = tuple[float, bool]  # (num_bits, symmetric) of a dynamic per-row quantizer


def _lens_ok(lens: torch.Tensor, B: int) -> bool:
    return lens.dtype == torch.int32 and tuple(lens.shape) == (B,) and lens.is_contiguous()


def _quantizer_args(name: str, k_quantizer: Quantizer, v_quantizer: Quantizer) -> tuple[list, list[torch.Tensor]]:
    """[k scale, k offset, k bits, v scale, v offset, v bits] as the append entry points take them, and the tensors to keep alive."""
    keep: list[torch.Tensor] = []
    params: list = []
    for quantizer, what in ((k_quantizer, "key"), (v_quantizer, "value")):
        s, o = _scalar(quantizer[0], f"{what} scale"), _scalar(quantizer[1], f"{what} offset")
        bits = float(quantizer[2])
        if s is None or not (2 <= bits <= 8 and bits == int(bits)):
            raise RuntimeError(f"{name}: the {what} quantizer needs a scale and an integral bit-width in 2..8, got {bits}")
        keep += [t for t in (s, o) if t is not None]
        params += [_ptr(s), _ptr(o), bits]
    return params, keep


def _spec_args(name: str, k_spec: Spec, v_spec: Spec) -> list:
    """[k bits, k symmetric, v bits, v symmetric] as ``ffq_kv_token_append`` takes them."""
    args: list = []
    for spec, what in ((k_spec, "key"), (v_spec, "value")):
        bits = float(spec[0])
        if not (2 <= bits <= 8 and bits == int(bits)):
            raise RuntimeError(f"{name}: the {what} quantizer needs an integral bit-width in 2..8, got {bits}")
        args += [bits, int(bool(spec[1]))]
    return args


def _params_ok(params: torch.Tensor, B: int, HKV: int, S_max: int) -> bool:
    return (params.dtype == torch.float32 and tuple(params.shape) == (B, HKV, S_max, 4) and params.stride(3) == 1
            and not any(st % 4 for st in _strides(params)) and params.data_ptr() % 16 == 0)


def _rope_tables(name: str, rope: tuple[torch.Tensor, torch.Tensor] | None, dt: torch.dtype, rows: int, E: int):
    """(cos, sin) checked: contiguous [P >= rows, E] tables in the data dtype, both the same shape; (None, None) without rotation."""
    if rope is None:
        return None, None
    cos, sin = rope
    for t in (cos, sin):
        if t.dtype != dt or t.dim() != 2 or t.shape[1] != E or t.shape[0] < rows or tuple(t.shape) != tuple(cos.shape) or not t.is_contiguous() or t.data_ptr() % 16:
            raise RuntimeError(f"{name}: the rotary tables are contiguous [P >= {rows}, {E}] in {dt}, got {tuple(t.shape)} {t.dtype}")
    return cos, sin


def _pools_ok(name: str, k_pool: torch.Tensor, v_pool: torch.Tensor, block_table: torch.Tensor, B: int, HKV: int, E: int) -> tuple[int, int, int]:
    """(num_pages, P, max_pages) of pools [num_pages, HKV, P, E] (int8, any page / head / row strides) and a block table int32
    [B, max_pages] whose rows are contiguous, else RuntimeError."""
    if k_pool.dim() != 4 or v_pool.dim() != 4 or k_pool.dtype != torch.int8 or v_pool.dtype != torch.int8:
        raise RuntimeError(f"{name}: the pools are 4-D [num_pages, H, P, E] int8 codes, got {tuple(k_pool.shape)} {k_pool.dtype}, {tuple(v_pool.shape)} {v_pool.dtype}")
    num_pages, _, P, _ = k_pool.shape
    if tuple(k_pool.shape) != (num_pages, HKV, P, E) or tuple(v_pool.shape) != (num_pages, HKV, P, E) or num_pages < 1:
        raise RuntimeError(f"{name}: pools {tuple(k_pool.shape)}, {tuple(v_pool.shape)} do not fit {HKV} kv heads of {E} columns")
    if not 16 <= P <= 256 or P & (P - 1):
        raise RuntimeError(f"{name}: the page size is a power of two in 16..256, got {P}")
    if block_table.dtype != torch.int32 or block_table.dim() != 2 or block_table.shape[0] != B or block_table.shape[1] < 1 or block_table.stride(1) != 1:
        raise RuntimeError(f"{name}: the block table is int32 [{B}, max_pages] with contiguous rows, got {block_table.dtype} {tuple(block_table.shape)}")
    max_pages = block_table.shape[1]
    if B > 1 and block_table.stride(0) < max_pages:
        raise RuntimeError(f"{name}: the block table's rows overlap (stride {block_table.stride(0)} < {max_pages})")
    if max_pages * P >= 1 << 30:
        raise RuntimeError(f"{name}: a sequence's capacity {max_pages} x {P} must stay below 2^30")
    return num_pages, P, max_pages


def _check_new_rows(name: str, k_new: torch.Tensor, v_new: torch.Tensor, k_store: torch.Tensor, v_store: torch.Tensor, lens: torch.Tensor) -> None:
    """What ``kv_append`` and ``kv_paged_append`` ask alike of 4-D new rows that fit their caches or pools (`k_store`, `v_store`): the
    dtype, E, a kv head, `lens`, and the rows of all four tensors in memory; else RuntimeError under the wrapper's `name`."""
    B, HKV, _, E = k_new.shape
    if k_new.dtype not in (torch.bfloat16, torch.float16) or v_new.dtype != k_new.dtype:
        raise RuntimeError(f"{name}: the new rows are bf16 or fp16, both the same, got {k_new.dtype} and {v_new.dtype}")
    if E not in (64, 128):
        raise RuntimeError(f"{name}: E must be 64 or 128, got {E}")
    if HKV < 1:
        raise RuntimeError(f"{name}: no kv head")
    if not _lens_ok(lens, B):
        raise RuntimeError(f"{name}: lens is a contiguous int32 [{B}], got {lens.dtype} {tuple(lens.shape)}")
    for t in (k_new, v_new, k_store, v_store):
        if not _rows_ok(t):
            raise RuntimeError(f"{name}: the last dimension must be contiguous with 16-byte aligned rows")


def _run_append(name: str, k_new: torch.Tensor, v_new: torch.Tensor, k_store: torch.Tensor, v_store: torch.Tensor, tables: Sequence[torch.Tensor],
                capacity: int, k_quantizer: Quantizer | Spec, v_quantizer: Quantizer | Spec, rope: tuple[torch.Tensor, torch.Tensor] | None,
                extents: tuple, row_params: torch.Tensor | None = None) -> None:
    """The tail of the append wrappers, after their checks: the rotary tables (`capacity` rows), the quantizers, the library and the
    call of ``ffq_<name>``. `tables` are the entry point's tensors between the stores and the extents (lens; lens and the block table;
    the parameter store and lens), `extents` its arguments between them and the strides. `row_params` (``kv_token_append``): the
    parameter store, whose strides end the table; the quantizers are then ``(num_bits, symmetric)`` specs."""
    dt, E = k_new.dtype, k_new.shape[3]
    cos, sin = _rope_tables(name, rope, dt, capacity, E)
    if row_params is None:
        params, keep = _quantizer_args(name, k_quantizer, v_quantizer)
    else:
        params, keep = _spec_args(name, k_quantizer, v_quantizer), []
    lib, stream = _base._prepare(k_new, v_new, k_store, v_store, *tables, cos, sin, *keep)
    entry = _entry(lib, f"ffq_{name}")
    strides = (ctypes.c_int64 * 12)(*_strides(k_new), *_strides(v_new), *_strides(k_store), *_strides(v_store))
    if row_params is not None:
        strides = (ctypes.c_int64 * 15)(*strides, *_strides(row_params))
    lib.check(
        entry(
            _ptr(k_new), _ptr(v_new), _tag(dt), _ptr(k_store), _ptr(v_store), *(_ptr(t) for t in tables), *extents, strides, *params, _ptr(cos),
            _ptr(sin), 0 if cos is None else cos.shape[0], stream,
        )
    )
    del keep
    # written through raw pointers: tell the version counters
    torch.autograd.graph.increment_version(k_store)
    torch.autograd.graph.increment_version(v_store)
    if row_params is not None:
        torch.autograd.graph.increment_version(row_params)


def kv_append(
    k_new: torch.Tensor,
    v_new: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    lens: torch.Tensor,
    k_quantizer: Quantizer,
    v_quantizer: Quantizer,
    rope: tuple[torch.Tensor, torch.Tensor] | None = None,
) -> None:
    """One call of ``ffq_kv_append``. k_new / v_new [B, H, L, E] plain bf16 / fp16; k_cache / v_cache int8 [B, H, S_max, E]; E in
    {64, 128}; the last dimension contiguous and rows 16-byte aligned, any other strides. `lens` int32 [B] holds every sequence's length
    INCLUDING these L rows: row l goes to position ``lens[b] - L + l``, and a row outside ``[0, S_max)`` is skipped. The quantizers are
    ``(scale, offset, num_bits)``, per-tensor, 2..8 bits. ``rope=(cos, sin)``, [P, E] tables in the data dtype with ``P >= S_max``: K is
    rotated with the row of its position before it is quantized."""
    if k_new.dim() != 4 or v_new.dim() != 4 or k_cache.dim() != 4 or v_cache.dim() != 4:
        raise RuntimeError("kv_append: the new rows and the caches are 4-D [B, H, L|S_max, E]")
    if k_cache.dtype != torch.int8 or v_cache.dtype != torch.int8:
        raise RuntimeError(f"kv_append: the caches hold int8 codes, got {k_cache.dtype}, {v_cache.dtype}")
    (B, HKV, L, E), S_max = k_new.shape, k_cache.shape[2]
    if tuple(v_new.shape) != (B, HKV, L, E) or tuple(k_cache.shape) != (B, HKV, S_max, E) or tuple(v_cache.shape) != (B, HKV, S_max, E):
        raise RuntimeError(f"kv_append: shapes {tuple(k_new.shape)}, {tuple(v_new.shape)}, {tuple(k_cache.shape)}, {tuple(v_cache.shape)} do not fit")
    _check_new_rows("kv_append", k_new, v_new, k_cache, v_cache, lens)
    _run_append("kv_append", k_new, v_new, k_cache, v_cache, (lens,), S_max, k_quantizer, v_quantizer, rope, (B, HKV, L, S_max, E))


def kv_decode(
    query: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    lens: torch.Tensor,
    is_causal: bool = False,
    scale: float | None = None,
    output_quantizer: tuple[torch.Tensor, torch.Tensor | None, float] | None = None,
    dequant: Sequence[Dequant | None] = (None, None, None),
    dtype: torch.dtype | None = None,
    splits: int = 0,
    plan_len: int | None = None,
) -> torch.Tensor:
    """One call of ``ffq_kv_decode``: :func:`~fastforward_amd.ops.decode.sdpa_decode` over caches [B, H, S_max, E] of which sequence b
    holds ``clamp(lens[b], 0, S_max)`` keys (`lens` int32 [B], read on the device). ``is_causal`` is BOTTOM-RIGHT: row l sees
    ``key <= l + (S_b - L)``; a row without a visible key, and every row of a sequence without keys, is exact zeros. ``splits=0`` takes
    ``sdpa_decode_plan(B, H, plan_len, rows, E)`` with ``plan_len`` (a host hint in ``1..S_max``) defaulting to ``S_max``;
    ``1 .. MAX_SPLITS`` forces a count. Each batch cuts its own keys over that count (``sdpa_decode_split_ranges(S_b, splits)``)."""
    if query.dim() != 4 or k_cache.dim() != 4 or v_cache.dim() != 4:
        raise RuntimeError("kv_decode: q / k / v are 4-D [B, H, L|S_max, E]")
    if k_cache.dtype != torch.int8 or v_cache.dtype != torch.int8 or dequant[1] is None or dequant[2] is None:
        raise RuntimeError(f"kv_decode: k / v are int8 codes with their (scale, offset), got {k_cache.dtype}, {v_cache.dtype}")
    S_max = k_cache.shape[2]
    dt, B, H, L, E, HKV, rows = _check_decode("kv_decode", query, k_cache, v_cache, dequant, dtype, k_cache.shape[1], splits)
    if k_cache.shape[0] != B or k_cache.shape[3] != E or tuple(v_cache.shape) != (B, HKV, S_max, E):
        raise RuntimeError(f"kv_decode: shapes {tuple(query.shape)}, {tuple(k_cache.shape)}, {tuple(v_cache.shape)} do not fit")
    if min(B, L, S_max) < 1:
        raise RuntimeError(f"kv_decode: empty operands {tuple(query.shape)}, {tuple(k_cache.shape)}")
    if not _lens_ok(lens, B):
        raise RuntimeError(f"kv_decode: lens is a contiguous int32 [{B}], got {lens.dtype} {tuple(lens.shape)}")
    if plan_len is not None and not 1 <= plan_len <= S_max:
        raise RuntimeError(f"kv_decode: plan_len is a key count in 1..{S_max}, got {plan_len}")
    return _run_decode("ffq_kv_decode", query, k_cache, v_cache, (lens,), dt, (B, H, HKV, L, E, rows), plan_len or S_max, splits, scale, dequant,
                       output_quantizer, (_ptr(lens), B, H, HKV, L, S_max, E), (int(bool(is_causal)),), (splits, plan_len or 0))


def kv_paged_append(
    k_new: torch.Tensor,
    v_new: torch.Tensor,
    k_pool: torch.Tensor,
    v_pool: torch.Tensor,
    lens: torch.Tensor,
    block_table: torch.Tensor,
    k_quantizer: Quantizer,
    v_quantizer: Quantizer,
    rope: tuple[torch.Tensor, torch.Tensor] | None = None,
) -> None:
    """One call of ``ffq_kv_paged_append``: :func:`kv_append` into pages. k_pool / v_pool int8 [num_pages, H, P, E] (any page / head /
    row strides: ``[num_pages, P, H, E].transpose(1, 2)`` is served), P a power of two in 16..256; `block_table` int32 [B, max_pages].
    Sequence b holds up to ``C = max_pages * P`` positions and position ``pos`` lives in page ``block_table[b, pos // P]`` at row
    ``pos % P``. Row l goes to ``lens[b] - L + l``; a row outside ``[0, C)``, or whose table entry lies outside ``[0, num_pages)``, is
    skipped. The codes are :func:`kv_append`'s; the rotary tables need ``C`` rows. Nothing is read on the host."""
    name = "kv_paged_append"
    if k_new.dim() != 4 or v_new.dim() != 4:
        raise RuntimeError(f"{name}: the new rows are 4-D [B, H, L, E]")
    B, HKV, L, E = k_new.shape
    if tuple(v_new.shape) != (B, HKV, L, E):
        raise RuntimeError(f"{name}: shapes {tuple(k_new.shape)}, {tuple(v_new.shape)} do not fit")
    num_pages, P, max_pages = _pools_ok(name, k_pool, v_pool, block_table, B, HKV, E)
    _check_new_rows(name, k_new, v_new, k_pool, v_pool, lens)
    table_stride = block_table.stride(0) if B > 1 else max_pages
    _run_append(name, k_new, v_new, k_pool, v_pool, (lens, block_table), max_pages * P, k_quantizer, v_quantizer, rope,
                (B, HKV, L, num_pages, P, max_pages, table_stride, E))


def kv_paged_decode(
    query: torch.Tensor,
    k_pool: torch.Tensor,
    v_pool: torch.Tensor,
    lens: torch.Tensor,
    block_table: torch.Tensor,
    is_causal: bool = False,
    scale: float | None = None,
    output_quantizer: tuple[torch.Tensor, torch.Tensor | None, float] | None = None,
    dequant: Sequence[Dequant | None] = (None, None, None),
    dtype: torch.dtype | None = None,
    splits: int = 0,
    plan_len: int | None = None,
) -> torch.Tensor:
    """One call of ``ffq_kv_paged_decode``: :func:`kv_decode` over pools [num_pages, H, P, E] addressed through `block_table` int32
    [B, max_pages] (:func:`kv_paged_append`), with the capacity ``C = max_pages * P`` in the place of ``S_max``: sequence b holds
    ``clamp(lens[b], 0, C)`` keys, ``plan_len`` is a hint in ``1..C``. The keys of a table entry outside ``[0, num_pages)`` are masked.
    The result is bit-equal to :func:`kv_decode` on the same codes laid out densely at the same split count."""
    name = "kv_paged_decode"
    if query.dim() != 4:
        raise RuntimeError(f"{name}: q is 4-D [B, H, L, E]")
    if dequant[1] is None or dequant[2] is None:
        raise RuntimeError(f"{name}: k / v are int8 codes with their (scale, offset)")
    dt, B, H, L, E, HKV, rows = _check_decode(name, query, k_pool, v_pool, dequant, dtype, k_pool.shape[1] if k_pool.dim() == 4 else 0, splits)
    if min(B, L) < 1:
        raise RuntimeError(f"{name}: empty operands {tuple(query.shape)}")
    num_pages, P, max_pages = _pools_ok(name, k_pool, v_pool, block_table, B, HKV, E)
    C = max_pages * P
    if not _lens_ok(lens, B):
        raise RuntimeError(f"{name}: lens is a contiguous int32 [{B}], got {lens.dtype} {tuple(lens.shape)}")
    if plan_len is not None and not 1 <= plan_len <= C:
        raise RuntimeError(f"{name}: plan_len is a key count in 1..{C}, got {plan_len}")
    table_stride = block_table.stride(0) if B > 1 else max_pages
    return _run_decode("ffq_kv_paged_decode", query, k_pool, v_pool, (lens, block_table), dt, (B, H, HKV, L, E, rows), plan_len or C, splits, scale,
                       dequant, output_quantizer, (_ptr(lens), _ptr(block_table), B, H, HKV, L, num_pages, P, max_pages, table_stride, E),
                       (int(bool(is_causal)),), (splits, plan_len or 0))


def kv_token_append(
    k_new: torch.Tensor,
    v_new: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    params: torch.Tensor,
    lens: torch.Tensor,
    k_spec: Spec,
    v_spec: Spec,
    rope: tuple[torch.Tensor, torch.Tensor] | None = None,
) -> None:
    """One call of ``ffq_kv_token_append``: :func:`kv_append` with a dynamic quantizer per row. The operands are :func:`kv_append`'s;
    `params` is fp32 ``[B, H, S_max, 4]`` (the last dimension contiguous, positions 16-byte aligned, any other strides) and receives
    ``(k_scale, k_offset, v_scale, v_offset)`` of every row written; ``k_spec`` / ``v_spec`` are ``(num_bits, symmetric)``, 2..8 bits.
    The codes and the parameters of a row are those of ``quantize_dynamic_by_tile(row, (1, 1, 1, E), num_bits, symmetric, False,
    torch.int8)``, K rotated first with ``rope``. A row outside ``[0, S_max)`` is skipped and its parameters stay as they were."""
    name = "kv_token_append"
    if k_new.dim() != 4 or v_new.dim() != 4 or k_cache.dim() != 4 or v_cache.dim() != 4:
        raise RuntimeError(f"{name}: the new rows and the caches are 4-D [B, H, L|S_max, E]")
    if k_cache.dtype != torch.int8 or v_cache.dtype != torch.int8:
        raise RuntimeError(f"{name}: the caches hold int8 codes, got {k_cache.dtype}, {v_cache.dtype}")
    (B, HKV, L, E), S_max = k_new.shape, k_cache.shape[2]
    if tuple(v_new.shape) != (B, HKV, L, E) or tuple(k_cache.shape) != (B, HKV, S_max, E) or tuple(v_cache.shape) != (B, HKV, S_max, E):
        raise RuntimeError(f"{name}: shapes {tuple(k_new.shape)}, {tuple(v_new.shape)}, {tuple(k_cache.shape)}, {tuple(v_cache.shape)} do not fit")
    if not _params_ok(params, B, HKV, S_max):
        raise RuntimeError(f"{name}: params is fp32 [{B}, {HKV}, {S_max}, 4] with 16-byte aligned positions, got {params.dtype} {tuple(params.shape)}")
    _check_new_rows(name, k_new, v_new, k_cache, v_cache, lens)
    _run_append(name, k_new, v_new, k_cache, v_cache, (params, lens), S_max, k_spec, v_spec, rope, (B, HKV, L, S_max, E), row_params=params)


def kv_token_decode(
    query: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    params: torch.Tensor,
    lens: torch.Tensor,
    is_causal: bool = False,
    scale: float | None = None,
    output_quantizer: tuple[torch.Tensor, torch.Tensor | None, float] | None = None,
    q_dequant: Dequant | None = None,
    dtype: torch.dtype | None = None,
    splits: int = 0,
    plan_len: int | None = None,
) -> torch.Tensor:
    """One call of ``ffq_kv_token_decode``: :func:`kv_decode` over codes whose ``(scale, offset)`` live per position in `params` (fp32
    ``[B, H, S_max, 4]``, as :func:`kv_token_append` writes them). ``q_dequant`` is the query's own ``(scale, offset)`` when it holds
    codes. Lengths, causality, ``splits`` / ``plan_len``, the output quantizer and the exact zeros are :func:`kv_decode`'s; with every
    position's parameters equal the result is bit-equal to it."""
    name = "kv_token_decode"
    if query.dim() != 4 or k_cache.dim() != 4 or v_cache.dim() != 4:
        raise RuntimeError(f"{name}: q / k / v are 4-D [B, H, L|S_max, E]")
    if k_cache.dtype != torch.int8 or v_cache.dtype != torch.int8:
        raise RuntimeError(f"{name}: k / v are int8 codes, got {k_cache.dtype}, {v_cache.dtype}")
    S_max = k_cache.shape[2]
    dequant = (q_dequant, None, None)
    dt, B, H, L, E, HKV, rows = _check_decode(name, query, k_cache, v_cache, dequant, dtype, k_cache.shape[1], splits)
    if k_cache.shape[0] != B or k_cache.shape[3] != E or tuple(v_cache.shape) != (B, HKV, S_max, E):
        raise RuntimeError(f"{name}: shapes {tuple(query.shape)}, {tuple(k_cache.shape)}, {tuple(v_cache.shape)} do not fit")
    if min(B, L, S_max) < 1:
        raise RuntimeError(f"{name}: empty operands {tuple(query.shape)}, {tuple(k_cache.shape)}")
    if not _params_ok(params, B, HKV, S_max):
        raise RuntimeError(f"{name}: params is fp32 [{B}, {HKV}, {S_max}, 4] with 16-byte aligned positions, got {params.dtype} {tuple(params.shape)}")
    if not _lens_ok(lens, B):
        raise RuntimeError(f"{name}: lens is a contiguous int32 [{B}], got {lens.dtype} {tuple(lens.shape)}")
    if plan_len is not None and not 1 <= plan_len <= S_max:
        raise RuntimeError(f"{name}: plan_len is a key count in 1..{S_max}, got {plan_len}")
    return _run_decode("ffq_kv_token_decode", query, k_cache, v_cache, (params, lens), dt, (B, H, HKV, L, E, rows), plan_len or S_max, splits, scale,
                       dequant, output_quantizer, (_ptr(params), _ptr(lens), B, H, HKV, L, S_max, E), (int(bool(is_causal)),), (splits, plan_len or 0),
                       row_params=params)


def kv_paged_token_append(
    k_new: torch.Tensor,
    v_new: torch.Tensor,
    k_pool: torch.Tensor,
    v_pool: torch.Tensor,
    param_pool: torch.Tensor,
    lens: torch.Tensor,
    block_table: torch.Tensor,
    k_spec: Spec,
    v_spec: Spec,
    rope: tuple[torch.Tensor, torch.Tensor] | None = None,
) -> None:
    """One call of ``ffq_kv_paged_token_append``: :func:`kv_token_append` into pages. The pools and the table are
    :func:`kv_paged_append`'s; `param_pool` is fp32 ``[num_pages, H, P, 4]`` (the last dimension contiguous, rows 16-byte aligned, any
    other strides) and receives ``(k_scale, k_offset, v_scale, v_offset)`` of every row written, at row ``pos % P`` of page
    ``block_table[b, pos // P]`` like the codes. Codes and parameters of a row are :func:`kv_token_append`'s. A row outside ``[0, C)``,
    or whose table entry lies outside ``[0, num_pages)``, is skipped, its parameters included. Nothing is read on the host."""
    name = "kv_paged_token_append"
    if k_new.dim() != 4 or v_new.dim() != 4:
        raise RuntimeError(f"{name}: the new rows are 4-D [B, H, L, E]")
    B, HKV, L, E = k_new.shape
    if tuple(v_new.shape) != (B, HKV, L, E):
        raise RuntimeError(f"{name}: shapes {tuple(k_new.shape)}, {tuple(v_new.shape)} do not fit")
    num_pages, P, max_pages = _pools_ok(name, k_pool, v_pool, block_table, B, HKV, E)
    if not _params_ok(param_pool, num_pages, HKV, P):
        raise RuntimeError(f"{name}: param_pool is fp32 [{num_pages}, {HKV}, {P}, 4] with 16-byte aligned rows, got {param_pool.dtype} {tuple(param_pool.shape)}")
    _check_new_rows(name, k_new, v_new, k_pool, v_pool, lens)
    table_stride = block_table.stride(0) if B > 1 else max_pages
    _run_append(name, k_new, v_new, k_pool, v_pool, (param_pool, lens, block_table), max_pages * P, k_spec, v_spec, rope,
                (B, HKV, L, num_pages, P, max_pages, table_stride, E), row_params=param_pool)


def kv_paged_token_decode(
    query: torch.Tensor,
    k_pool: torch.Tensor,
    v_pool: torch.Tensor,
    param_pool: torch.Tensor,
    lens: torch.Tensor,
    block_table: torch.Tensor,
    is_causal: bool = False,
    scale: float | None = None,
    output_quantizer: tuple[torch.Tensor, torch.Tensor | None, float] | None = None,
    q_dequant: Dequant | None = None,
    dtype: torch.dtype | None = None,
    splits: int = 0,
    plan_len: int | None = None,
) -> torch.Tensor:
    """One call of ``ffq_kv_paged_token_decode``: :func:`kv_token_decode` over pools ``[num_pages, H, P, E]`` and the parameter pool
    ``[num_pages, H, P, 4]`` addressed through `block_table` (:func:`kv_paged_token_append`), with the capacity ``C = max_pages * P`` in
    the place of ``S_max``. The keys of a table entry outside ``[0, num_pages)`` are masked and their parameters never read. The result
    is bit-equal to :func:`kv_token_decode` on the same codes and parameters laid out densely at the same split count."""
    name = "kv_paged_token_decode"
    if query.dim() != 4:
        raise RuntimeError(f"{name}: q is 4-D [B, H, L, E]")
    dequant = (q_dequant, None, None)
    dt, B, H, L, E, HKV, rows = _check_decode(name, query, k_pool, v_pool, dequant, dtype, k_pool.shape[1] if k_pool.dim() == 4 else 0, splits)
    if min(B, L) < 1:
        raise RuntimeError(f"{name}: empty operands {tuple(query.shape)}")
    num_pages, P, max_pages = _pools_ok(name, k_pool, v_pool, block_table, B, HKV, E)
    C = max_pages * P
    if not _params_ok(param_pool, num_pages, HKV, P):
        raise RuntimeError(f"{name}: param_pool is fp32 [{num_pages}, {HKV}, {P}, 4] with 16-byte aligned rows, got {param_pool.dtype} {tuple(param_pool.shape)}")
    if not _lens_ok(lens, B):
        raise RuntimeError(f"{name}: lens is a contiguous int32 [{B}], got {lens.dtype} {tuple(lens.shape)}")
    if plan_len is not None and not 1 <= plan_len <= C:
        raise RuntimeError(f"{name}: plan_len is a key count in 1..{C}, got {plan_len}")
    table_stride = block_table.stride(0) if B > 1 else max_pages
    return _run_decode("ffq_kv_paged_token_decode", query, k_pool, v_pool, (param_pool, lens, block_table), dt, (B, H, HKV, L, E, rows), plan_len or C,
                       splits, scale, dequant, output_quantizer,
                       (_ptr(param_pool), _ptr(lens), _ptr(block_table), B, H, HKV, L, num_pages, P, max_pages, table_stride, E),
                       (int(bool(is_causal)),), (splits, plan_len or 0), row_params=param_pool)
