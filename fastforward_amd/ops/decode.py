"""``scaled_dot_product_attention`` for a short query over int8 K / V codes — a quantized KV cache — split over the keys
(csrc/ffq_sdpa_decode.hip, include/ffq_sdpa_decode.h): two plain launches. The partial kernel gives one workgroup to every (batch,
kv head, key split), with the ``rows = L * (H_q / H)`` query rows of that kv head on one MFMA tile, so the codes are read once per
(batch, kv head); the combine kernel merges the splits' fp32 partials, applies the optional output quantizer and rounds once.

k / v are int8 codes with per-tensor ``(scale, offset)`` in ``dequant[1]`` / ``dequant[2]``; q is plain bf16 / fp16 (``dequant[0]``
None) or per-tensor codes of it in that dtype or in int8. Returns the value [B, H_q, L, E] in the data dtype."""

from __future__ import annotations

import ctypes
import math

from typing import Sequence

import torch

from fastforward_amd import _cabi
from fastforward_amd.ops import _base
from fastforward_amd.ops._base import _ptr, _tag
from fastforward_amd.ops.modules import _entry
from fastforward_amd.ops.sdpa import MASK_KINDS, _scalar, _strides

MAX_ROWS = _cabi.SDPA_DECODE_MAX_ROWS
KEY_TILE = _cabi.SDPA_DECODE_KEY_TILE
MAX_SPLITS = _cabi.SDPA_DECODE_MAX_SPLITS
TARGET_GROUPS = 256  # workgroups the rule asks for: one per compute unit (docs/kernels.md has the sweep)
MIN_TILES_PER_SPLIT = 2

Dequant = tuple[torch.Tensor, torch.Tensor | None]


def sdpa_decode_plan(B: int, HKV: int, S: int, rows: int = 1, E: int = 128) -> int:
    """The number of key splits the kernel takes at ``splits=0``: ``ffq_sdpa_decode_splits`` restated (a pure function of the
    shape, so the same under graph capture). Every split takes ``ceil(tiles / splits)`` tiles of ``KEY_TILE`` keys, the last one
    what is left; none is empty."""
    tiles, groups = -(-S // KEY_TILE), B * HKV
    if tiles <= 0 or groups <= 0:
        return 1
    want = max(1, min(-(-TARGET_GROUPS // groups), tiles // MIN_TILES_PER_SPLIT, MAX_SPLITS))
    per = -(-tiles // want)
    return -(-tiles // per)


def sdpa_decode_split_ranges(S: int, splits: int) -> list[tuple[int, int]]:
    """The keys ``[begin, end)`` of each of `splits` splits (a forced split may be empty)."""
    per = -(-(-(-S // KEY_TILE)) // splits) * KEY_TILE
    return [(min(i * per, S), min((i + 1) * per, S)) for i in range(splits)]


def sdpa_decode_workspace_bytes(B: int, HKV: int, rows: int, E: int, splits: int) -> int:
    """``ffq_sdpa_decode_workspace_bytes`` restated: O[rows][E], m[rows] and l[rows] in fp32 for every (batch, kv head, split)."""
    return 0 if min(B, HKV, rows, E, splits) <= 0 else B * HKV * splits * rows * (E + 2) * 4


def _rows_ok(t: torch.Tensor) -> bool:
    return t.stride(-1) == 1 and not any(st * t.element_size() % 16 for st in _strides(t)) and t.data_ptr() % 16 == 0


def _check_decode(name: str, query: torch.Tensor, k: torch.Tensor, v: torch.Tensor, dequant: Sequence[Dequant | None], dtype: torch.dtype | None,
                  HKV: int, splits: int) -> tuple[torch.dtype, int, int, int, int, int, int]:
    """What ``sdpa_decode``, ``kv_decode`` and ``kv_paged_decode`` ask alike of a 4-D query over `HKV` kv heads: the data dtype, int8 q
    codes, E, the GQA group, the rows of one kv head, `splits`, and the rows of q / k / v in memory. ``(dt, B, H, L, E, HKV, rows)``, else
    RuntimeError under the wrapper's `name`."""
    dt = dtype or (query.dtype if query.dtype != torch.int8 else None)
    if dt not in (torch.bfloat16, torch.float16) or query.dtype not in (dt, torch.int8):
        raise RuntimeError(f"{name}: the data dtype is bf16 or fp16 and q is held in it or in int8, got {dt} and {query.dtype}")
    if query.dtype == torch.int8 and dequant[0] is None:
        raise RuntimeError(f"{name}: int8 q codes need their (scale, offset)")
    B, H, L, E = query.shape
    if E not in (64, 128):
        raise RuntimeError(f"{name}: E must be 64 or 128, got {E}")
    if HKV < 1 or H % HKV:
        raise RuntimeError(f"{name}: {H} query heads are not a multiple of {HKV} kv heads")
    rows = L * (H // HKV)
    if rows > MAX_ROWS:
        raise RuntimeError(f"{name}: L * (H_q / H) = {rows} query rows per kv head, at most {MAX_ROWS}")
    if not 0 <= splits <= MAX_SPLITS:
        raise RuntimeError(f"{name}: splits is 0 (the rule) or 1..{MAX_SPLITS}, got {splits}")
    for t in (query, k, v):
        if not _rows_ok(t):
            raise RuntimeError(f"{name}: the last dimension must be contiguous with 16-byte aligned rows")
    return dt, B, H, L, E, HKV, rows


def _decode_tables(dequant: Sequence[Dequant | None], output_quantizer):
    """(deq_scale[3], deq_offset[3], out scale, out offset, out bits, the tensors to keep alive) as the decode entry points take them."""
    keep: list[torch.Tensor] = []
    deq_s, deq_o = (ctypes.c_void_p * 3)(), (ctypes.c_void_p * 3)()
    for i, d in enumerate(dequant):
        if d is not None:
            s, o = _scalar(d[0], "dequant scale"), _scalar(d[1], "dequant offset")
            keep += [t for t in (s, o) if t is not None]
            deq_s[i], deq_o[i] = _ptr(s), _ptr(o)
    out_s = out_o = None
    bits = 8.0
    if output_quantizer is not None:
        out_s, out_o = _scalar(output_quantizer[0], "output scale"), _scalar(output_quantizer[1], "output offset")
        bits = float(output_quantizer[2])
        keep += [t for t in (out_s, out_o) if t is not None]
    return deq_s, deq_o, out_s, out_o, bits, keep


def _split_workspace(B: int, HKV: int, rows: int, E: int, keys: int, splits: int, device: torch.device):
    """(the split count, the workspace's bytes, the workspace) of a decode call that plans over `keys` keys: `splits`, or the rule.
    The count and the size are the restatements above, which tests/test_sdpa_decode_cpu.py holds equal to the library's queries; the
    entry point checks the size again (FFQ_ERR_WORKSPACE)."""
    count = splits or sdpa_decode_plan(B, HKV, keys, rows, E)
    nbytes = sdpa_decode_workspace_bytes(B, HKV, rows, E, count)
    return count, nbytes, torch.empty(nbytes, dtype=torch.uint8, device=device)


def _run_decode(symbol: str, query: torch.Tensor, k: torch.Tensor, v: torch.Tensor, others: Sequence[torch.Tensor | None], dt: torch.dtype,
                shape: tuple[int, ...], plan_keys: int, splits: int, scale: float | None, dequant: Sequence[Dequant | None], output_quantizer,
                extents: tuple, selection: tuple, split_args: tuple | None = None, row_params: torch.Tensor | None = None) -> torch.Tensor:
    """The tail of the three decode wrappers, after their checks: the tables, the library, the split count and the workspace, the
    output, and the call of `symbol`. `others` are the entry point's own tensors (a mask; lens; lens and the block table); `extents`
    and `selection` are its own arguments on either side of the strides; `split_args` is what it takes in the place of the split
    count (``splits`` and ``plan_len`` as given, for the cache forms). `row_params` (``ffq_kv_token_decode``): the per-position
    parameter store; the entry point then takes the query's two pointers in the place of the two tables, and the store's strides at the
    end of a table of fifteen."""
    B, H, HKV, L, E, rows = shape
    deq_s, deq_o, out_s, out_o, bits, keep = _decode_tables(dequant, output_quantizer)
    lib, stream = _base._prepare(query, k, v, *others, *keep)
    entry = _entry(lib, symbol)
    count, nbytes, workspace = _split_workspace(B, HKV, rows, E, plan_keys, splits, query.device)
    out = torch.empty((B, H, L, E), dtype=dt, device=query.device)
    strides = (ctypes.c_int64 * 9)(*_strides(query), *_strides(k), *_strides(v))
    tables: tuple = (deq_s, deq_o)
    if row_params is not None:
        strides = (ctypes.c_int64 * 15)(*strides, 0, 0, 0, *_strides(row_params))
        tables = (deq_s[0], deq_o[0])
    sqrt_scale = math.sqrt(1.0 / math.sqrt(E) if scale is None else scale)  # the math path's scale_factor_sqrt
    lib.check(
        entry(
            _ptr(query), _tag(query.dtype), _ptr(k), _ptr(v), _tag(dt), *tables, *extents, strides, *selection, sqrt_scale, _ptr(out_s),
            _ptr(out_o), bits, *(split_args or (count,)), _ptr(out), _ptr(workspace), nbytes, stream,
        )
    )
    del keep
    return out


def sdpa_decode(
    query: torch.Tensor,
    key: torch.Tensor,
    value: torch.Tensor,
    attn_mask: torch.Tensor | None = None,
    is_causal: bool = False,
    scale: float | None = None,
    output_quantizer: tuple[torch.Tensor, torch.Tensor | None, float] | None = None,
    dequant: Sequence[Dequant | None] = (None, None, None),
    dtype: torch.dtype | None = None,
    splits: int = 0,
) -> torch.Tensor:
    """One call of ``ffq_sdpa_decode``. query [B, H_q, L, E] in `dtype` (bf16 / fp16; plain, or codes with ``dequant[0]``) or int8
    codes; key / value [B, H, S, E] int8 codes with ``dequant[1]`` / ``dequant[2]``; ``L * (H_q / H) <= 32``; E in {64, 128}; the last
    dimension contiguous and rows 16-byte aligned, any other strides. `attn_mask` (bool or float, last two dims [L, S]) broadcasts over
    the leading dims and excludes `is_causal` (top-left). `output_quantizer` is ``(scale, offset, num_bits)``. ``splits=0`` takes the
    rule (:func:`sdpa_decode_plan`); ``1 .. MAX_SPLITS`` forces a count."""
    if query.dim() != 4 or key.dim() != 4 or value.dim() != 4:
        raise RuntimeError("sdpa_decode: q / k / v are 4-D [B, H, L|S, E]")
    if key.dtype != torch.int8 or value.dtype != torch.int8 or dequant[1] is None or dequant[2] is None:
        raise RuntimeError(f"sdpa_decode: k / v are int8 codes with their (scale, offset), got {key.dtype}, {value.dtype}")
    S = key.shape[2]
    dt, B, H, L, E, HKV, rows = _check_decode("sdpa_decode", query, key, value, dequant, dtype, key.shape[1], splits)
    if key.shape[0] != B or key.shape[3] != E or tuple(value.shape) != (B, HKV, S, E):
        raise RuntimeError(f"sdpa_decode: shapes {tuple(query.shape)}, {tuple(key.shape)}, {tuple(value.shape)} do not fit")
    if min(B, L, S) < 1:
        raise RuntimeError(f"sdpa_decode: empty operands {tuple(query.shape)}, {tuple(key.shape)}")
    if attn_mask is not None and is_causal:
        raise ValueError("Explicit attn_mask should not be set when is_causal=True")
    mask, mask_kind, mask_dt, mask_strides = None, MASK_KINDS["causal" if is_causal else "none"], _tag(torch.float32), None
    if attn_mask is not None:
        if not 2 <= attn_mask.dim() <= 4 or tuple(attn_mask.shape[-2:]) != (L, S):
            raise RuntimeError(f"sdpa_decode: the mask's last two dims must be [{L}, {S}], got {tuple(attn_mask.shape)}")
        mask = attn_mask.detach().expand(B, H, L, S)
        if mask.dtype == torch.bool:
            mask_kind = MASK_KINDS["bool"]
        elif mask.dtype in (torch.float32, torch.bfloat16, torch.float16):
            mask_kind, mask_dt = MASK_KINDS["float"], _tag(mask.dtype)
        else:
            raise RuntimeError(f"sdpa_decode: a mask is bool or float, got {mask.dtype}")
        mask_strides = (ctypes.c_int64 * 4)(*mask.stride())
    return _run_decode("ffq_sdpa_decode", query, key, value, (mask,), dt, (B, H, HKV, L, E, rows), S, splits, scale, dequant, output_quantizer,
                       (B, H, HKV, L, S, E), (_ptr(mask), mask_kind, mask_dt, mask_strides))
