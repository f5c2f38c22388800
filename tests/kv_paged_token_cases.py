"""Shapes, page tables and operands shared by tests/test_kv_paged_token_cpu.py and tests/test_kv_paged_token_gpu.py: the paged int8 KV
cache with one dynamic (scale, offset) per (sequence, kv head, position) (include/ffq_kv_paged_token.h, ops/kv_cache.py,
nn/kv_cache.py).

The grid is tests/kv_paged_cases.py's and the per-row helpers are tests/kv_token_cases.py's, both by import. This module adds only the
scatter and the gather of a parameter store through a block table, and the uniform store at this grid's shape."""

from __future__ import annotations

import torch

import kv_token_cases as token

from kv_paged_cases import (B, C, DTYPE_IDS, DTYPES, ES, GROUPS, HKV, LAYOUTS, LENS_SETS, LS, PAGE_SIZES, SENTINEL, SPLITS, UNOWNED,  # noqa: F401
                            bottom_right, clamp_len, exact_case, page_table, pool_of, positions, scatter, table_tensor)
from kv_token_cases import PARAM_SENTINEL, pack, quantizer, reexpress, shift_rows  # noqa: F401


def param_pool_of(num_pages: int, P: int, layout: str, device, fill: float = 0.0, heads: int = HKV) -> torch.Tensor:
    """A parameter pool fp32 [num_pages, heads, P, 4] filled with `fill`, in either memory layout."""
    shape = (num_pages, heads, P, 4) if layout == "phse" else (num_pages, P, heads, 4)
    t = torch.full(shape, fill, dtype=torch.float32, device=device)
    return t if layout == "phse" else t.transpose(1, 2)


def scatter_params(dense: torch.Tensor, rows, pool: torch.Tensor) -> torch.Tensor:
    """Write a dense parameter store [B, H, capacity, 4] into `pool` at the pages `rows` names (entries outside the pool are
    skipped): kv_paged_cases.scatter, whose copy does not ask what the last dimension holds."""
    return scatter(dense, rows, pool)


def gather_dense(pool: torch.Tensor, rows, fill=0) -> torch.Tensor:
    """The dense [B, H, capacity, E | 4] view of a pool (codes or parameters) through the table rows `rows`; `fill` where an entry
    lies outside the pool."""
    num_pages, H, P, W = pool.shape
    out = torch.full((len(rows), H, len(rows[0]) * P, W), fill, dtype=pool.dtype, device=pool.device)
    for b, row in enumerate(rows):
        for slot, page in enumerate(row):
            if 0 <= page < num_pages:
                out[b, :, slot * P:(slot + 1) * P] = pool[page]
    return out


def uniform_store(k, v, device="cpu") -> torch.Tensor:
    """kv_token_cases.uniform_params at this grid's shape: every position's parameters one (scale, rne(offset)) per tensor,
    fp32 [B, HKV, C, 4]."""
    one = token.uniform_params(k, v)[:1, :1, :1]
    return one.expand(B, HKV, C, 4).contiguous().to(device)
