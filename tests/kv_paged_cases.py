"""Shapes, page tables and operands shared by tests/test_kv_paged_cpu.py and tests/test_kv_paged_gpu.py: the int8 KV cache in pages
(include/ffq_kv_paged.h, ops/kv_cache.py, nn/kv_cache.py).

Four sequences of capacity C = 512 (four key tiles) over page sizes 16 (two pages per 32-key wave step), 32 (one), 128 (a page is a
key tile) and 256 (a page spans two tiles). The lengths sit on and beside every boundary: 0, 1, one key short of a page of 16 / on it
/ past it, the same around a key tile, mid-cache, full, past the end, and below L = 4 / 5. Every sequence's pages are a seeded
permutation of the pool in which no two logical neighbours are physical neighbours, and some pool pages belong to nobody."""

from __future__ import annotations

import functools

import torch

import attention_exact as ax
import kv_cache_cases as dense_cases

from kv_cache_cases import DTYPE_IDS, DTYPES, K_SPEC, SENTINEL, V_SPEC, bottom_right, params, quantizer  # noqa: F401

B, HKV, C = 4, 2, 512
LENS_SETS = ((0, 1, 15, 16), (17, 127, 128, 129), (300, 512, 530, 2))
LS = (1, 4, 5)
GROUPS = (1, 4)
ES = (64, 128)
PAGE_SIZES = (16, 32, 128, 256)
SPLITS = (0, 1, 2, 3, 64)
LAYOUTS = ("phse", "pshe")
UNOWNED = 5  # pool pages that no sequence is given


def clamp_len(n: int) -> int:
    return min(max(n, 0), C)


def positions(n: int, L: int) -> list[tuple[int, int]]:
    """(row l, position) of the rows of an append that land inside a sequence when the length AFTER it is `n`."""
    return dense_cases.positions(n, L, C)


@functools.lru_cache(maxsize=None)
def page_table(P: int, batch: int = B, capacity: int = C, seed: int = 0) -> tuple[tuple[tuple[int, ...], ...], int]:
    """(table rows, num_pages): `batch` rows of capacity / P pool pages, a seeded permutation of a pool with UNOWNED pages left over;
    inside a row no two consecutive entries are consecutive pool pages."""
    per = capacity // P
    num_pages = batch * per + UNOWNED
    for attempt in range(1000):
        perm = torch.randperm(num_pages, generator=torch.Generator().manual_seed(1000 * seed + attempt)).tolist()
        rows = tuple(tuple(perm[b * per:(b + 1) * per]) for b in range(batch))
        if all(abs(x - y) != 1 for row in rows for x, y in zip(row, row[1:])):
            return rows, num_pages
    raise AssertionError("no scattered page assignment found")


def pool_of(num_pages: int, P: int, E: int, layout: str, device, fill: int = 0, heads: int = HKV) -> torch.Tensor:
    """A pool [num_pages, heads, P, E] filled with `fill`, in either memory layout."""
    shape = (num_pages, heads, P, E) if layout == "phse" else (num_pages, P, heads, E)
    t = torch.full(shape, fill, dtype=torch.int8, device=device)
    return t if layout == "phse" else t.transpose(1, 2)


def scatter(dense: torch.Tensor, rows, pool: torch.Tensor) -> torch.Tensor:
    """Write dense codes [B, H, capacity, E] into `pool` at the pages `rows` names (entries outside the pool are skipped)."""
    P = pool.shape[2]
    for b, row in enumerate(rows):
        for slot, page in enumerate(row):
            if 0 <= page < pool.shape[0]:
                pool[page].copy_(dense[b, :, slot * P:(slot + 1) * P])
    return pool


def table_tensor(rows, device) -> torch.Tensor:
    return torch.tensor(rows, dtype=torch.int32, device=device)


# ---- operands whose answer is known exactly ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_case(kind: str, causal: bool, L: int, G: int, E: int, dtype: torch.dtype, lens: tuple[int, ...]):
    """kv_cache_cases.exact_case at this module's batch and capacity: (q [B, H, L, E], dense K and V codes [B, HKV, C, E] with random
    codes past every length, (k scale, k offset), (v scale, v offset), the expected output in float64). Built once, left unchanged."""
    H = HKV * G
    gen = ax.generator("kv_paged_exact", kind, causal, L, G, E, str(dtype), lens)
    q = torch.zeros(B, H, L, E, dtype=dtype)
    kc = torch.randint(-128, 128, (B, HKV, C, E), generator=gen).to(torch.int8)
    vc = torch.randint(-128, 128, (B, HKV, C, E), generator=gen).to(torch.int8)
    expected = torch.zeros(B, H, L, E, dtype=torch.float64)
    k_param = {"select": (1.0, 100.0), "staircase": (1.0, 8.0), "uniform": (2.0**-2, 100.0)}[kind]
    v_scale, v_offset = (1.0, 100.0) if kind == "uniform" else dense_cases.v_parameters(gen)
    for b, n in enumerate(lens):
        S = clamp_len(n)
        if S == 0:
            q[b] = torch.randn(H, L, E, generator=gen).to(dtype)
            continue
        shape = ax.Shape(1, H, HKV, L, S, E)
        if kind == "uniform":
            p = ax.uniform(shape, dtype, variant=b % 2, mask=bottom_right(L, S) if causal else None, seed=b)
            q[b], expected[b] = p.q[0], p.expected[0]
            kc[b, :, :S], vc[b, :, :S] = dense_cases.k_codes(p.k[0], *k_param), dense_cases.k_codes(p.v[0], v_scale, v_offset)
            continue
        assert kind == "staircase" or not causal
        p = ax.select(shape, dtype, causal=False, seed=b) if kind == "select" else ax.staircase(shape, dtype, causal=False, seed=b)
        assert p.residual <= ax.RESIDUAL_LIMIT
        values = ((vc[b, :, :S].float() + v_offset) * v_scale).to(dtype)  # (c + o) * s, rounded once: what the kernels contract
        target = p.target[0] if not causal else (torch.arange(L) + (S - L)).expand(H, L)
        seen = target >= 0
        rows = values.double().repeat_interleave(G, 0).gather(1, target.clamp_min(0).unsqueeze(-1).expand(-1, -1, E))
        q[b], expected[b] = p.q[0], torch.where(seen.unsqueeze(-1), rows, torch.zeros_like(rows))
        kc[b, :, :S] = dense_cases.k_codes(p.k[0], *k_param)
    return q, kc, vc, k_param, (v_scale, v_offset), expected
