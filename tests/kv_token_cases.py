"""Shapes, operands and restatements shared by tests/test_kv_token_cpu.py and tests/test_kv_token_gpu.py: the int8 KV cache with one
dynamic (scale, offset) per (sequence, kv head, position) (include/ffq_kv_token.h, ops/kv_cache.py, nn/kv_cache.py).

The grid is tests/kv_cache_cases.py's, by import. Two things are added: ``reexpress``, which rewrites a per-tensor cache row by row
into other codes and parameters that dequantize to the same numbers with every fp32 step exact (so the dense kernel on the original
cache is an exact reference for the per-row kernel), and the per-row dequantization restated in float64."""

from __future__ import annotations

import math

import torch

import fastforward_amd as ff

import attention_exact as ax
import kv_cache_cases as dense

from kv_cache_cases import B, DTYPE_IDS, DTYPES, ES, GROUPS, HKV, LENS_SETS, LS, S_MAX, SENTINEL, SPLITS  # noqa: F401

PARAM_SENTINEL = -7.0  # what an untouched parameter holds (integral: a stored offset is a rounded one, and tests read sentinel rows as parameters too)
SHIFTS = (-17, -3, 5, 17)
IDENTITY, DOUBLE, QUADRUPLE = 0, 5, 6  # variant ids; 1..4 are the shifts


def quantizer(bits, symmetric=False, E=64, tile=False):
    """A dynamic quantizer the cache takes: one tile per row, int8 container."""
    granularity = ff.PerTile((1, 1, 1, E)) if tile else ff.PerChannel((0, 1, 2))
    return ff.nn.DynamicLinearQuantizer(bits, granularity=granularity, quantized_dtype=torch.int8, symmetric=symmetric, allow_one_sided=False)


def reexpress(codes: torch.Tensor, s: float, o: float, gen: torch.Generator, variants=tuple(range(7))):
    """The per-tensor codes [B, H, S, E] of a cache with a power-of-two scale `s` and an integer offset `o`, re-expressed row by row.
    One variant is drawn per (sequence, head, position): (c, s, o); (c - d, s, o + d) with d in SHIFTS; (2c, s / 2, 2o);
    (4c, s / 4, 4o); it is applied only where every code of the row stays inside int8, else the row keeps the identity. Every
    variant dequantizes to the same real number with every fp32 step exact. Returns (new codes int8, scale [B, H, S] fp32, offset
    [B, H, S] fp32, the variant each row took)."""
    assert math.frexp(s)[0] == 0.5 and o == round(o)
    c = codes.to(torch.int32)
    drawn = torch.tensor(variants)[torch.randint(0, len(variants), c.shape[:3], generator=gen)]
    lo, hi = c.amin(-1), c.amax(-1)
    new, scale, offset = c.clone(), torch.full(c.shape[:3], float(s)), torch.full(c.shape[:3], float(o))
    took = torch.zeros_like(drawn)
    for variant in variants:
        if variant == IDENTITY:
            continue
        if variant in (DOUBLE, QUADRUPLE):
            f = 2 if variant == DOUBLE else 4
            fits = (lo * f >= -128) & (hi * f <= 127)
            rows = (drawn == variant) & fits
            new[rows], scale[rows], offset[rows] = c[rows] * f, s / f, float(o * f)
        else:
            d = SHIFTS[variant - 1]
            fits = (lo - d >= -128) & (hi - d <= 127)
            rows = (drawn == variant) & fits
            new[rows], offset[rows] = c[rows] - d, float(o + d)
        took[rows] = variant
    assert int(new.min()) >= -128 and int(new.max()) <= 127
    return new.to(torch.int8), scale, offset, took


def shift_rows(codes: torch.Tensor, s: float, o: float):
    """Every row that allows it shifted by d = 5 (every code >= -123) or else d = -5 (every code <= 122): (codes, scale, offset,
    shifted bool [B, H, S])."""
    c = codes.to(torch.int32)
    lo, hi = c.amin(-1), c.amax(-1)
    down, up = lo >= -123, hi <= 122
    d = torch.where(down, 5, torch.where(up, -5, 0))
    new = c - d.unsqueeze(-1)
    return new.to(torch.int8), torch.full(c.shape[:3], float(s)), float(o) + d.float(), d != 0


def pack(ks, ko, vs, vo, device="cpu") -> torch.Tensor:
    """fp32 [B, H, S, 4] of four [B, H, S] tensors (or numbers)."""
    shape = next(t.shape for t in (ks, ko, vs, vo) if isinstance(t, torch.Tensor))
    return torch.stack([t.float() if isinstance(t, torch.Tensor) else torch.full(shape, float(t)) for t in (ks, ko, vs, vo)], dim=-1).contiguous().to(device)


def uniform_params(k, v, device="cpu") -> torch.Tensor:
    """Every position's parameters set to one (scale, rne(offset)) per tensor."""
    return pack(torch.full((B, HKV, S_MAX), k[0]), round(k[1]), v[0], round(v[1]), device)


def dequant64(codes: torch.Tensor, params: torch.Tensor, which: int, dtype: torch.dtype) -> torch.Tensor:
    """The per-row dequantization restated: (c + o) * s exact in float64, rounded to fp32 as the kernel's one fp32 product is, then once
    to the data dtype; float64 of that. `which` 0: K's pair of `params` [.., S, 4], 1: V's."""
    s, o = params[..., 2 * which].cpu().double().unsqueeze(-1), params[..., 2 * which + 1].cpu().double().unsqueeze(-1)
    return ((codes.cpu().double() + o) * s).float().to(dtype).double()


def attend64(q, k_cache, v_cache, params, lens, causal: bool, scale=None) -> torch.Tensor:
    """kv_cache_cases.attend64 with the per-row parameters."""
    Bq, H, L, E = q.shape
    out = torch.zeros(Bq, H, L, E, dtype=torch.float64)
    for b, n in enumerate(lens):
        S = dense.clamp_len(n, k_cache.shape[2])
        if S == 0:
            continue
        k = dequant64(k_cache[b:b + 1, :, :S], params[b:b + 1, :, :S], 0, q.dtype)
        v = dequant64(v_cache[b:b + 1, :, :S], params[b:b + 1, :, :S], 1, q.dtype)
        out[b] = ax.reference64(q[b:b + 1].cpu(), k, v, mask=dense.bottom_right(L, S) if causal else None, scale=scale)[0]
    return out


def meets_the_contract(got, want, ref, what=""):
    """The attention contract of tests/test_kv_cache_gpu.py (tests/test_sdpa_decode_gpu.py holds the helper, in a module that needs a
    device to import), restated: the error against float64 is at most the device math path's own on the same call + 2^-9."""
    err_got = float((got.cpu().double() - ref).abs().max())
    err_math = float((want.cpu().double() - ref).abs().max())
    assert err_got <= err_math + 2.0**-9, f"{what}: {err_got:.3e} from float64, math path {err_math:.3e}"


def dynamic_rows(rows: torch.Tensor, bits, symmetric):
    """(codes, scale [..], offset [..]) of ``_host.quantize_dynamic_by_tile`` on rows [..., E], one tile per row."""
    from fastforward_amd import _host

    flat = rows.reshape(1, 1, -1, rows.shape[-1])
    codes, scale, offset = _host.quantize_dynamic_by_tile(flat, (1, 1, 1, rows.shape[-1]), float(bits), symmetric, False, torch.int8)
    return codes.reshape(rows.shape), scale.reshape(rows.shape[:-1]), offset.reshape(rows.shape[:-1])
