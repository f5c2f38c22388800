"""Shapes, operands and restatements shared by tests/test_kv_cache_cpu.py and tests/test_kv_cache_gpu.py: the preallocated int8 KV
cache (include/ffq_kv_cache.h, ops/kv_cache.py, nn/kv_cache.py).

The GPU shapes are the smallest at which the kernels can go wrong: five sequences whose lengths sit on and beside every boundary of
a three-tile cache (0, 1, one key short of a tile, a tile, one key past it, mid-cache, full, and past the end), queries of 1, 4 and
5 rows (5 with lengths below it: rows without a visible key), one and four query heads per kv head, every forced split count
beside the rule's."""

from __future__ import annotations

import functools
import math

import torch

import fastforward_amd as ff

import attention_exact as ax

B, HKV, S_MAX = 5, 2, 384
LENS_SETS = ((0, 1, 127, 128, 129), (300, 384, 400, 2, 4))  # {0, 1, 127, 128, 129, 300, 384}, one past S_max, and two below L = 5
LS = (1, 4, 5)
GROUPS = (1, 4)
ES = (64, 128)
SPLITS = (0, 1, 2, 3, 64)
DTYPES = (torch.bfloat16, torch.float16)
DTYPE_IDS = ("bf16", "fp16")
SENTINEL = 0x5A
K_SPEC, V_SPEC = (8, 0.031, 300.5), (4, 0.2, -200.25)  # (bits, scale, offset): real offsets beyond int8


def quantizer(spec, device="cpu", container=torch.int8):
    """An initialised per-tensor static LinearQuantizer with the given (bits, scale, offset)."""
    bits, scale, offset = spec
    q = ff.nn.LinearQuantizer(bits, symmetric=False, granularity=ff.PerTensor(), quantized_dtype=container, device=device)
    q.quantization_range = (torch.tensor(-1.0, device=device), torch.tensor(1.0, device=device))
    with torch.no_grad():
        q.scale.fill_(scale)
        q.offset.fill_(offset)
    return q


def params(spec, device):
    """(scale, offset, bits) as ``ops.kv_append`` takes them."""
    bits, scale, offset = spec
    return torch.tensor([scale], device=device), None if offset is None else torch.tensor([offset], device=device), float(bits)


def clamp_len(n: int, s_max: int = S_MAX) -> int:
    return min(max(n, 0), s_max)


def positions(n: int, L: int, s_max: int = S_MAX) -> list[tuple[int, int]]:
    """(row l, position) of the rows of an append that land inside the cache when the length AFTER it is `n`."""
    return [(l, n - L + l) for l in range(L) if 0 <= n - L + l < s_max]


def bottom_right(L: int, S: int, device="cpu") -> torch.Tensor:
    """bool [L, S]: row l sees key <= l + (S - L)."""
    return torch.arange(S, device=device).unsqueeze(0) <= torch.arange(L, device=device).unsqueeze(1) + (S - L)


def rotate_rounded(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """rd(rd(x1 cos_lo) + rd(-x2 sin_lo)) | rd(rd(x2 cos_hi) + rd(x1 sin_hi)) restated: float64 products (exact for two 16-bit
    floats) rounded to the dtype, their fp32 sum rounded once. x [..., E], cos / sin broadcastable rows in x's dtype."""
    dt, half = x.dtype, x.shape[-1] // 2
    x1, x2 = x[..., :half].double(), x[..., half:].double()
    c, s = cos.double(), sin.double()
    lo = ((x1 * c[..., :half]).to(dt).float() + (-x2 * s[..., :half]).to(dt).float()).to(dt)
    hi = ((x2 * c[..., half:]).to(dt).float() + (x1 * s[..., half:]).to(dt).float()).to(dt)
    return torch.cat((lo, hi), dim=-1)


def codes64(x: torch.Tensor, spec) -> torch.Tensor:
    """A1 restated in float64, for parameters with which every step is exact there AND in fp32 (a power-of-two scale, an integral
    offset): clamp(rne(x / scale - rne(offset)))."""
    bits, scale, offset = spec
    assert math.frexp(scale)[0] == 0.5 and offset == round(offset)
    return torch.clamp(torch.round(x.double() / scale - offset), -(2 ** (bits - 1)), 2 ** (bits - 1) - 1).to(torch.int8)


def attend64(q, k_cache, v_cache, lens, k_spec, v_spec, causal: bool, scale=None) -> torch.Tensor:
    """The cache's attention in float64 on the dequantized codes: per batch over its own keys, bottom-right causality, exact zeros
    for a row (or a sequence) without a visible key."""
    Bq, H, L, E = q.shape
    out = torch.zeros(Bq, H, L, E, dtype=torch.float64)
    for b, n in enumerate(lens):
        S = clamp_len(n, k_cache.shape[2])
        if S == 0:
            continue
        k = (k_cache[b:b + 1, :, :S].cpu().double() + round(k_spec[2])) * k_spec[1]
        v = (v_cache[b:b + 1, :, :S].cpu().double() + round(v_spec[2])) * v_spec[1]
        k, v = (t.to(q.dtype).double() for t in (k, v))  # (the value the kernels contract: rounded once to the data dtype)
        out[b] = ax.reference64(q[b:b + 1].cpu(), k, v, mask=bottom_right(L, S) if causal else None, scale=scale)[0]
    return out


# ---- operands whose answer is known exactly ------------------------------------------------------------------------------------------------
def k_codes(k: torch.Tensor, scale: float, offset: float) -> torch.Tensor:
    """The pattern's keys (small integers times `scale`) as int8 codes c = k / scale - offset; refuses what does not fit."""
    c = k.double() / scale - offset
    assert bool((c == c.round()).all()) and float(c.min()) >= -128 and float(c.max()) <= 127
    return c.to(torch.int8)


def v_parameters(gen: torch.Generator) -> tuple[float, float]:
    """(scale, offset) of one-hot V codes: V = (c + o) * 2^-e with c over all of [-128, 127] and o = +-200. No value is zero and the
    largest is less than five times the smallest, so a one-hot row's answer V[target], a number of the dtype, keeps its bits under the
    2^-24 of probability mass the other keys hold: the test may ask for equality."""
    return 2.0 ** -(0, 3, 7)[int(torch.randint(0, 3, (1,), generator=gen))], (200.0, -200.0)[int(torch.randint(0, 2, (1,), generator=gen))]


@functools.lru_cache(maxsize=None)
def exact_case(kind: str, causal: bool, L: int, G: int, E: int, dtype: torch.dtype, lens: tuple[int, ...]):
    """One ragged batch built from a pattern of tests/attention_exact.py cut to each sequence's own key count: (q [B, H, L, E],
    K codes and V codes [B, HKV, S_MAX, E] with random codes past every length, (k scale, k offset), (v scale, v offset), the expected
    output in float64). Built once and left unchanged.
      select     row (h, l) asks for one drawn key among the S_b (no mask);
      staircase  scores rise with the key index, so a row returns the LAST key it sees: S_b - 1 without a mask, l + (S_b - L)
                 under bottom-right causality, nothing (zeros) where that is negative;
      uniform    q = 0: a row returns the mean of the indicator V over the keys it sees, rounded as attention_exact rounds it."""
    H = HKV * G
    gen = ax.generator("kv_cache_exact", kind, causal, L, G, E, str(dtype), lens)
    q = torch.zeros(B, H, L, E, dtype=dtype)
    kc = torch.randint(-128, 128, (B, HKV, S_MAX, E), generator=gen).to(torch.int8)
    vc = torch.randint(-128, 128, (B, HKV, S_MAX, E), generator=gen).to(torch.int8)
    expected = torch.zeros(B, H, L, E, dtype=torch.float64)
    k_param = {"select": (1.0, 100.0), "staircase": (1.0, 8.0), "uniform": (2.0**-2, 100.0)}[kind]
    v_scale, v_offset = (1.0, 100.0) if kind == "uniform" else v_parameters(gen)
    for b, n in enumerate(lens):
        S = clamp_len(n)
        if S == 0:
            q[b] = torch.randn(H, L, E, generator=gen).to(dtype)
            continue
        shape = ax.Shape(1, H, HKV, L, S, E)
        if kind == "uniform":
            p = ax.uniform(shape, dtype, variant=b % 2, mask=bottom_right(L, S) if causal else None, seed=b)
            q[b], expected[b] = p.q[0], p.expected[0]
            kc[b, :, :S], vc[b, :, :S] = k_codes(p.k[0], *k_param), k_codes(p.v[0], v_scale, v_offset)
            continue
        assert kind == "staircase" or not causal
        p = ax.select(shape, dtype, causal=False, seed=b) if kind == "select" else ax.staircase(shape, dtype, causal=False, seed=b)
        assert p.residual <= ax.RESIDUAL_LIMIT
        codes = vc[b, :, :S]
        values = ((codes.float() + v_offset) * v_scale).to(dtype)  # (c + o) * s, rounded once: what the kernels contract
        target = p.target[0] if not causal else (torch.arange(L) + (S - L)).expand(H, L)
        seen = target >= 0
        rows = values.double().repeat_interleave(G, 0).gather(1, target.clamp_min(0).unsqueeze(-1).expand(-1, -1, E))
        q[b], expected[b] = p.q[0], torch.where(seen.unsqueeze(-1), rows, torch.zeros_like(rows))
        kc[b, :, :S] = k_codes(p.k[0], *k_param)
    return q, kc, vc, k_param, (v_scale, v_offset), expected
