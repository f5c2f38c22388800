"""Shared cases of the MX tests (tests/test_mx_cpu.py, tests/test_w8_mx_gpu.py).

* A scalar statement of the quantization rule of docs/numerics.md ("MX formats") in plain Python — ``math.frexp``, integers, float64 —
  that shares nothing with torch's casts or with ``fastforward_amd._host``.
* The exhaustive bf16 table: every one of the 65 536 bf16 patterns inside a block beside an amax-setter, at five amax exponents.
* Exact operands for the linear: element values, scale codes and biases chosen so that every term and every partial sum, in any order, is a
  multiple of 2^-3 below 2^21: fp32 holds the sum exactly however the instruction orders or aligns it, and the expected output is the
  float64 product rounded once to the output dtype. ``exact_case`` asserts that bound for every case it builds."""

from __future__ import annotations

import bisect
import functools
import math

import torch

BLOCK = 32
EMAX = {"e4m3": 8, "e2m1": 2}
E2M1_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def e4m3_value(code: int) -> float:
    """The value of an OCP e4m3fn code (0x7F / 0xFF: NaN)."""
    e, m = (code >> 3) & 15, code & 7
    if e == 15 and m == 7:
        return math.nan
    v = math.ldexp(1 + m / 8, e - 7) if e else math.ldexp(m / 8, -6)
    return -v if code & 0x80 else v


def e2m1_value(code: int) -> float:
    v = E2M1_GRID[code & 7]
    return -v if code & 8 else v


GRID = {"e4m3": tuple(e4m3_value(c) for c in range(127)), "e2m1": E2M1_GRID}  # the non-negative values, indexed by magnitude code
SIGN = {"e4m3": 0x80, "e2m1": 0x8}


def scalar_scale(amax: float, fmt: str) -> int:
    """The E8M0 code of a block with finite |x| maximum `amax`: max(biased fp32 exponent - emax, 0)."""
    if amax < math.ldexp(1.0, -126):
        e = 0
    else:
        _, ex = math.frexp(amax)  # amax = m * 2^ex, 0.5 <= m < 1
        e = ex - 1 + 127
    return max(e - EMAX[fmt], 0)


def scalar_element(x: float, scale: int, fmt: str) -> int:
    grid = GRID[fmt]
    y = math.ldexp(x, 127 - scale)  # exact in float64; where fp32 would round (below 2^-126) both round to zero
    sign = SIGN[fmt] if math.copysign(1.0, x) < 0 else 0
    ay = min(abs(y), grid[-1])
    hi = bisect.bisect_left(grid, ay)
    if hi < len(grid) and grid[hi] == ay:
        return sign | hi
    lo = hi - 1  # grid[lo] < ay < grid[hi]
    below, above = ay - grid[lo], grid[hi] - ay
    if below != above:
        return sign | (lo if below < above else hi)
    return sign | (lo if lo % 2 == 0 else hi)


def scalar_quantize_block(values: list[float], fmt: str) -> tuple[list[int], int]:
    """(32 element codes, scale code) of one block by the rule, in Python scalars."""
    if any(math.isnan(v) or math.isinf(v) for v in values):
        return [0] * len(values), 255
    scale = scalar_scale(max(abs(v) for v in values), fmt)
    return [scalar_element(v, scale, fmt) for v in values], scale


def scalar_quantize(x: torch.Tensor, fmt: str) -> tuple[torch.Tensor, torch.Tensor]:
    """The scalar rule over a tensor ``[rows, K]``: (codes uint8 [rows, K], scales uint8 [rows, K / 32])."""
    rows, K = x.shape
    flat = x.to(torch.float64).reshape(-1, BLOCK).tolist()
    codes, scales = [], []
    for block in flat:
        c, s = scalar_quantize_block(block, fmt)
        codes.append(c)
        scales.append(s)
    return torch.tensor(codes, dtype=torch.uint8).reshape(rows, K), torch.tensor(scales, dtype=torch.uint8).reshape(rows, K // BLOCK)


def scalar_dequantize(code: int, scale: int, fmt: str) -> float:
    if scale == 255:
        return math.nan
    return math.ldexp(e4m3_value(code) if fmt == "e4m3" else e2m1_value(code), scale - 127)


# ---- every bf16 pattern ---------------------------------------------------------------------------------------------------------------------
DEPTHS = (0, 1, 3, 10, 16)  # binades between the block's amax-setter and its largest pattern


@functools.lru_cache(maxsize=None)
def exhaustive_bf16() -> torch.Tensor:
    """bf16 ``[rows, 32]``: every bf16 pattern in a block of 31 patterns of neighbouring magnitude plus an amax-setter in element 0 that
    is 2^d above the block's largest finite pattern (capped at the largest binade), once per d in DEPTHS — so every pattern is seen at
    the top of the grid, inside it, among the subnormals and below half the smallest step. The 256 patterns that are NaN or Inf come
    last, each in a block of ones (their blocks are poisoned whole)."""
    bits = torch.arange(65536, dtype=torch.int32)
    finite = bits[((bits >> 7) & 0xFF) != 0xFF]
    nonfinite = bits[((bits >> 7) & 0xFF) == 0xFF]
    pad = (-finite.numel()) % 31
    finite = torch.cat([finite, torch.zeros(pad, dtype=torch.int32)]).reshape(-1, 31)
    top_exponent = ((finite >> 7) & 0xFF).amax(dim=1)  # biased exponent of the largest magnitude of the block
    tables = []
    for d in DEPTHS:
        setter = ((top_exponent + d).clamp(max=254) << 7) | 0x60  # 1.75 * 2^(e + d - 127)
        tables.append(torch.cat([setter[:, None], finite], dim=1))
    poisoned = torch.full((nonfinite.numel(), 32), 0x3F80, dtype=torch.int32)
    poisoned[:, 5] = nonfinite
    tables.append(poisoned)
    return torch.cat(tables).to(torch.int16).view(torch.bfloat16)


# ---- exact operands for the linear ------------------------------------------------------------------------------------------------------------
E4M3_OF_INT = {int(e4m3_value(c)): c for c in range(256) if not math.isnan(e4m3_value(c)) and abs(e4m3_value(c)) <= 15 and e4m3_value(c) == int(e4m3_value(c))
               and not (c == 0x80)}
EXACT_SHAPES = [(1, 1, 128), (31, 127, 128), (32, 64, 256), (33, 129, 256), (127, 200, 640), (129, 128, 128), (300, 129, 640)]  # (M, N, K)
PAIRS = [("e4m3", "e4m3"), ("e4m3", "e2m1"), ("e2m1", "e2m1")]


def element_values(codes: torch.Tensor, fmt: str) -> torch.Tensor:
    """float64 values of element codes (one per byte), from the scalar tables."""
    table = torch.tensor([e4m3_value(c) if fmt == "e4m3" else e2m1_value(c & 15) for c in range(256)], dtype=torch.float64)
    return table[codes.long()]


def dequantize64(codes: torch.Tensor, scales: torch.Tensor, fmt: str) -> torch.Tensor:
    """float64 ``value(code) * 2^(scale - 127)`` (scale 255: NaN), exact."""
    s = torch.where(scales == 255, torch.full((), math.nan, dtype=torch.float64), torch.ldexp(torch.ones((), dtype=torch.float64), scales.to(torch.int32) - 127))
    return element_values(codes, fmt) * s.repeat_interleave(BLOCK, dim=-1)


def _codes(rows: int, K: int, fmt: str, g: torch.Generator) -> torch.Tensor:
    if fmt == "e2m1":
        return torch.randint(0, 16, (rows, K), generator=g, dtype=torch.uint8)  # any grid value, either sign
    ints = torch.randint(-15, 16, (rows, K), generator=g)
    table = torch.zeros(31, dtype=torch.uint8)
    for v, c in E4M3_OF_INT.items():
        table[v + 15] = c
    return table[ints + 15]


def exact_case(M: int, N: int, K: int, a_fmt: str, w_fmt: str, seed: int = 0) -> dict:
    """Operands (codes one per byte, scale bytes), a bias and the float64 result of ``A . W^T`` with and without it."""
    assert K % 128 == 0 and K <= 640 and len(E4M3_OF_INT) == 31
    g = torch.Generator().manual_seed(1000 * seed + 7 * M + 3 * N + K + (a_fmt == "e2m1") + 2 * (w_fmt == "e2m1"))
    a_codes, w_codes = _codes(M, K, a_fmt, g), _codes(N, K, w_fmt, g)
    a_scales = torch.randint(127, 130, (M, K // BLOCK), generator=g, dtype=torch.uint8)
    w_scales = torch.randint(126, 129, (N, K // BLOCK), generator=g, dtype=torch.uint8)
    bias = torch.randint(-1024, 1025, (N,), generator=g).to(torch.float64) / 8  # multiples of 2^-3, |b| <= 128
    a, w = dequantize64(a_codes, a_scales, a_fmt), dequantize64(w_codes, w_scales, w_fmt)
    # the bound: every term is a multiple of 2^-3, and the sum of magnitudes (so every partial sum in any order, the bias included) is
    # below 2^21: 24 bits, an fp32 significand
    for t in (a, w):
        assert torch.equal(t * 4, (t * 4).round())  # A: multiples of 2^-1 at worst (e2m1 0.5 x 2^0), W: of 2^-2 (0.5 x 2^-1)
    magnitude = a.abs() @ w.abs().T + bias.abs()
    assert float(magnitude.max()) < 2.0**21, float(magnitude.max())
    product = a @ w.T
    assert torch.equal(product * 8, (product * 8).round())
    if M > 1 and M == N:
        assert not torch.equal(a, w)
    return dict(a_codes=a_codes, a_scales=a_scales, w_codes=w_codes, w_scales=w_scales, bias=bias, product=product, with_bias=product + bias)
