"""Operand patterns for the int8 contractions where accumulators exceed 2^24, and the shared fp32 epilogue restated.

Every int8 contraction of the library (csrc/ffq_linear.hip's tail and persistent kernels, batched matmul, the gate / up launch,
conv and conv_transpose through csrc/ffq_conv_tile.h) ends in one epilogue (include/ffq.h, docs/numerics.md A6):

    v = float(acc);  v = v + ox * rsw;  v = v + ow * rsx;  v = v + (K * ox) * ow;  y = (sx * sw) * v  (+ bias)

every step its own fp32 rounding. With uniform codes and small offsets all of these are integers below 2^24 and any order, any
contraction into an FMA and any int -> float conversion gives the same bits. The patterns here leave that regime:

* ``low``: activations at -128 except a seeded 10 % drawn uniformly (post-SiLU / post-ReLU tensors under an asymmetric quantizer),
  weights ``round(clamp(20 randn + 60))`` (a non-zero mean code), ``ox = 119`` (not a power of two: ``ox * rsw`` rounds),
  ``ow[n] = -(50 + n % 23)``. At K = 4096 every |acc| and each of the three offset products is about 3e7 while |v| <= 4e5.
* ``mirror``: ``low`` with all signs flipped.
* ``ties``: rows of 127 against rows of 127 with a row-dependent number of entries lowered by one. Even weight rows span all of K
  (accumulators in [2^25, 2^26), halfway cases where = 2 mod 4), odd weight rows the first 1536 entries (accumulators in
  [2^24, 2^25), halfway cases where odd). Unit scales, no offsets: the fp32 output is the round-half-even of the integer.
* ``saturated``: every sign pairing of {-128, 127} on both sides, with a row-dependent number of entries at the other extreme.

Expected values never come from the library: the accumulator is a float64 matmul of the codes (exact below 2^53; ``.float()`` is
the round-half-even the hardware's int32 -> fp32 conversion performs), the epilogue is elementwise torch ops, one IEEE operation
each. Seeded and deterministic; codes are drawn on the device they are used on.
"""

from __future__ import annotations

import dataclasses

import torch

PATTERNS = ("low", "mirror", "ties", "saturated")
TIES_SHORT = 1536  # the support of the odd weight rows of `ties`: 127 * 127 * 1536 lies in [2^24, 2^25)


@dataclasses.dataclass
class Operands:
    """Codes [M, K] / [N, K] (int8) and the parameters the pattern brings: fp32 tensors, offsets None where the pattern has none."""

    xq: torch.Tensor
    wq: torch.Tensor
    sx: torch.Tensor
    ox: torch.Tensor | None
    sw: torch.Tensor
    ow: torch.Tensor | None


def _generator(device, seed):
    return torch.Generator(device=device).manual_seed(seed)


def _low_codes(m, n, k, device, seed):
    g = _generator(device, seed)
    drawn = torch.randint(-128, 128, (m, k), device=device, generator=g)
    keep = torch.rand(m, k, device=device, generator=g) < 0.1
    xq = torch.where(keep, drawn, torch.full_like(drawn, -128))
    wq = torch.round(torch.clamp(20.0 * torch.randn(n, k, device=device, generator=g) + 60.0, -128, 127)).long()
    return xq, wq


def _lowered(rows, k, counts, start, device):
    """[rows, k] of 0 / 1: row r has counts[r] ones from column `start` on."""
    col = torch.arange(k, device=device)[None, :]
    return ((col >= start) & (col < start + counts[:, None])).long()


def codes(pattern: str, m: int, n: int, k: int, device="cpu", seed: int = 1) -> tuple[torch.Tensor, torch.Tensor]:
    """(xq [m, k], wq [n, k]) as int8 on `device`."""
    rm, rn = torch.arange(m, device=device), torch.arange(n, device=device)
    if pattern == "low":
        xq, wq = _low_codes(m, n, k, device, seed)
    elif pattern == "mirror":  # -(-128) has no int8 code: it becomes 127
        xq, wq = (torch.clamp(-t, -128, 127) for t in _low_codes(m, n, k, device, seed))
    elif pattern == "ties":
        assert k >= TIES_SHORT
        xq = 127 - _lowered(m, k, rm % 1024, 0, device)
        support = torch.where(rn % 2 == 0, k, TIES_SHORT)
        wq = 127 - _lowered(n, k, (rn // 2) % 256, 1024, device)
        wq = wq * (torch.arange(k, device=device)[None, :] < support[:, None])
    elif pattern == "saturated":
        # row r: the extreme its parity names, with (r // 2) % 64 entries at the other one
        hi_x = ((rm % 2)[:, None] ^ _lowered(m, k, (rm // 2) % 64, 0, device)).bool()
        hi_w = (((rn // 2) % 2)[:, None] ^ _lowered(n, k, (rn // 4) % 64, 64, device)).bool()
        xq, wq = torch.where(hi_x, 127, -128), torch.where(hi_w, 127, -128)
    else:
        raise ValueError(pattern)
    return xq.to(torch.int8), wq.to(torch.int8)


def parameters(pattern: str, m: int, n: int, device="cpu", per_token: bool = False, ow_kind: str = "native", native: bool = True):
    """(sx, ox, sw, ow). ``native``: what the pattern states (unit scales and no offsets for ``ties`` / ``saturated``); otherwise,
    and for per-token or explicit weight-offset variants, the heavy parameters of ``low`` (``mirror``: signs flipped).
    ``ow_kind``: "native", "none", "zero" or "real"."""
    rm, rn = torch.arange(m, device=device), torch.arange(n, device=device)
    unit = native and pattern in ("ties", "saturated") and not per_token and ow_kind in ("native", "none")
    if unit:
        return torch.ones(1, device=device), None, torch.ones(n, device=device), None
    sign = -1.0 if pattern == "mirror" else 1.0
    if per_token:
        sx = 0.02 * (1.0 + (rm % 7).float() / 8.0)
        ox = sign * (119.0 - (rm % 5).float())
    else:
        sx = torch.tensor([0.02], device=device)
        ox = torch.tensor([sign * 119.0], device=device)
    sw = 1e-3 * (1.0 + (rn % 11).float() / 16.0)
    if ow_kind in ("native", "real"):
        ow = -sign * (50.0 + (rn % 23).float())
    elif ow_kind == "zero":
        ow = torch.zeros(n, device=device)
    else:
        ow = None
    return sx, ox, sw, ow


def operands(pattern: str, m: int, n: int, k: int, device="cpu", seed: int = 1, **kw) -> Operands:
    xq, wq = codes(pattern, m, n, k, device, seed)
    return Operands(xq, wq, *parameters(pattern, m, n, device, **kw))


# ---- expected values ---------------------------------------------------------------------------------------------------------------
def accumulator64(xq: torch.Tensor, wq: torch.Tensor) -> torch.Tensor:
    """sum_k xq[m, k] * wq[n, k] in float64: exact (every partial sum is an integer below 2^53). No bound on its size is assumed."""
    w64 = wq.double().T.contiguous()
    return torch.cat([xq[r0:r0 + 4096].double() @ w64 for r0 in range(0, xq.shape[0], 4096)])


def terms64(acc, xq, wq, ox, ow):
    """(a, p1, p2, p3) of the epilogue in float64, each exact: the accumulator and the three offset products."""
    k = xq.shape[-1]
    zero = torch.zeros(1, 1, device=acc.device, dtype=torch.float64)
    oxr = zero if ox is None else torch.round(ox).double().reshape(-1, 1)
    owr = zero if ow is None else torch.round(ow).double().reshape(1, -1)
    rsw = wq.sum(dim=1, dtype=torch.int64).double()[None, :]
    rsx = xq.sum(dim=1, dtype=torch.int64).double()[:, None]
    return acc, oxr * rsw + 0 * acc, owr * rsx + 0 * acc, (k * oxr) * owr + 0 * acc


def restated_v(acc, xq, wq, ox, ow):
    """The v chain in fp32, one IEEE operation per torch op, in the order of csrc/ffq_linear.hip's tail kernel (the normative copy)."""
    k = xq.shape[-1]
    v = acc.float()
    oxr = None if ox is None else torch.round(ox.float()).reshape(-1, 1)
    if oxr is not None:
        v = v + oxr * wq.sum(dim=1, dtype=torch.int64).float()[None, :]
    if ow is not None:
        owr = torch.round(ow.float()).reshape(1, -1)
        v = v + owr * xq.sum(dim=1, dtype=torch.int64).float()[:, None]
        v = v + (float(k) * (oxr if oxr is not None else torch.zeros(1, 1, device=acc.device))) * owr
    return v


def restated_linear(acc, xq, wq, sx, ox, sw, ow, bias=None):
    """y = (sx * sw) * v (+ bias) in fp32 — the caller rounds to the output dtype with ``.to(dtype)``."""
    y = (sx.float().reshape(-1, 1) * sw.float().reshape(1, -1)) * restated_v(acc, xq, wq, ox, ow)
    return y if bias is None else y + bias.float()[None, :]


def restated_requant(y32, y_dt, out_scale, out_offset, bits, container, quantize_by_tile):
    """The requantizing epilogue: y rounded once to `y_dt`, then A1 (the A1 kernel, pinned by fixtures G1-G3) on that tensor."""
    y = y32.to(y_dt)
    return quantize_by_tile(y, out_scale, y.shape, bits, container, out_offset)


def restated_gated(gate_bf16, up32):
    """bf16(silu(gate)) * bf16(up), one bf16 rounding each — ATen's F.silu(gate) * up on the two bf16 tensors."""
    return torch.nn.functional.silu(gate_bf16) * up32.to(torch.bfloat16)


def rounding_bound(a, p1, p2, p3):
    """|v - v_exact| <= 2^-24 (|a| + 2|p1| + 2|p2| + 2|p3| + |a + p1| + |a + p1 + p2|): the half-ulps of the seven roundings of the
    chain (conversion; product and sum for each of the three terms, the third product counted twice for K * ox), each taken at
    the exact value it rounds plus the error carried so far — derived, not measured. float64 in, float64 out."""
    return 2.0**-24 * (a.abs() + 2 * p1.abs() + 2 * p2.abs() + 2 * p3.abs() + (a + p1).abs() + (a + p1 + p2).abs())


# ---- the wrong epilogues of tests/test_heavy_codes_cpu.py ---------------------------------------------------------------------------
def wrong_epilogues(a, p1, p2, p3):
    """{name: v in fp32} for the forms today's uniform-code tests cannot tell from the stated chain. `a`, `p1`, `p2`, `p3` are the
    exact float64 terms; every float64 sum below is exact (integers below 2^53), so ``.float()`` is the single rounding meant."""
    f = lambda t: t.float()  # noqa: E731
    fma = f(f(f(a).double() + p1).double() + p2)
    fma = f(fma.double() + p3)  # v = fma(ox, rsw, v) ...: the product is not rounded
    trunc = torch.where(f(a).double().abs() > a.abs(), torch.nextafter(f(a), torch.zeros_like(f(a))), f(a))  # round toward zero
    return {
        "fma_contracted": fma,
        "p1_plus_p2_first": (f(a) + (f(p1) + f(p2))) + f(p3),
        "p2_plus_p3_first": (f(a) + f(p1)) + (f(p2) + f(p3)),
        "truncating_conversion": ((trunc + f(p1)) + f(p2)) + f(p3),
        "exact_sum_rounded_once": f(a + p1 + p2 + p3),
    }


# ---- convolutions ------------------------------------------------------------------------------------------------------------------
def conv_codes(pattern: str, B, C, OC, spatial, kernel, device="cpu", seed: int = 1, transposed: bool = False):
    """(x codes [B, C, *spatial], w codes [OC, C, *kernel] or, transposed, [C, OC, *kernel]) from the linear patterns: the filter
    bank is the [OC, C * taps] weight matrix, the image the first rows of the activation matrix laid out channel-last."""
    taps = 1
    for e in kernel:
        taps *= e
    pixels = B
    for e in spatial:
        pixels *= e
    xq, wq = codes(pattern, pixels, OC, max(C * taps, TIES_SHORT), device, seed)
    xc = xq[:, :C].reshape(B, *spatial, C).movedim(-1, 1).contiguous()
    wc = wq[:, :C * taps].reshape(OC, *kernel, C).movedim(-1, 1).contiguous()
    return xc, (wc.transpose(0, 1).contiguous() if transposed else wc)


def restated_conv2d(xc, wc, sx, ox, sw, ow, bias, stride, padding, dilation=(1, 1), transposed=False, output_padding=(0, 0)):
    """(y fp32 [B, OC, OH, OW], (a, p1, p2, p3) float64) on the host. include/ffq.h: the offset terms run over the taps inside the
    image, so rsw, rsx and cnt = C * |V(p)| vary per output pixel at the border."""
    xc, wc = xc.cpu().double(), wc.cpu().double()
    B, C, H, W = xc.shape
    kh, kw = wc.shape[2:]
    OC = wc.shape[1] if transposed else wc.shape[0]
    if transposed:
        ct = lambda x, w: torch.nn.functional.conv_transpose2d(x, w, None, stride, padding, output_padding, 1, dilation)  # noqa: E731
        ones = torch.ones(B, 1, H, W, dtype=torch.float64)
        acc = ct(xc, wc)
        rsx = ct(xc, torch.ones(C, 1, kh, kw, dtype=torch.float64))
        rsw = ct(ones, wc.sum(0, keepdim=True))
        cnt = C * ct(ones, torch.ones(1, 1, kh, kw, dtype=torch.float64))
    else:
        cv = lambda x, w: torch.nn.functional.conv2d(x, w, None, stride, padding, dilation)  # noqa: E731
        ones = torch.ones(B, 1, H, W, dtype=torch.float64)
        acc = cv(xc, wc)
        rsx = cv(xc, torch.ones(1, C, kh, kw, dtype=torch.float64))
        rsw = cv(ones, wc.sum(1, keepdim=True))
        cnt = C * cv(ones, torch.ones(1, 1, kh, kw, dtype=torch.float64))
    sxf = sx.float().cpu().reshape(())
    swf = sw.float().cpu().reshape(1, -1, 1, 1)
    oxf = torch.zeros(()) if ox is None else torch.round(ox.float().cpu().reshape(()))
    owf = torch.zeros(1, 1, 1, 1) if ow is None else torch.round(ow.float().cpu()).reshape(1, -1, 1, 1)
    v = acc.float()
    v = v + oxf * rsw.float()
    v = v + owf * rsx.float()
    v = v + cnt.float() * oxf * owf
    y = (sxf * swf) * v
    if bias is not None:
        y = y + bias.float().cpu().reshape(1, OC, 1, 1)
    terms = (acc, oxf.double() * rsw, owf.double() * rsx + 0 * acc, (cnt * oxf.double()) * owf.double() + 0 * acc)
    return y, terms
