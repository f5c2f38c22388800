"""Attention operands whose right answer is known by construction: the patterns, their expectations and elementwise bounds, and the
float64 reference that tests/test_attention_exact_cpu.py and tests/test_attention_exact_gpu.py share (docs/numerics.md, "Attention on
operands with a known answer").

Every q / k value is a small integer times a power of two, exact in bf16 AND fp16, and every score product and partial sum is an integer
times a power of two below 2^24: the scores do not depend on the order of the sums. V is ``randn * 2^randint(-6, 7)`` rounded to the
dtype (magnitudes held at or above 2^-13: no subnormals) unless the pattern fixes V itself.

Patterns (all tensors in the heads layout ``q [B, H, L, E]``, ``k / v [B, HKV, S, E]``; :func:`bsd` gives the projections' layout
``[B, S, H * E]`` of ``ops.attention``):

``select``       keys are +-1 vectors (Hadamard rows where S <= E, a seeded random code otherwise), ``q_t = 8 k_pi(t)`` with a random
                 ``pi(t) <= t`` (any index without causality): row t must return ``V[pi(t)]``. Key <-> V-row pairing inside a tile, the
                 head / kv-head / batch mapping, all columns.
``staircase``    ``q_t = (a, 128 a, 0...)``, ``k_j = (j mod 128, j div 128, 0...)``: ``score(t, j) = a j`` in every row, so under the
                 causal mask row t must return ``V[min(t, S - 1)]`` (a key leaking from above gives ``V[t + 1]``, a mask one too
                 strict ``V[t - 1]`` — in EVERY row) and without it ``V[S - 1]``. The unused columns carry noise where the other
                 operand is zero.
``uniform``      ``q = 0`` and V an indicator (variant 0: ``c == j mod E``; variant 1: ``c == j div G``): ``out[t, c] = count /
                 n_visible(t)`` with exact small integers — one dropped or double-counted key moves a count of at most 16 by one.
``mask_select``  (SDPA) ``q = 0`` and a float mask that is 0 at ``pi(t)`` and -64 elsewhere: row t must return ``V[pi(t)]``.
``rotated``      a ``select`` / ``staircase`` whose q is handed in rotated BACKWARDS by rotary tables that are the identity on some rows
                 and the quarter turn (cos 0, sin 1: ``(x1, x2) -> (-x2, x1)``, exact) on the others.

Bounds — derived, none measured:

* one-hot patterns: ``|got - V[target]| <= 2^-7 |V[target]| + 2 r max|V|`` in bf16 (the target's un-normalised p is 2^eps with eps from
  the rounding of the running maximum; bf16(p) / p is within 2^-8 of 1 and the output rounding adds another 2^-8), 2^-10 in place of
  2^-7 in fp16. r is the probability mass outside the target in float64; a pattern is refused (AssertionError) unless
  ``r <= 2^-24``: a condition on the inputs, checked before any kernel runs.
* ``uniform``: one ulp of the output dtype from ``count / n`` rounded to that dtype (the kernels multiply by 1 / l).
* with the weights quantizer (8 bits, scale 2^-8, offset 128) P = 1 becomes 255 / 256 and a probability below 2^-9 becomes 0, so a
  one-hot pattern must equal the dtype's rounding of ``(255 / 256) V[target]`` bit for bit, and a ``uniform`` row is
  ``min(rne(256 / n), 255) * count / 256`` rounded once (one ulp allowed): :func:`weights_quantized`.
"""

from __future__ import annotations

import dataclasses
import functools
import math
import zlib

from typing import Any

import torch

MANTISSA = {torch.bfloat16: 7, torch.float16: 10}  # explicit mantissa bits
RESIDUAL_LIMIT = 2.0**-24
STAIR_A = 256  # at the default scales adjacent staircase scores are 22.6 (E = 128) or 32 (E = 64) apart: r <= 1.6e-10
GAIN = 8  # of the select query: the target's score is 8 E / sqrt(E) above 0, off-target scores are 8 |k_i . k_j| / sqrt(E)
MASK_OFF = -64.0  # exp(-64) = 1.6e-28
KEEP = 0.7  # of the random bool mask
WEIGHTS_QUANTIZER = (8, 2.0**-8, 128.0)  # bits, scale, offset


@dataclasses.dataclass(frozen=True)
class Shape:
    B: int
    H: int
    HKV: int
    L: int
    S: int
    E: int

    def __str__(self) -> str:
        return f"B={self.B} H={self.H} HKV={self.HKV} L={self.L} S={self.S} E={self.E}"


def llama(B: int, S: int, H: int, HKV: int) -> Shape:
    """A shape of ``ops.attention``: L = S, head_dim 128."""
    return Shape(B, H, HKV, S, S, 128)


@dataclasses.dataclass(frozen=True)
class Pattern:
    name: str
    kind: str  # "onehot" or "uniform"
    shape: Shape
    dtype: torch.dtype
    q: torch.Tensor  # [B, H, L, E] — what the kernel must contract (after its rotation, if any)
    k: torch.Tensor  # [B, HKV, S, E]
    v: torch.Tensor  # [B, HKV, S, E]
    causal: bool
    mask: torch.Tensor | None  # as handed to the call: bool or float, leading dims not broadcast
    scale: float | None
    expected: torch.Tensor  # float64 [B, H, L, E]
    bound: torch.Tensor  # float64 [B, H, L, E]
    target: torch.Tensor | None = None  # one-hot: int64 [B, H, L], the key each row must return
    residual: float = 0.0  # one-hot: the largest probability mass outside a row's target
    visible: torch.Tensor | None = None  # uniform: bool [B, H, L, S]
    rope: tuple[torch.Tensor, torch.Tensor] | None = None  # rotated: (cos, sin), [S, E] each in dtype
    q_in: torch.Tensor | None = None  # rotated: the q to hand in ([B, H, L, E])
    turned: torch.Tensor | None = None  # rotated: bool [S], the rows on the quarter turn

    def __str__(self) -> str:
        mask = "causal" if self.causal else "none" if self.mask is None else f"{str(self.mask.dtype).removeprefix('torch.')}{tuple(self.mask.shape)}"
        return f"{self.name} {self.shape} {str(self.dtype).removeprefix('torch.')} mask={mask}"


# ---- layouts ---------------------------------------------------------------------------------------------------------------------
def bsd(x: torch.Tensor) -> torch.Tensor:
    """[B, H, L, E] -> the projections' layout [B, L, H * E], contiguous."""
    B, H, L, E = x.shape
    return x.transpose(1, 2).reshape(B, L, H * E).contiguous()


def heads(x: torch.Tensor, head_dim: int) -> torch.Tensor:
    """[B, L, H * E] -> [B, H, L, E]."""
    B, L, HE = x.shape
    return x.reshape(B, L, HE // head_dim, head_dim).transpose(1, 2)


# ---- the float64 reference -----------------------------------------------------------------------------------------------------------
def softmax64(scores: torch.Tensor, visible: torch.Tensor | None = None, weight: torch.Tensor | None = None) -> torch.Tensor:
    """The safe softmax over the last dim in float64: a row without a visible key (or with -inf everywhere) gives zeros. `weight`
    multiplies each key's un-normalised probability (a key counted twice has weight 2)."""
    if visible is not None:
        scores = scores.masked_fill(~visible, -math.inf)
    m = scores.amax(-1, keepdim=True)
    e = torch.exp(scores - torch.where(torch.isinf(m), torch.zeros_like(m), m))
    if weight is not None:
        e = e * weight
    total = e.sum(-1, keepdim=True)
    return torch.where(total > 0, e / torch.where(total > 0, total, torch.ones_like(total)), torch.zeros_like(e))


def reference64(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, head_dim: int | None = None, causal: bool = False,
                mask: torch.Tensor | None = None, scale: float | None = None, probabilities: bool = False) -> torch.Tensor:
    """Plain softmax attention in float64 on the operands as given. 4-D operands are ``[B, H, L, E]`` / ``[B, HKV, S, E]``; 3-D ones
    the projections ``[B, S, H * head_dim]`` (the result comes back in the same layout). Causality is top-left (row t sees keys
    <= t); a bool mask keeps where True, a float mask is added; both broadcast over their leading dims; kv heads repeat by
    ``repeat_interleave``. `probabilities`: return P ``[B, H, L, S]`` instead of P V."""
    flat = q.dim() == 3
    if flat:
        assert head_dim is not None
        q, k, v = heads(q, head_dim), heads(k, head_dim), heads(v, head_dim)
    q, k, v = q.double().cpu(), k.double().cpu(), v.double().cpu()
    groups = q.shape[1] // k.shape[1]
    k, v = k.repeat_interleave(groups, 1), v.repeat_interleave(groups, 1)
    L, S, E = q.shape[-2], k.shape[-2], q.shape[-1]
    scores = q @ k.transpose(-1, -2) * (1.0 / math.sqrt(E) if scale is None else scale)
    visible = torch.ones(L, S, dtype=torch.bool)
    if causal:
        visible = visible.tril()
    if mask is not None:
        mask = mask.cpu()
        if mask.dtype == torch.bool:
            visible = visible & mask
        else:
            scores = scores + mask.double()
    p = softmax64(scores, visible)
    if probabilities:
        return p
    out = p @ v
    return bsd(out) if flat else out


# ---- pieces --------------------------------------------------------------------------------------------------------------------------
def generator(*key: Any) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def hadamard(n: int) -> torch.Tensor:
    """Sylvester's n x n matrix of +-1 (n a power of two): orthogonal rows."""
    h = torch.ones(1, 1, dtype=torch.float64)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    assert h.shape[0] == n
    return h


def random_v(shape: tuple[int, ...], dtype: torch.dtype, gen: torch.Generator) -> torch.Tensor:
    """randn * 2^randint(-6, 7) in `dtype`: twelve binades and more, no subnormals (|v| >= 2^-13)."""
    v = torch.randn(shape, generator=gen, dtype=torch.float64) * torch.exp2(torch.randint(-6, 7, shape, generator=gen).double())
    v = torch.where(v < 0, -1.0, 1.0) * v.abs().clamp_min(2.0**-13)
    return v.to(torch.float32).to(dtype)


def ulp(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """The spacing of `dtype` at |x| (float64 in, float64 out); 0 at 0."""
    _, e = torch.frexp(x.abs())
    return torch.where(x == 0, torch.zeros_like(x), torch.ldexp(torch.ones_like(x), e - 1 - MANTISSA[dtype]))


def rounded(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """float64 -> dtype -> float64. The values handed in are exact in fp32, or far from a tie of `dtype` (count / n is at least
    1 / (n 2^9) away from one, relatively): the step through fp32 rounds nothing that matters."""
    return x.to(torch.float32).to(dtype).double()


def _visible(shape: Shape, causal: bool, mask: torch.Tensor | None) -> torch.Tensor:
    vis = torch.ones(shape.L, shape.S, dtype=torch.bool)
    if causal:
        vis = vis.tril()
    if mask is not None:
        vis = vis & mask
    return vis.expand(shape.B, shape.H, shape.L, shape.S)


def _onehot(name: str, shape: Shape, dtype: torch.dtype, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, target: torch.Tensor,
            causal: bool = False, mask: torch.Tensor | None = None, scale: float | None = None) -> Pattern:
    """Expectation, residual and bound of a pattern whose row t must return V[target[t]]; refuses inputs with r > 2^-24."""
    q, k = q.to(dtype), k.to(dtype)
    p = reference64(q, k, v, causal=causal, mask=mask, scale=scale, probabilities=True)
    r = p.scatter(-1, target.unsqueeze(-1), 0.0).sum(-1)  # the mass outside the target, without cancellation
    assert float(r.max()) <= RESIDUAL_LIMIT, f"{name} {shape}: residual {float(r.max()):.3e} > 2^-24"
    groups = shape.H // shape.HKV
    expected = v.double().repeat_interleave(groups, 1).gather(2, target.unsqueeze(-1).expand(-1, -1, -1, shape.E))
    bound = 2.0 ** -MANTISSA[dtype] * expected.abs() + 2.0 * r.unsqueeze(-1) * float(v.double().abs().max())
    return Pattern(name, "onehot", shape, dtype, q, k, v, causal, mask, scale, expected, bound, target=target, residual=float(r.max()))


# ---- the patterns ----------------------------------------------------------------------------------------------------------------------
def select(shape: Shape, dtype: torch.dtype = torch.bfloat16, causal: bool = True, seed: int = 0) -> Pattern:
    B, H, HKV, L, S, E = dataclasses.astuple(shape)
    gen = generator("select", dataclasses.astuple(shape), str(dtype), causal, seed)
    if S <= E:  # rows of the Hadamard matrix: a seeded choice of rows and column signs per (batch, kv head)
        had = hadamard(E)
        rows = torch.stack([torch.randperm(E, generator=gen)[:S] for _ in range(B * HKV)]).reshape(B, HKV, S)
        signs = torch.randint(0, 2, (B, HKV, 1, E), generator=gen).double() * 2 - 1
        k = had[rows] * signs
    else:
        k = torch.randint(0, 2, (B, HKV, S, E), generator=gen).double() * 2 - 1
    v = random_v((B, HKV, S, E), dtype, gen)
    if causal:
        seen = (torch.arange(L).clamp(max=S - 1) + 1).double()  # row t sees keys 0 .. min(t, S - 1)
        target = (torch.rand(B, H, L, generator=gen, dtype=torch.float64) * seen).floor().long().clamp(max=S - 1)
    else:
        target = torch.randint(0, S, (B, H, L), generator=gen)
    q = GAIN * k.repeat_interleave(H // HKV, 1).gather(2, target.unsqueeze(-1).expand(-1, -1, -1, E))
    return _onehot("select", shape, dtype, q, k, v, target, causal=causal)


def staircase(shape: Shape, dtype: torch.dtype = torch.bfloat16, causal: bool = True, seed: int = 0, a: int = STAIR_A,
              scale: float | None = None) -> Pattern:
    B, H, HKV, L, S, E = dataclasses.astuple(shape)
    assert S <= 128 * 128 and 128 * a <= 32768
    gen = generator("staircase", dataclasses.astuple(shape), str(dtype), causal, seed)
    j = torch.arange(S)
    q = torch.zeros(B, H, L, E, dtype=torch.float64)
    k = torch.zeros(B, HKV, S, E, dtype=torch.float64)
    q[..., 0], q[..., 1] = a, 128 * a
    k[..., 0], k[..., 1] = (j % 128).double(), (j // 128).double()
    # noise on the unused columns: each column belongs to q or to k, the other operand is zero there (the products vanish exactly)
    owner = torch.randint(0, 2, (E - 2,), generator=gen).bool()
    q[..., 2:] = torch.randint(-8, 9, (B, H, L, E - 2), generator=gen).double() * owner
    k[..., 2:] = torch.randint(-8, 9, (B, HKV, S, E - 2), generator=gen).double() * ~owner
    v = random_v((B, HKV, S, E), dtype, gen)
    target = (torch.arange(L).clamp(max=S - 1) if causal else torch.full((L,), S - 1)).expand(B, H, L).contiguous()
    return _onehot("staircase", shape, dtype, q, k, v, target, causal=causal, scale=scale)


def indicator_group(shape: Shape) -> int:
    """G of the second uniform variant: 16 keys per column wherever that fits."""
    return 16 if shape.S <= 16 * shape.E else -(-shape.S // shape.E)


def uniform(shape: Shape, dtype: torch.dtype = torch.bfloat16, variant: int = 0, causal: bool = False, mask: torch.Tensor | None = None,
            seed: int = 0) -> Pattern:
    B, H, HKV, L, S, E = dataclasses.astuple(shape)
    assert mask is None or (mask.dtype == torch.bool and not causal)
    gen = generator("uniform", dataclasses.astuple(shape), str(dtype), variant, causal, seed)
    q = torch.zeros(B, H, L, E, dtype=dtype)
    k = (torch.randint(-16, 17, (B, HKV, S, E), generator=gen).double() * 2.0**-2).to(dtype)
    j = torch.arange(S)
    column = j % E if variant == 0 else j // indicator_group(shape)
    v = torch.zeros(B, HKV, S, E, dtype=torch.float64)
    v[:, :, j, column] = 1.0
    v = v.to(dtype)
    visible = _visible(shape, causal, mask)
    n = visible.sum(-1, keepdim=True).double()
    count = visible.double() @ v[0, 0].double()
    expected = rounded(torch.where(n > 0, count / n.clamp_min(1.0), torch.zeros_like(count)), dtype)
    return Pattern(f"uniform{variant}", "uniform", shape, dtype, q, k, v, causal, mask, None, expected, ulp(expected, dtype), visible=visible)


MASK_LEADS = ("LS", "1HLS", "B1LS")


def _lead(shape: Shape, lead: str) -> tuple[int, ...]:
    return {"LS": (), "1HLS": (1, shape.H), "B1LS": (shape.B, 1)}[lead]


def mask_select(shape: Shape, dtype: torch.dtype = torch.bfloat16, lead: str = "LS", mask_dtype: torch.dtype | None = None, seed: int = 0) -> Pattern:
    """q = 0 and a float mask 0 at pi(t), -64 elsewhere; pi differs along every leading dim the mask has."""
    B, H, HKV, L, S, E = dataclasses.astuple(shape)
    gen = generator("mask_select", dataclasses.astuple(shape), str(dtype), lead, seed)
    q = torch.zeros(B, H, L, E, dtype=dtype)
    k = (torch.randint(-16, 17, (B, HKV, S, E), generator=gen).double() * 2.0**-2).to(dtype)
    v = random_v((B, HKV, S, E), dtype, gen)
    pi = torch.randint(0, S, (*_lead(shape, lead), L), generator=gen)
    mask = torch.full((*pi.shape, S), MASK_OFF, dtype=torch.float64).scatter(-1, pi.unsqueeze(-1), 0.0).to(mask_dtype or dtype)
    return _onehot(f"mask_select[{lead}]", shape, dtype, q, k, v, pi.expand(B, H, L).contiguous(), mask=mask)


def bool_mask(shape: Shape, lead: str = "LS", seed: int = 0) -> torch.Tensor:
    """A random bool mask (keep probability 0.7) with two fully masked rows (L // 3 and L - 1) where L >= 3."""
    gen = generator("bool_mask", dataclasses.astuple(shape), lead, seed)
    mask = torch.rand((*_lead(shape, lead), shape.L, shape.S), generator=gen) < KEEP
    if shape.L >= 3:
        mask[..., shape.L // 3, :] = False
        mask[..., shape.L - 1, :] = False
    return mask


def masked_uniform(shape: Shape, dtype: torch.dtype = torch.bfloat16, variant: int = 0, lead: str = "LS", seed: int = 0) -> Pattern:
    p = uniform(shape, dtype, variant, mask=bool_mask(shape, lead, seed), seed=seed)
    return dataclasses.replace(p, name=f"uniform{variant}[bool {lead}]")


def rotate(q: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """The rotary embedding q cos + rotate_half(q) sin on [B, H, S, E] with [S, E] tables, in float64."""
    half = q.shape[-1] // 2
    q = q.double()
    return q * cos.double() + torch.cat([-q[..., half:], q[..., :half]], -1) * sin.double()


def rotated(base: Pattern, seed: int = 0) -> Pattern:
    """`base` (a select or staircase of ops.attention) with q handed in rotated backwards: tables that are the identity (cos 1,
    sin 0) on some rows and the quarter turn (cos 0, sin 1) on the others, the choice seeded and not periodic in 32."""
    S, E = base.shape.S, base.shape.E
    assert base.shape.L == S
    turned = torch.rand(S, generator=generator("rotated", base.name, dataclasses.astuple(base.shape), seed)) < 0.5
    assert bool((turned != turned[torch.arange(S) % 32]).any()), "the choice of rows is periodic in 32"
    cos = (~turned).double().unsqueeze(-1).expand(S, E).contiguous().to(base.dtype)
    sin = turned.double().unsqueeze(-1).expand(S, E).contiguous().to(base.dtype)
    half = E // 2
    q = base.q.double()
    back = torch.cat([q[..., half:], -q[..., :half]], -1)  # the quarter turn sends (x1, x2) to (-x2, x1): this to q
    q_in = torch.where(turned.reshape(1, 1, S, 1), back, q).to(base.dtype)
    assert torch.equal(rotate(q_in, cos, sin), q)
    return dataclasses.replace(base, name=f"rotated {base.name}", rope=(cos, sin), q_in=q_in, turned=turned)


# ---- with the weights quantizer ------------------------------------------------------------------------------------------------------
def weights_quantized(p: Pattern) -> tuple[torch.Tensor, torch.Tensor]:
    """(expected, bound) of `p` under the weights quantizer (8 bits, 2^-8, 128) alone: probability codes in [0, 255] times 2^-8."""
    if p.kind == "onehot":
        return rounded(p.expected * (255.0 / 256.0), p.dtype), torch.zeros_like(p.expected)  # 16 / 19 bits: exact before the rounding
    assert p.visible is not None
    n = p.visible.sum(-1, keepdim=True).double()
    code = torch.where(n > 0, torch.round(256.0 / n.clamp_min(1.0)).clamp(max=255.0), torch.zeros_like(n))  # torch.round: halves to even
    count = p.visible.double() @ p.v[0, 0].double()
    expected = rounded(code * count / 256.0, p.dtype)
    return expected, ulp(expected, p.dtype)


# ---- judging a result ----------------------------------------------------------------------------------------------------------------
def failures(got: torch.Tensor, expected: torch.Tensor, bound: torch.Tensor) -> torch.Tensor:
    """bool [B, H, L, E]: outside the bound, or not a number."""
    got = got.detach().cpu().double()
    return ~((got - expected).abs() <= bound)


def explain(p: Pattern, got: torch.Tensor, expected: torch.Tensor | None = None, bound: torch.Tensor | None = None) -> str | None:
    """None when `got` ([B, H, L, E]) meets the expectation; else the first failing (batch, head, row) and, for a one-hot pattern,
    which V row the output actually matches."""
    expected = p.expected if expected is None else expected
    bound = p.bound if bound is None else bound
    got = got.detach().cpu().double()
    if got.shape != expected.shape:
        return f"{p}: shape {tuple(got.shape)} against {tuple(expected.shape)}"
    bad = failures(got, expected, bound)
    if not bool(bad.any()):
        return None
    b, h, t, c = (int(i) for i in bad.nonzero()[0])
    rows = int(bad.any(-1).sum())
    text = (f"{p}: {rows} of {bad.shape[0] * bad.shape[1] * bad.shape[2]} rows fail, first at (batch {b}, head {h}, row {t}) column {c}: "
            f"got {got[b, h, t, c].item()!r}, expected {expected[b, h, t, c].item()!r} +- {bound[b, h, t, c].item():.3e}")
    if p.kind == "onehot":
        assert p.target is not None
        every = p.v.double().reshape(-1, p.shape.E)
        factor = float((expected[b, h, t].abs().sum() / p.expected[b, h, t].abs().sum()))  # 255 / 256 under the weights quantizer
        distance = (every * factor - got[b, h, t]).abs().amax(-1)
        at = int(distance.argmin())
        vb, vh, vj = at // (p.shape.HKV * p.shape.S), at // p.shape.S % p.shape.HKV, at % p.shape.S
        text += (f"; the row should be V[batch {b}, kv head {h // (p.shape.H // p.shape.HKV)}, key {int(p.target[b, h, t])}] and is closest to "
                 f"V[batch {vb}, kv head {vh}, key {vj}] (max distance {float(distance[at]):.3e})")
    else:
        text += f"; the row sees {int(p.visible[b, h, t].sum())} keys"
    return text


# ---- the cases both test files run -----------------------------------------------------------------------------------------------------
ATTENTION_SHAPES = ((1, 64, 1, 1), (2, 128, 4, 2), (1, 192, 2, 2), (1, 256, 8, 1), (1, 320, 4, 1), (3, 576, 4, 4), (1, 832, 8, 2))  # (B, S, H, HKV)
ROTATED_SHAPES = ((2, 128, 4, 2), (1, 832, 8, 2))
QUANTIZED_SHAPES = ((2, 128, 4, 2), (3, 576, 4, 4))  # with the fused o_proj input quantizer
# (the last pair puts all four waves of a query block past the first on their diagonal tiles, with keys beyond them and rows beyond S)
SDPA_LS = ((1, 1), (1, 65), (31, 31), (33, 127), (64, 64), (65, 129), (127, 33), (129, 129), (257, 191), (130, 300), (384, 320))
SDPA_KINDS = ("none", "causal", "float", "bool")
SDPA_DTYPES = (torch.bfloat16, torch.float16)


# Staircases under an explicit softmax scale, (a, scale): the step a * scale is 32 on both, so the residual rule holds; with the first
# a kernel that applies the scale twice has a step of 4 (under the default 1 / sqrt(128) it would still pass), with the second a kernel
# that ignores the scale has a step of 1.4 (applied twice it would still pass). Together they pin the scale from both sides.
SCALED_STAIRS = ((256, 2.0**-3), (16, 2.0))
SCALED_ATTENTION_SHAPE = (1, 320, 4, 1)  # (B, S, H, HKV)
SCALED_SDPA_SHAPE = Shape(2, 4, 2, 130, 300, 128)


@functools.lru_cache(maxsize=None)
def scaled_patterns(shape: Shape, dtype: torch.dtype, causal: bool) -> tuple[Pattern, ...]:
    return tuple(dataclasses.replace(staircase(shape, dtype, causal, a=a, scale=scale), name=f"staircase[a={a}, scale={scale}]")
                 for a, scale in SCALED_STAIRS)


@functools.lru_cache(maxsize=None)
def attention_patterns(B: int, S: int, H: int, HKV: int, causal: bool) -> tuple[Pattern, ...]:
    """select, staircase and both uniform variants of one ``ops.attention`` shape (built once: both test files read the same
    objects, unchanged)."""
    shape = llama(B, S, H, HKV)
    return (select(shape, causal=causal), staircase(shape, causal=causal), uniform(shape, variant=0, causal=causal),
            uniform(shape, variant=1, causal=causal))


@functools.lru_cache(maxsize=None)
def rotated_patterns(B: int, S: int, H: int, HKV: int, causal: bool) -> tuple[Pattern, ...]:
    sel, stair = attention_patterns(B, S, H, HKV, causal)[:2]
    return rotated(sel), rotated(stair)


@functools.lru_cache(maxsize=None)
def sdpa_patterns(L: int, S: int, kind: str, dtype: torch.dtype) -> tuple[Pattern, ...]:
    """The named SDPA case ``(L, S) x mask kind x dtype``: 2 batches, 4 query heads on 2 kv heads; E, the mask's leading dims, its
    dtype and the uniform variant rotate with the case's position in the table, so every value of each meets both dtypes."""
    at = SDPA_LS.index((L, S)) + SDPA_KINDS.index(kind) + SDPA_DTYPES.index(dtype)
    shape = Shape(2, 4, 2, L, S, (64, 128)[at % 2])
    lead = MASK_LEADS[(SDPA_LS.index((L, S)) + SDPA_DTYPES.index(dtype)) % 3]
    if kind in ("none", "causal"):
        causal = kind == "causal"
        return (select(shape, dtype, causal), staircase(shape, dtype, causal), uniform(shape, dtype, (at // 2) % 2, causal))
    if kind == "float":
        return (mask_select(shape, dtype, lead, mask_dtype=(None, torch.float32)[(at // 2) % 2]),)
    return (masked_uniform(shape, dtype, 0, lead), masked_uniform(shape, dtype, 1, lead))


def first_mismatch(got: torch.Tensor, want: torch.Tensor) -> str:
    if got.shape != want.shape:
        return f"shape {tuple(got.shape)} against {tuple(want.shape)}"
    differ = (got != want).nonzero()
    if differ.numel() == 0:
        return "no element differs"
    at = tuple(int(i) for i in differ[0])
    return f"{differ.shape[0]} of {want.numel()} differ, first at {at}: {got[at].item()!r} against {want[at].item()!r}"
