"""The patterns of tests/attention_exact.py earn their place — conditions on the inputs, not on a kernel.

* Every pattern of every shape the GPU file runs meets the residual rule (r <= 2^-24: the constructors refuse anything else), is
  deterministic, and its expectation equals ``reference64`` within its bound.
* Wrong forms: a float64 attention with one hook per indexing mistake a kernel rewrite can make (``FORMS``). Each must push at least
  one named pattern out of its bound.
* Second implementation: the oracle's ``ops.attention`` (the reference's bf16 eager chain) and the CPU math path
  (``scaled_dot_product_attention_math``, fp32 after the upcast) meet the same expectations wherever their rounding can resolve the
  pattern. What the bf16 chain cannot resolve, and is therefore held against ``reference64`` alone (the first test below):

  - ``staircase`` at every shape: the chain rounds the score 256 j and then its product with 1 / sqrt(128) to bf16, 8 significant
    bits; beyond j = 45 (scores above 1024, spacing 8 and more against a step of 22.6) neighbouring keys collapse or come within a
    few units, and the bound's r (1.5e-10 in float64) no longer describes the row.

  ``select`` and ``uniform`` are resolved by the chain at every shape and held to the patterns' own bounds. The oracle is a scalar
  loop, so of the two largest shapes, (3, 576, 4, 4) and (1, 832, 8, 2), it runs the causal form only; their full form is omitted for
  time, not for rounding, and is held against ``reference64`` alone.

  The fp32 math path resolves every pattern: staircase scores reach 2^19 / 8, where fp32 rounds by 2^-8 and less against a step of 22.6.
"""

import dataclasses

import pytest
import torch

import attention_exact as ax

from fastforward_amd import ops
from fastforward_amd.nn.sdpa import scaled_dot_product_attention_math

LLAMA_CASES = [(*shape, causal) for shape in ax.ATTENTION_SHAPES for causal in (True, False)]
SDPA_CASES = [(L, S, kind) for (L, S) in ax.SDPA_LS for kind in ax.SDPA_KINDS]


def reference(p: ax.Pattern) -> torch.Tensor:
    return ax.reference64(p.q, p.k, p.v, causal=p.causal, mask=p.mask, scale=p.scale)


# ---- the inputs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,H,HKV,causal", LLAMA_CASES)
def test_llama_patterns_meet_the_residual_rule_and_reference64(B, S, H, HKV, causal):
    for p in ax.attention_patterns(B, S, H, HKV, causal):  # (a residual above 2^-24 raises inside the constructor)
        assert p.residual <= ax.RESIDUAL_LIMIT
        assert ax.explain(p, reference(p)) is None, ax.explain(p, reference(p))
        # the projections' layout of reference64 says the same
        flat = ax.reference64(ax.bsd(p.q), ax.bsd(p.k), ax.bsd(p.v), head_dim=128, causal=p.causal)
        assert torch.equal(ax.heads(flat, 128), reference(p))


@pytest.mark.parametrize("L,S,kind", SDPA_CASES)
def test_sdpa_patterns_meet_the_residual_rule_and_reference64(L, S, kind):
    for dtype in ax.SDPA_DTYPES:
        for p in ax.sdpa_patterns(L, S, kind, dtype):
            assert p.residual <= ax.RESIDUAL_LIMIT
            assert ax.explain(p, reference(p)) is None, ax.explain(p, reference(p))
            assert all(t.dtype == dtype for t in (p.q, p.k, p.v))


@pytest.mark.parametrize("B,S,H,HKV", ax.ROTATED_SHAPES)
def test_rotated_patterns_turn_back_into_their_base(B, S, H, HKV):
    for causal in (True, False):
        for p, base in zip(ax.rotated_patterns(B, S, H, HKV, causal), ax.attention_patterns(B, S, H, HKV, causal)):
            cos, sin = p.rope
            assert torch.equal(ax.rotate(p.q_in, cos, sin), base.q.double()) and torch.equal(p.expected, base.expected)
            # both kinds of rows occur, within the first 32 rows and beyond, and row t's choice is not row (t mod 32)'s
            assert 0 < int(p.turned[:32].sum()) < 32 and bool((p.turned != p.turned[torch.arange(S) % 32]).any())
            assert not torch.equal(p.q_in, base.q)


def test_patterns_are_deterministic_and_exact_in_both_dtypes():
    shape = ax.Shape(2, 4, 2, 65, 129, 64)
    builders = (lambda dt: ax.select(shape, dt, True), lambda dt: ax.staircase(shape, dt, False), lambda dt: ax.uniform(shape, dt, 1, True),
                lambda dt: ax.mask_select(shape, dt, "B1LS"), lambda dt: ax.masked_uniform(shape, dt, 0, "1HLS"))
    for build in builders:
        a, b = build(torch.bfloat16), build(torch.bfloat16)
        for f in dataclasses.fields(a):
            x, y = getattr(a, f.name), getattr(b, f.name)
            assert torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y, (a.name, f.name)
        for p in (a, build(torch.float16)):  # (the draw is seeded per dtype) q, k and a float mask are exact in bf16 AND fp16
            for x in (p.q, p.k, *([p.mask] if p.mask is not None and p.mask.dtype != torch.bool else [])):
                assert torch.equal(x.double(), x.bfloat16().double()) and torch.equal(x.double(), x.half().double()), p.name
            assert p.kind == "uniform" or 2.0**-13 <= float(p.v.double().abs().min()) <= float(p.v.double().abs().max()) < 2.0**10
    other = ax.select(shape, torch.bfloat16, True, seed=1)
    assert not torch.equal(other.target, ax.select(shape, torch.bfloat16, True).target)


def test_scores_are_integers_below_2_to_24():
    """Every product and partial sum of q . k is an integer (times 2^-2 for the noise keys of q = 0 patterns, which contribute
    nothing) below 2^24: fp32 adds them exactly in any order."""
    for p in (*ax.attention_patterns(1, 832, 8, 2, True)[:2], *ax.sdpa_patterns(130, 300, "none", torch.float16)[:2]):
        q, k = p.q.double(), p.k.double().repeat_interleave(p.shape.H // p.shape.HKV, 1)
        assert torch.equal(q, q.round()) and torch.equal(k, k.round())
        assert float((q.abs() @ k.abs().transpose(-1, -2)).max()) < 2.0**24, str(p)


def test_uniform_variants_identify_every_key():
    """(j mod E, j div G) is a different pair for every key: a key that goes missing or comes twice shows in a known column of each."""
    for shape in (ax.llama(1, 832, 8, 2), ax.Shape(2, 4, 2, 130, 300, 64)):
        j = torch.arange(shape.S)
        pairs = {(int(a), int(b)) for a, b in zip(j % shape.E, j // ax.indicator_group(shape))}
        assert len(pairs) == shape.S and int((j // ax.indicator_group(shape)).max()) < shape.E
        for variant in (0, 1):
            p = ax.uniform(shape, variant=variant)
            assert float(p.v.double().sum(-2).max()) <= 16  # counts of at most 16: one key is a relative 1 / 16 and more


def test_weights_quantizer_expectations():
    """255 / 256 of the target for a one-hot row; min(rne(256 / n), 255) / 256 per visible key for a uniform one (n = 1 clamps)."""
    p = ax.staircase(ax.Shape(1, 2, 1, 5, 5, 64), torch.float16, True)
    expected, bound = ax.weights_quantized(p)
    assert float(bound.max()) == 0.0 and torch.equal(expected, (p.expected.float() * (255.0 / 256.0)).half().double())
    u = ax.uniform(ax.Shape(1, 1, 1, 6, 6, 64), torch.bfloat16, 0, True)
    expected, bound = ax.weights_quantized(u)
    codes = [255, 128, 85, 64, 51, 43]  # rne(256 / n), clamped
    for t, code in enumerate(codes):
        assert torch.equal(expected[0, 0, t, : t + 1], torch.full((t + 1,), code / 256.0, dtype=torch.float64).bfloat16().double())
        assert float(expected[0, 0, t, t + 1:].abs().max()) == 0.0


# ---- the wrong forms -------------------------------------------------------------------------------------------------------------------
def mask_as_read(p: ax.Pattern, wrong_strides: bool) -> torch.Tensor:
    """The mask as [B, H, L, S]. `wrong_strides`: indexed with the strides its own (unbroadcast) shape has in memory instead of 0
    along the broadcast dims — head h of batch b then reads the slab of (b, h) as if every (batch, head) had one; the emulation
    wraps at the end of the storage, where the kernel would read past it."""
    sh = p.shape
    m4 = p.mask.reshape((1,) * (4 - p.mask.dim()) + tuple(p.mask.shape))
    if not wrong_strides:
        return m4.expand(sh.B, sh.H, sh.L, sh.S)
    flat = m4.contiguous().flatten()
    b, h, t, j = torch.meshgrid(torch.arange(sh.B), torch.arange(sh.H), torch.arange(sh.L), torch.arange(sh.S), indexing="ij")
    slab = sh.L * sh.S
    return flat[(b * m4.shape[1] * slab + h * slab + t * sh.S + j) % flat.numel()]


def middle_key(p: ax.Pattern) -> int:
    """Key 17 of the middle 64-key tile."""
    tiles = -(-p.shape.S // 64)
    return min(64 * (tiles // 2) + 17, p.shape.S - 1)


def attend(p: ax.Pattern, form: str | None = None) -> torch.Tensor:
    """Float64 attention on the operands of `p` as a kernel gets them, with the mistake `form` built in (None: none)."""
    sh = p.shape
    B, H, HKV, L, S, E = dataclasses.astuple(sh)
    groups = H // HKV
    q = p.q.double()
    if p.rope is not None:
        rows = torch.arange(S) % 32 if form == "rotary table row modulo 32" else torch.arange(S)
        q = ax.rotate(p.q_in, p.rope[0][rows], p.rope[1][rows])
    head_map = torch.arange(H) % HKV if form == "kv head h mod HKV" else torch.arange(H) // groups
    k, v = p.k.double()[:, head_map], p.v.double()[:, head_map]
    if form == "batch b reads batch 0":
        k, v = k[:1].expand(B, -1, -1, -1), v[:1].expand(B, -1, -1, -1)
    t, j = torch.arange(L).unsqueeze(-1), torch.arange(S).unsqueeze(0)
    visible = (j <= t) if p.causal else torch.ones(L, S, dtype=torch.bool)
    bias = torch.zeros(1, dtype=torch.float64)
    if p.mask is not None:
        m = mask_as_read(p, form == "mask strides of the unbroadcast shape")
        if m.dtype == torch.bool:
            visible = visible & m
        else:
            bias = m.double()
    visible = visible.expand(B, H, L, S).clone()
    weight = torch.ones(S, dtype=torch.float64)
    j0 = middle_key(p)
    if form == "row t also sees key t + 1":
        visible |= j == t + 1
    elif form == "row t misses key t":
        visible &= j != t
    elif form == "one key of a middle tile dropped":
        visible[..., j0] = False
    elif form == "one key counted twice":
        weight[j0] = 2.0
    elif form == "two V rows of one tile swapped":
        order = torch.arange(S)
        order[j0], order[j0 ^ 1] = j0 ^ 1, j0
        v = v[:, :, order]
    elif form == "last tile skipped for a partial last query block":
        assert L == S and S % 256
        visible[:, :, 256 * (L // 256):, S - 64:] = False
    elif form == "key bound S + 1":  # the key past the end is staged as zeros: score 0, value 0 — and counted
        k, v = (torch.cat([x, torch.zeros(B, H, 1, E, dtype=torch.float64)], 2) for x in (k, v))
        beyond = (t >= S) if p.causal else torch.ones(L, 1, dtype=torch.bool)
        visible = torch.cat([visible, beyond.expand(B, H, L, 1)], -1)
        weight = torch.cat([weight, torch.ones(1, dtype=torch.float64)])
        assert p.mask is None
    else:
        assert form is None or form in FORMS, form
    scale = E**-0.5 if p.scale is None else p.scale
    if form == "softmax scale ignored":
        scale = E**-0.5
    elif form == "softmax scale applied twice":
        scale = scale * scale
    scores = q @ k.transpose(-1, -2) * scale + bias
    return ax.softmax64(scores, visible, weight) @ v


def _candidates() -> dict[str, ax.Pattern]:
    sel, stair, uni0, uni1 = ax.attention_patterns(1, 320, 4, 1, True)
    gqa_sel, gqa_stair = ax.attention_patterns(2, 128, 4, 2, True)[:2]
    sdpa = ax.Shape(2, 4, 2, 33, 127, 64)
    return {
        "causal select 320": sel, "causal staircase 320": stair, "causal uniform0 320": uni0, "causal uniform1 320": uni1,
        "full staircase 320": ax.attention_patterns(1, 320, 4, 1, False)[1], "full uniform0 320": ax.attention_patterns(1, 320, 4, 1, False)[2],
        "full uniform1 320": ax.attention_patterns(1, 320, 4, 1, False)[3],
        "causal select 2x128 gqa": gqa_sel, "causal staircase 2x128 gqa": gqa_stair,
        "rotated select 2x128": ax.rotated_patterns(2, 128, 4, 2, True)[0], "rotated staircase 2x128": ax.rotated_patterns(2, 128, 4, 2, True)[1],
        "sdpa full uniform0 33x127": ax.uniform(sdpa, torch.float16, 0), "sdpa full staircase 33x127": ax.staircase(sdpa, torch.float16, False),
        "sdpa causal uniform1 127x33": ax.uniform(ax.Shape(2, 4, 2, 127, 33, 64), torch.float16, 1, True),
        "sdpa mask_select B1LS": ax.mask_select(sdpa, torch.float16, "B1LS"), "sdpa bool uniform0 B1LS": ax.masked_uniform(sdpa, torch.float16, 0, "B1LS"),
        "sdpa mask_select 1HLS": ax.mask_select(sdpa, torch.float16, "1HLS"),
        **{f"scaled staircase a={a} {'causal' if causal else 'full'}": p for causal in (True, False)
           for (a, _), p in zip(ax.SCALED_STAIRS, ax.scaled_patterns(ax.llama(*ax.SCALED_ATTENTION_SHAPE), torch.bfloat16, causal))},
    }


# form -> the patterns that must catch it (every other candidate the form applies to is tried too, and reported)
FORMS = {
    "row t also sees key t + 1": ("causal staircase 320", "causal uniform0 320"),
    "row t misses key t": ("causal staircase 320", "causal uniform1 320"),
    "one key of a middle tile dropped": ("causal uniform0 320", "full uniform1 320"),
    "one key counted twice": ("full uniform0 320", "causal uniform1 320"),
    "two V rows of one tile swapped": ("causal select 320", "causal staircase 320"),
    "kv head h mod HKV": ("causal select 2x128 gqa", "causal staircase 2x128 gqa"),
    "last tile skipped for a partial last query block": ("causal staircase 320", "full staircase 320", "full uniform0 320"),
    "batch b reads batch 0": ("causal select 2x128 gqa", "causal staircase 2x128 gqa"),
    "rotary table row modulo 32": ("rotated select 2x128", "rotated staircase 2x128"),
    "key bound S + 1": ("sdpa full uniform0 33x127", "sdpa causal uniform1 127x33"),
    "mask strides of the unbroadcast shape": ("sdpa mask_select B1LS", "sdpa bool uniform0 B1LS"),
    "softmax scale ignored": ("scaled staircase a=16 causal", "scaled staircase a=16 full"),
    "softmax scale applied twice": ("scaled staircase a=256 causal", "scaled staircase a=256 full"),
}


def _applies(form: str, name: str, p: ax.Pattern) -> bool:
    if form in ("row t also sees key t + 1", "row t misses key t"):
        return p.causal
    if form == "last tile skipped for a partial last query block":
        return p.shape.L == p.shape.S and p.shape.S % 256 != 0 and p.shape.S > 256
    if form == "rotary table row modulo 32":
        return p.rope is not None
    if form == "key bound S + 1":
        return p.mask is None and name.startswith("sdpa")
    if form == "mask strides of the unbroadcast shape":
        return p.mask is not None
    if form.startswith("softmax scale"):
        return p.scale is not None
    return True


def test_the_hookless_attention_is_reference64():
    for name, p in _candidates().items():
        # (the same float64 operations on differently laid-out operands: the last bits of the sums may differ)
        assert float((attend(p) - reference(p)).abs().max()) <= 2.0**-40 * float(p.v.double().abs().max()), name


@pytest.mark.parametrize("form", sorted(FORMS))
def test_every_wrong_form_breaks_a_named_pattern(form):
    candidates = _candidates()
    caught, missed = [], []
    for name, p in candidates.items():
        if _applies(form, name, p):
            (caught if ax.explain(p, attend(p, form)) is not None else missed).append(name)
    assert caught, f"'{form}' goes unnoticed by every pattern (tried: {missed})"
    for name in FORMS[form]:
        assert name in caught, f"'{form}' must break '{name}'; it breaks {caught} and not {missed}"
    print(f"'{form}' breaks {caught}; unnoticed by {missed}")


def test_a_leak_shows_in_every_row_of_the_staircase():
    """The point of the staircase: not one boundary, every row. With the leak row t returns V[t + 1], with the strict mask V[t - 1]."""
    p = ax.attention_patterns(1, 320, 4, 1, True)[1]
    leak = ax.failures(attend(p, "row t also sees key t + 1"), p.expected, p.bound).any(-1)
    assert bool(leak[..., :-1].all()) and not bool(leak[..., -1].any())  # (the last row has no key above it)
    strict = ax.failures(attend(p, "row t misses key t"), p.expected, p.bound).any(-1)
    assert bool(strict.all())
    text = ax.explain(p, attend(p, "row t also sees key t + 1"))
    assert "(batch 0, head 0, row 0)" in text and "should be V[batch 0, kv head 0, key 0]" in text and "closest to V[batch 0, kv head 0, key 1]" in text, text


# ---- the second implementations --------------------------------------------------------------------------------------------------------
def oracle_attention(p: ax.Pattern) -> torch.Tensor:
    q = p.q if p.q_in is None else p.q_in
    ctx, _ = ops.attention(ax.bsd(q), ax.bsd(p.k), ax.bsd(p.v), 128, causal=p.causal, q_rope=p.rope)
    return ax.heads(ctx, 128)


@pytest.mark.parametrize("B,S,H,HKV,causal", [c for c in LLAMA_CASES if c[1] <= 320 or c[4]])
def test_the_oracle_chain_meets_the_expectations(oracle_backend, B, S, H, HKV, causal):
    """select and uniform to the patterns' own bounds; the staircase is beyond the chain's bf16 scores (module docstring, which also
    says which cases are left out for time)."""
    sel, _, uni0, uni1 = ax.attention_patterns(B, S, H, HKV, causal)
    assert ax.explain(sel, oracle_attention(sel)) is None, ax.explain(sel, oracle_attention(sel))
    for p in (uni0, uni1):
        text = ax.explain(p, oracle_attention(p))
        assert text is None, text


def test_the_oracle_chain_rotates_q(oracle_backend):
    p = ax.rotated_patterns(2, 128, 4, 2, True)[0]
    assert ax.explain(p, oracle_attention(p)) is None, ax.explain(p, oracle_attention(p))
    # ... and without the tables the backwards-rotated q does not find its keys
    plain = dataclasses.replace(p, rope=None)
    assert ax.explain(p, oracle_attention(plain)) is not None


@pytest.mark.parametrize("causal", [True, False])
def test_scaled_staircases_meet_the_residual_rule_and_both_implementations(oracle_backend, causal):
    """The staircases under an explicit scale: reference64 and the math path (with and without the weights quantizer) on the SDPA
    shape in both dtypes, reference64 on the ops.attention shape (the oracle's bf16 scores do not resolve a staircase)."""
    import fastforward_amd as ff

    bits, scale, offset = ax.WEIGHTS_QUANTIZER
    quantizer = ff.nn.LinearQuantizer(bits, symmetric=False, granularity=ff.PerTensor())
    quantizer.quantization_range = (torch.tensor(-1.0), torch.tensor(1.0))
    with torch.no_grad():
        quantizer.scale.fill_(scale)
        quantizer.offset.fill_(offset)
    for p in ax.scaled_patterns(ax.llama(*ax.SCALED_ATTENTION_SHAPE), torch.bfloat16, causal):
        assert p.scale is not None and p.residual <= ax.RESIDUAL_LIMIT and ax.explain(p, reference(p)) is None
    for dtype in ax.SDPA_DTYPES:
        for p in ax.scaled_patterns(ax.SCALED_SDPA_SHAPE, dtype, causal):
            assert p.residual <= ax.RESIDUAL_LIMIT and ax.explain(p, reference(p)) is None
            with torch.no_grad():
                plain = scaled_dot_product_attention_math(p.q, p.k, p.v, is_causal=p.causal, scale=p.scale, enable_gqa=True, strict_quantization=False)
                coded = scaled_dot_product_attention_math(p.q, p.k, p.v, is_causal=p.causal, scale=p.scale, enable_gqa=True, strict_quantization=False,
                                                          attn_weights_quantizer=quantizer)
            assert ax.explain(p, plain) is None, ax.explain(p, plain)
            assert ax.explain(p, coded, *ax.weights_quantized(p)) is None, ax.explain(p, coded, *ax.weights_quantized(p))


@pytest.mark.parametrize("L,S,kind", SDPA_CASES)
def test_the_math_path_meets_the_expectations(L, S, kind):
    for dtype in ax.SDPA_DTYPES:
        for p in ax.sdpa_patterns(L, S, kind, dtype):
            with torch.no_grad():
                got = scaled_dot_product_attention_math(p.q, p.k, p.v, attn_mask=p.mask, is_causal=p.causal, scale=p.scale, enable_gqa=True,
                                                        strict_quantization=False)
            assert got.dtype == dtype
            assert ax.explain(p, got) is None, ax.explain(p, got)


@pytest.mark.parametrize("L,S", [(65, 129), (127, 33), (130, 300)])
def test_the_math_path_with_the_weights_quantizer_meets_the_quantized_expectations(oracle_backend, L, S):
    """The chain's probabilities through the weights quantizer (8 bits, 2^-8, 128): 255 / 256 of the target bit for bit, and the
    codes min(rne(256 / n), 255) of a uniform row — ``weights_quantized`` is what the chain computes, not only what the kernel does."""
    import fastforward_amd as ff

    bits, scale, offset = ax.WEIGHTS_QUANTIZER
    quantizer = ff.nn.LinearQuantizer(bits, symmetric=False, granularity=ff.PerTensor())
    quantizer.quantization_range = (torch.tensor(-1.0), torch.tensor(1.0))
    with torch.no_grad():
        quantizer.scale.fill_(scale)
        quantizer.offset.fill_(offset)
        for kind in ax.SDPA_KINDS:
            for dtype in ax.SDPA_DTYPES:
                for p in ax.sdpa_patterns(L, S, kind, dtype):
                    got = scaled_dot_product_attention_math(p.q, p.k, p.v, attn_mask=p.mask, is_causal=p.causal, scale=p.scale, enable_gqa=True,
                                                            strict_quantization=False, attn_weights_quantizer=quantizer)
                    text = ax.explain(p, got, *ax.weights_quantized(p))
                    assert text is None, text
