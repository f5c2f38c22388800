"""The KV cache with per-token dynamic scales on the MI355X (kv_token_store_kernel in csrc/ffq_kv_cache.hip, kv_token_partial_kernel
in csrc/ffq_sdpa_decode.hip, ops/kv_cache.py, nn/kv_cache.py; include/ffq_kv_token.h).

Append: codes and parameters start as sentinels inside a guarded arena; after ONE launch exactly the rows ``lens[b] - L .. lens[b] - 1``
inside ``[0, S_max)`` hold the codes AND the parameters of ``ops.quantize_dynamic_by_tile`` on the new rows (of the rotated rows, with
tables) with one tile per row, bit for bit, NaN as NaN; everything else is the sentinel and no guard byte moved. Decode: with uniform
parameters the bits of ``ops.kv_decode``; with rows re-expressed into other codes and parameters of the same exact values
(tests/kv_token_cases.py) the bits of ``ops.kv_decode`` on the ORIGINAL per-tensor cache: existing code against new code on identical
contracted values, no tolerance; known answers exactly; random operands inside the attention contract. The class: a ragged decode loop,
eager and replayed from one captured graph. Every test counts the calls of the two new entry points and of the dense ones on the loaded
library: a silent fallback fails."""

import pytest
import torch

import fastforward_amd as ff

import attention_exact as ax
import guards
import kv_cache_cases as dense_cases
import kv_token_cases as cases

from fastforward_amd import _native, ops
from kv_token_cases import B, HKV, S_MAX
from test_kv_cache_gpu import lens_tensor, new_rows, random_cache, rope_reference_bf16, rope_reference_fp16, rule_count, scalars, step_inputs
from test_sdpa_decode_gpu import math_path

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("ffq_kv_token_append", "ffq_kv_token_decode", "ffq_kv_append", "ffq_kv_decode")
K_BITS, V_BITS = (8, False), (4, True)  # (bits, symmetric)


@pytest.fixture
def entries(monkeypatch):
    """Calls of the four C entry points, counted on the loaded library itself."""
    lib = _native.library()
    count = dict.fromkeys(NAMES, 0)
    for name in NAMES:
        def counting(*args, _real=getattr(lib, name), _name=name):
            count[_name] += 1
            return _real(*args)
        monkeypatch.setattr(lib, name, counting)
    return count


def bits_of(t):
    return t.contiguous().view(torch.int32)


def same_parameters(got, want):
    """Equal as bit patterns, NaN as NaN."""
    return bool(((bits_of(got) == bits_of(want)) | (got.isnan() & want.isnan())).all())


# ---- append ---------------------------------------------------------------------------------------------------------------------------
SPECIAL = ("constant", "zero", "one-sided", "nan", "+inf", "-inf")


def special_rows(k, v):
    """Rows l = 0 of six (batch, head) pairs overwritten in place, in K and in V: constant, all zero, one-sided, and holding NaN, +Inf,
    -Inf. Between the two length sets every one of them lands inside the cache once."""
    E = k.shape[-1]
    ramp = torch.linspace(0.25, 3.0, E, device=k.device).to(k.dtype)
    for t in (k, v):
        t[0, 0, 0], t[0, 1, 0], t[1, 0, 0] = 2.5, 0.0, ramp
        t[1, 1, 0, 5], t[3, 0, 0, 7], t[3, 1, 0, 9] = float("nan"), float("inf"), -float("inf")
        t[4, 0, 0], t[4, 1, 0, 11], t[2, 0, 0] = -ramp, float("nan"), -1.75   # (sequence 2 is the one past S_max in the second set)
        t[4, 1, 0, 12] = float("inf")


def sentinel_stores(arena, layout, E):
    lead = (B, HKV, S_MAX) if layout == "bhse" else (B, S_MAX, HKV)
    stores = [arena.adopt(torch.full((*lead, E), cases.SENTINEL, dtype=torch.int8, device=DEV), f"{name} cache") for name in ("k", "v")]
    stores.append(arena.adopt(torch.full((*lead, 4), cases.PARAM_SENTINEL, dtype=torch.float32, device=DEV), "params"))
    return [t if layout == "bhse" else t.transpose(1, 2) for t in stores]


def expected(rows, spec, lens, L):
    """(codes [B, HKV, S_MAX, E], scale and offset [B, HKV, S_MAX]) after the append: the dynamic quantizer's on the rows that land."""
    codes, scale, offset = ops.quantize_dynamic_by_tile(rows.contiguous(), (1, 1, 1, rows.shape[-1]), float(spec[0]), spec[1], False, torch.int8)
    scale, offset = scale.view(B, HKV, L), offset.view(B, HKV, L)
    want_c = torch.full((B, HKV, S_MAX, rows.shape[-1]), cases.SENTINEL, dtype=torch.int8, device=DEV)
    want_s, want_o = (torch.full((B, HKV, S_MAX), cases.PARAM_SENTINEL, device=DEV) for _ in range(2))
    for b, n in enumerate(lens):
        for l, pos in dense_cases.positions(n, L):
            want_c[b, :, pos], want_s[b, :, pos], want_o[b, :, pos] = codes[b, :, l], scale[b, :, l], offset[b, :, l]
    return want_c, want_s, want_o


def check_append(entries, dtype, E, L, lens, layout, view, k_spec, v_spec, rotated=None, special=False, seed=0):
    gen = torch.Generator().manual_seed(seed + L + E)
    k_new, v_new = new_rows(L, E, dtype, view, gen)
    if special:
        special_rows(k_new, v_new)
    arena = guards.Arena(guards.POISON_A)
    kc, vc, params = sentinel_stores(arena, layout, E)
    rope = None
    if rotated is not None:
        rope = tuple((torch.randn(S_MAX + 5, E, generator=gen)).to(dtype).to(DEV) for _ in range(2))
    before = dict(entries)
    ops.kv_token_append(k_new, v_new, kc, vc, params, lens_tensor(lens), k_spec, v_spec, rope=rope)
    torch.cuda.synchronize()
    assert entries["ffq_kv_token_append"] == before["ffq_kv_token_append"] + 1 and entries["ffq_kv_append"] == before["ffq_kv_append"]
    k_rows = k_new.contiguous() if rope is None else rotated(k_new, rope, lens, L)
    want_k, want_ks, want_ko = expected(k_rows, k_spec, lens, L)
    want_v, want_vs, want_vo = expected(v_new, v_spec, lens, L)
    what = f"E={E} L={L} lens={lens}"
    assert torch.equal(kc, want_k), f"K {what}: {int((kc != want_k).sum())} bytes differ"
    assert torch.equal(vc, want_v), f"V {what}: {int((vc != want_v).sum())} bytes differ"
    for i, want in enumerate((want_ks, want_ko, want_vs, want_vo)):
        assert same_parameters(params[..., i], want), f"{what}: parameter {i} differs in {int((bits_of(params[..., i]) != bits_of(want)).sum())} rows"
    if special and v_spec[1]:
        assert bool((want_vo[want_vs != cases.PARAM_SENTINEL] == 0).all())  # a symmetric quantizer's offsets are 0.0
    assert not arena.touched_guards(), arena.touched_guards()


@pytest.mark.parametrize("view", ["contiguous", "projection", "strided"])
@pytest.mark.parametrize("layout", ["bhse", "bshe"])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_append_writes_exactly_its_rows_and_their_parameters(entries, dtype, layout, view):
    """8-bit asymmetric K with 4-bit symmetric V, and the reverse; L = 1, 4, 5 over both length sets (below L, on the tile edges, past
    S_max). The drawn rows hold +-1e4, +-Inf and NaN in one row of the first sequence (tests/test_kv_cache_gpu.py: new_rows)."""
    for E in cases.ES:
        for L in cases.LS:
            for i, lens in enumerate(cases.LENS_SETS):
                k_spec, v_spec = (K_BITS, V_BITS) if (L + i) % 2 else (V_BITS, K_BITS)
                check_append(entries, dtype, E, L, lens, layout, view, k_spec, v_spec)
    assert entries["ffq_kv_token_append"] == 12 and entries["ffq_kv_append"] == 0


@pytest.mark.parametrize("specs", [(K_BITS, V_BITS), (V_BITS, K_BITS), ((3, False), (8, True))], ids=["k8a-v4s", "k4s-v8a", "k3a-v8s"])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_append_on_constant_zero_one_sided_and_non_finite_rows(entries, dtype, specs):
    for E in cases.ES:
        for L in (1, 4):
            for lens in cases.LENS_SETS:
                check_append(entries, dtype, E, L, lens, "bshe", "projection", *specs, special=True, seed=7)
    assert entries["ffq_kv_token_append"] == 8


@pytest.mark.parametrize("layout", ["bhse", "bshe"])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_append_rotates_k_at_each_rows_own_position_then_quantizes(entries, dtype, layout):
    rotated = rope_reference_bf16 if dtype == torch.bfloat16 else rope_reference_fp16
    for E in cases.ES:
        for L, view in ((1, "projection"), (4, "contiguous"), (5, "strided")):
            for i, lens in enumerate(cases.LENS_SETS):
                k_spec, v_spec = (K_BITS, V_BITS) if i else (V_BITS, K_BITS)
                check_append(entries, dtype, E, L, lens, layout, view, k_spec, v_spec, rotated=rotated, seed=11)
    assert entries["ffq_kv_token_append"] == 12


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_a_prompt_goes_through_the_same_call(entries, dtype):
    """L = 300 in one launch at ragged targets: whole in the cache, cut at its end, cut at its start."""
    gen = torch.Generator().manual_seed(5)
    L, E, lens = 300, 128, (300, 384, 450, 120, 0)
    k_new, v_new = (torch.randn(B, HKV, L, E, generator=gen).to(dtype).to(DEV) for _ in range(2))
    rope = tuple(torch.randn(S_MAX, E, generator=gen).to(dtype).to(DEV) for _ in range(2))
    arena = guards.Arena(guards.POISON_B)
    kc, vc, params = sentinel_stores(arena, "bshe", E)
    ops.kv_token_append(k_new, v_new, kc, vc, params, lens_tensor(lens), K_BITS, V_BITS, rope=rope)
    torch.cuda.synchronize()
    assert entries["ffq_kv_token_append"] == 1 and [len(dense_cases.positions(n, L)) for n in lens] == [300, 300, 234, 120, 0]
    rotated = (rope_reference_bf16 if dtype == torch.bfloat16 else rope_reference_fp16)(k_new, rope, lens, L)
    want_k, want_ks, want_ko = expected(rotated, K_BITS, lens, L)
    want_v, want_vs, want_vo = expected(v_new, V_BITS, lens, L)
    assert torch.equal(kc, want_k) and torch.equal(vc, want_v)
    for i, want in enumerate((want_ks, want_ko, want_vs, want_vo)):
        assert same_parameters(params[..., i], want), i
    assert not arena.touched_guards(), arena.touched_guards()


# ---- decode -----------------------------------------------------------------------------------------------------------------------------
K_DEQ, V_DEQ = (0.031, 3.4), (0.027, -9.0)  # (a real K offset: the dense entry rounds it, the store holds it rounded)


@pytest.mark.parametrize("G", cases.GROUPS)
@pytest.mark.parametrize("E", cases.ES)
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_uniform_parameters_give_the_dense_kernels_bits(entries, dtype, E, G):
    """Every position's parameters set to one (s, rne(o)): bit-equal to ``ops.kv_decode`` with that per-tensor dequantization, over the
    grid at every split count, without a mask and causal, the exact zeros included."""
    kc, vc = random_cache(E, seed=E + G)
    deq = (None, scalars(*K_DEQ), scalars(*V_DEQ))
    params = cases.uniform_params(K_DEQ, V_DEQ, DEV)
    gen = torch.Generator().manual_seed(G)
    calls = 0
    for L in cases.LS:
        q = torch.randn(B, HKV * G, L, E, generator=gen).to(dtype).to(DEV)
        for lens in cases.LENS_SETS:
            device_lens = lens_tensor(lens)
            for causal in (False, True):
                for splits in cases.SPLITS:
                    got = ops.kv_token_decode(q, kc, vc, params, device_lens, is_causal=causal, splits=splits)
                    want = ops.kv_decode(q, kc, vc, device_lens, is_causal=causal, dequant=deq, splits=splits)
                    calls += 1
                    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (L, lens, causal, splits)
                    for b, n in enumerate(lens):
                        S = dense_cases.clamp_len(n)
                        if S == 0:
                            assert torch.equal(got[b], torch.zeros_like(got[b])), (L, lens, causal, splits)
                        elif causal and S < L:
                            assert torch.equal(got[b, :, :L - S], torch.zeros_like(got[b, :, :L - S]))
    assert entries["ffq_kv_token_decode"] == entries["ffq_kv_decode"] == calls == 3 * 2 * 2 * 5


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_a_quantized_query_brings_its_own_parameters(entries, dtype):
    """q as per-tensor codes in an int8 container and in a value-dtype container, with ``q_dequant``: the dense entry's bits again."""
    E, G, L, lens = 128, 4, 4, cases.LENS_SETS[1]
    kc, vc = random_cache(E, seed=9)
    params = cases.uniform_params(K_DEQ, V_DEQ, DEV)
    q_deq = scalars(0.05, -11.0)
    codes = torch.randint(-128, 128, (B, HKV * G, L, E), generator=torch.Generator().manual_seed(9))
    for q in (codes.to(torch.int8).to(DEV), codes.to(dtype).to(DEV)):
        for splits in (0, 3):
            got = ops.kv_token_decode(q, kc, vc, params, lens_tensor(lens), is_causal=True, q_dequant=q_deq, dtype=dtype, splits=splits)
            want = ops.kv_decode(q, kc, vc, lens_tensor(lens), is_causal=True, dequant=(q_deq, scalars(*K_DEQ), scalars(*V_DEQ)), dtype=dtype, splits=splits)
            assert got.dtype == dtype and torch.equal(got.view(torch.int16), want.view(torch.int16)) and bool(got.any())
    assert entries["ffq_kv_token_decode"] == entries["ffq_kv_decode"] == 4


OFFSETS = (0.0, 200.0, -200.0, 37.0)


@pytest.mark.parametrize("G", cases.GROUPS)
@pytest.mark.parametrize("E", cases.ES)
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_reexpressed_rows_give_the_bits_of_the_per_tensor_cache(entries, dtype, E, G):
    """Codes in [-31, 31], a power-of-two scale, an integer offset; K and V re-expressed independently, row by row, into other codes and
    parameters that dequantize to the same numbers with every fp32 step exact (kv_token_cases.reexpress). The per-row kernel then
    contracts the values the dense kernel contracts on the original cache: the same bits at the same split count."""
    gen = torch.Generator().manual_seed(100 + E + G)
    calls = 0
    for i, L in enumerate(cases.LS):
        kc, vc = (torch.randint(-31, 32, (B, HKV, S_MAX, E), generator=gen).to(torch.int8) for _ in range(2))
        (ks, ko), (vs, vo) = (2.0**-4, OFFSETS[(i + G) % 4]), (2.0**-(i + 1), OFFSETS[(i + G + 2) % 4])
        new_k, k_scale, k_offset, k_took = cases.reexpress(kc, ks, ko, gen)
        new_v, v_scale, v_offset, v_took = cases.reexpress(vc, vs, vo, gen)
        assert float((k_took != 0).float().mean()) >= 0.5 and float((v_took != 0).float().mean()) >= 0.5
        params = cases.pack(k_scale, k_offset, v_scale, v_offset, DEV)
        kc, vc, new_k, new_v = (t.to(DEV) for t in (kc, vc, new_k, new_v))
        deq = (None, scalars(ks, ko), scalars(vs, vo))
        q = torch.randn(B, HKV * G, L, E, generator=gen).to(dtype).to(DEV)
        for lens in cases.LENS_SETS:
            device_lens = lens_tensor(lens)
            for causal in (False, True):
                for splits in cases.SPLITS:
                    got = ops.kv_token_decode(q, new_k, new_v, params, device_lens, is_causal=causal, splits=splits)
                    want = ops.kv_decode(q, kc, vc, device_lens, is_causal=causal, dequant=deq, splits=splits)
                    calls += 1
                    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (L, lens, causal, splits)
    assert entries["ffq_kv_token_decode"] == entries["ffq_kv_decode"] == calls == 3 * 2 * 2 * 5


@pytest.mark.parametrize("L,G", [(1, 1), (1, 4), (4, 4), (5, 1), (5, 4)])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_known_answers_with_every_k_row_shifted(entries, dtype, L, G):
    """select / staircase / uniform of kv_cache_cases.exact_case with K re-expressed on every row (d = +-5): the answer itself, with ==,
    under every split count."""
    for E in cases.ES:
        for kind, causal in (("select", False), ("staircase", False), ("staircase", True), ("uniform", False), ("uniform", True)):
            for lens in cases.LENS_SETS:
                q, kc, vc, k_param, v_param, want = dense_cases.exact_case(kind, causal, L, G, E, dtype, lens)
                new_k, k_scale, k_offset, shifted = cases.shift_rows(kc, *k_param)
                for b, n in enumerate(lens):
                    assert bool(shifted[b, :, :dense_cases.clamp_len(n)].all())
                params = cases.pack(k_scale, k_offset, v_param[0], v_param[1], DEV)
                operands = [t.to(DEV) for t in (q, new_k, vc)]
                for splits in cases.SPLITS:
                    got = ops.kv_token_decode(*operands, params, lens_tensor(lens), is_causal=causal, splits=splits)
                    same = got.cpu().double() == want
                    assert bool(same.all()), f"{kind} causal={causal} E={E} lens={lens} splits={splits}: {int((~same).sum())} elements differ, first at {(~same).nonzero()[0].tolist()}"
    assert entries["ffq_kv_token_decode"] == 2 * 5 * 2 * 5 and entries["ffq_kv_decode"] == 0


def appended_cache(E, dtype, seed, k_spec=K_BITS, v_spec=V_BITS, spread=1.0):
    """randn K / V rows for every position, appended through ``ops.kv_token_append`` in one call: (K rows, V rows, codes, codes, params)."""
    gen = torch.Generator().manual_seed(seed)
    rows = torch.exp2(torch.randint(-3, 4, (B, HKV, S_MAX, 1), generator=gen).float() * spread)  # rows of very different magnitude
    k_all, v_all = ((torch.randn(B, HKV, S_MAX, E, generator=gen) * rows).to(dtype).to(DEV) for _ in range(2))
    kc, vc = (torch.zeros(B, HKV, S_MAX, E, dtype=torch.int8, device=DEV) for _ in range(2))
    params = torch.zeros(B, HKV, S_MAX, 4, device=DEV)
    ops.kv_token_append(k_all, v_all, kc, vc, params, lens_tensor([S_MAX] * B), k_spec, v_spec)
    return k_all, v_all, kc, vc, params


@pytest.mark.parametrize("E", cases.ES)
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_random_operands_meet_the_attention_contract(entries, dtype, E):
    """The rule of tests/test_kv_cache_gpu.py, per sequence: the error against float64 attention of the dequantized slice is at most
    the device math path's own on the same operands + 2^-9. The float64 side dequantizes with the per-row parameters the append wrote."""
    _, _, kc, vc, params = appended_cache(E, dtype, seed=E, k_spec=(8, False), v_spec=(8, False))
    gen = torch.Generator().manual_seed(E + 1)
    for L, G, lens, causal in ((1, 4, cases.LENS_SETS[0], False), (4, 4, cases.LENS_SETS[1], True), (5, 1, cases.LENS_SETS[1], True)):
        q = torch.randn(B, HKV * G, L, E, generator=gen).to(dtype).to(DEV)
        got = ops.kv_token_decode(q, kc, vc, params, lens_tensor(lens), is_causal=causal)
        for b, n in enumerate(lens):
            S = dense_cases.clamp_len(n)
            if S == 0:
                continue
            k64 = cases.dequant64(kc[b:b + 1, :, :S], params[b:b + 1, :, :S], 0, dtype)
            v64 = cases.dequant64(vc[b:b + 1, :, :S], params[b:b + 1, :, :S], 1, dtype)
            mask = dense_cases.bottom_right(L, S, DEV) if causal else None
            want = math_path(q[b:b + 1], k64.to(dtype).to(DEV), v64.to(dtype).to(DEV), attn_mask=mask, enable_gqa=True)
            ref = ax.reference64(q[b:b + 1].cpu(), k64, v64, mask=None if mask is None else mask.cpu())
            cases.meets_the_contract(got[b:b + 1], want, ref, f"L={L} G={G} S={S}")
    assert entries["ffq_kv_token_decode"] == 3 and entries["ffq_kv_token_append"] == 1


@pytest.mark.parametrize("which", ["k", "v"])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_a_nan_row_makes_its_own_sequence_nan_and_no_other(entries, dtype, which):
    """One appended row of sequence 1 holds a NaN (in every kv head): its scale is NaN, every key or value of that row dequantizes to
    NaN, and every output of that sequence is NaN. The other sequences' bits are those of a run without it."""
    E, G, L, lens = 64, 4, 1, (300, 200, 384, 129, 5)
    k_all, v_all, kc, vc, params = appended_cache(E, dtype, seed=3)
    q = torch.randn(B, HKV * G, L, E, generator=torch.Generator().manual_seed(4)).to(dtype).to(DEV)
    clean = [ops.kv_token_decode(q, kc, vc, params, lens_tensor(lens), splits=splits) for splits in (0, 3)]
    assert not any(bool(t.isnan().any()) for t in clean)
    k_row, v_row = k_all[:, :, 77:78].clone(), v_all[:, :, 77:78].clone()
    (k_row if which == "k" else v_row)[1, :, 0, 9] = float("nan")
    # position 77 of sequence 1 alone is written again: the other sequences' lengths park their row before position 0
    ops.kv_token_append(k_row, v_row, kc, vc, params, lens_tensor([0, 78, 0, 0, 0]), K_BITS, V_BITS)
    assert bool(params[1, :, 77, 0 if which == "k" else 2].isnan().all()) and int(params.isnan().sum()) == (2 * HKV if which == "k" else HKV)
    for splits, before in zip((0, 3), clean):
        got = ops.kv_token_decode(q, kc, vc, params, lens_tensor(lens), splits=splits)
        assert bool(got[1].isnan().all())
        others = [0, 2, 3, 4]
        assert torch.equal(got[others].view(torch.int16), before[others].view(torch.int16))
    assert entries["ffq_kv_token_decode"] == 4 and entries["ffq_kv_token_append"] == 2


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_the_output_quantizer_runs_on_the_fp32_value(entries, dtype):
    """The three properties tests/test_kv_cache_gpu.py asks of the dense entry, per sequence: every output a multiple of the scale,
    inside the grid, within one step of the fake-quantized float64 attention."""
    E, L, G, lens = 128, 2, 4, cases.LENS_SETS[1]
    _, _, kc, vc, params = appended_cache(E, dtype, seed=31)
    q = torch.randn(B, HKV * G, L, E, generator=torch.Generator().manual_seed(31)).to(dtype).to(DEV)
    bits, step, offset = 8, 2.0**-5, 3.0
    for splits in (0, 3):
        got = ops.kv_token_decode(q, kc, vc, params, lens_tensor(lens), is_causal=True, output_quantizer=(*scalars(step, offset), float(bits)), splits=splits)
        assert got.dtype == dtype
        units = got.cpu().double() / step
        assert torch.equal(units, units.round()), "an output is not a multiple of the scale"
        assert float((units - offset).min()) >= -2 ** (bits - 1) and float((units - offset).max()) <= 2 ** (bits - 1) - 1
        ref = cases.attend64(q, kc, vc, params, lens, causal=True)
        fake = (torch.clamp(torch.round(ref / step - offset), -2 ** (bits - 1), 2 ** (bits - 1) - 1) + offset) * step
        assert float((got.cpu().double() - fake).abs().max()) <= step
    assert entries["ffq_kv_token_decode"] == 2


@pytest.mark.parametrize("plan_len", [None, 1, 200, 1024])
def test_the_plan_hint_the_guards_and_a_store_that_is_only_read(entries, plan_len):
    """``splits = 0`` takes ``sdpa_decode_plan`` at `plan_len` keys (S_max by default): seen in the workspace the call allocates inside a
    guarded arena, under two poisons; the result is the forced count's, whatever the workspace held. No guard byte around the output,
    the workspace or the parameter store moves, and the store itself (sentinels past the length included) is left as it was."""
    Bp, Hp, S_max, E, L, G = 1, 2, 1024, 128, 2, 4
    assert [ops.sdpa_decode_plan(Bp, Hp, n, L * G, E) for n in (1, 200, 1024)] == [1, 1, 4]
    count = ops.sdpa_decode_plan(Bp, Hp, plan_len or S_max, L * G, E)
    gen = torch.Generator().manual_seed(2)
    q = torch.randn(Bp, Hp * G, L, E, generator=gen).bfloat16().to(DEV)
    kc, vc = (torch.randint(-128, 128, (Bp, Hp, S_max, E), generator=gen).to(torch.int8).to(DEV) for _ in range(2))
    store = torch.full((Bp, Hp, S_max, 4), cases.PARAM_SENTINEL)
    store[:, :, :700] = torch.stack([torch.rand(Bp, Hp, 700, generator=gen) * 0.05 + 0.01, torch.randint(-20, 21, (Bp, Hp, 700), generator=gen).float(),
                                     torch.rand(Bp, Hp, 700, generator=gen) * 0.05 + 0.01, torch.randint(-20, 21, (Bp, Hp, 700), generator=gen).float()], dim=-1)
    lens = lens_tensor([700])
    results = []
    for poison in (guards.POISON_A, guards.POISON_B):
        arena = guards.Arena(poison)
        params = arena.adopt(store.to(DEV), "params")
        with guards.capture(arena):
            out = ops.kv_token_decode(q, kc, vc, params, lens, is_causal=True, plan_len=plan_len)
        torch.cuda.synchronize()
        fresh = sorted(b.nbytes for b in arena.blocks if b.kind == "fresh")
        assert fresh == sorted([out.numel() * 2, ops.sdpa_decode_workspace_bytes(Bp, Hp, L * G, E, count)]) and arena.find(out.data_ptr()) is not None
        assert not arena.touched_guards(), arena.touched_guards()
        assert torch.equal(bits_of(params), bits_of(store.to(DEV))), "the decode wrote the parameter store"
        results.append(out.clone())
    forced = ops.kv_token_decode(q, kc, vc, store.to(DEV), lens, is_causal=True, splits=count)
    assert torch.equal(results[0].view(torch.int16), results[1].view(torch.int16)) and torch.equal(results[0].view(torch.int16), forced.view(torch.int16))
    assert not bool(forced.isnan().any()) and entries["ffq_kv_token_decode"] == 3


# ---- the class --------------------------------------------------------------------------------------------------------------------------
def make_cache(dtype, E, layout="bshe"):
    return ff.nn.DynamicQuantizedKVCache(B, HKV, S_MAX, E, cases.quantizer(*K_BITS, E=E), cases.quantizer(*V_BITS, E=E, tile=True), dtype, DEV, layout=layout)


def composed_step(cache, k, v, rope):
    ff.nn.kv_cache.composed_token_append(cache.k_cache, cache.v_cache, cache.params, cache.lengths, k, v, cache.key_quantizer, cache.value_quantizer, rope)


def same_stores(a, b):
    return torch.equal(a.k_cache, b.k_cache) and torch.equal(a.v_cache, b.v_cache) and torch.equal(bits_of(a.params), bits_of(b.params))


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_a_ragged_decode_loop_eager_and_replayed_from_one_graph(entries, dtype):
    """The prompt goes in at per-batch lengths, then 12 steps of append + attend at L = 1, one launch of each per step; the codes and
    the parameters are the composed route's. Step 6 is then captured ONCE on a side stream and steps 6 .. 11 replayed from it with new
    inputs in static buffers: the same outputs, lengths, codes and parameters as the eager loop."""
    E, G, start = 128, 4, (0, 100, 127, 255, 380)  # (the last sequence runs past S_max after four steps: its rows are dropped)
    gen = torch.Generator().manual_seed(17)
    rope = tuple(torch.randn(S_MAX, E, generator=gen).to(dtype).to(DEV) for _ in range(2))
    prompt = tuple(torch.randn(B, HKV, max(start), E, generator=gen).to(dtype).to(DEV) for _ in range(2))
    inputs = step_inputs(E, dtype, G, 12, seed=18)

    eager = make_cache(dtype, E)
    eager.reset([n - max(start) for n in start])  # (append adds L = max(start) itself: sequence b keeps the prompt's last start[b] rows)
    eager.append(*prompt, rope=rope)
    assert eager.lengths.tolist() == list(start) and entries["ffq_kv_token_append"] == 1
    composed = make_cache(dtype, E)                # the same loop's cache through the composed route (lengths read on the host)
    composed.reset(start)
    composed_step(composed, *prompt, rope)
    snapshot = None
    outs = []
    for step, (k_t, v_t, q_t) in enumerate(inputs):
        if step == 6:
            snapshot = (eager.k_cache.clone(), eager.v_cache.clone(), eager.params.clone(), eager.lengths.clone())
        eager.append(k_t, v_t, rope=rope)
        outs.append(eager.attend(q_t))
        composed.lengths.add_(1)
        composed_step(composed, k_t, v_t, rope)
    torch.cuda.synchronize()
    assert entries["ffq_kv_token_append"] == 13 and entries["ffq_kv_token_decode"] == 12 and eager.lengths.tolist() == [n + 12 for n in start]
    assert entries["ffq_kv_append"] == 0 and entries["ffq_kv_decode"] == 0
    assert same_stores(eager, composed)
    for b, n in enumerate(eager.lengths.tolist()):  # the last step against the entry point on every sequence alone
        alone = ops.kv_token_decode(inputs[-1][2][b:b + 1], eager.k_cache[b:b + 1], eager.v_cache[b:b + 1], eager.params[b:b + 1], lens_tensor([n]),
                                    is_causal=True, splits=rule_count(G, E))
        assert torch.equal(outs[-1][b:b + 1].view(torch.int16), alone.view(torch.int16)), b

    # ---- capture step 6 once, on a side stream, with static input buffers
    def restore(cache):
        for buffer, saved in zip((cache.k_cache, cache.v_cache, cache.params, cache.lengths), snapshot):
            buffer.copy_(saved)

    replayed = make_cache(dtype, E)
    restore(replayed)
    static = [t.clone() for t in inputs[6]]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):               # (a warm-up outside the capture, undone below)
        replayed.append(static[0], static[1], rope=rope)
        replayed.attend(static[2])
    torch.cuda.current_stream().wait_stream(stream)
    restore(replayed)
    before = dict(entries)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        replayed.append(static[0], static[1], rope=rope)
        captured = replayed.attend(static[2])
    assert entries["ffq_kv_token_append"] == before["ffq_kv_token_append"] + 1 and entries["ffq_kv_token_decode"] == before["ffq_kv_token_decode"] + 1
    assert replayed.lengths.tolist() == snapshot[3].tolist()                       # (a capture runs nothing)
    for i, step in enumerate(range(6, 12)):
        for buffer, new in zip(static, inputs[step]):
            buffer.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured.view(torch.int16), outs[step].view(torch.int16)), f"replay {i}"
        assert replayed.lengths.tolist() == [n + step + 1 for n in start]
    assert same_stores(replayed, eager)
    assert entries["ffq_kv_token_append"] == before["ffq_kv_token_append"] + 1     # (six replays, no further call)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_keys_and_values_dequantize_to_the_per_row_restatement(entries, dtype):
    E, S = 64, 300
    cache = make_cache(dtype, E, layout="bhse")
    gen = torch.Generator().manual_seed(23)
    k, v = ((torch.randn(B, HKV, S, E, generator=gen) * torch.exp2(torch.randint(-4, 5, (B, HKV, S, 1), generator=gen).float())).to(dtype).to(DEV) for _ in range(2))
    cache.append(k, v)
    assert cache.lengths.tolist() == [S] * B and entries["ffq_kv_token_append"] == 1
    with torch.no_grad():
        for got, quantizer, data, which, codes in ((cache.keys(S), cache.key_quantizer, k, 0, cache.k_cache), (cache.values(S), cache.value_quantizer, v, 1, cache.v_cache)):
            own = quantizer(data)                   # what the dynamic quantizer itself returns for those rows
            assert isinstance(got, ff.QuantizedTensor) and torch.equal(got.raw_data, own.raw_data)
            assert torch.equal(got.dequantize().view(torch.int16), own.dequantize().view(torch.int16)) and got.dequantize().dtype == dtype
            assert torch.equal(got.dequantize().cpu().double(), cases.dequant64(codes[:, :, :S], cache.params[:, :, :S], which, dtype))
