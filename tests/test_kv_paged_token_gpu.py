"""The paged KV cache with per-token dynamic scales on the MI355X (kv_paged_token_store_kernel in csrc/ffq_kv_cache.hip,
kv_paged_token_partial_kernel in csrc/ffq_sdpa_decode.hip, ops/kv_cache.py, nn/kv_cache.py; include/ffq_kv_paged_token.h).

Every assertion is an equality with code that already ships. Append: the three pools start as sentinels inside a guarded arena; after
ONE launch exactly the rows ``(table[b][pos / P], pos % P)`` hold the codes and the parameters ``ops.kv_token_append`` writes into a
dense cache for the same inputs (parameters as bit patterns, NaN as NaN), every other byte of the three pools is the sentinel and no
guard byte moved. Decode: the bits of ``ops.kv_token_decode`` on the gathered dense codes and parameters at the same split count; with
uniform parameters, and with rows re-expressed into other codes and parameters of the same exact values, the bits of
``ops.kv_paged_decode`` on the per-tensor pools; known answers with ``==``. Table entries outside the pool touch nothing: each pool is
the middle of a larger allocation the test owns. Every test counts the calls of the two new entry points and of the six older cache
entry points on the loaded library: a served call is one call of the new one and none of an older one, so a silent fallback fails.

The cases are plain functions (``case_*``) and three tests at the end of the file walk them over their grids, zeroing the call counts
ahead of every case and naming the case in a failure: the whole file takes a few seconds, and the suite grows by three items."""

import itertools

import pytest
import torch

import fastforward_amd as ff

import guards
import kv_paged_token_cases as cases

from fastforward_amd import _native, ops
from kv_paged_token_cases import B, C, HKV
from test_kv_paged_gpu import EXTRA, START, bad_table, bits, feed_prompt, lens_tensor, new_rows, prompt_and_steps, random_codes, scalars, sentinel_pools

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEW = ("ffq_kv_paged_token_append", "ffq_kv_paged_token_decode")
OLDER = ("ffq_kv_token_append", "ffq_kv_token_decode", "ffq_kv_paged_append", "ffq_kv_paged_decode", "ffq_kv_append", "ffq_kv_decode")
K_BITS, V_BITS = (8, False), (4, True)  # (bits, symmetric)
K_DEQ, V_DEQ = (0.031, 3.4), (0.027, -9.0)  # (a real K offset: the per-tensor entries round it, a store holds it rounded)


@pytest.fixture
def entries(monkeypatch):
    """Calls of the eight C entry points, counted on the loaded library itself."""
    lib = _native.library()
    count = dict.fromkeys(NEW + OLDER, 0)
    for name in NEW + OLDER:
        def counting(*args, _real=getattr(lib, name), _name=name):
            count[_name] += 1
            return _real(*args)
        monkeypatch.setattr(lib, name, counting)
    return count


def counts(entries, **want):
    """True when the named entry points were called that often and every other one never."""
    return all(entries[name] == want.get(name.removeprefix("ffq_kv_"), 0) for name in NEW + OLDER)


def bits_of(t):
    return t.contiguous().view(torch.int32)


def same_parameters(got, want):
    """Equal as bit patterns, NaN as NaN."""
    return bool(((bits_of(got) == bits_of(want)) | (got.isnan() & want.isnan()).contiguous()).all())


# ---- append ---------------------------------------------------------------------------------------------------------------------------
def special_rows(k, v):
    """Rows l = 0 of the eight (batch, head) pairs overwritten in place, in K and in V: constant, all zero, one-sided (both signs), and
    holding NaN, +Inf, -Inf. Over the three length sets every one of them lands inside its sequence at least once."""
    E = k.shape[-1]
    ramp = torch.linspace(0.25, 3.0, E, device=k.device).to(k.dtype)
    for t in (k, v):
        t[0, 0, 0], t[0, 1, 0], t[1, 0, 0], t[2, 0, 0] = 2.5, 0.0, ramp, -ramp
        t[1, 1, 0, 5], t[3, 0, 0, 7], t[3, 1, 0, 9] = float("nan"), float("inf"), -float("inf")
        t[2, 1, 0, 11], t[2, 1, 0, 12] = float("nan"), float("inf")


def sentinel_param_pool(arena, num_pages, P, layout):
    plain = cases.param_pool_of(num_pages, P, layout, DEV, fill=cases.PARAM_SENTINEL)
    inside = arena.adopt(plain if layout == "phse" else plain.transpose(1, 2), "param pool")
    return inside if layout == "phse" else inside.transpose(1, 2)


def dense_reference(k_new, v_new, lens, k_spec, v_spec, rope, capacity=C):
    """What ``ops.kv_token_append`` writes for the same inputs into a dense sentinel cache [B, HKV, capacity, E | 4]."""
    batch, E = k_new.shape[0], k_new.shape[-1]
    kc, vc = (torch.full((batch, HKV, capacity, E), cases.SENTINEL, dtype=torch.int8, device=DEV) for _ in range(2))
    params = torch.full((batch, HKV, capacity, 4), cases.PARAM_SENTINEL, device=DEV)
    ops.kv_token_append(k_new, v_new, kc, vc, params, lens_tensor(lens), k_spec, v_spec, rope=rope)
    return kc, vc, params


def expected_pools(dense, rows, num_pages, P, extra=0):
    """Sentinel pools [num_pages + 2 * extra, HKV, P, E | 4] with the dense reference scattered through the table into the middle."""
    kc, vc, params = dense
    want_k, want_v = (cases.pool_of(num_pages + 2 * extra, P, kc.shape[-1], "phse", DEV, fill=cases.SENTINEL) for _ in range(2))
    want_p = cases.param_pool_of(num_pages + 2 * extra, P, "phse", DEV, fill=cases.PARAM_SENTINEL)
    cases.scatter(kc, rows, want_k[extra:extra + num_pages])
    cases.scatter(vc, rows, want_v[extra:extra + num_pages])
    cases.scatter_params(params, rows, want_p[extra:extra + num_pages])
    return want_k, want_v, want_p


def check_append(entries, dtype, E, L, lens, P, layout, view, k_spec, v_spec, with_rope, special=False, seed=0):
    gen = torch.Generator().manual_seed(seed + L + E + P)
    k_new, v_new = new_rows(L, E, dtype, view, gen)
    if special:
        special_rows(k_new, v_new)
    rows, num_pages = cases.page_table(P)
    arena = guards.Arena(guards.POISON_A)
    kp, vp = sentinel_pools(arena, num_pages, P, E, layout)
    pp = sentinel_param_pool(arena, num_pages, P, layout)
    rope = tuple(torch.randn(C + 5, E, generator=gen).to(dtype).to(DEV) for _ in range(2)) if with_rope else None
    before = dict(entries)
    ops.kv_paged_token_append(k_new, v_new, kp, vp, pp, lens_tensor(lens), cases.table_tensor(rows, DEV), k_spec, v_spec, rope=rope)
    torch.cuda.synchronize()
    assert entries == {**before, NEW[0]: before[NEW[0]] + 1}          # one call of the new entry point, none of any other
    dense = dense_reference(k_new, v_new, lens, k_spec, v_spec, rope)
    want_k, want_v, want_p = expected_pools(dense, rows, num_pages, P)
    what = f"{dtype}, E={E}, L={L}, lens={lens}, P={P}"
    assert torch.equal(kp, want_k), f"K: {int((kp != want_k).sum())} bytes differ ({what})"
    assert torch.equal(vp, want_v), f"V: {int((vp != want_v).sum())} bytes differ ({what})"
    assert same_parameters(pp, want_p), f"parameters: {int((bits_of(pp) != bits_of(want_p)).sum())} words differ ({what})"
    landed = sum(len(cases.positions(n, L)) for n in lens) * HKV
    assert int((kp != cases.SENTINEL).sum()) <= landed * E            # (a code may equal the sentinel; nothing else may differ from it)
    assert int((bits_of(pp) != bits_of(torch.full_like(pp, cases.PARAM_SENTINEL))).sum()) <= landed * 4
    if special and v_spec[1]:
        assert bool((pp[..., 3][pp[..., 2] != cases.PARAM_SENTINEL] == 0).all())   # a symmetric quantizer's offsets are 0.0
    assert not arena.touched_guards(), arena.touched_guards()


def case_append_writes_exactly_its_rows_and_their_parameters(entries, dtype, layout, view):
    """8-bit asymmetric K with 4-bit symmetric V, and the reverse; L = 1, 4, 5 over the three length sets (below L, on the page and tile
    edges, past the capacity) and the four page sizes. The drawn rows hold +-1e4, +-Inf and NaN in one row of the first sequence."""
    for E in cases.ES:
        for L in cases.LS:
            for i, lens in enumerate(cases.LENS_SETS):
                for j, P in enumerate(cases.PAGE_SIZES):
                    k_spec, v_spec = (K_BITS, V_BITS) if (L + i + j) % 2 else (V_BITS, K_BITS)
                    check_append(entries, dtype, E, L, lens, P, layout, view, k_spec, v_spec, with_rope=False)
    assert counts(entries, paged_token_append=2 * 3 * 3 * 4, token_append=2 * 3 * 3 * 4)
    # a refused call reaches no entry point
    rows, num_pages = cases.page_table(16)
    k_new, v_new = new_rows(1, 64, dtype, view, torch.Generator().manual_seed(0))
    pool = cases.pool_of(num_pages, 16, 64, layout, DEV)
    with pytest.raises(RuntimeError):
        ops.kv_paged_token_append(k_new, v_new, pool, pool, cases.param_pool_of(num_pages, 16, layout, DEV)[:-1], lens_tensor((1, 1, 1, 1)),
                                  cases.table_tensor(rows, DEV), K_BITS, V_BITS)
    assert counts(entries, paged_token_append=2 * 3 * 3 * 4, token_append=2 * 3 * 3 * 4)


def case_append_on_constant_zero_one_sided_and_non_finite_rows(entries, dtype, specs):
    for E in cases.ES:
        for L in (1, 4):
            for lens in cases.LENS_SETS:
                for P, layout in ((16, "pshe"), (128, "phse")):
                    check_append(entries, dtype, E, L, lens, P, layout, "projection", *specs, with_rope=False, special=True, seed=7)
    assert counts(entries, paged_token_append=2 * 2 * 3 * 2, token_append=2 * 2 * 3 * 2)


def case_append_rotates_k_at_each_rows_own_position_then_quantizes(entries, dtype, layout):
    """With rotary tables the table row is the row's position in its SEQUENCE, whatever page it lands in, and the row's min and max are
    taken after the rotation."""
    for E in cases.ES:
        for L, view in ((1, "projection"), (4, "contiguous"), (5, "projection")):
            for i, lens in enumerate(cases.LENS_SETS):
                for P in (16, 128):
                    k_spec, v_spec = (K_BITS, V_BITS) if i % 2 else (V_BITS, K_BITS)
                    check_append(entries, dtype, E, L, lens, P, layout, view, k_spec, v_spec, with_rope=True, seed=11)
    assert counts(entries, paged_token_append=2 * 3 * 3 * 2, token_append=2 * 3 * 3 * 2)


def case_a_prompt_crosses_many_pages_in_one_call(entries, dtype, P):
    """L = 300 in one launch at ragged targets: whole inside the sequence, ending on its last position, cut at the capacity, cut at its
    start."""
    L, E, lens = 300, 128, (300, 512, 600, 120)
    assert [len(cases.positions(n, L)) for n in lens] == [300, 300, 212, 120]
    check_append(entries, dtype, E, L, lens, P, "pshe", "contiguous", K_BITS, V_BITS, with_rope=True, seed=5)
    assert counts(entries, paged_token_append=1, token_append=1)


# ---- decode -----------------------------------------------------------------------------------------------------------------------------
def random_params(seed, batch=B, capacity=C, heads=HKV):
    """A dense parameter store [batch, heads, capacity, 4]: positive scales and integral offsets, every row its own."""
    gen = torch.Generator().manual_seed(seed)
    shape = (batch, heads, capacity)
    return torch.stack([torch.rand(shape, generator=gen) * 0.05 + 0.01, torch.randint(-20, 21, shape, generator=gen).float(),
                        torch.rand(shape, generator=gen) * 0.05 + 0.01, torch.randint(-20, 21, shape, generator=gen).float()], dim=-1).to(DEV)


def paged(dense_k, dense_v, dense_p, P, layout, fill=0, param_fill=0.0):
    """(k_pool, v_pool, param_pool, table tensor): the dense codes and parameters scattered over the seeded page assignment."""
    rows, num_pages = cases.page_table(P, batch=dense_k.shape[0], capacity=dense_k.shape[2])
    E = dense_k.shape[-1]
    kp = cases.scatter(dense_k, rows, cases.pool_of(num_pages, P, E, layout, DEV, fill=fill))
    vp = cases.scatter(dense_v, rows, cases.pool_of(num_pages, P, E, layout, DEV, fill=fill))
    pp = cases.scatter_params(dense_p, rows, cases.param_pool_of(num_pages, P, layout, DEV, fill=param_fill))
    return kp, vp, pp, cases.table_tensor(rows, DEV)


def zeros_where_nothing_is_seen(got, lens, L, causal):
    for b, n in enumerate(lens):
        S = cases.clamp_len(n)
        if S == 0 and not torch.equal(got[b], torch.zeros_like(got[b])):
            return False
        if 0 < S < L and causal and not torch.equal(got[b, :, :L - S], torch.zeros_like(got[b, :, :L - S])):
            return False
    return True


def case_decode_is_the_dense_token_kernel_on_the_same_codes_and_parameters(entries, dtype, E, G, P):
    """Bit for bit against ``ops.kv_token_decode`` on the densely laid out codes and parameters (every row its own), at every forced
    split count and at the rule's, without a mask and with bottom-right causality, in both pool layouts; exact zeros for a sequence
    without keys and for rows that see none. Unowned pages hold sentinels, NaN parameters among them: they are never read."""
    kc, vc = random_codes(E, seed=E + G)
    params = random_params(E + G + P)
    gen = torch.Generator().manual_seed(G)
    pools = [paged(kc, vc, params, P, layout, fill=cases.SENTINEL, param_fill=float("nan")) for layout in cases.LAYOUTS]
    calls = 0
    for L in cases.LS:
        q = torch.randn(B, HKV * G, L, E, generator=gen).to(dtype).to(DEV)
        for lens in cases.LENS_SETS:
            device_lens = lens_tensor(lens)
            for causal in (False, True):
                for splits in cases.SPLITS:
                    dense = ops.kv_token_decode(q, kc, vc, params, device_lens, is_causal=causal, splits=splits)
                    calls += 1
                    for kp, vp, pp, table in pools:
                        got = ops.kv_paged_token_decode(q, kp, vp, pp, device_lens, table, is_causal=causal, splits=splits)
                        assert torch.equal(bits(got), bits(dense)), (L, lens, causal, splits)
                        assert zeros_where_nothing_is_seen(got, lens, L, causal), (L, lens, causal, splits)
    assert calls == 3 * 3 * 2 * 5 and counts(entries, paged_token_decode=2 * calls, token_decode=calls)


def case_uniform_parameters_give_the_static_paged_kernels_bits(entries, dtype, E, P):
    """Every position's parameters set to one (s, rne(o)): bit-equal to ``ops.kv_paged_decode`` with that per-tensor dequantization on
    the same pools and table, over the grid at every split count."""
    G = 4
    kc, vc = random_codes(E, seed=E + P)
    kp, vp, pp, table = paged(kc, vc, cases.uniform_store(K_DEQ, V_DEQ, DEV), P, "pshe" if P == 16 else "phse")
    deq = (None, scalars(*K_DEQ), scalars(*V_DEQ))
    gen = torch.Generator().manual_seed(P)
    calls = 0
    for L in cases.LS:
        q = torch.randn(B, HKV * G, L, E, generator=gen).to(dtype).to(DEV)
        for lens in cases.LENS_SETS:
            device_lens = lens_tensor(lens)
            for causal in (False, True):
                for splits in cases.SPLITS:
                    got = ops.kv_paged_token_decode(q, kp, vp, pp, device_lens, table, is_causal=causal, splits=splits)
                    want = ops.kv_paged_decode(q, kp, vp, device_lens, table, is_causal=causal, dequant=deq, splits=splits)
                    calls += 1
                    assert torch.equal(bits(got), bits(want)), (L, lens, causal, splits)
    assert calls == 3 * 3 * 2 * 5 and counts(entries, paged_token_decode=calls, paged_decode=calls)


OFFSETS = (0.0, 200.0, -200.0, 37.0)


def case_reexpressed_rows_give_the_bits_of_the_per_tensor_pools(entries, dtype, E, G):
    """Codes in [-31, 31], a power-of-two scale, an integer offset in {0, +-200, 37}; K and V re-expressed independently, row by row,
    into other codes and parameters that dequantize to the same numbers with every fp32 step exact (kv_token_cases.reexpress). The
    per-row paged kernel then contracts the values the static paged kernel contracts on the ORIGINAL pools: the same bits at the same
    split count."""
    gen = torch.Generator().manual_seed(100 + E + G)
    calls = 0
    for i, L in enumerate(cases.LS):
        P = cases.PAGE_SIZES[(i + G) % 4]
        kc, vc = (torch.randint(-31, 32, (B, HKV, C, E), generator=gen).to(torch.int8) for _ in range(2))
        (ks, ko), (vs, vo) = (2.0**-4, OFFSETS[(i + G) % 4]), (2.0**-(i + 1), OFFSETS[(i + G + 2) % 4])
        new_k, k_scale, k_offset, k_took = cases.reexpress(kc, ks, ko, gen)
        new_v, v_scale, v_offset, v_took = cases.reexpress(vc, vs, vo, gen)
        assert float((k_took != 0).float().mean()) >= 0.5 and float((v_took != 0).float().mean()) >= 0.5
        store = cases.pack(k_scale, k_offset, v_scale, v_offset, DEV)
        layout = cases.LAYOUTS[i % 2]
        kp, vp, pp, table = paged(new_k.to(DEV), new_v.to(DEV), store, P, layout)
        old_k, old_v, _, _ = paged(kc.to(DEV), vc.to(DEV), store, P, layout)
        deq = (None, scalars(ks, ko), scalars(vs, vo))
        q = torch.randn(B, HKV * G, L, E, generator=gen).to(dtype).to(DEV)
        for lens in cases.LENS_SETS:
            device_lens = lens_tensor(lens)
            for causal in (False, True):
                for splits in cases.SPLITS:
                    got = ops.kv_paged_token_decode(q, kp, vp, pp, device_lens, table, is_causal=causal, splits=splits)
                    want = ops.kv_paged_decode(q, old_k, old_v, device_lens, table, is_causal=causal, dequant=deq, splits=splits)
                    calls += 1
                    assert torch.equal(bits(got), bits(want)), (L, P, lens, causal, splits)
    assert calls == 3 * 3 * 2 * 5 and counts(entries, paged_token_decode=calls, paged_decode=calls)


def case_known_answers_with_every_k_row_shifted(entries, dtype, L, G, P):
    """select / staircase / uniform of kv_paged_cases.exact_case with K re-expressed on every row inside a length (d = +-5): the answer
    itself, with ==, under every split count, with and without bottom-right causality."""
    for E in cases.ES:
        for kind, causal in (("select", False), ("staircase", False), ("staircase", True), ("uniform", False), ("uniform", True)):
            for lens in cases.LENS_SETS:
                q, kc, vc, k_param, v_param, expected = cases.exact_case(kind, causal, L, G, E, dtype, lens)
                new_k, k_scale, k_offset, shifted = cases.shift_rows(kc, *k_param)
                for b, n in enumerate(lens):
                    assert bool(shifted[b, :, :cases.clamp_len(n)].all())
                store = cases.pack(k_scale, k_offset, v_param[0], v_param[1], DEV)
                kp, vp, pp, table = paged(new_k.to(DEV), vc.to(DEV), store, P, "pshe" if P == 16 else "phse")
                for splits in cases.SPLITS:
                    got = ops.kv_paged_token_decode(q.to(DEV), kp, vp, pp, lens_tensor(lens), table, is_causal=causal, splits=splits)
                    same = got.cpu().double() == expected
                    assert bool(same.all()), f"{kind} causal={causal} E={E} lens={lens} splits={splits}: {int((~same).sum())} elements differ, first at {(~same).nonzero()[0].tolist()}"
    assert counts(entries, paged_token_decode=2 * 5 * 3 * 5)


def case_a_quantized_query_brings_its_own_parameters(entries, dtype):
    """q as per-tensor codes in an int8 container and in a value-dtype container, with ``q_dequant``: the dense token entry's bits."""
    E, G, L, lens = 128, 4, 4, cases.LENS_SETS[1]
    kc, vc = random_codes(E, seed=9)
    params = random_params(9)
    q_deq = scalars(0.05, -11.0)
    codes = torch.randint(-128, 128, (B, HKV * G, L, E), generator=torch.Generator().manual_seed(9))
    for P, layout in ((16, "phse"), (256, "pshe")):
        kp, vp, pp, table = paged(kc, vc, params, P, layout)
        for q in (codes.to(torch.int8).to(DEV), codes.to(dtype).to(DEV)):
            for splits in (0, 3):
                got = ops.kv_paged_token_decode(q, kp, vp, pp, lens_tensor(lens), table, is_causal=True, q_dequant=q_deq, dtype=dtype, splits=splits)
                want = ops.kv_token_decode(q, kc, vc, params, lens_tensor(lens), is_causal=True, q_dequant=q_deq, dtype=dtype, splits=splits)
                assert got.dtype == dtype and torch.equal(bits(got), bits(want)) and bool(got.any())
    assert counts(entries, paged_token_decode=8, token_decode=8)


def appended_pools(E, dtype, seed, P, layout):
    """randn K / V rows of very different magnitude for every position, appended through ``ops.kv_paged_token_append`` in one call:
    (K rows, V rows, the three pools, the table tensor, its rows)."""
    gen = torch.Generator().manual_seed(seed)
    spread = torch.exp2(torch.randint(-3, 4, (B, HKV, C, 1), generator=gen).float())
    k_all, v_all = ((torch.randn(B, HKV, C, E, generator=gen) * spread).to(dtype).to(DEV) for _ in range(2))
    rows, num_pages = cases.page_table(P)
    kp, vp = (cases.pool_of(num_pages, P, E, layout, DEV) for _ in range(2))
    pp = cases.param_pool_of(num_pages, P, layout, DEV)
    table = cases.table_tensor(rows, DEV)
    ops.kv_paged_token_append(k_all, v_all, kp, vp, pp, lens_tensor([C] * B), table, K_BITS, V_BITS)
    return k_all, v_all, kp, vp, pp, table, rows


def case_a_nan_row_makes_its_own_sequence_nan_and_no_other(entries, dtype, which):
    """One appended row of sequence 1 holds a NaN (in every kv head): its scale is NaN, every key or value of that row dequantizes to
    NaN, and every output of that sequence is NaN. The other sequences' bits are those of a run without it."""
    E, G, L, P, lens = 64, 4, 1, 16, (300, 200, 512, 129)
    k_all, v_all, kp, vp, pp, table, rows = appended_pools(E, dtype, 3, P, "pshe")
    q = torch.randn(B, HKV * G, L, E, generator=torch.Generator().manual_seed(4)).to(dtype).to(DEV)
    clean = [ops.kv_paged_token_decode(q, kp, vp, pp, lens_tensor(lens), table, splits=splits) for splits in (0, 3)]
    assert not any(bool(t.isnan().any()) for t in clean) and not bool(pp.isnan().any())
    k_row, v_row = k_all[:, :, 77:78].clone(), v_all[:, :, 77:78].clone()
    (k_row if which == "k" else v_row)[1, :, 0, 9] = float("nan")
    # position 77 of sequence 1 alone is written again: the other sequences' lengths park their row before position 0
    ops.kv_paged_token_append(k_row, v_row, kp, vp, pp, lens_tensor([0, 78, 0, 0]), table, K_BITS, V_BITS)
    page, at = rows[1][77 // P], 77 % P
    assert bool(pp[page, :, at, 0 if which == "k" else 2].isnan().all()) and int(pp.isnan().sum()) == (2 * HKV if which == "k" else HKV)
    for splits, before in zip((0, 3), clean):
        got = ops.kv_paged_token_decode(q, kp, vp, pp, lens_tensor(lens), table, splits=splits)
        assert bool(got[1].isnan().all())
        others = [0, 2, 3]
        assert torch.equal(bits(got[others]), bits(before[others]))
    assert counts(entries, paged_token_decode=4, paged_token_append=2)


def case_the_output_quantizer_gives_the_dense_token_calls_bits(entries, dtype):
    E, L, G = 128, 2, 4
    kc, vc = random_codes(E, seed=31)
    params = random_params(31)
    q = torch.randn(B, HKV * G, L, E, generator=torch.Generator().manual_seed(31)).to(dtype).to(DEV)
    for P, layout in ((16, "phse"), (128, "pshe")):
        kp, vp, pp, table = paged(kc, vc, params, P, layout)
        for lens in cases.LENS_SETS:
            for out_bits, step, offset in ((8, 2.0**-5, 3.0), (4, 2.0**-2, -1.0), (8, 0.013, None)):
                for splits in (0, 3):
                    quantizer = (*scalars(step, offset), float(out_bits))
                    got = ops.kv_paged_token_decode(q, kp, vp, pp, lens_tensor(lens), table, is_causal=True, output_quantizer=quantizer, splits=splits)
                    dense = ops.kv_token_decode(q, kc, vc, params, lens_tensor(lens), is_causal=True, output_quantizer=quantizer, splits=splits)
                    assert got.dtype == dtype and torch.equal(bits(got), bits(dense)), (P, lens, out_bits, splits)
    assert counts(entries, paged_token_decode=2 * 3 * 3 * 2, token_decode=2 * 3 * 3 * 2)


def case_the_plan_hint_the_guards_and_pools_that_are_only_read(entries, plan_len):
    """``splits = 0`` takes ``sdpa_decode_plan`` at `plan_len` keys (the capacity C = 1024 by default): seen in the workspace the call
    allocates inside a guarded arena, under two poisons; the result is the forced count's, whatever the workspace held. No guard byte
    around the output, the workspace or the three pools moves, and the pools (sentinels in unowned pages included) are left as they were."""
    Bp, Hp, cap, E, L, G, P = 1, 2, 1024, 128, 2, 4, 128
    assert [ops.sdpa_decode_plan(Bp, Hp, n, L * G, E) for n in (1, 200, 1024)] == [1, 1, 4]
    count = ops.sdpa_decode_plan(Bp, Hp, plan_len or cap, L * G, E)
    gen = torch.Generator().manual_seed(2)
    q = torch.randn(Bp, Hp * G, L, E, generator=gen).bfloat16().to(DEV)
    kc, vc = (torch.randint(-128, 128, (Bp, Hp, cap, E), generator=gen).to(torch.int8).to(DEV) for _ in range(2))
    params = random_params(2, Bp, cap, Hp)
    pools = paged(kc, vc, params, P, "phse", fill=cases.SENTINEL, param_fill=cases.PARAM_SENTINEL)
    table, lens = pools[3], lens_tensor([700])
    results = []
    for poison in (guards.POISON_A, guards.POISON_B):
        arena = guards.Arena(poison)
        kp, vp, pp = (arena.adopt(t, name) for t, name in zip(pools[:3], ("k pool", "v pool", "param pool")))
        with guards.capture(arena):
            out = ops.kv_paged_token_decode(q, kp, vp, pp, lens, table, is_causal=True, plan_len=plan_len)
        torch.cuda.synchronize()
        fresh = sorted(b.nbytes for b in arena.blocks if b.kind == "fresh")
        assert fresh == sorted([out.numel() * 2, ops.sdpa_decode_workspace_bytes(Bp, Hp, L * G, E, count)]) and arena.find(out.data_ptr()) is not None
        assert not arena.touched_guards(), arena.touched_guards()
        assert torch.equal(kp, pools[0]) and torch.equal(vp, pools[1]) and torch.equal(bits_of(pp), bits_of(pools[2])), "the decode wrote a pool"
        results.append(out.clone())
    forced = ops.kv_paged_token_decode(q, *pools[:3], lens, table, is_causal=True, splits=count)
    assert torch.equal(bits(results[0]), bits(results[1])) and torch.equal(bits(results[0]), bits(forced))
    assert torch.equal(bits(forced), bits(ops.kv_token_decode(q, kc, vc, params, lens, is_causal=True, splits=count)))
    assert not bool(forced.isnan().any()) and counts(entries, paged_token_decode=3, token_decode=1)


# ---- table entries outside the pool ---------------------------------------------------------------------------------------------------
def middle_pools(num_pages, P, E, layout, fill, param_fill):
    """Three allocations of num_pages + 2 * EXTRA pages holding the fills, and their middle `num_pages` pages as the pools."""
    whole = [cases.pool_of(num_pages + 2 * EXTRA, P, E, layout, DEV, fill=fill) for _ in range(2)]
    whole.append(cases.param_pool_of(num_pages + 2 * EXTRA, P, layout, DEV, fill=param_fill))
    return whole, [t[EXTRA:EXTRA + num_pages] for t in whole]


def case_a_table_entry_outside_the_pool_touches_nothing(entries, dtype, P):
    """Each of the three pools is the middle of an allocation with two extra pages on each side: entries -1 and `num_pages` would land
    there. Append leaves those pages and the skipped rows at the sentinel, parameters included. Decode, by the route
    tests/test_kv_paged_gpu.py takes: per sequence against a call on the dense gather with the hidden keys cut out by a bool mask.
    Only ``ops.sdpa_decode`` takes a mask and it dequantizes per tensor, so the rows are re-expressed ones (every row its own codes
    and parameters, the same exact values): the reference is ``ops.sdpa_decode`` on the original per-tensor codes. Where the hidden
    pages are the END of a sequence the cut is a shorter length, and the reference is ``ops.kv_token_decode`` itself on the dense
    gather with arbitrary per-row parameters. The extra pages hold random codes and NaN parameters: reading one would show."""
    E, G = 128, 4
    good, num_pages = cases.page_table(P)
    rows = bad_table(P, good, num_pages)
    table = cases.table_tensor(rows, DEV)
    layout = "phse" if P in (16, 128) else "pshe"
    # ---- append: a prompt over the whole capacity, so that every entry is in use
    L, lens = 300, (300, 512, 512, 10)
    gen = torch.Generator().manual_seed(P)
    k_new, v_new = (torch.randn(B, HKV, L, E, generator=gen).to(dtype).to(DEV) for _ in range(2))
    whole, (kp, vp, pp) = middle_pools(num_pages, P, E, layout, cases.SENTINEL, cases.PARAM_SENTINEL)
    ops.kv_paged_token_append(k_new, v_new, kp, vp, pp, lens_tensor(lens), table, K_BITS, V_BITS)
    torch.cuda.synchronize()
    want = expected_pools(dense_reference(k_new, v_new, lens, K_BITS, V_BITS, None), rows, num_pages, P, extra=EXTRA)  # (scatter skips the outside entries)
    assert torch.equal(whole[0], want[0]) and torch.equal(whole[1], want[1]) and same_parameters(whole[2], want[2])
    for got, fill in zip(whole, (cases.SENTINEL, cases.SENTINEL, cases.PARAM_SENTINEL)):
        assert bool((got[:EXTRA] == fill).all()) and bool((got[-EXTRA:] == fill).all())
    assert counts(entries, paged_token_append=1, token_append=1)
    # ---- decode, interior holes: re-expressed rows against the bool-masked per-tensor call
    kc, vc = (torch.randint(-31, 32, (B, HKV, C, E), generator=gen).to(torch.int8) for _ in range(2))
    (ks, ko), (vs, vo) = (2.0**-4, 37.0), (2.0**-2, -200.0)
    new_k, k_scale, k_offset, _ = cases.reexpress(kc, ks, ko, gen)
    new_v, v_scale, v_offset, _ = cases.reexpress(vc, vs, vo, gen)
    kc, vc = kc.to(DEV), vc.to(DEV)
    whole, (kp, vp, pp) = middle_pools(num_pages, P, E, layout, 0, float("nan"))
    for t in whole[:2]:
        t.copy_(torch.randint(-128, 128, tuple(t.shape), generator=gen).to(torch.int8))
    cases.scatter(new_k.to(DEV), rows, kp)
    cases.scatter(new_v.to(DEV), rows, vp)
    cases.scatter_params(cases.pack(k_scale, k_offset, v_scale, v_offset, DEV), rows, pp)
    deq = (None, scalars(ks, ko), scalars(vs, vo))
    hidden = torch.tensor([[not 0 <= page < num_pages for page in row] for row in rows]).repeat_interleave(P, dim=1).to(DEV)   # [B, C]
    calls = 0
    for L in (1, 5):
        q = torch.randn(B, HKV * G, L, E, generator=gen).to(dtype).to(DEV)
        for lens in ((300, 512, 530, P), (P + 1, 17, 512, 1)):
            for causal in (False, True):
                for splits in (0, 1, 3):
                    got = ops.kv_paged_token_decode(q, kp, vp, pp, lens_tensor(lens), table, is_causal=causal, splits=splits)
                    calls += 1
                    count = splits or ops.sdpa_decode_plan(B, HKV, C, L * G, E)
                    for b, n in enumerate(lens):
                        S = cases.clamp_len(n)
                        mask = ~hidden[b, :S].unsqueeze(0).expand(L, S)
                        if causal:
                            mask = mask & cases.bottom_right(L, S, DEV)
                        want = ops.sdpa_decode(q[b:b + 1], kc[b:b + 1, :, :S], vc[b:b + 1, :, :S], attn_mask=mask, dequant=deq, splits=count)
                        assert torch.equal(bits(got[b:b + 1]), bits(want)), (L, lens, b, causal, splits)
                    assert torch.equal(got[3], torch.zeros_like(got[3]))     # (its keys are all on the invalid first page)
    assert calls == 2 * 2 * 2 * 3 and counts(entries, paged_token_decode=calls, paged_token_append=1, token_append=1)
    # ---- decode, hidden pages at the end of a sequence: arbitrary per-row parameters against ops.kv_token_decode at the cut length
    per = C // P
    keep = (per - 1, per // 2, 1, 0)                                          # whole pages sequence b keeps; the rest alternate -1 / num_pages
    rows = [list(r[:n]) + [(-1, num_pages)[i % 2] for i in range(per - n)] for r, n in zip(good, keep)]
    table = cases.table_tensor(rows, DEV)
    dense_k, dense_v = random_codes(E, seed=P)
    params = random_params(P)
    cases.scatter(dense_k, rows, kp)
    cases.scatter(dense_v, rows, vp)
    cases.scatter_params(params, rows, pp)
    assert bool(whole[2][:EXTRA].isnan().all()) and bool(whole[2][-EXTRA:].isnan().all())
    for L in (1, 5):
        q = torch.randn(B, HKV * G, L, E, generator=gen).to(dtype).to(DEV)
        for lens in ((512, 300, 530, 40), (17, C, P + 3, P)):
            cut = [min(cases.clamp_len(n), pages * P) for n, pages in zip(lens, keep)]
            for splits in (1, 64):            # (one split, or one per key tile: counts at which the shorter length cuts the keys the same way)
                got = ops.kv_paged_token_decode(q, kp, vp, pp, lens_tensor(lens), table, splits=splits)
                want = ops.kv_token_decode(q, dense_k, dense_v, params, lens_tensor(cut), splits=splits)
                assert torch.equal(bits(got), bits(want)), (L, lens, splits)
                assert torch.equal(got[3], torch.zeros_like(got[3]))         # (no valid page at all)
    assert counts(entries, paged_token_decode=calls + 8, token_decode=8, paged_token_append=1, token_append=1)


# ---- sharing --------------------------------------------------------------------------------------------------------------------------
def case_two_sequences_share_their_prefix_pages_and_their_parameters(entries, dtype, P):
    """Two table rows that point at the same physical prefix pages give identical bits for identical queries; appending to one of them
    after the shared prefix leaves the other's output and every shared page's codes and parameters as they were."""
    E, G, L, num_pages = 64, 4, 3, 11
    shared = 2 * P
    rows = [[7, 2, 9, 4], [7, 2, 5, 0]]
    table = cases.table_tensor(rows, DEV)
    gen = torch.Generator().manual_seed(P)
    kp, vp = (cases.pool_of(num_pages, P, E, "pshe", DEV) for _ in range(2))
    for t in (kp, vp):
        t.copy_(torch.randint(-128, 128, tuple(t.shape), generator=gen).to(torch.int8))
    pp = cases.param_pool_of(num_pages, P, "pshe", DEV)
    pp.copy_(random_params(P, num_pages, P))                                  # (a pool has a store's shape: [num_pages, HKV, P, 4])
    q = torch.randn(1, HKV * G, L, E, generator=gen).to(dtype).to(DEV).expand(2, -1, -1, -1).contiguous()
    first = ops.kv_paged_token_decode(q, kp, vp, pp, lens_tensor((shared, shared)), table, is_causal=True)
    assert torch.equal(bits(first[0]), bits(first[1])) and bool(first.any())
    # three rows for sequence 1 alone (sequence 0's target is parked below zero: its rows are dropped)
    k_new, v_new = new_rows(L, E, dtype, "contiguous", gen, batch=2)
    untouched = [t.clone() for t in (kp, vp, pp)]
    ops.kv_paged_token_append(k_new, v_new, kp, vp, pp, lens_tensor((-L, shared + L)), table, K_BITS, V_BITS)
    changed = [(bits_of(a) != bits_of(b)).flatten(1).any(1).nonzero().flatten().tolist() if a.dtype == torch.float32 else
               (a != b).flatten(1).any(1).nonzero().flatten().tolist() for a, b in zip((kp, vp, pp), untouched)]
    assert all(set(pages) <= {5} for pages in changed) and changed[1] == [5] and changed[2] == [5]      # only sequence 1's own third page
    second = ops.kv_paged_token_decode(q, kp, vp, pp, lens_tensor((shared, shared + L)), table, is_causal=True)
    assert torch.equal(bits(second[0]), bits(first[0])) and not torch.equal(bits(second[1]), bits(first[1]))
    dense_k, dense_v, dense_p = (ff.nn.kv_cache.gather_pages(t, table) for t in (kp, vp, pp))
    want = ops.kv_token_decode(q, dense_k, dense_v, dense_p, lens_tensor((shared, shared + L)), is_causal=True)
    assert torch.equal(bits(second), bits(want))
    assert counts(entries, paged_token_append=1, paged_token_decode=2, token_decode=1)


# ---- the class --------------------------------------------------------------------------------------------------------------------------
def make_caches(dtype, E, P, num_pages, layout="pshe"):
    kq, vq = cases.quantizer(*K_BITS, E=E), cases.quantizer(*V_BITS, E=E, tile=True)
    paged_cache = ff.nn.PagedDynamicQuantizedKVCache(num_pages, P, HKV, E, kq, vq, B, C // P, dtype, DEV, layout=layout)
    return paged_cache, ff.nn.DynamicQuantizedKVCache(B, HKV, C, E, kq, vq, dtype, DEV)


def case_a_ragged_decode_loop_through_the_class(entries, dtype):
    """A ragged prompt, then 40 steps of append + attend at P = 16 (every sequence crosses at least two page boundaries), pages
    reserved ahead of the step that needs them: one call of each new entry point per step, every step's output the bits of the dense
    ``DynamicQuantizedKVCache`` fed the same rows, out of a pool a quarter of the dense cache's size."""
    E, G, P, steps, num_pages = 128, 4, 16, 40, 32
    rope, prompt, inputs = prompt_and_steps(E, dtype, G, steps, seed=17)
    cache, dense = make_caches(dtype, E, P, num_pages)
    assert num_pages * P == B * C // 4
    feed_prompt(cache, prompt, rope, reserve=True)
    feed_prompt(dense, prompt, rope, reserve=False)
    assert cache.lengths.tolist() == list(START) and counts(entries, paged_token_append=1, token_append=1)
    crossed = [0] * B
    for step, (k_t, v_t, q_t) in enumerate(inputs):
        for b in range(B):
            held = len(cache.pages(b))
            cache.reserve(b, START[b] + step + 1)
            crossed[b] += len(cache.pages(b)) - held
        cache.append(k_t, v_t, rope=rope)
        dense.append(k_t, v_t, rope=rope)
        got, want = cache.attend(q_t), dense.attend(q_t)
        assert torch.equal(bits(got), bits(want)), step
    torch.cuda.synchronize()
    assert counts(entries, paged_token_append=1 + steps, paged_token_decode=steps, token_append=1 + steps, token_decode=steps)
    assert cache.lengths.tolist() == [n + steps for n in START] and min(crossed) >= 2
    got_k, got_v, got_p = cache.dense()
    for b, n in enumerate(cache.lengths.tolist()):
        assert torch.equal(got_k[b, :, :n], dense.k_cache[b, :, :n]) and torch.equal(got_v[b, :, :n], dense.v_cache[b, :, :n])
        assert torch.equal(bits_of(got_p[b, :, :n]), bits_of(dense.params[b, :, :n]))
    assert cache.free_pages == num_pages - sum(-(-(n + steps) // P) for n in START)


def case_one_captured_step_replayed_while_the_table_grows(entries, dtype):
    """One step (append + attend) captured ONCE in a ``torch.cuda.graph`` on a side stream and replayed 20 times with new inputs in
    static buffers; between replays ``reserve`` writes a sequence's new page into ``block_table`` with a copy, outside the graph. The
    outputs, the table, the lengths and the three pools are the eager loop's."""
    E, G, P, steps, num_pages = 64, 4, 16, 20, 32
    rope, prompt, inputs = prompt_and_steps(E, dtype, G, steps, seed=18)
    eager, _ = make_caches(dtype, E, P, num_pages)
    feed_prompt(eager, prompt, rope, reserve=True)
    outs = []
    for step, (k_t, v_t, q_t) in enumerate(inputs):
        for b in range(B):
            eager.reserve(b, START[b] + step + 1)
        eager.append(k_t, v_t, rope=rope)
        outs.append(eager.attend(q_t))
    torch.cuda.synchronize()
    assert counts(entries, paged_token_append=1 + steps, paged_token_decode=steps)

    replayed, _ = make_caches(dtype, E, P, num_pages)
    feed_prompt(replayed, prompt, rope, reserve=True)
    for b in range(B):
        replayed.reserve(b, START[b] + 1)
    stores = (replayed.k_pool, replayed.v_pool, replayed.param_pool, replayed.lengths)
    snapshot = [t.clone() for t in stores]
    static = [t.clone() for t in inputs[0]]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):               # (a warm-up outside the capture, undone below)
        replayed.append(static[0], static[1], rope=rope)
        replayed.attend(static[2])
    torch.cuda.current_stream().wait_stream(stream)
    for buffer, saved in zip(stores, snapshot):
        buffer.copy_(saved)
    before = dict(entries)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        replayed.append(static[0], static[1], rope=rope)
        captured = replayed.attend(static[2])
    assert entries == {**before, NEW[0]: before[NEW[0]] + 1, NEW[1]: before[NEW[1]] + 1}
    assert replayed.lengths.tolist() == list(START)                                 # (a capture runs nothing)
    grew = 0
    for step in range(steps):
        for b in range(B):                        # host bookkeeping and the table's copy_, outside the graph
            held = len(replayed.pages(b))
            replayed.reserve(b, START[b] + step + 1)
            grew += len(replayed.pages(b)) - held
        for buffer, new in zip(static, inputs[step]):
            buffer.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(captured), bits(outs[step])), f"replay {step}"
        assert replayed.lengths.tolist() == [n + step + 1 for n in START]
    assert grew >= B                                                                # (every sequence took a page between replays)
    assert torch.equal(replayed.block_table, eager.block_table) and torch.equal(replayed.lengths, eager.lengths)
    assert torch.equal(replayed.k_pool, eager.k_pool) and torch.equal(replayed.v_pool, eager.v_pool)
    assert torch.equal(bits_of(replayed.param_pool), bits_of(eager.param_pool))
    assert entries[NEW[0]] == before[NEW[0]] + 1 and entries[NEW[1]] == before[NEW[1]] + 1   # (twenty replays, no further call)


# ---- the three tests: every case above over its grid ----------------------------------------------------------------------------------
DT = cases.DTYPES


def grid(**axes):
    """The product of the named axes as keyword dicts, the first axis slowest."""
    return [dict(zip(axes, values)) for values in itertools.product(*axes.values())]


def walk(entries, case, points):
    """`case(entries, **point)` at every point, the call counts zeroed ahead of each; a failure names the case and the point."""
    for point in points:
        for name in entries:
            entries[name] = 0
        try:
            case(entries, **point)
        except AssertionError as error:
            raise AssertionError(f"{case.__name__} at {point}: {error}") from error


APPEND = [
    (case_append_writes_exactly_its_rows_and_their_parameters, grid(dtype=DT, layout=cases.LAYOUTS, view=("contiguous", "projection"))),
    (case_append_on_constant_zero_one_sided_and_non_finite_rows, grid(dtype=DT, specs=((K_BITS, V_BITS), (V_BITS, K_BITS)))),
    (case_append_rotates_k_at_each_rows_own_position_then_quantizes, grid(dtype=DT, layout=cases.LAYOUTS)),
    (case_a_prompt_crosses_many_pages_in_one_call, grid(dtype=DT, P=(16, 256))),
]
DECODE = [
    (case_decode_is_the_dense_token_kernel_on_the_same_codes_and_parameters, grid(dtype=DT, E=cases.ES, G=cases.GROUPS, P=cases.PAGE_SIZES)),
    (case_uniform_parameters_give_the_static_paged_kernels_bits, grid(dtype=DT, E=cases.ES, P=(16, 128))),
    (case_reexpressed_rows_give_the_bits_of_the_per_tensor_pools, grid(dtype=DT, E=cases.ES, G=cases.GROUPS)),
    (case_known_answers_with_every_k_row_shifted, [dict(dtype=dtype, L=L, G=G, P=P) for dtype in DT for L, G in ((1, 4), (4, 4), (5, 1)) for P in (16, 256)]),
    (case_a_quantized_query_brings_its_own_parameters, grid(dtype=DT)),
    (case_a_nan_row_makes_its_own_sequence_nan_and_no_other, grid(dtype=DT, which=("k", "v"))),
    (case_the_output_quantizer_gives_the_dense_token_calls_bits, grid(dtype=DT)),
    (case_the_plan_hint_the_guards_and_pools_that_are_only_read, grid(plan_len=(None, 1, 200, 1024))),
]
TABLE_AND_CLASS = [
    (case_a_table_entry_outside_the_pool_touches_nothing, grid(dtype=DT, P=cases.PAGE_SIZES)),
    (case_two_sequences_share_their_prefix_pages_and_their_parameters, grid(dtype=DT, P=(16, 128))),
    (case_a_ragged_decode_loop_through_the_class, grid(dtype=DT)),
    (case_one_captured_step_replayed_while_the_table_grows, grid(dtype=DT)),
]


def test_append(entries):
    """Every append case: 20 points."""
    for case, points in APPEND:
        walk(entries, case, points)
    assert sum(len(points) for _, points in APPEND) == 8 + 4 + 4 + 4


def test_decode(entries):
    """Every decode case over valid tables: 72 points."""
    for case, points in DECODE:
        walk(entries, case, points)
    assert sum(len(points) for _, points in DECODE) == 32 + 8 + 8 + 12 + 2 + 4 + 2 + 4


def test_outside_entries_sharing_and_the_class(entries):
    """Table entries outside the pool, shared prefix pages, and the class eager and replayed from one graph: 16 points."""
    for case, points in TABLE_AND_CLASS:
        walk(entries, case, points)
    assert sum(len(points) for _, points in TABLE_AND_CLASS) == 8 + 4 + 2 + 2
