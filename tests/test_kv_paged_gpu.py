"""The int8 KV cache in pages on the MI355X (kv_paged_store_kernel in csrc/ffq_kv_cache.hip, kv_paged_partial_kernel in
csrc/ffq_sdpa_decode.hip, ops/kv_cache.py, nn/kv_cache.py; include/ffq_kv_paged.h).

Every assertion is an equality. Append: the pools start as a sentinel pattern inside a guarded arena; after ONE launch exactly the rows
``(table[b][pos / P], pos % P)`` of the positions an append covers hold the codes ``ops.kv_append`` writes for the same inputs into a
dense cache, every other byte of both pools (unowned pages included) is the sentinel and no guard byte moved. Decode: bit-equal to
``ops.kv_decode`` on the same codes laid out densely, at the same forced split count and at the rule's; operands whose answer is
known by construction give that answer. Table entries outside the pool touch nothing: the pool handed to the kernels is the middle
of a larger allocation, so a dereferenced -1 or `num_pages` would land in memory the test owns and would show. Every test counts the
calls of the two C entry points on the loaded library (one per served call, none for a refused one): a silent fallback fails."""

import pytest
import torch

import fastforward_amd as ff

import guards
import kv_paged_cases as cases

from fastforward_amd import _native, ops
from kv_paged_cases import B, C, HKV

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("ffq_kv_paged_append", "ffq_kv_paged_decode")
K_DEQ, V_DEQ = (0.031, 3.0), (0.027, -9.0)


@pytest.fixture
def entries(monkeypatch):
    """Calls of the two C entry points, counted on the loaded library itself."""
    lib = _native.library()
    count = dict.fromkeys(NAMES, 0)
    for name in NAMES:
        def counting(*args, _real=getattr(lib, name), _name=name):
            count[_name] += 1
            return _real(*args)
        monkeypatch.setattr(lib, name, counting)
    return count


def lens_tensor(lens):
    return torch.tensor(lens, dtype=torch.int32, device=DEV)


def scalars(scale, offset):
    return torch.tensor([scale], device=DEV), None if offset is None else torch.tensor([offset], device=DEV)


def bits(t):
    return t.view(torch.int16)


# ---- append ---------------------------------------------------------------------------------------------------------------------------
def new_rows(L, E, dtype, view, gen, batch=B):
    """k_new / v_new [batch, HKV, L, E] as `view` lays them out, with values on both clamps, on exact ties and not numbers at all."""
    def draw(centre, spread):
        x = torch.randn(batch, HKV, L, E, generator=gen) * spread + centre
        x[0, 0, 0, :8] = torch.tensor([1e4, -1e4, float("inf"), -float("inf"), float("nan"), 0.0, -0.0, centre])
        x[-1, -1, -1, :4] = torch.tensor([0.5, 1.5, 2.5, -0.5]) * spread
        return x.to(dtype).to(DEV)

    k, v = draw(-9.3, 2.0), draw(40.0, 0.5)
    if view == "projection":    # the projection's [B, L, HKV * E] output seen as [B, L, HKV, E].transpose(1, 2)
        k, v = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (k, v))
        assert L == 1 or not k.is_contiguous()
    return k, v


def sentinel_pools(arena, num_pages, P, E, layout):
    pools = []
    for name in ("k", "v"):
        plain = cases.pool_of(num_pages, P, E, layout, DEV, fill=cases.SENTINEL)
        inside = arena.adopt(plain if layout == "phse" else plain.transpose(1, 2), f"{name} pool")
        pools.append(inside if layout == "phse" else inside.transpose(1, 2))
    return pools


def dense_reference(k_new, v_new, lens, k_spec, v_spec, rope, capacity=C):
    """What ``ops.kv_append`` writes for the same inputs into dense sentinel caches [B, HKV, capacity, E]."""
    batch, E = k_new.shape[0], k_new.shape[-1]
    kc, vc = (torch.full((batch, HKV, capacity, E), cases.SENTINEL, dtype=torch.int8, device=DEV) for _ in range(2))
    ops.kv_append(k_new, v_new, kc, vc, lens_tensor(lens), cases.params(k_spec, DEV), cases.params(v_spec, DEV), rope=rope)
    return kc, vc


def check_append(entries, dtype, E, L, lens, P, layout, view, k_spec, v_spec, with_rope, seed=0):
    gen = torch.Generator().manual_seed(seed + L + E + P)
    k_new, v_new = new_rows(L, E, dtype, view, gen)
    rows, num_pages = cases.page_table(P)
    arena = guards.Arena(guards.POISON_A)
    kp, vp = sentinel_pools(arena, num_pages, P, E, layout)
    rope = tuple(torch.randn(C + 5, E, generator=gen).to(dtype).to(DEV) for _ in range(2)) if with_rope else None
    before = entries["ffq_kv_paged_append"]
    ops.kv_paged_append(k_new, v_new, kp, vp, lens_tensor(lens), cases.table_tensor(rows, DEV), cases.params(k_spec, DEV), cases.params(v_spec, DEV), rope=rope)
    torch.cuda.synchronize()
    assert entries["ffq_kv_paged_append"] == before + 1
    kc, vc = dense_reference(k_new, v_new, lens, k_spec, v_spec, rope)
    want_k = cases.scatter(kc, rows, cases.pool_of(num_pages, P, E, "phse", DEV, fill=cases.SENTINEL))
    want_v = cases.scatter(vc, rows, cases.pool_of(num_pages, P, E, "phse", DEV, fill=cases.SENTINEL))
    assert torch.equal(kp, want_k), f"K: {int((kp != want_k).sum())} bytes differ ({dtype}, E={E}, L={L}, lens={lens}, P={P})"
    assert torch.equal(vp, want_v), f"V: {int((vp != want_v).sum())} bytes differ ({dtype}, E={E}, L={L}, lens={lens}, P={P})"
    written = sum(len(cases.positions(n, L)) for n in lens) * HKV * E
    assert int((kp != cases.SENTINEL).sum()) <= written                    # (a code may equal the sentinel; nothing else may differ from it)
    assert not arena.touched_guards(), arena.touched_guards()


@pytest.mark.parametrize("view", ["contiguous", "projection"])
@pytest.mark.parametrize("layout", cases.LAYOUTS)
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_append_writes_exactly_its_rows(entries, dtype, layout, view):
    """8-bit K and 4-bit V with real offsets beyond int8, NaN and +-Inf among the inputs; L = 1, 4, 5 over the three length sets and
    the four page sizes."""
    for E in cases.ES:
        for L in cases.LS:
            for lens in cases.LENS_SETS:
                for P in cases.PAGE_SIZES:
                    check_append(entries, dtype, E, L, lens, P, layout, view, cases.K_SPEC, cases.V_SPEC, with_rope=False)
    assert entries["ffq_kv_paged_append"] == 2 * 3 * 3 * 4
    # exact ties of a power-of-two scale, and a quantizer without an offset
    check_append(entries, dtype, 128, 4, (4, 130, 511, 3), 32, layout, view, (8, 2.0, None), (4, 0.5, -2.0), with_rope=False, seed=3)
    # a refused call reaches no entry point
    rows, num_pages = cases.page_table(16)
    k_new, v_new = new_rows(1, 64, dtype, view, torch.Generator().manual_seed(0))
    pool = cases.pool_of(num_pages, 16, 64, layout, DEV)
    with pytest.raises(RuntimeError):
        ops.kv_paged_append(k_new, v_new, pool, pool, lens_tensor((1, 1, 1, 1)).long(), cases.table_tensor(rows, DEV), cases.params(cases.K_SPEC, DEV),
                            cases.params(cases.V_SPEC, DEV))
    assert entries["ffq_kv_paged_append"] == 2 * 3 * 3 * 4 + 1


@pytest.mark.parametrize("layout", cases.LAYOUTS)
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_append_rotates_k_at_each_rows_own_position(entries, dtype, layout):
    """With rotary tables the table row is the row's position in its SEQUENCE, whatever page it lands in."""
    for E in cases.ES:
        for L, view in ((1, "projection"), (4, "contiguous"), (5, "projection")):
            for lens in cases.LENS_SETS:
                for P in (16, 128):
                    check_append(entries, dtype, E, L, lens, P, layout, view, (8, 0.11, 20.5), cases.V_SPEC, with_rope=True, seed=11)
    assert entries["ffq_kv_paged_append"] == 2 * 3 * 3 * 2


@pytest.mark.parametrize("P", [16, 256])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_a_prompt_crosses_many_pages_in_one_call(entries, dtype, P):
    """L = 300 in one launch at ragged targets: whole inside the sequence, ending on its last position, cut at the capacity, cut at its
    start."""
    L, E, lens = 300, 128, (300, 512, 600, 120)
    assert [len(cases.positions(n, L)) for n in lens] == [300, 300, 212, 120]
    check_append(entries, dtype, E, L, lens, P, "pshe", "contiguous", cases.K_SPEC, cases.V_SPEC, with_rope=True, seed=5)
    assert entries["ffq_kv_paged_append"] == 1


# ---- decode -----------------------------------------------------------------------------------------------------------------------------
def random_codes(E, seed, batch=B, capacity=C):
    gen = torch.Generator().manual_seed(seed)
    return tuple(torch.randint(-128, 128, (batch, HKV, capacity, E), generator=gen).to(torch.int8).to(DEV) for _ in range(2))


def paged(dense_k, dense_v, P, layout, fill=0):
    """(k_pool, v_pool, table tensor): the dense codes scattered over the seeded page assignment; unowned pages hold `fill`."""
    rows, num_pages = cases.page_table(P, batch=dense_k.shape[0], capacity=dense_k.shape[2])
    E = dense_k.shape[-1]
    kp = cases.scatter(dense_k, rows, cases.pool_of(num_pages, P, E, layout, DEV, fill=fill))
    vp = cases.scatter(dense_v, rows, cases.pool_of(num_pages, P, E, layout, DEV, fill=fill))
    return kp, vp, cases.table_tensor(rows, DEV)


@pytest.mark.parametrize("P", cases.PAGE_SIZES)
@pytest.mark.parametrize("G", cases.GROUPS)
@pytest.mark.parametrize("E", cases.ES)
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_decode_is_the_dense_kernel_on_the_same_codes(entries, dtype, E, G, P):
    """Bit for bit against ``ops.kv_decode`` on the densely laid out codes, at every forced split count and at the rule's, without a
    mask and with bottom-right causality, in both pool layouts; exact zeros for a sequence without keys and for rows that see none."""
    kc, vc = random_codes(E, seed=E + G)
    deq = (None, scalars(*K_DEQ), scalars(*V_DEQ))
    gen = torch.Generator().manual_seed(G)
    calls = 0
    for layout in cases.LAYOUTS:
        kp, vp, table = paged(kc, vc, P, layout, fill=cases.SENTINEL)
        for L in cases.LS:
            q = torch.randn(B, HKV * G, L, E, generator=gen).to(dtype).to(DEV)
            for lens in cases.LENS_SETS:
                device_lens = lens_tensor(lens)
                for causal in (False, True):
                    for splits in cases.SPLITS:
                        got = ops.kv_paged_decode(q, kp, vp, device_lens, table, is_causal=causal, dequant=deq, splits=splits)
                        calls += 1
                        dense = ops.kv_decode(q, kc, vc, device_lens, is_causal=causal, dequant=deq, splits=splits)
                        assert torch.equal(bits(got), bits(dense)), (layout, L, lens, causal, splits)
                        for b, n in enumerate(lens):
                            S = cases.clamp_len(n)
                            if S == 0:
                                assert torch.equal(got[b], torch.zeros_like(got[b])), (L, lens, causal, splits)
                            elif causal and S < L:
                                assert torch.equal(got[b, :, :L - S], torch.zeros_like(got[b, :, :L - S]))
    assert entries["ffq_kv_paged_decode"] == calls == 2 * 3 * 3 * 2 * 5


@pytest.mark.parametrize("P", [16, 256])
@pytest.mark.parametrize("L,G", [(1, 4), (4, 4), (5, 1)])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_known_answers_through_the_block_table(entries, dtype, L, G, P):
    """select / staircase / uniform cut to each sequence's own key count (kv_paged_cases.exact_case): the answer itself, with ``==``,
    under every split count, with and without bottom-right causality."""
    for E in cases.ES:
        for kind, causal in (("select", False), ("staircase", False), ("staircase", True), ("uniform", False), ("uniform", True)):
            for lens in cases.LENS_SETS:
                q, kc, vc, k_param, v_param, expected = cases.exact_case(kind, causal, L, G, E, dtype, lens)
                kp, vp, table = paged(kc.to(DEV), vc.to(DEV), P, "pshe" if P == 16 else "phse")
                deq = (None, scalars(*k_param), scalars(*v_param))
                for splits in cases.SPLITS:
                    got = ops.kv_paged_decode(q.to(DEV), kp, vp, lens_tensor(lens), table, is_causal=causal, dequant=deq, splits=splits)
                    same = got.cpu().double() == expected
                    assert bool(same.all()), f"{kind} causal={causal} E={E} lens={lens} splits={splits}: {int((~same).sum())} elements differ, first at {(~same).nonzero()[0].tolist()}"
    assert entries["ffq_kv_paged_decode"] == 2 * 5 * 3 * 5


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_the_output_quantizer_gives_the_dense_calls_bits(entries, dtype):
    E, L, G = 128, 2, 4
    kc, vc = random_codes(E, seed=31)
    q = torch.randn(B, HKV * G, L, E, generator=torch.Generator().manual_seed(31)).to(dtype).to(DEV)
    deq = (None, scalars(*K_DEQ), scalars(*V_DEQ))
    for P, layout in ((16, "phse"), (128, "pshe")):
        kp, vp, table = paged(kc, vc, P, layout)
        for lens in cases.LENS_SETS:
            for out_bits, step, offset in ((8, 2.0**-5, 3.0), (4, 2.0**-2, -1.0), (8, 0.013, None)):
                for splits in (0, 3):
                    quantizer = (*scalars(step, offset), float(out_bits))
                    got = ops.kv_paged_decode(q, kp, vp, lens_tensor(lens), table, is_causal=True, dequant=deq, output_quantizer=quantizer, splits=splits)
                    dense = ops.kv_decode(q, kc, vc, lens_tensor(lens), is_causal=True, dequant=deq, output_quantizer=quantizer, splits=splits)
                    assert got.dtype == dtype and torch.equal(bits(got), bits(dense)), (P, lens, out_bits, splits)
    assert entries["ffq_kv_paged_decode"] == 2 * 3 * 3 * 2


@pytest.mark.parametrize("plan_len", [None, 1, 200, 1024])
def test_the_output_and_the_workspace_are_guarded_and_the_plan_hint_names_the_count(entries, plan_len):
    """``splits = 0`` takes ``sdpa_decode_plan`` at `plan_len` keys (the capacity by default): seen in the workspace the call takes
    inside a guarded arena (tests/guards.py), under two poisons; the result is the forced count's, whatever the workspace held."""
    Bp, Hp, cap, E, L, G, P = 1, 2, 1024, 128, 2, 4, 128
    assert [ops.sdpa_decode_plan(Bp, Hp, n, L * G, E) for n in (1, 200, 1024)] == [1, 1, 4]
    count = ops.sdpa_decode_plan(Bp, Hp, plan_len or cap, L * G, E)
    gen = torch.Generator().manual_seed(2)
    q = torch.randn(Bp, Hp * G, L, E, generator=gen).bfloat16().to(DEV)
    kc, vc = (torch.randint(-128, 128, (Bp, Hp, cap, E), generator=gen).to(torch.int8).to(DEV) for _ in range(2))
    kp, vp, table = paged(kc, vc, P, "phse")
    lens, deq = lens_tensor([700]), (None, scalars(*K_DEQ), scalars(*V_DEQ))
    results = []
    for poison in (guards.POISON_A, guards.POISON_B):
        arena = guards.Arena(poison)
        with guards.capture(arena):
            out = ops.kv_paged_decode(q, kp, vp, lens, table, is_causal=True, dequant=deq, plan_len=plan_len)
        torch.cuda.synchronize()
        fresh = sorted(b.nbytes for b in arena.blocks if b.kind == "fresh")
        assert fresh == sorted([out.numel() * 2, ops.sdpa_decode_workspace_bytes(Bp, Hp, L * G, E, count)]) and arena.find(out.data_ptr()) is not None
        assert not arena.touched_guards(), arena.touched_guards()
        results.append(out.clone())
    forced = ops.kv_paged_decode(q, kp, vp, lens, table, is_causal=True, dequant=deq, splits=count)
    assert torch.equal(bits(results[0]), bits(results[1])) and torch.equal(bits(results[0]), bits(forced))
    assert torch.equal(bits(forced), bits(ops.kv_decode(q, kc, vc, lens, is_causal=True, dequant=deq, splits=count)))
    assert entries["ffq_kv_paged_decode"] == 3


# ---- table entries outside the pool ---------------------------------------------------------------------------------------------------
EXTRA = 2  # pages the test owns on either side of the pool it hands to the kernels


def middle_pools(num_pages, P, E, layout, fill):
    """Two allocations of num_pages + 2 * EXTRA pages holding `fill`, and their middle `num_pages` pages as the pools."""
    whole = [cases.pool_of(num_pages + 2 * EXTRA, P, E, layout, DEV, fill=fill) for _ in range(2)]
    return whole, [t[EXTRA:EXTRA + num_pages] for t in whole]


def bad_table(P, rows, num_pages):
    """The seeded assignment with entries in use replaced by -1 and by `num_pages` (the pages just outside the pool on either side);
    the last sequence's FIRST page is invalid, so at a length within one page it has no valid key at all."""
    rows = [list(r) for r in rows]
    rows[0][1 % len(rows[0])] = -1
    rows[1][0] = num_pages
    rows[2][-1] = num_pages
    rows[2][len(rows[2]) // 2] = -1
    rows[3][0] = -1
    return rows


@pytest.mark.parametrize("P", cases.PAGE_SIZES)
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_a_table_entry_outside_the_pool_touches_nothing(entries, dtype, P):
    """The pool is the middle of an allocation with two sentinel pages on each side: entries -1 and `num_pages` would land there.
    Append leaves those pages and the skipped rows at the sentinel. Decode equals ``ops.sdpa_decode`` on the densely laid out codes
    with a bool mask that hides the keys of those entries; a sequence whose only page is invalid gives exact zeros."""
    E, G = 128, 4
    good, num_pages = cases.page_table(P)
    rows = bad_table(P, good, num_pages)
    table = cases.table_tensor(rows, DEV)
    layout = "phse" if P in (16, 128) else "pshe"
    # ---- append: a prompt over the whole capacity, so that every entry is in use
    L, lens = 300, (300, 512, 512, 10)
    gen = torch.Generator().manual_seed(P)
    k_new, v_new = (torch.randn(B, HKV, L, E, generator=gen).to(dtype).to(DEV) for _ in range(2))
    whole, (kp, vp) = middle_pools(num_pages, P, E, layout, cases.SENTINEL)
    ops.kv_paged_append(k_new, v_new, kp, vp, lens_tensor(lens), table, cases.params(cases.K_SPEC, DEV), cases.params(cases.V_SPEC, DEV))
    torch.cuda.synchronize()
    kc, vc = dense_reference(k_new, v_new, lens, cases.K_SPEC, cases.V_SPEC, None)
    for got, dense in ((whole[0], kc), (whole[1], vc)):
        want = cases.pool_of(num_pages + 2 * EXTRA, P, E, "phse", DEV, fill=cases.SENTINEL)
        cases.scatter(dense, rows, want[EXTRA:EXTRA + num_pages])       # (scatter skips the entries outside the pool)
        assert torch.equal(got, want), f"{int((got != want).sum())} bytes differ"
        assert bool((got[:EXTRA] == cases.SENTINEL).all()) and bool((got[-EXTRA:] == cases.SENTINEL).all())
    assert entries["ffq_kv_paged_append"] == 1
    # ---- decode: random codes everywhere, the extra pages included
    dense_k, dense_v = random_codes(E, seed=P)
    whole, (kp, vp) = middle_pools(num_pages, P, E, layout, 0)
    for t in whole:
        t.copy_(torch.randint(-128, 128, tuple(t.shape), generator=gen).to(torch.int8))
    cases.scatter(dense_k, rows, kp)
    cases.scatter(dense_v, rows, vp)
    deq = (None, scalars(*K_DEQ), scalars(*V_DEQ))
    hidden = torch.tensor([[not 0 <= page < num_pages for page in row] for row in rows]).repeat_interleave(P, dim=1).to(DEV)   # [B, C]
    calls = 0
    for L in (1, 5):
        q = torch.randn(B, HKV * G, L, E, generator=gen).to(dtype).to(DEV)
        for lens in ((300, 512, 530, P), (P + 1, 17, 512, 1)):
            for causal in (False, True):
                for splits in (0, 1, 3):
                    got = ops.kv_paged_decode(q, kp, vp, lens_tensor(lens), table, is_causal=causal, dequant=deq, splits=splits)
                    calls += 1
                    count = splits or ops.sdpa_decode_plan(B, HKV, C, L * G, E)
                    for b, n in enumerate(lens):
                        S = cases.clamp_len(n)
                        mask = ~hidden[b, :S].unsqueeze(0).expand(L, S)
                        if causal:
                            mask = mask & cases.bottom_right(L, S, DEV)
                        want = ops.sdpa_decode(q[b:b + 1], dense_k[b:b + 1, :, :S], dense_v[b:b + 1, :, :S], attn_mask=mask, dequant=deq, splits=count)
                        assert torch.equal(bits(got[b:b + 1]), bits(want)), (L, lens, b, causal, splits)
                    assert torch.equal(got[3], torch.zeros_like(got[3]))     # (its keys are all on the invalid first page)
    assert entries["ffq_kv_paged_decode"] == calls == 2 * 2 * 2 * 3


# ---- sharing --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [16, 128])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_two_sequences_share_their_prefix_pages(entries, dtype, P):
    """Two table rows that point at the same physical prefix pages give identical bits for identical queries; appending to one of them
    after the shared prefix leaves the other's output as it was."""
    E, G, L, per, num_pages = 64, 4, 3, 4, 11
    shared = 2 * P
    rows = [[7, 2, 9, 4], [7, 2, 5, 0]]
    table = cases.table_tensor(rows, DEV)
    gen = torch.Generator().manual_seed(P)
    kp, vp = (cases.pool_of(num_pages, P, E, "pshe", DEV) for _ in range(2))
    for t in (kp, vp):
        t.copy_(torch.randint(-128, 128, tuple(t.shape), generator=gen).to(torch.int8))
    deq = (None, scalars(cases.K_SPEC[1], cases.K_SPEC[2]), scalars(cases.V_SPEC[1], cases.V_SPEC[2]))
    q = torch.randn(1, HKV * G, L, E, generator=gen).to(dtype).to(DEV).expand(2, -1, -1, -1).contiguous()
    first = ops.kv_paged_decode(q, kp, vp, lens_tensor((shared, shared)), table, is_causal=True, dequant=deq)
    assert torch.equal(bits(first[0]), bits(first[1])) and bool(first.any())
    # three rows for sequence 1 alone (sequence 0's target is parked below zero: its rows are dropped)
    k_new, v_new = new_rows(L, E, dtype, "contiguous", gen, batch=2)
    untouched = [t.clone() for t in (kp, vp)]
    ops.kv_paged_append(k_new, v_new, kp, vp, lens_tensor((-L, shared + L)), table, cases.params(cases.K_SPEC, DEV), cases.params(cases.V_SPEC, DEV))
    changed = [(a != b).flatten(1).any(1).nonzero().flatten().tolist() for a, b in zip((kp, vp), untouched)]
    assert all(set(pages) <= {5} for pages in changed) and changed[1] == [5]      # only sequence 1's own third page
    second = ops.kv_paged_decode(q, kp, vp, lens_tensor((shared, shared + L)), table, is_causal=True, dequant=deq)
    assert torch.equal(bits(second[0]), bits(first[0])) and not torch.equal(bits(second[1]), bits(first[1]))
    dense_k, dense_v = (ff.nn.kv_cache.gather_pages(t, table) for t in (kp, vp))
    want = ops.kv_decode(q, dense_k, dense_v, lens_tensor((shared, shared + L)), is_causal=True, dequant=deq)
    assert torch.equal(bits(second), bits(want))
    assert entries["ffq_kv_paged_append"] == 1 and entries["ffq_kv_paged_decode"] == 2


# ---- the class --------------------------------------------------------------------------------------------------------------------------
START = (0, 5, 20, 100)


def make_caches(dtype, E, P, num_pages, layout="pshe"):
    kq, vq = cases.quantizer(cases.K_SPEC, DEV), cases.quantizer(cases.V_SPEC, DEV)
    paged_cache = ff.nn.PagedQuantizedKVCache(num_pages, P, HKV, E, kq, vq, B, C // P, dtype, DEV, layout=layout)
    return paged_cache, ff.nn.QuantizedKVCache(B, HKV, C, E, kq, vq, dtype, DEV)


def prompt_and_steps(E, dtype, G, steps, seed):
    gen = torch.Generator().manual_seed(seed)
    rope = tuple(torch.randn(C, E, generator=gen).to(dtype).to(DEV) for _ in range(2))
    prompt = tuple(torch.randn(B, HKV, max(START), E, generator=gen).to(dtype).to(DEV) for _ in range(2))
    inputs = [tuple(torch.randn(B, heads, 1, E, generator=gen).to(dtype).to(DEV) for heads in (HKV, HKV, HKV * G)) for _ in range(steps)]
    return rope, prompt, inputs


def feed_prompt(cache, prompt, rope, reserve):
    """Sequence b keeps the prompt's last START[b] rows: the lengths start below zero and ``append`` adds L = max(START) itself."""
    if reserve:
        for b in (2, 0, 3, 1):                 # (out of order, so that the sequences' pages interleave in the pool)
            cache.reserve(b, START[b])
    cache.lengths.copy_(torch.tensor([n - max(START) for n in START], dtype=torch.int32))
    cache.append(*prompt, rope=rope)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_a_ragged_decode_loop_through_the_class(entries, dtype):
    """A ragged prompt, then 40 steps of append + attend at P = 16 (every sequence crosses at least two page boundaries), pages
    reserved ahead of the step that needs them: one call of each entry point per step, every step's output the bits of the dense
    ``QuantizedKVCache`` fed the same rows, out of a pool a quarter of the dense cache's size."""
    E, G, P, steps, num_pages = 128, 4, 16, 40, 32
    rope, prompt, inputs = prompt_and_steps(E, dtype, G, steps, seed=17)
    cache, dense = make_caches(dtype, E, P, num_pages)
    assert num_pages * P == B * C // 4
    feed_prompt(cache, prompt, rope, reserve=True)
    feed_prompt(dense, prompt, rope, reserve=False)
    assert cache.lengths.tolist() == list(START) and entries["ffq_kv_paged_append"] == 1
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
    assert entries["ffq_kv_paged_append"] == 1 + steps and entries["ffq_kv_paged_decode"] == steps
    assert cache.lengths.tolist() == [n + steps for n in START] and min(crossed) >= 2
    got_k, got_v = cache.dense()
    for b, n in enumerate(cache.lengths.tolist()):
        assert torch.equal(got_k[b, :, :n], dense.k_cache[b, :, :n]) and torch.equal(got_v[b, :, :n], dense.v_cache[b, :, :n])
    assert cache.free_pages == num_pages - sum(-(-(n + steps) // P) for n in START)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_one_captured_step_replayed_while_the_table_grows(entries, dtype):
    """One step (append + attend) captured ONCE in a ``torch.cuda.graph`` on a side stream and replayed 20 times with new inputs in
    static buffers; between replays ``reserve`` writes a sequence's new page into ``block_table`` with a copy, outside the graph. The
    outputs are the eager loop's bits and the pools the eager pools."""
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
    assert entries["ffq_kv_paged_append"] == 1 + steps and entries["ffq_kv_paged_decode"] == steps

    replayed, _ = make_caches(dtype, E, P, num_pages)
    feed_prompt(replayed, prompt, rope, reserve=True)
    for b in range(B):
        replayed.reserve(b, START[b] + 1)
    snapshot = (replayed.k_pool.clone(), replayed.v_pool.clone(), replayed.lengths.clone())
    static = [t.clone() for t in inputs[0]]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):               # (a warm-up outside the capture, undone below)
        replayed.append(static[0], static[1], rope=rope)
        replayed.attend(static[2])
    torch.cuda.current_stream().wait_stream(stream)
    replayed.k_pool.copy_(snapshot[0])
    replayed.v_pool.copy_(snapshot[1])
    replayed.lengths.copy_(snapshot[2])
    before = dict(entries)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        replayed.append(static[0], static[1], rope=rope)
        captured = replayed.attend(static[2])
    assert entries["ffq_kv_paged_append"] == before["ffq_kv_paged_append"] + 1 and entries["ffq_kv_paged_decode"] == before["ffq_kv_paged_decode"] + 1
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
    assert torch.equal(replayed.block_table, eager.block_table)
    assert torch.equal(replayed.k_pool, eager.k_pool) and torch.equal(replayed.v_pool, eager.v_pool)
    assert entries["ffq_kv_paged_append"] == before["ffq_kv_paged_append"] + 1      # (twenty replays, no further call)
