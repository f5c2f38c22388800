"""The drawn decode-attention cases (tests/decode_cases.py) without a GPU: the coverage the list promises, the premises of every
case (its known-answer patterns build, its keys and queries fit int8 codes, the predicate takes the call as built, views and mask
forms included, and the split plan covers every key once), the fp32 domain of the kernel's biased dequantization, and the relations
of tests/test_sdpa_decode_cases_gpu.py applied to a pure-torch model of the kernel's indexing, where each planted defect must make
its relation fail."""

import collections
import dataclasses
import itertools

import pytest
import torch

import attention_exact as ax
import decode_cases as dc

from fastforward_amd import fused_sdpa_decode, ops
from fastforward_amd.ops import decode
from test_sdpa_decode_cpu import as_codes

CASES = dc.drawn()
IDS = [f"{c.index:02d}" for c in CASES]


# ---- the list -----------------------------------------------------------------------------------------------------------------------------
def test_the_list_is_the_same_every_time_and_holds_what_it_promises():
    assert len(CASES) == 48 and CASES == dc.drawn(48) and len({c.id for c in CASES}) == 48
    assert len({c.seed for c in CASES}) == 48
    domain = {"row": dc.ROWS, "group": dc.GROUPS, "S": dc.KEYS, "E": dc.WIDTHS, "dtype": dc.DTYPES, "mask": dc.MASKS, "mask_form": dc.FORMS,
              "q_container": dc.CONTAINERS, "splits": dc.SPLITS, "layout": dc.LAYOUTS}
    seen = {name: collections.Counter() for name in domain}
    for c in CASES:
        for name, value in (("row", (c.L, c.G)), ("group", (c.B, c.HKV)), ("S", c.S), ("E", c.E), ("dtype", c.dtype), ("mask", c.mask),
                            ("q_container", c.q_container), ("splits", c.splits), ("layout", c.layout)):
            assert value in domain[name], (name, value)
            seen[name][value] += 1
        assert (c.mask_form is not None) is (c.mask in dc.EXPLICIT)
        if c.mask_form is not None:
            seen["mask_form"][c.mask_form] += 1
            assert c.mask_form != "byte_offset" or c.mask == "bool"
    for name, values in domain.items():
        assert all(seen[name][v] >= 3 for v in values), (name, seen[name])
    # the five (L, G) with a non-power-of-two L and G > 1 meet every mask kind
    assert all(L & (L - 1) and G > 1 for L, G in dc.FIRST_FIVE)
    assert {((c.L, c.G), c.mask) for c in CASES} >= set(itertools.product(dc.FIRST_FIVE, dc.MASKS))
    # every layout meets an explicit mask, int8 q and a forced split count above one
    for layout in dc.LAYOUTS:
        mine = [c for c in CASES if c.layout == layout]
        assert any(c.mask in dc.EXPLICIT for c in mine) and any(c.q_container == "int8" for c in mine) and any(c.splits > 1 for c in mine), layout
    # no case is refused by the kernel's own limits, and every layout and mask form claims something at its case's shape
    for c in CASES:
        assert c.rows <= decode.MAX_ROWS and c.H % c.HKV == 0 and 1 <= c.count <= decode.MAX_SPLITS
        assert c.layout in dc.layouts_of(c) and (c.mask_form is None or c.mask_form in dc.forms_of(c, c.mask))
        assert len(c.picks) == 3 and all(b < c.B and head < c.H and l < c.L for b, head, l in c.picks)
    assert max(c.B * c.H * c.S * c.E for c in CASES) < 2**27


# ---- the premises of every case ---------------------------------------------------------------------------------------------------------------
def _quantized(c, dtype):
    return c.raw if c.scale is None else as_codes(c.raw, c.scale, c.offset, dtype)


def _accepted(case, q, k, v, mask, causal, scale=None):
    with torch.no_grad():
        return fused_sdpa_decode.KERNELS.supported(query=_quantized(q, case.dtype), key=_quantized(k, case.dtype), value=_quantized(v, case.dtype),
                                                   attn_mask=mask, is_causal=causal, scale=scale, enable_gqa=True, strict_quantization=False)


@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_premises(monkeypatch, index):
    monkeypatch.setattr("fastforward_amd.fused_sdpa_decode._on_device", lambda *t: True)
    case = CASES[index]
    print(case.id)
    patterns = dc.known(index)  # (an AssertionError here is a pattern over the residual limit or a value that does not fit its codes)
    want = {"none": ["select", "staircase", "uniform"], "causal": ["select", "staircase"], "bool": ["uniform"], "float32": ["mask_select"], "float": ["mask_select"]}
    assert [w in known.pattern.name for known, w in zip(patterns, want[case.mask])] == [True] * len(want[case.mask]) == [True] * len(patterns)
    for known in patterns:
        p = known.pattern
        assert p.residual <= ax.RESIDUAL_LIMIT and p.shape == case.shape and p.dtype == case.dtype and p.causal is (case.mask == "causal")
        # the codes dequantize to exactly what the expectation was built from, in every container
        for coded, plain in ((known.q, p.q), (known.k, p.k), (known.v, p.v)):
            assert torch.equal(dc.values(coded, case.dtype).double(), plain.double())
        assert known.k.raw.dtype == known.v.raw.dtype == torch.int8
        assert known.q.raw.dtype == {"plain": case.dtype, "int8": torch.int8, "dtype": case.dtype}[case.q_container] and (known.q.scale is None) is (case.q_container == "plain")
        if case.layout == "batch_expand":
            assert torch.equal(p.k, p.k[:1].expand_as(p.k)) and torch.equal(p.v, p.v[:1].expand_as(p.v))
        # the call as the GPU test makes it: views and mask form included
        q, k, v = dc.laid_out(case.layout, known.q, known.k, known.v)
        assert all(torch.equal(view.raw, c.raw) for view, c in zip((q, k, v), known[1:]))
        mask = None if p.mask is None else dc.in_form(case, case.mask_form, p.mask)
        if mask is not None:
            assert torch.equal(dc.dense(case, mask), dc.dense(case, p.mask)) and mask.dtype == {"bool": torch.bool, "float32": torch.float32, "float": case.dtype}[case.mask]
        assert _accepted(case, q, k, v, mask, p.causal, p.scale), p
    # the random operands of the relations, in the case's layout and in every other one
    for layout in dc.layouts_of(case):
        call = dc.call_of(case, layout=layout)
        assert _accepted(case, call.q, call.k, call.v, call.mask, call.causal), layout
    call = dc.call_of(case, trade=True)
    assert all(int(c.raw.min()) >= -100 and int(c.raw.max()) <= 100 for c in (call.k, call.v))
    for kind in dc.EXPLICIT:
        for form in dc.forms_of(case, kind):
            assert _accepted(case, call.q, call.k, call.v, dc.in_form(case, form, dc.random_mask(case, kind, form)), False), (kind, form)
    # the plan: the C query's count, every key in exactly one split (a forced count may leave splits empty)
    assert case.count == (case.splits or ops.sdpa_decode_plan(case.B, case.HKV, case.S, case.rows, case.E))
    ranges = decode.sdpa_decode_split_ranges(case.S, case.count)
    assert len(ranges) == case.count and ranges[0][0] == 0 and ranges[-1][1] == case.S and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    assert all(begin <= end for begin, end in ranges) and (case.splits or all(begin < end for begin, end in ranges))


def test_the_rule_takes_more_than_one_branch_on_the_list():
    """`plan_splits` at the list's group counts and key lengths: one split up to three tiles, two from the fourth tile on (385 keys),
    more at 2049; a rule's count and a forced one both occur above one split."""
    counts = {(c.B * c.HKV, c.S): ops.sdpa_decode_plan(c.B, c.HKV, c.S, c.rows, c.E) for c in CASES}
    assert {n for (_, S), n in counts.items() if S <= 384} == {1} and {n for (_, S), n in counts.items() if 385 <= S <= 513} == {2}
    assert min(n for (_, S), n in counts.items() if S == 2049) > 2 and len({groups for groups, _ in counts}) == 5
    assert any(c.splits == 0 and c.count > 1 for c in CASES)


# ---- the biased dequantization in fp32 -------------------------------------------------------------------------------------------------------------
EXACT_BELOW = 2**24 - 127  # the identity holds for every |rne(offset)| below this


def _both_forms(offsets):
    """((c + 128) + (rne(o) - 128), c + rne(o)) in float32 for all 256 codes x `offsets` (float32)."""
    c = torch.arange(-128, 128, dtype=torch.float32).reshape(-1, 1)
    ro = torch.round(offsets.to(torch.float32)).reshape(1, -1)
    biased = (c + torch.tensor(128.0)) + (ro - torch.tensor(128.0))
    return biased, c + ro


def test_the_biased_dequantization_is_exact_below_2_24_minus_127_and_not_beyond():
    """dequant4 adds the unsigned byte c + 128 to rne(o) - 128. Both operands and the sum c + rne(o) are integers: below 2^24 each is
    exact in fp32 and the addition rounds nothing, so it has the bits of (float)c + rne(o). At rne(o) = -(2^24 - 127) the bias term is
    -(2^24 + 1), which fp32 rounds to -2^24 before any code is added: from there on the two forms may differ by one ulp."""
    near_23 = torch.arange(2**23 - 300, 2**23 + 301, dtype=torch.float64)
    near_24 = torch.arange(2**24 - 300, 2**24 - 127, dtype=torch.float64)
    assert float(near_24.max()) == EXACT_BELOW - 1
    small = torch.tensor([0.5, 2.5, 200.0], dtype=torch.float64)
    offsets = torch.cat([small, -small, near_23, -near_23, near_24, -near_24])
    assert bool((offsets.to(torch.float32).double() == offsets).all())
    biased, direct = _both_forms(offsets)
    assert biased.dtype == direct.dtype == torch.float32 and biased.shape == (256, offsets.numel())
    assert torch.equal(biased.view(torch.int32), direct.view(torch.int32))
    assert float(offsets.abs().max()) == EXACT_BELOW - 1
    # an offset of 2.5 is 2, one of -0.5 is -0 (ties to even)
    assert torch.equal(_both_forms(torch.tensor([2.5, -0.5]))[0], _both_forms(torch.tensor([2.0, 0.0]))[0])
    # just beyond: -(2^24 - 127) is the first offset at which some code differs; +(2^24 - 127) still holds (its bias term 2^24 - 255 is exact)
    biased, direct = _both_forms(torch.tensor([-float(EXACT_BELOW), float(EXACT_BELOW)], dtype=torch.float64))
    differ = (biased.view(torch.int32) != direct.view(torch.int32)).sum(0)
    assert int(differ[0]) > 0 and float((biased - direct).abs().max()) == 1.0, differ
    assert int(differ[1]) == 0
    # further out many codes differ: near -2^28 the bias term has lost four bits
    biased, direct = _both_forms(torch.tensor([-(2.0**28) + 3 * 16.0]))
    assert int((biased != direct).sum()) >= 100


# ---- the relations bite: a model of the kernel's indexing with planted defects ------------------------------------------------------------------------
def _small(L, G, B=2, HKV=2, mask="bool", form="BHLS", S=33, layout="contiguous"):
    gen = ax.generator("decode_cases_model", L, G, B, HKV, mask, form)
    picks = tuple((b, head, l) for b in range(B) for head in range(HKV * G) for l in range(L))
    return dc.Case(900, L, G, B, HKV, S, 64, torch.bfloat16, mask, form if mask in dc.EXPLICIT else None, "plain", 1, layout,
                   int(torch.randint(0, 2**31 - 1, (1,), generator=gen)), picks)


def _fails(relation, *args, **kwargs):
    try:
        relation(*args, **kwargs)
    except AssertionError:
        return True
    return False


def _row_alone_fails(defect, L, G, mask="bool"):
    call = dc.call_of(_small(L, G, B=1, mask=mask))
    run = dc.model(defect)
    return _fails(dc.row_alone, run, call, call.full(run))


def test_the_sound_model_passes_every_relation():
    run = dc.model()
    for L, G in ((3, 5), (1, 1), (2, 4)):
        for mask, form in (("bool", "byte_offset"), ("float32", "transposed" if L > 1 else "1HLS"), ("causal", None), ("none", None)):
            case = _small(L, G, mask=mask, form=form, layout="fused_kv")
            call = dc.call_of(case)
            full = call.full(run)
            dc.row_alone(run, call, full, case.picks[::7])
            dc.kv_head_alone(run, call, full, 1)
            dc.batch_alone(run, call, full, 1)
    call = dc.call_of(_small(3, 2, mask="none", layout="bshe"))
    assert dc.causal_is_tril(run, call) == 4 and dc.mask_forms(run, call, "bool") == 12 and dc.mask_forms(run, call, "float") == 10
    assert dc.containers(run, call) == 3 and dc.layouts_agree(run, call, call.full(run)) == 11
    trade = dc.call_of(dataclasses.replace(_small(3, 2, mask="bool"), q_container="int8"), trade=True)
    for d in dc.TRADE_SHIFTS:
        assert dc.code_offset_trade(run, trade, d, (2.5, -0.5, 3.0)) == 5


def test_the_literal_trade_fails_on_a_half_integer_offset_and_an_odd_shift():
    """Why the trade is stated on rne(o): rne(o - d) != rne(o) - d for o = 2.5 and every odd d (ties go to even)."""
    for d in dc.TRADE_SHIFTS:
        assert dc.rne(2.5 - d) != dc.rne(2.5) - d and dc.rne(-0.5 - d) != dc.rne(-0.5) - d
        assert dc.rne(3.0 - d) == 3.0 - d and dc.rne(-9.0 - d) == -9.0 - d


@pytest.mark.parametrize("L,G", dc.FIRST_FIVE, ids=[f"L{L}xG{G}" for L, G in dc.FIRST_FIVE])
def test_row_alone_sees_a_wrong_slot_decoding(L, G):
    assert not _row_alone_fails(None, L, G)
    assert _row_alone_fails("g_l_swapped", L, G) and _row_alone_fails("shift_and_mask", L, G)
    assert _row_alone_fails("g_l_swapped", L, G, mask="none")  # (through q alone)


def test_what_the_earlier_grid_of_rows_could_see():
    """The grid of tests/test_sdpa_decode_gpu.py, ``ROWS``. A slot decoded with L rounded up to a power of two (a shift and a mask in
    place of ``row / L`` and ``row % L``) passes on every one of its shapes: its only L that is no power of two has G = 1. A plain
    swap of g and l passes wherever L = 1 or G = 1 — five of the seven, and (1, 1) here — and is seen at (2, 4) and (8, 4)."""
    earlier = ((1, 1), (1, 4), (1, 8), (2, 4), (5, 1), (8, 4), (32, 1))
    import test_sdpa_decode_gpu

    assert test_sdpa_decode_gpu.ROWS == earlier
    assert [_row_alone_fails("shift_and_mask", L, G) for L, G in earlier] == [False] * 7
    assert [_row_alone_fails("g_l_swapped", L, G) for L, G in earlier] == [L > 1 and G > 1 for L, G in earlier] == [False, False, False, True, False, True, False]
    assert not _row_alone_fails("g_l_swapped", 1, 1) and not _row_alone_fails("shift_and_mask", 1, 1)


def test_mask_forms_see_swapped_mask_strides():
    call = dc.call_of(_small(3, 5, mask="none"))
    for kind in dc.EXPLICIT:
        assert not _fails(dc.mask_forms, dc.model(), call, kind)
        assert _fails(dc.mask_forms, dc.model("mask_strides_swapped"), call, kind)
    # the transposed storage on its own
    assert _fails(dc.mask_forms, dc.model("mask_strides_swapped"), call, "bool", ("transposed",))


def test_kv_head_alone_sees_a_wrong_kv_head():
    for B, HKV in ((1, 2), (3, 3), (2, 4)):
        call = dc.call_of(_small(3, 5, B=B, HKV=HKV, mask="causal"))
        sound, wrong = dc.model(), dc.model("kv_head_modulo")
        assert not _fails(dc.kv_head_alone, sound, call, call.full(sound), HKV - 1)
        assert _fails(dc.kv_head_alone, wrong, call, call.full(wrong), HKV - 1)
