"""The operands of tests/quantizer_exact.py earn their place, without a GPU: every case of the two route tables meets the
representability assertions and the exactness condition (the builders raise otherwise) and holds the decision points; the restated
launch plans give each case the route its table row names and agree with the two workspace queries of libffq_hip.so; the float64
references are checked by something that is not a kernel — the package's fp32 composite, a plain fp32 restatement of the grid-error
chain (both again after a seeded permutation inside every tile: the sums do not depend on their order) and the C oracle through the
C ABI; and each wrong form of the operations this file is about changes the expected bits, on every route row."""

import ctypes
import functools

import pytest
import torch

import quantizer_exact as qe

from conftest import HIP_SO
from fastforward_amd import ops
from fastforward_amd._cabi import FFQLibrary, Tiling

BACKWARD_SHAPES = [(row, s) for row, shapes in qe.BACKWARD_TABLE.items() for s in shapes]
GRID_SHAPES = [(row, s) for row, shapes in qe.GRID_TABLE.items() for s in shapes]
_ids = lambda v: str(v)  # noqa: E731


@functools.lru_cache(maxsize=None)
def backward_case(shape, dtype, num_bits, with_offset):
    return qe.backward_case(shape, dtype, num_bits, with_offset)


@functools.lru_cache(maxsize=None)
def grid_case(shape, dtype, num_bits, with_offset):
    return qe.grid_case(shape, dtype, num_bits, with_offset)


def backward_variants(shape):
    return [backward_case(shape, dtype, bits, off) for dtype in qe.DTYPES for bits in qe.BACKWARD_BITS for off in (True, False)]


def grid_variants(shape):
    return [grid_case(shape, dtype, bits, off) for dtype in qe.DTYPES for bits in qe.grid_bits(shape) for off in (True, False)]


# ---- conditions -------------------------------------------------------------------------------------------------------------------------
def _assert_census(case):
    if qe.tile_elems(case.tile) >= 64:
        for name, per_tile in case.census.items():
            assert bool(per_tile.all()), f"{case.shape} {case.dtype} {case.num_bits} bits: tile {int((~per_tile).nonzero()[0])} holds no {name}"


@pytest.mark.parametrize("row,shape", BACKWARD_SHAPES, ids=_ids)
def test_backward_cases_meet_the_conditions(row, shape):
    for case in backward_variants(shape):  # (the builder asserts representability and the exactness condition)
        _assert_census(case)
        assert case.x.dtype == case.g.dtype == case.dtype and case.x.shape == case.g.shape == torch.Size(shape.shape)
        exps = torch.log2(case.scale.double())
        assert bool((exps == exps.round()).all()) and -6 <= float(exps.min()) and float(exps.max()) <= 2
        if case.scale.numel() > 1:
            assert bool((case.scale[1:] != case.scale[:-1]).all())
        if case.offset is not None:
            assert bool((case.offset * 2 == (case.offset * 2).round()).all()) and float(case.offset.abs().max()) <= 3
            assert float(case.offset[0]) == -2.5  # round-half-even: -2, half away: -3, unrounded: -2.5
        assert float(case.g.float().abs().max()) <= 3
        if case.dtype != torch.float32 and case.g.numel() >= 64 and qe.tile_elems(case.tile) >= 3:  # (the first and last g of a tile are not zero)
            assert bool(((case.g == 0) & torch.signbit(case.g)).any())


@pytest.mark.parametrize("row,shape", GRID_SHAPES, ids=_ids)
def test_grid_cases_meet_the_conditions(row, shape):
    for case in grid_variants(shape):
        _assert_census(case)
        assert case.scales.shape == (33, qe.num_tiles(shape.shape, shape.tile)) and bool(torch.isfinite(case.want_accumulated).all())
        ratio = torch.log2(case.scales.double() / case.scales.double().min(0, keepdim=True).values)
        assert bool((ratio == ratio.round()).all()) and float(ratio.max()) <= 3
        assert bool((case.want > 0).any())
        if case.scales.shape[1] * 33 >= 64:
            assert bool((case.prefill > 0).any())


def test_the_tables_hold_the_bit_widths_and_dtypes_the_cases_are_stated_for():
    assert qe.DTYPES == (torch.bfloat16, torch.float16, torch.float32) and qe.BACKWARD_BITS == (2, 3, 4, 8) and qe.NCANDS == (1, 16, 17, 33)
    assert len(BACKWARD_SHAPES) == 20 and len(GRID_SHAPES) == 14
    for _, shape in GRID_SHAPES:
        assert qe.grid_bits(shape) == ((2, 3, 4, 8) if qe.tile_elems(shape.tile) <= 1032 else (2, 3, 4))
    assert qe.grid_exponents(8) == (0, 1, 2) and qe.grid_exponents(4) == (-1, 0, 1, 2)
    assert [qe.grid_offset_limit(b) for b in (2, 3, 4, 8)] == [1, 3, 3, 3]
    assert qe.backward_far_share(67584) == 0.03 and qe.backward_far_share(526336) <= 0.005


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip_library():
    return FFQLibrary(HIP_SO)  # loads without a device: the two queries are host code


@pytest.mark.parametrize("row,shape", BACKWARD_SHAPES, ids=_ids)
def test_backward_plan_gives_the_case_its_route(row, shape, hip_library):
    route = qe.backward_route(shape.shape, shape.tile)
    assert (route.name, route.units) == (shape.route, shape.units)
    numel = qe.tile_elems(shape.shape)
    want_bytes = {"tiles": 0, "chunk": 8 * numel // 8, "block": 8 * numel // 2048}[route.name.split("_")[0]]
    assert route.nbytes == want_bytes
    assert hip_library.ffq_quantize_backward_workspace_bytes(ctypes.byref(Tiling.make(shape.shape, shape.tile))) == want_bytes
    if row in qe.BACKWARD_SMALL_ROWS:
        assert route.small
        if row == "by_tile_block_per_tile_small":
            assert route.planned  # only the small-problem rule keeps these off the streaming kernel
    if row == "by_tile_not_small":
        assert not route.planned


@pytest.mark.parametrize("row,shape", GRID_SHAPES, ids=_ids)
def test_grid_plan_gives_the_case_its_route(row, shape, hip_library):
    numel = qe.tile_elems(shape.shape)
    for ncand in qe.NCANDS:
        route = qe.grid_route(shape.shape, shape.tile, ncand)
        assert (route.name, route.units) == (shape.route, shape.units)
        want_bytes = 4 * ((numel // 8 + 255) // 256) * ncand if route.name == "mode0" else 0
        assert route.nbytes == want_bytes
        assert hip_library.ffq_grid_sqerror_workspace_bytes(ctypes.byref(Tiling.make(shape.shape, shape.tile)), ncand) == want_bytes


def test_the_plans_at_their_edges():
    """The restatement itself, next to the edges the tables sit on."""
    assert qe.backward_route((4, 4096), (1, 4096)).name == "tiles_block" and qe.backward_route((3, 4096), (1, 4096)).name == "block_small"
    assert qe.backward_route((4, 4104), (1, 4104)).name == "chunk_big"       # beyond the small rule's 4096 elements per tile
    assert qe.backward_route((2, 65536), (1, 65536)).units == 32 and qe.backward_route((2, 67584), (1, 67584)).units == 33
    assert qe.backward_route((8, 24), (1, 24)).small and not qe.backward_route((3, 24), (1, 24)).small
    assert qe.grid_route((3, 1024), (1, 1024), 4).name == "tiles_block"     # 128 chunks: a power of two above 64 lanes
    assert qe.grid_route((3, 2048), (1, 2048), 4).name == "mode0" and qe.grid_route((5, 512), (1, 512), 4) == qe.Route("mode1", 64, 0, True)
    assert qe.grid_route((8, 24), (1, 24), 4).name == "tiles_lane"          # 3 chunks: not a power of two


# ---- order-independence: the references against fp32 tensor ops -----------------------------------------------------------------------
def _permutation(nt, ne, seed):
    return torch.rand(nt, ne, generator=torch.Generator().manual_seed(seed)).argsort(dim=1)


def _assert_backward(got, case, tag):
    assert qe.same_bits(got[0], case.want[0]), f"{tag}: dinput"
    assert got[1].dtype == torch.float32 and torch.equal(got[1], case.want[1]), f"{tag}: dscale"
    assert got[2].shape == case.want[2].shape and torch.equal(got[2], case.want[2]), f"{tag}: doffset"


@pytest.mark.parametrize("row,shape", BACKWARD_SHAPES, ids=_ids)
def test_backward_composite_equals_the_reference_in_any_order(row, shape):
    for case in backward_variants(shape):
        tag = f"{shape} {case.dtype} {case.num_bits} bits offset={case.offset is not None}"
        got = ops._quantize_by_tile_backward_composite(case.x, case.g, case.scale, case.tile, float(case.num_bits), case.offset)
        _assert_backward(got, case, tag)
        xr, gr = qe.to_rows(case.x, case.tile), qe.to_rows(case.g, case.tile)
        perm = _permutation(*xr.shape, seed=xr.numel())
        xp, gp = qe.from_rows(xr.gather(1, perm), case.shape, case.tile), qe.from_rows(gr.gather(1, perm), case.shape, case.tile)
        got = ops._quantize_by_tile_backward_composite(xp, gp, case.scale, case.tile, float(case.num_bits), case.offset)
        back = torch.empty_like(xr).scatter_(1, perm, qe.to_rows(got[0], case.tile))
        _assert_backward([qe.from_rows(back, case.shape, case.tile), got[1], got[2]], case, tag + " (permuted)")


@pytest.mark.parametrize("row,shape", GRID_SHAPES, ids=_ids)
def test_grid_chain_in_fp32_equals_the_reference_in_any_order(row, shape):
    for case in grid_variants(shape):
        tag = f"{shape} {case.dtype} {case.num_bits} bits offsets={case.offsets is not None}"
        assert torch.equal(qe.grid_reference(case.x, case.scales, case.offsets, case.tile, case.num_bits), case.want), tag
        assert torch.equal(qe.grid_chain_fp32(case.x, case.scales, case.offsets, case.tile, case.num_bits), case.want), tag
        perm = _permutation(case.scales.shape[1], qe.tile_elems(case.tile), seed=case.x.numel() + 1)
        assert torch.equal(qe.grid_chain_fp32(case.x, case.scales, case.offsets, case.tile, case.num_bits, perm), case.want), tag + " (permuted)"
        assert torch.equal(case.want + case.prefill, case.want_accumulated), tag  # one fp32 add of the prefilled output is exact too


# ---- the oracle through the C ABI ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row,shape", BACKWARD_SHAPES, ids=_ids)
def test_backward_oracle_gives_the_same_bits(row, shape, oracle_backend):
    for case in backward_variants(shape):
        got = ops.quantize_by_tile_backward(case.x, case.g, case.scale, case.tile, float(case.num_bits), case.offset)
        _assert_backward(got, case, f"{shape} {case.dtype} {case.num_bits} bits offset={case.offset is not None}")


@pytest.mark.parametrize("dtype", qe.DTYPES, ids=_ids)
@pytest.mark.parametrize("row,shape", GRID_SHAPES, ids=_ids)
def test_grid_oracle_gives_the_same_bits(row, shape, dtype, oracle_backend):
    for case in (c for c in grid_variants(shape) if c.dtype == dtype):
        tag = f"{shape} {case.dtype} {case.num_bits} bits offsets={case.offsets is not None}"
        got = ops.grid_sqerror_by_tile(case.x, case.scales, case.offsets, case.tile, float(case.num_bits))
        assert got is not None and torch.equal(got, case.want), tag
        n = 17
        out = case.prefill[:n].clone()
        got = ops.grid_sqerror_by_tile(case.x, case.scales[:n], None if case.offsets is None else case.offsets[:n], case.tile, float(case.num_bits), out=out)
        assert got is out and torch.equal(got, case.want_accumulated[:n]), tag + " (accumulating)"


# ---- sensitivity: the draws see the errors this file is about ---------------------------------------------------------------------------
# mutation -> the output that must change (None: any of the three)
BACKWARD_MUTATIONS = {
    "drop_last": 1, "count_twice": 1, "neighbour_scale": None, "half_away": 1, "offset_unrounded": None, "offset_half_away": None,
    "swap_bounds": 1, "hi_clipped": None,
}


def _changed(got, want, which):
    differs = [not qe.same_bits(got[0], want[0]), not torch.equal(got[1], want[1]), not torch.equal(got[2], want[2])]
    return differs[which] if which is not None else any(differs)


@pytest.mark.parametrize("mutation", list(BACKWARD_MUTATIONS), ids=_ids)
@pytest.mark.parametrize("row", list(qe.BACKWARD_TABLE), ids=_ids)
def test_each_wrong_backward_changes_the_expected_bits_on_every_route_row(row, mutation):
    cases = [c for shape in qe.BACKWARD_TABLE[row] for c in backward_variants(shape)]
    if mutation == "neighbour_scale":
        cases = [c for c in cases if c.scale.numel() > 1]
        if row == "per_tensor":
            assert not cases  # one tile: there is no other tile's scale to read
            return
    seen = 0
    for c in cases:
        if mutation.startswith("offset") and c.offset is None:
            continue
        seen += _changed(qe.backward_reference(c.x, c.g, c.scale, c.offset, c.tile, c.num_bits, mutation), c.want, BACKWARD_MUTATIONS[mutation])
    print(f"{row}: {mutation} changes the bits of {seen} of {len(cases)} cases")
    assert seen >= 1, f"{row}: no case sees {mutation}"


@pytest.mark.parametrize("mutation,dtypes", [("skip_cast_d", (torch.bfloat16,)), ("skip_cast_e", (torch.bfloat16, torch.float16)), ("drop_candidate_16", qe.DTYPES)], ids=_ids)
def test_each_wrong_grid_error_changes_the_expected_bits(mutation, dtypes):
    """The mutations without a backward counterpart. A skipped cast of the difference shows for bf16 only: y has few significant
    bits and x the dtype's own, so y - x needs more than the dtype holds only where |x| >= 2^p steps of y (p: the significand) —
    128 steps for bf16, which the elements planted at hi + 126 and lo - 125 reach; for fp16 that is 1024 steps, whose square alone
    is 2^24 quanta of the smallest square of its tile: no tile with exact sums holds one."""
    for dtype in dtypes:
        seen = total = 0
        for _, shape in GRID_SHAPES:
            for bits in qe.grid_bits(shape):
                for off in (True, False):
                    c = grid_case(shape, dtype, bits, off)
                    seen += not torch.equal(qe.grid_reference(c.x, c.scales, c.offsets, c.tile, c.num_bits, mutation), c.want)
                    total += 1
        print(f"{mutation} {dtype}: changes the bits of {seen} of {total} cases")
        assert seen >= (total if mutation == "drop_candidate_16" else 1), f"{dtype}: {mutation} is seen by {seen} of {total} cases"


def test_builders_are_deterministic():
    shape = qe.BACKWARD_TABLE["chunk_partials_finalize_small"][0]
    a, b = qe.backward_case(shape, torch.bfloat16, 4, True), qe.backward_case(shape, torch.bfloat16, 4, True)
    assert qe.same_bits(a.x, b.x) and qe.same_bits(a.g, b.g) and torch.equal(a.scale, b.scale) and torch.equal(a.offset, b.offset)
    shape = qe.GRID_TABLE["mode1_sub_wave_groups"][2]
    a, b = qe.grid_case(shape, torch.float16, 3, True), qe.grid_case(shape, torch.float16, 3, True)
    assert qe.same_bits(a.x, b.x) and torch.equal(a.scales, b.scales) and torch.equal(a.offsets, b.offsets) and torch.equal(a.prefill, b.prefill)
