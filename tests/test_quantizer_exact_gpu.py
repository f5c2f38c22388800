"""The quantizer backward kernels (csrc/ffq_backward.hip) and the grid-error kernels (csrc/ffq_griderror.hip) against the float64
statement of the operation, bit for bit, on the operands of tests/quantizer_exact.py whose sums do not depend on the order they are
taken in (tests/test_quantizer_exact_cpu.py proves that of the operands, ties every case to its launch route, and shows that the
draws see a dropped or doubled element, a neighbour's scale, half-away rounding, an unrounded offset, swapped bounds and a
skipped cast). There is no tolerance in this file.

Every call runs twice, and the workspace it is handed is a buffer of this test's with every byte 0xFF (a NaN in each fp32 word)
before each call: a partial read before it is written, or left over from another tiling, is a NaN in the result. The composite of
tensor ops is patched to raise and the grid-error call must not decline, so a silent fallback fails."""

import functools

import pytest
import torch

import fastforward_amd as ff
import quantizer_exact as qe

from fastforward_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BACKWARD_SHAPES = [(row, s) for row, shapes in qe.BACKWARD_TABLE.items() for s in shapes]
GRID_SHAPES = [(row, s) for row, shapes in qe.GRID_TABLE.items() for s in shapes]
_ids = lambda v: str(v)  # noqa: E731


class Scratch:
    """Stands in for ops._workspace."""

    def __init__(self):
        self.buffer, self.handed = None, 0

    def __call__(self, nbytes, device):
        if nbytes <= 0:
            return None
        if self.buffer is None or self.buffer.numel() < nbytes:
            self.buffer = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        self.buffer.fill_(0xFF)
        self.handed += 1
        return self.buffer[:nbytes]


_SCRATCH = Scratch()


@pytest.fixture(autouse=True)
def scratch(hip_backend, monkeypatch):
    def never(*a, **k):
        raise AssertionError("the composite was called: the HIP kernel did not cover this tiling")

    monkeypatch.setattr(ops.static, "_quantize_by_tile_backward_composite", never)  # (the caller looks the composite up in its own module)
    monkeypatch.setattr(ops.static, "_workspace", _SCRATCH)
    monkeypatch.setattr(ops.packing, "_workspace", _SCRATCH)
    _SCRATCH.handed = 0
    return _SCRATCH


@functools.lru_cache(maxsize=64)
def backward_case(shape, dtype, num_bits, with_offset):
    """built once on the host, shared, never written"""
    return qe.backward_case(shape, dtype, num_bits, with_offset)


@functools.lru_cache(maxsize=64)
def grid_case(shape, dtype, num_bits, with_offset):
    return qe.grid_case(shape, dtype, num_bits, with_offset)


def _dev(t):
    return None if t is None else t.to(DEV)


def _backward_twice(x, g, scale, offset, tile, num_bits):
    first = ops.quantize_by_tile_backward(x, g, scale, tile, float(num_bits), offset)
    second = ops.quantize_by_tile_backward(x, g, scale, tile, float(num_bits), offset)
    return [t.cpu() for t in first], [t.cpu() for t in second]


# ---- backward: bit equality on every case, twice ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("row,shape", BACKWARD_SHAPES, ids=_ids)
def test_backward_kernels_give_the_reference_bits(row, shape, scratch):
    for dtype in qe.DTYPES:
        _backward_bits(shape, dtype, scratch)


def _backward_bits(shape, dtype, scratch):
    route = qe.backward_route(shape.shape, shape.tile)
    assert route.name == shape.route
    scratch.handed = 0
    for num_bits in qe.BACKWARD_BITS:
        for with_offset in (True, False):
            case = backward_case(shape, dtype, num_bits, with_offset)
            tag = f"{shape} {dtype} {num_bits} bits offset={with_offset}"
            for got in _backward_twice(_dev(case.x), _dev(case.g), _dev(case.scale), _dev(case.offset), case.tile, num_bits):
                assert qe.same_bits(got[0], case.want[0]), f"{tag}: dinput"
                assert got[1].dtype == torch.float32 and torch.equal(got[1], case.want[1]), f"{tag}: dscale"
                assert got[2].shape == case.want[2].shape and torch.equal(got[2], case.want[2]), f"{tag}: doffset"
    assert scratch.handed == (16 if route.nbytes else 0)  # the streaming routes, and only they, take a workspace


# ---- grid error: bit equality on every case, both `out` modes, twice -------------------------------------------------------------------
@pytest.mark.parametrize("row,shape", GRID_SHAPES, ids=_ids)
def test_grid_error_kernels_give_the_reference_bits(row, shape, scratch):
    for dtype in qe.DTYPES:
        _grid_error_bits(shape, dtype, scratch)


def _grid_error_bits(shape, dtype, scratch):
    route = qe.grid_route(shape.shape, shape.tile, 1)
    assert route.name == shape.route
    calls = scratch.handed = 0
    for num_bits in qe.grid_bits(shape):
        for with_offset in (True, False):
            case = grid_case(shape, dtype, num_bits, with_offset)
            x, scales, offsets, prefill = _dev(case.x), _dev(case.scales), _dev(case.offsets), _dev(case.prefill)
            for ncand in qe.NCANDS:
                tag = f"{shape} {dtype} {num_bits} bits offsets={with_offset} {ncand} candidates"
                sc = scales[:ncand].contiguous()
                of = None if offsets is None else offsets[:ncand].contiguous()
                for _ in range(2):
                    got = ops.grid_sqerror_by_tile(x, sc, of, case.tile, float(num_bits))
                    assert got is not None, f"{tag}: the HIP kernel declined"
                    assert torch.equal(got.cpu(), case.want[:ncand]), f"{tag}: fresh out"
                    out = prefill[:ncand].clone()
                    got = ops.grid_sqerror_by_tile(x, sc, of, case.tile, float(num_bits), out=out)
                    assert got is out and torch.equal(got.cpu(), case.want_accumulated[:ncand]), f"{tag}: accumulating"
                    calls += 2
    assert scratch.handed == (calls if route.name == "mode0" else 0)


# ---- special values stay in their tile ----------------------------------------------------------------------------------------------------
_SPECIAL_SHAPE = {"chunk_partials_finalize_small": 2, "chunk_partials_finalize_big": 2}  # row -> index of its shape (default: the first)


def _groups(kinds, ntiles):
    """all kinds in one call, each in a tile of its own, where a clean tile is left over; else one call per kind"""
    if ntiles > len(kinds):
        return [(kinds, tuple(range(len(kinds))))]
    return [((kind,), (i % ntiles,)) for i, kind in enumerate(kinds)]


@pytest.mark.parametrize("row", list(qe.BACKWARD_TABLE), ids=_ids)
def test_backward_special_values_stay_in_their_tile(row):
    for dtype in qe.DTYPES:
        _backward_specials(qe.BACKWARD_TABLE[row][_SPECIAL_SHAPE.get(row, 0)], dtype)


def _backward_specials(shape, dtype):
    ntiles, e = qe.num_tiles(shape.shape, shape.tile), min(1, qe.tile_elems(shape.tile) - 1)
    for num_bits in (4, 8):
        for with_offset in (True, False):
            case = backward_case(shape, dtype, num_bits, with_offset)
            for kinds, tiles in _groups(qe.BACKWARD_SPECIALS, ntiles):
                tag = f"{shape} {dtype} {num_bits} bits offset={with_offset} {kinds}"
                x, g = qe.backward_with_specials(case, kinds, tiles)
                want = qe.backward_reference(x, g, case.scale, case.offset, case.tile, num_bits)
                for got in _backward_twice(_dev(x), _dev(g), _dev(case.scale), _dev(case.offset), case.tile, num_bits):
                    for name, a, b in zip(("dinput", "dscale", "doffset"), got, want):
                        assert qe.same_bits_or_both_nan(a, b), f"{tag}: {name}"
                    # what the reference formulas give, stated: (rows of dinput and g, the sums per tile)
                    di, gr = qe.to_rows(got[0], case.tile), qe.to_rows(g, case.tile)
                    ds, do = got[1].reshape(-1), (got[2].reshape(-1) if with_offset else None)
                    for kind, t in zip(kinds, tiles):
                        if kind == "nan_x":  # not clipped: the gradient passes, the term (q - u) g is NaN, doffset takes nothing
                            assert qe.same_bits(di[t, e], gr[t, e]) and bool(ds[t] != ds[t]) and (do is None or bool(do[t] == do[t])), f"{tag}: {kind}"
                        elif kind == "nan_g":  # clipped: no data gradient, both sums take the NaN
                            assert float(di[t, e]) == 0.0 and bool(ds[t] != ds[t]) and (do is None or bool(do[t] != do[t])), f"{tag}: {kind}"
                        else:  # clipped: the term is (bound + ro) g, doffset takes s g — both finite
                            assert float(di[t, e]) == 0.0 and bool(torch.isfinite(ds[t])) and (do is None or bool(torch.isfinite(do[t]))), f"{tag}: {kind}"
                    clean = [t for t in range(ntiles) if t not in tiles]
                    assert qe.same_bits(di[clean], qe.to_rows(case.want[0], case.tile)[clean]), f"{tag}: dinput of the other tiles"
                    assert torch.equal(ds[clean], case.want[1].reshape(-1)[clean]), f"{tag}: dscale of the other tiles"
                    if with_offset:
                        assert torch.equal(do[clean], case.want[2].reshape(-1)[clean]), f"{tag}: doffset of the other tiles"


GRID_SPECIALS = (float("nan"), float("inf"), float("-inf"))


@pytest.mark.parametrize("row", list(qe.GRID_TABLE), ids=_ids)
def test_grid_error_special_values_stay_in_their_tile(row):
    for shape in qe.GRID_TABLE[row]:
        for dtype in qe.DTYPES:
            _grid_error_specials(shape, dtype)


def _grid_error_specials(shape, dtype):
    ntiles, ncand, num_bits = qe.num_tiles(shape.shape, shape.tile), 17, 4
    for with_offset in (True, False):
        case = grid_case(shape, dtype, num_bits, with_offset)
        scales = _dev(case.scales[:ncand].contiguous())
        offsets = None if case.offsets is None else _dev(case.offsets[:ncand].contiguous())
        for values, tiles in _groups(GRID_SPECIALS, ntiles):
            tag = f"{shape} {dtype} offsets={with_offset} {values}"
            x = case.x
            for value, t in zip(values, tiles):
                x = qe.grid_with_special(x, case.tile, value, t)
            want = qe.grid_reference(x, case.scales[:ncand], None if case.offsets is None else case.offsets[:ncand], case.tile, num_bits)
            for _ in range(2):
                got = ops.grid_sqerror_by_tile(_dev(x), scales, offsets, case.tile, float(num_bits))
                assert got is not None, f"{tag}: the HIP kernel declined"
                got = got.cpu()
                assert qe.same_bits_or_both_nan(got, want), tag
                for value, t in zip(values, tiles):  # a NaN element: NaN for every candidate; an infinite one: +Inf
                    assert bool((got[:, t] != got[:, t]).all()) if value != value else bool((got[:, t] == float("inf")).all()), f"{tag}: tile {t}"
                clean = [t for t in range(ntiles) if t not in tiles]
                assert torch.equal(got[:, clean], case.want[:ncand][:, clean]), f"{tag}: the other tiles"


# ---- the public autograd route --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [qe.BACKWARD_TABLE["chunk_partials_finalize_big"][2], qe.BACKWARD_TABLE["by_tile_not_small"][0]], ids=_ids)
def test_linear_quantizer_backward_gives_the_reference_bits(shape):
    """Where training calls the kernels: LinearQuantizer forward in grad mode, dequantize(), backward(g) — a ROWS tiling on the
    streaming kernel and strided channels on the by-tile kernel."""
    for dtype in qe.DTYPES:
        for with_offset in (True, False):
            _linear_quantizer_backward(shape, dtype, with_offset)


def _linear_quantizer_backward(shape, dtype, with_offset):
    num_bits = 4
    case = backward_case(shape, dtype, num_bits, with_offset)
    quantizer = ff.nn.LinearQuantizer(num_bits, symmetric=not with_offset, allow_one_sided=False, granularity=ff.PerTile(case.tile), device=DEV)
    quantizer.scale = torch.nn.Parameter(_dev(case.scale))
    if with_offset:
        quantizer.offset = torch.nn.Parameter(_dev(case.offset))
    else:
        assert quantizer.offset is None
    x = _dev(case.x).requires_grad_(True)
    with torch.enable_grad():
        quantizer(x).dequantize().backward(_dev(case.g))
    tag = f"{shape} {dtype} offset={with_offset}"
    assert qe.same_bits(x.grad.cpu(), case.want[0]), tag
    assert torch.equal(quantizer.scale.grad.cpu(), case.want[1]), tag
    if with_offset:
        assert torch.equal(quantizer.offset.grad.cpu(), case.want[2]), tag
