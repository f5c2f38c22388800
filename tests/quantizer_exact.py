"""Operands on which the sums of the quantizer backward (A8, csrc/ffq_backward.hip) and of the grid-error kernels
(csrc/ffq_griderror.hip) do not depend on the order they are taken in, the float64 statement of both operations, and the two
launch plans restated — no library code is imported here.

The construction, per tile t (docs/numerics.md, "A8 and the grid estimator: when the sums are exact"):

* ``scale[t]`` is a power of two, ``offset[t]`` a multiple of 1/2 in [-3, 3] (``round`` decides its ties to even);
* ``u = x / s - round(o)`` lies on the quarter grid over ``[lo - 1, hi + 1]``: rounding ties, ``lo - 0.5`` and ``hi + 0.5``
  (half-even decides whether they clip), ``q == lo`` and ``q == hi`` are planted into every tile that has room, a seeded share
  of elements is pushed 4 .. 32 whole steps outside on both sides;
* ``v = u + round(o)`` is cast to the data dtype (which snaps it onto that dtype's grid) and ``x = v * s``;
* ``g`` holds integers in [-3, 3] (and ``-0.0`` for the half-precision dtypes).

Then ``x / s``, ``u``, ``q - u``, every term and every ``s * g`` are exact in fp32, and the builders assert THE EXACTNESS CONDITION for
each sum of each tile: with ``quantum`` the largest power of two dividing every term, ``sum |term| / quantum < 2^24``. Every
partial sum in any order, split or FMA contraction is then a multiple of the quantum below 2^24 quanta, i.e. an fp32 number: the
fp32 sum IS the float64 sum. The assertion is the condition; a case that misses it changes its draws, never the bound.

Seeded and deterministic; everything is built on the host.
"""

from __future__ import annotations

import dataclasses

import torch

DTYPES = (torch.bfloat16, torch.float16, torch.float32)
BACKWARD_BITS = (2, 3, 4, 8)
NCANDS = (1, 16, 17, 33)
KBLOCK, CHUNK = 256, 8
LIMIT = 2.0**24


# ---- tiles as rows (row-major over the grid of tiles, row-major inside a tile: the parameter order of every kernel) ------------------
def _split_perm(shape, tile):
    split = []
    for n, t in zip(shape, tile):
        split += [n // t, t]
    rank = len(shape)
    return split, [2 * k for k in range(rank)] + [2 * k + 1 for k in range(rank)]


def tile_elems(tile) -> int:
    n = 1
    for t in tile:
        n *= t
    return n


def num_tiles(shape, tile) -> int:
    n = 1
    for s, t in zip(shape, tile):
        n *= s // t
    return n


def to_rows(data: torch.Tensor, tile) -> torch.Tensor:
    split, perm = _split_perm(tuple(data.shape), tile)
    return data.reshape(split).permute(perm).reshape(-1, tile_elems(tile))


def from_rows(rows: torch.Tensor, shape, tile) -> torch.Tensor:
    split, perm = _split_perm(shape, tile)
    inverse = [0] * len(perm)
    for dst, src in enumerate(perm):
        inverse[src] = dst
    return rows.reshape([split[p] for p in perm]).permute(inverse).reshape(shape).contiguous()


# ---- the launch plans restated (analyse of csrc/ffq_core.hip; backward_plan + backward_small; grid_plan) ------------------------------
@dataclasses.dataclass(frozen=True)
class Route:
    name: str        # backward: tiles_lane / tiles_block / chunk_small / chunk_big / block_small / block_big
    units: int       # grid error: tiles_lane / tiles_block / mode1 / mode0. `units`: partials per tile (mode1: lanes per tile)
    nbytes: int      # what the library's workspace query answers
    planned: bool    # the streaming plan covers the tiling (backward: it may still take the by-tile kernel as a small problem)
    small: bool = False


def _layout(shape, tile):
    """(numel, ntiles, run): run > 0 where every tile is one contiguous run (one tile: the whole tensor), else 0."""
    numel = tile_elems(shape)
    ntiles = num_tiles(shape, tile)
    if ntiles == 1:
        return numel, 1, numel
    dims = [(s, t) for s, t in zip(shape, tile) if s != 1]  # extent-1 dimensions do not influence the flat -> tile map
    j = 0
    while j < len(dims) and dims[j][1] == 1:
        j += 1
    run = 1
    if j < len(dims):
        run = dims[j][1]
        for s, t in dims[j + 1:]:
            if t != s:
                return numel, ntiles, 0
            run *= s
    return numel, ntiles, run


def _chunks_per_tile(shape, tile):
    numel, ntiles, run = _layout(shape, tile)
    if numel % CHUNK != 0 or numel // CHUNK >= 2**32 - KBLOCK or run == 0 or run % CHUNK != 0:
        return None
    return run // CHUNK


def _by_tile(shape, tile, planned, small=False) -> Route:
    return Route("tiles_lane" if tile_elems(tile) < 64 else "tiles_block", 0, 0, planned, small)


def backward_route(shape, tile) -> Route:
    numel, ntiles, _ = _layout(shape, tile)
    cpr = _chunks_per_tile(shape, tile)
    small = numel <= 2**16 and ntiles >= 4 and numel // ntiles <= 4096
    if small or cpr is None:
        return _by_tile(shape, tile, cpr is not None, small)
    if cpr % KBLOCK == 0:
        units = cpr // KBLOCK
        return Route("block_small" if units <= 32 else "block_big", units, 8 * (numel // CHUNK // KBLOCK), True)
    return Route("chunk_small" if cpr <= 32 else "chunk_big", cpr, 8 * (numel // CHUNK), True)


def grid_route(shape, tile, ncand) -> Route:
    numel, _, _ = _layout(shape, tile)
    cpr = _chunks_per_tile(shape, tile)
    if cpr is None:
        return _by_tile(shape, tile, False)
    if cpr % KBLOCK == 0:
        blocks = (numel // CHUNK + KBLOCK - 1) // KBLOCK
        return Route("mode0", cpr // KBLOCK, 4 * blocks * ncand, True)
    if cpr <= 64 and cpr & (cpr - 1) == 0:
        return Route("mode1", cpr, 0, True)
    return _by_tile(shape, tile, False)


@dataclasses.dataclass(frozen=True)
class Shape:
    shape: tuple
    tile: tuple
    route: str
    units: int = 0

    def __str__(self):
        return "x".join(map(str, self.shape)) + "_" + "x".join(map(str, self.tile))


def _rows(rows, cols, route, units=0):
    return Shape((rows, cols), (1, cols), route, units)


def _whole(shape, route, units=0):
    return Shape(shape, shape, route, units)


# route row -> its shapes; every shape names the route (and the partials per tile) the plan must give it
BACKWARD_TABLE = {
    "by_tile_lane_per_tile": [_rows(8, 24, "tiles_lane"), Shape((33, 17), (1, 1), "tiles_lane")],
    "by_tile_block_per_tile_small": [_rows(5, 72, "tiles_block"), _rows(6, 264, "tiles_block"), _rows(4, 4096, "tiles_block")],
    "chunk_partials_finalize_small": [_rows(3, 136, "chunk_small", 17), _rows(2, 256, "chunk_small", 32), _rows(600, 128, "chunk_small", 16)],
    "chunk_partials_finalize_big": [_rows(3, 264, "chunk_big", 33), _rows(3, 2056, "chunk_big", 257), _rows(300, 264, "chunk_big", 33)],
    "block_partials_finalize_small": [_rows(2, 2048, "block_small", 1), _rows(2, 65536, "block_small", 32)],
    "block_partials_finalize_big": [_rows(2, 67584, "block_big", 33), _whole((1, 526336), "block_big", 257)],
    "per_tensor": [_whole((3, 1000), "chunk_big", 375), _whole((7, 9), "tiles_lane")],
    "by_tile_not_small": [Shape((96, 160), (96, 1), "tiles_block"), Shape((16, 24, 20), (8, 8, 4), "tiles_block"), Shape((128, 96), (32, 32), "tiles_block")],
}
BACKWARD_SMALL_ROWS = ("by_tile_lane_per_tile", "by_tile_block_per_tile_small")  # taken as small problems: the plan would cover them

GRID_TABLE = {
    "mode1_sub_wave_groups": [_rows(40, 8, "mode1", 1), _rows(7, 16, "mode1", 2), _rows(9, 64, "mode1", 8), _rows(5, 512, "mode1", 64)],
    "mode0_partials": [_rows(2, 2048, "mode0", 1), _rows(3, 4096, "mode0", 2), _whole((1, 133120), "mode0", 65)],
    "by_tile_lane_per_tile": [_rows(8, 24, "tiles_lane"), Shape((33, 17), (1, 1), "tiles_lane")],
    "by_tile_block_per_tile": [_rows(5, 72, "tiles_block"), _rows(3, 1024, "tiles_block"), _rows(3, 1032, "tiles_block")],
    "by_tile_strided_and_nd": [Shape((96, 160), (96, 1), "tiles_block"), Shape((16, 24, 20), (8, 8, 4), "tiles_block")],
}


def grid_bits(shape: Shape):
    """2, 3 and 4 bits everywhere; 8 bits where a tile has at most 1032 elements (beyond, a candidate that clips half the tile
    leaves the exactness condition: measured 2^24.9 at 2048 elements)."""
    return (2, 3, 4, 8) if tile_elems(shape.tile) <= 1032 else (2, 3, 4)


def grid_exponents(num_bits):
    """candidate scales are s0 * 2^k"""
    return (0, 1, 2) if num_bits == 8 else (-1, 0, 1, 2)


def grid_offset_limit(num_bits):
    """candidate offsets are multiples of 1/2 in [-limit, limit]: 3, but 1 at 2 bits — a rounded offset of 3 moves a grid that is
    four steps wide off the data at every candidate scale, the whole tile clips and the 133120-element tile is at 2^24.95"""
    return min(3, 2 ** (num_bits - 1) - 1)


# ---- shared pieces ----------------------------------------------------------------------------------------------------------------------
def _bounds(num_bits):
    lo = -(2 ** (num_bits - 1))
    return float(lo), float(-lo - 1)


def _half_away(v):
    return torch.sign(v) * torch.floor(v.abs() + 0.5)


def _seed(shape: Shape, dtype, num_bits, with_offset, salt):
    return (tile_elems(shape.shape) * 131 + len(shape.shape) * 17 + shape.tile[-1] * 7 + DTYPES.index(dtype) * 3 + num_bits * 1009 + int(with_offset)) * 8 + salt


def assert_exact_sums(terms: torch.Tensor, what: str, extra_quanta: torch.Tensor | None = None) -> torch.Tensor:
    """THE EXACTNESS CONDITION on every sum over the last dimension of float64 `terms` (`extra_quanta`: one more term per sum, in
    whole quanta — a prefilled output). Returns the quantum per sum (1 where every term is zero)."""
    scaled = terms.abs() * 2.0**40
    assert bool((scaled == scaled.round()).all()) and float(scaled.max()) < 2.0**62, f"{what}: a term is not a finite multiple of 2^-40"
    ints = scaled.to(torch.int64)
    low = torch.where(ints == 0, 2**62, ints & -ints).amin(dim=-1)
    quantum = torch.where(low == 2**62, 1.0, low.double() * 2.0**-40)
    load = terms.abs().sum(dim=-1) / quantum + (0 if extra_quanta is None else extra_quanta)
    assert float(load.max()) < LIMIT, f"{what}: sum |term| / quantum = 2^{torch.log2(load.max()).item():.2f} in sum {int(load.argmax())}"
    return quantum


def _draw_u(nt, ne, num_bits, far_share, gen, very_far=False):
    """[nt, ne] float64 on the quarter grid over [lo - 1, hi + 1], the far-clipped share, and the planted decision points."""
    lo, hi = _bounds(num_bits)
    span = int(4 * (hi - lo + 2))
    r = torch.randint(0, 2**40, (nt, ne), generator=gen)  # one draw per element: its quarter, far-clipped or not, how far, which side
    u = lo - 1 + 0.25 * (r % (span + 1)).double()
    far = (r >> 11) % 1000 < round(far_share * 1000)
    steps = (4 + (r >> 22) % 29).double()
    u = torch.where(far, torch.where((r >> 30) % 2 == 1, hi + steps, lo - steps), u)
    planted = [lo - 0.5, lo + 0.5, hi + 0.5, hi - 0.5, lo, hi, lo - 1, hi + 1, 0.5, -1.5, hi + 4, lo - 4, hi + 32, lo - 32, lo - 0.25, hi + 0.25]
    if very_far:  # |y - x| with nine significant bits: a bf16 cast of the difference that is skipped shows (tests/test_quantizer_exact_cpu.py)
        planted += [hi + 126, lo - 125]
    if ne >= len(planted) + 2:
        # evenly spaced from a drawn start, never the first or the last element
        start = torch.randint(0, ne - 2, (nt, 1), generator=gen)
        at = 1 + (start + (ne - 2) // len(planted) * torch.arange(len(planted))[None, :]) % (ne - 2)
        u.scatter_(1, at, torch.tensor(planted, dtype=torch.float64).expand(nt, -1))
    # the first and the last element of a tile carry a term that is not zero: a dropped or a doubled element shows
    inside_lo, inside_hi = int(max(lo, -8)), int(min(hi, 8))
    first = torch.randint(inside_lo, inside_hi, (nt,), generator=gen).double() + 0.25
    last = torch.randint(inside_lo, inside_hi, (nt,), generator=gen).double() + 0.75
    if ne == 1:
        t = torch.arange(nt)
        u[:, 0] = torch.where(t % 2 == 0, first, hi + 4 + (t % 5).double())
    else:
        u[:, 0], u[:, -1] = first, last
    return u


def _snap(u, ro, scale, dtype):
    """v = u + ro cast to `dtype`, x = v * s: (x in `dtype`, the u the cast left)."""
    v = (u + ro[:, None]).to(dtype)
    x64 = v.double() * scale.double()[:, None]
    x = x64.to(dtype)
    assert bool((x.double() == x64).all()), "x = v * s is not representable in the data dtype"
    return x, v.double() - ro[:, None]


def census(u, num_bits):
    """per tile: does it hold a rounding tie, q == lo, q == hi, a far-clipped element below and one above"""
    lo, hi = _bounds(num_bits)
    q = torch.round(u)
    return {
        "tie": ((u - torch.floor(u)) == 0.5).any(1),
        "at_lo": (q == lo).any(1),
        "at_hi": (q == hi).any(1),
        "far_below": (q <= lo - 4).any(1),
        "far_above": (q >= hi + 4).any(1),
    }


# ---- backward ---------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class BackwardCase:
    shape: tuple
    tile: tuple
    dtype: torch.dtype
    num_bits: int
    x: torch.Tensor
    g: torch.Tensor
    scale: torch.Tensor
    offset: torch.Tensor | None
    census: dict
    want: list  # [dinput, dscale, doffset or an empty tensor]: the float64 reference


def backward_far_share(ne):
    """about 3 % up to 70 k elements; beyond (the 526336-element tile) 0.4 %: at 3 % and 8 bits that tile is at 2^24.01"""
    return 0.03 if ne <= 70000 else 0.004


def backward_sums(xr, gr, s, o, num_bits, mutation=None):
    """The reference formulas (_quantizer_impl.py:193-237) on float64 rows: (clip mask, dscale terms, doffset terms).
    `mutation`: one of the wrong forms tests/test_quantizer_exact_cpu.py shows the draws can see."""
    lo, hi = _bounds(num_bits)
    if o is None:
        ro = torch.zeros_like(s)
    elif mutation == "offset_unrounded":
        ro = o
    elif mutation == "offset_half_away":
        ro = _half_away(o)
    else:
        ro = torch.round(o)
    if mutation == "neighbour_scale":
        s = s.roll(-1)
    s, ro = s[:, None], ro[:, None]
    u = xr / s - ro
    q = _half_away(u) if mutation == "half_away" else torch.round(u)
    below = q < lo
    above = q >= hi if mutation == "hi_clipped" else q > hi
    clip = below | above
    bound = (torch.where(below, hi, lo) if mutation == "swap_bounds" else torch.where(below, lo, hi)) + ro
    terms = torch.where(clip, bound.expand_as(u), q - u) * gr
    oterms = torch.where(clip, s * gr, torch.zeros_like(gr))
    return clip, terms, oterms


def backward_reference(x, g, scale, offset, tile, num_bits, mutation=None):
    """[dinput, dscale, doffset] as ops.quantize_by_tile_backward returns them, from float64 sums rounded once."""
    gr = to_rows(g, tile)
    s = scale.reshape(-1).double()
    o = None if offset is None else offset.reshape(-1).double()
    return _backward_outputs(backward_sums(to_rows(x, tile).double(), gr.double(), s, o, num_bits, mutation), gr, x.shape, tile, scale, offset, mutation)


def _backward_outputs(sums, gr, shape, tile, scale, offset, mutation=None):
    clip, terms, oterms = sums
    dscale, doffset = terms.sum(1), oterms.sum(1)
    if mutation == "drop_last":
        dscale[-1] -= terms[-1, -1]
        doffset[-1] -= oterms[-1, -1]
    if mutation == "count_twice":
        dscale[0] += terms[0, 0]
        doffset[0] += oterms[0, 0]
    dinput = from_rows(torch.where(clip, torch.zeros_like(gr), gr), tuple(shape), tile)
    return [dinput, dscale.float().reshape(scale.shape), scale.new_empty(0) if offset is None else doffset.float().reshape(scale.shape)]


def backward_case(shape: Shape, dtype, num_bits, with_offset) -> BackwardCase:
    nt, ne = num_tiles(shape.shape, shape.tile), tile_elems(shape.tile)
    gen = torch.Generator().manual_seed(_seed(shape, dtype, num_bits, with_offset, 1))
    t = torch.arange(nt)
    scale = (2.0 ** ((4 * t + num_bits) % 9 - 6).double()).float()                      # 2^-6 .. 2^2, neighbours differ
    offset = (-3.0 + 0.5 * ((7 * t + 1) % 13).double()).float() if with_offset else None  # halves; tile 0 holds -2.5
    ro = torch.round(offset.double()) if with_offset else torch.zeros(nt, dtype=torch.float64)
    x, u = _snap(_draw_u(nt, ne, num_bits, backward_far_share(ne), gen), ro, scale, dtype)
    r = torch.randint(0, 14, (nt, ne), generator=gen)  # one draw per element: g in [-3, 3], and which of its zeros are -0.0
    g = (r % 7 - 3).double()
    g[:, 0] = torch.where(g[:, 0] == 0, 1.0, g[:, 0])
    g[:, -1] = torch.where(g[:, -1] == 0, -2.0, g[:, -1])
    if dtype != torch.float32:
        g = torch.where((g == 0) & (r >= 7), -0.0, g)
    g = g.to(dtype)
    # the exactness condition, on the terms the reference formulas give
    sums = backward_sums(x.double(), g.double(), scale.double(), None if offset is None else offset.double(), num_bits)
    _, terms, oterms = sums
    assert bool((terms.float().double() == terms).all()) and bool((oterms.float().double() == oterms).all())
    assert_exact_sums(terms, f"dscale of {shape} {dtype} {num_bits} bits")
    if with_offset:
        assert_exact_sums(oterms, f"doffset of {shape} {dtype} {num_bits} bits")
    xs, gs = from_rows(x, shape.shape, shape.tile), from_rows(g, shape.shape, shape.tile)
    return BackwardCase(shape.shape, shape.tile, dtype, num_bits, xs, gs, scale, offset, census(u, num_bits),
                        _backward_outputs(sums, g, shape.shape, shape.tile, scale, offset))


BACKWARD_SPECIALS = ("nan_x", "pos_inf_x", "neg_inf_x", "nan_g")


def backward_with_specials(case: BackwardCase, kinds, tiles):
    """(x, g) with one special value per (kind, tile) at element 1 of that tile (element 0 of a one-element tile); the NaN gradient
    sits on an element made to clip (eight steps above the grid)."""
    xr, gr = to_rows(case.x, case.tile).clone(), to_rows(case.g, case.tile).clone()
    e = min(1, xr.shape[1] - 1)
    _, hi = _bounds(case.num_bits)
    for kind, t in zip(kinds, tiles):
        if kind == "nan_x":
            xr[t, e] = float("nan")
        elif kind == "pos_inf_x":
            xr[t, e] = float("inf")
        elif kind == "neg_inf_x":
            xr[t, e] = float("-inf")
        else:
            ro = 0.0 if case.offset is None else float(torch.round(case.offset[t]))
            xr[t, e] = (hi + 8 + ro) * float(case.scale[t])
            gr[t, e] = float("nan")
    return from_rows(xr, case.shape, case.tile), from_rows(gr, case.shape, case.tile)


# ---- grid error -------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class GridCase:
    shape: tuple
    tile: tuple
    dtype: torch.dtype
    num_bits: int
    x: torch.Tensor
    scales: torch.Tensor           # [33, tiles]; a run with fewer candidates takes the first rows
    offsets: torch.Tensor | None
    prefill: torch.Tensor          # [33, tiles]: exact multiples of each sum's quantum, for the accumulating call
    census: dict
    want: torch.Tensor             # [33, tiles] fp32: the float64 reference into a fresh `out`
    want_accumulated: torch.Tensor  # ... added to `prefill`


def grid_far_share(ne):
    """3 % in small tiles, 0.2 % beyond 4200 elements (the 133120-element tile is then at about 2^23.6)"""
    return 0.03 if ne <= 4200 else 0.002


def _fp32_representable(v, what):
    assert bool((v.float().double() == v).all()), f"{what} is not an fp32 number: float64 -> T would not be fp32 -> T"


def grid_squares(xr, s, o, num_bits, dtype, check=False, mutation=None):
    """Candidates `s`, `o` ([..., tiles]) on float64 rows `xr` ([tiles, elements]): the eager chain of min_error.py:218-231 with its three casts to the data dtype `T` —
    y = ((q + ro) * s).to(T); d = (y - x).to(T); e = (d * d).to(T). With `check`, every value is asserted to be an fp32 number
    before it is cast (rounding float64 -> T is then rounding fp32 -> T, which is what the kernels do) and every e to be finite."""
    lo, hi = _bounds(num_bits)
    ro = torch.zeros_like(s) if o is None else torch.round(o)
    s, ro = s[..., None], ro[..., None]
    cast = lambda v: v.to(dtype).double()  # noqa: E731
    r = torch.round(xr / s - ro)
    q = torch.where(r != r, r, r.clamp(lo, hi))
    y = (q + ro) * s
    if check:
        _fp32_representable(xr / s - ro, "x / s - ro")
        _fp32_representable(y, "(q + ro) * s")
    y = cast(y)
    d = y - xr
    if check:
        _fp32_representable(d, "y - x")
    if mutation != "skip_cast_d":
        d = cast(d)
    e = d * d
    if check:
        _fp32_representable(e, "d * d")
    if mutation != "skip_cast_e":
        e = cast(e)
    if check:
        assert bool(torch.isfinite(e).all()), "a squared difference overflows the data dtype"
    return e


def grid_reference(x, scales, offsets, tile, num_bits, mutation=None):
    """err[c][t] in fp32 from float64 sums; no assertion on the operands (special values pass)."""
    xr = to_rows(x, tile).double()
    out = torch.zeros(scales.shape, dtype=torch.float64)
    for c in _batches(scales.shape[0], xr.numel()):
        out[c] = grid_squares(xr, scales[c].double(), None if offsets is None else offsets[c].double(), num_bits, x.dtype, mutation=mutation).sum(-1)
    if mutation == "drop_candidate_16":
        out[16:17] = 0
    return out.float()


def _batches(ncand, numel):
    """slices of the candidates, about two million elements at a time"""
    step = max(1, 2**21 // numel)
    return [slice(c, min(c + step, ncand)) for c in range(0, ncand, step)]


def grid_chain_fp32(x, scales, offsets, tile, num_bits, perm=None):
    """The same chain in plain fp32 tensor ops, summed in fp32 (optionally over permuted tiles): what the reference is checked by."""
    lo, hi = _bounds(num_bits)
    xr = to_rows(x, tile).float()
    if perm is not None:
        xr = xr.gather(1, perm)
    T = x.dtype
    out = torch.zeros(scales.shape, dtype=torch.float32)
    for c in _batches(scales.shape[0], xr.numel()):
        s = scales[c].float()[..., None]
        ro = torch.zeros_like(s) if offsets is None else torch.round(offsets[c].float())[..., None]
        q = torch.round(xr / s - ro).clamp(lo, hi)
        y = ((q + ro) * s).to(T).float()
        d = (y - xr).to(T).float()
        out[c] = (d * d).to(T).float().sum(-1)
    return out


def grid_case(shape: Shape, dtype, num_bits, with_offset) -> GridCase:
    nt, ne = num_tiles(shape.shape, shape.tile), tile_elems(shape.tile)
    ncand = max(NCANDS)
    gen = torch.Generator().manual_seed(_seed(shape, dtype, num_bits, with_offset, 2))
    t, c = torch.arange(nt), torch.arange(ncand)
    span = 7 if dtype == torch.float16 else 9  # fp16: 2^-6 .. 2^0, so that no squared difference overflows
    s0 = (2.0 ** ((4 * t + num_bits) % span - 6).double()).float()
    very_far = num_bits <= 4 and 64 <= ne <= 1032
    x, u = _snap(_draw_u(nt, ne, num_bits, grid_far_share(ne), gen, very_far), torch.zeros(nt, dtype=torch.float64), s0, dtype)
    ks = torch.tensor(grid_exponents(num_bits), dtype=torch.float64)
    scales = (s0.double()[None, :] * 2.0 ** ks[(c[:, None] + t[None, :]) % len(ks)]).float()
    limit = grid_offset_limit(num_bits)
    offsets = (-limit + 0.5 * ((5 * c[:, None] + 7 * t[None, :] + 1) % (4 * limit + 1)).double()).float() if with_offset else None
    xr = x.double()
    sums = torch.zeros(ncand, nt, dtype=torch.float64)
    prefill = torch.zeros(ncand, nt, dtype=torch.float64)
    quanta = ((3 * c[:, None] + 5 * t[None, :]) % 8).double()  # the prefilled output, in quanta of the sum it is added to
    for k in _batches(ncand, xr.numel()):
        e = grid_squares(xr, scales[k].double(), None if offsets is None else offsets[k].double(), num_bits, dtype, check=True)
        prefill[k] = quanta[k] * assert_exact_sums(e, f"candidates {k.start}.. of {shape} {dtype} {num_bits} bits, prefilled", quanta[k])
        sums[k] = e.sum(-1)
    return GridCase(shape.shape, shape.tile, dtype, num_bits, from_rows(x, shape.shape, shape.tile), scales, offsets, prefill.float(),
                    census(u, num_bits), sums.float(), (sums + prefill).float())


def grid_with_special(x: torch.Tensor, tile, value: float, tile_index: int):
    """`x` with `value` at element 1 of that tile (element 0 of a one-element tile)"""
    xr = to_rows(x, tile).clone()
    xr[tile_index, min(1, xr.shape[1] - 1)] = value
    return from_rows(xr, tuple(x.shape), tile)


# ---- comparisons ------------------------------------------------------------------------------------------------------------------------
_INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}


def same_bits(got: torch.Tensor, want: torch.Tensor) -> bool:
    """Bit for bit, the sign of zero included."""
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(got.contiguous().view(_INT_VIEW[got.dtype]), want.contiguous().view(_INT_VIEW[want.dtype]))


def same_bits_or_both_nan(got: torch.Tensor, want: torch.Tensor) -> bool:
    """`same_bits` where neither side is a NaN, and NaN exactly where the other side is NaN (a NaN's payload is not compared)."""
    if got.dtype != want.dtype or got.shape != want.shape or not torch.equal(got != got, want != want):
        return False
    keep = want == want
    return same_bits(torch.where(keep, got, torch.zeros_like(got)), torch.where(keep, want, torch.zeros_like(want)))
