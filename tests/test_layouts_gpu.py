"""Every family of entry points on the layouts callers really pass (tests/layouts.py): contiguous views at an element offset
(``data_ptr() % 16`` of 1, 2, 4, 8, and 16-byte aligned but not 128-byte aligned), transposed, step-2, stride-0 and channels-last
views. The result on a view must be the result on ``view.clone()`` (fresh, contiguous, aligned): bit for bit, since the same
values reach the same kernels. The streaming kernels branch on ``aligned16``: the core codec falls through to its generic kernels,
the newer entry points are handed an aligned copy by the package (``ops._base._dense``). The codec's generic route is also pinned
to the C oracle, and zero-size operands are checked against the reference chain. Test ids name the view kind and the pointer's
remainder mod 16."""

from __future__ import annotations

import contextlib
import math

import pytest
import torch

import fastforward_amd as ff

from conftest import use_backend
from fastforward_amd import dispatcher, ops
from fastforward_amd.nn import functional as F
from fastforward_amd.nn.sdpa import scaled_dot_product_attention_math
from helpers import same_with_nan
from layouts import Layout, every, misaligned
from test_conv_gpu import accumulator64
from test_elementwise_gpu import check_softmax_contract
from test_modules_gpu import act_quantizer, check_layer_norm_contract
from test_skinny_gpu import _check as wq_within_bound

pytestmark = pytest.mark.gpu
DEV = "cuda"
CPP = torch.ops.fastforward_amd
VALUES = (torch.bfloat16, torch.float16, torch.float32)
NAME = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32", torch.int8: "i8", torch.uint8: "u8", torch.int32: "i32",
        torch.int64: "i64"}


def cases(dtypes, **kinds):
    """(dtype, layout) pairs with ids '<dtype>-<kind>@<bytes>B-ptr<remainder>'."""
    out = [(dt, layout) for dt in dtypes for layout in every(torch.empty(0, dtype=dt).element_size(), **kinds)]
    return pytest.mark.parametrize("dtype,layout", out, ids=[f"{NAME[dt]}-{layout.id}" for dt, layout in out])


def layouts_of(dtype, **kinds):
    ls = every(torch.empty(0, dtype=dtype).element_size(), **kinds)
    return pytest.mark.parametrize("layout", ls, ids=[layout.id for layout in ls])


def gen(seed):
    return torch.Generator(DEV).manual_seed(seed)


def same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and (same_with_nan(a, b) if a.is_floating_point() else torch.equal(a, b))


# ---- the helper itself -----------------------------------------------------------------------------------------------------------
def test_dense_returns_an_aligned_contiguous_operand_itself_and_copies_the_rest():
    from fastforward_amd.ops._base import _dense

    t = torch.randn(64, 32, device=DEV).to(torch.bfloat16)
    assert _dense(t) is t and _dense(None) is None
    assert _dense(t[16:]) is not None and _dense(t[16:]).data_ptr() == t[16:].data_ptr()  # 16 rows of 64 B: still aligned
    for view in (Layout("offset", 2).make(t), Layout("offset", 8).make(t), Layout("step2", 0).make(t), t.t()):
        d = _dense(view)
        assert d is not view and d.is_contiguous() and d.data_ptr() % 16 == 0 and torch.equal(d, view)
    cl = Layout("channels_last", 0).make(torch.randn(2, 16, 3, 5, device=DEV))
    assert _dense(cl, torch.channels_last) is cl
    cl8 = Layout("channels_last", 4).make(torch.randn(2, 16, 3, 5, device=DEV))
    d = _dense(cl8, torch.channels_last)
    assert d.is_contiguous(memory_format=torch.channels_last) and d.data_ptr() % 16 == 0 and torch.equal(d, cl8)


# ---- core codec: bit for bit against the clone (fast and generic kernel families are bit-identical) -----------------------------
SHAPE = (24, 64)
TILES = {"tensor": SHAPE, "channel": (1, 64), "block32": (1, 32), "tile4x16": (4, 16)}


def params(tile, seed, with_offset=True):
    n = math.prod(s // t for s, t in zip(SHAPE, tile))
    g = gen(seed)
    scale = torch.rand(n, device=DEV, generator=g) * 0.05 + 0.02
    offset = torch.randint(-3, 4, (n,), device=DEV, generator=g).float() if with_offset else None
    return scale, offset


def data(dtype, seed=0, shape=SHAPE):
    x = torch.randn(shape, device=DEV, generator=gen(seed)) * 3
    n = min(3, x.numel())
    x.view(-1)[:n] = torch.tensor([0.0, -0.0, 1e-30], device=DEV)[:n]
    return x.to(dtype)


@cases(VALUES)
def test_quantize_by_tile(dtype, layout):
    v = layout.make(data(dtype))
    c = v.clone()
    for name, tile in TILES.items():
        scale, offset = params(tile, len(name))
        for bits in (8, 4, 3):
            for out_dtype in (torch.int8, None):
                want = ops.quantize_by_tile(c, scale, tile, bits, out_dtype, offset)
                assert same(ops.quantize_by_tile(v, scale, tile, bits, out_dtype, offset), want), (name, bits, out_dtype)
                assert same(CPP.quantize_by_tile(v, scale, list(tile), float(bits), out_dtype, offset), want), (name, bits, out_dtype)


@pytest.mark.parametrize("out_dtype", VALUES, ids=[NAME[d] for d in VALUES])
@cases((torch.int8, torch.bfloat16))
def test_dequantize_by_tile(dtype, layout, out_dtype):
    codes = torch.randint(-128, 128, SHAPE, device=DEV, generator=gen(1)).to(dtype)
    v = layout.make(codes)
    c = v.clone()
    for name, tile in TILES.items():
        scale, offset = params(tile, len(name))
        want = ops.dequantize_by_tile(c, scale, tile, offset, out_dtype)
        assert same(ops.dequantize_by_tile(v, scale, tile, offset, out_dtype), want), name
        assert same(CPP.dequantize_by_tile(v, scale, list(tile), offset, out_dtype), want), name


@pytest.mark.parametrize("shape", [(1,), (7,), (3, 5), (17,), (2, 3, 7), (8,), (16,), (5, 24)], ids=str)
@pytest.mark.parametrize("layout", misaligned(2), ids=[layout.id for layout in misaligned(2)])
def test_codec_at_sizes_around_the_vector_width(shape, layout):
    """numel = 1 ... 15 mod 16, and exactly 8 and 16: the tails of the generic and the vector kernels."""
    x = data(torch.bfloat16, 3, shape)
    v, c = layout.make(x), x.clone()
    scale, offset = torch.tensor([0.03], device=DEV), torch.tensor([2.0], device=DEV)
    q = ops.quantize_by_tile(v, scale, shape, 8, torch.int8, offset)
    assert same(q, ops.quantize_by_tile(c, scale, shape, 8, torch.int8, offset))
    qb = q.to(torch.bfloat16)
    assert same(ops.dequantize_by_tile(layout.make(qb), scale, shape, offset, torch.float32), ops.dequantize_by_tile(qb, scale, shape, offset, torch.float32))
    assert same(ops.minmax_by_tile(v, shape), ops.minmax_by_tile(c, shape))
    assert same(ops.quantize_dynamic_by_tile(v, shape, 8, False, False, torch.int8), ops.quantize_dynamic_by_tile(c, shape, 8, False, False, torch.int8))


@cases(VALUES)
def test_quantize_dynamic_by_tile(dtype, layout):
    v = layout.make(data(dtype, 2))
    c = v.clone()
    for tile in (SHAPE, (1, 64), (1, 32)):  # per tensor, per token (the one-launch form), per block
        for sym, one in ((False, False), (True, False), (True, True)):
            want = ops.quantize_dynamic_by_tile(c, tile, 8, sym, one, torch.int8)
            assert same(ops.quantize_dynamic_by_tile(v, tile, 8, sym, one, torch.int8), want), (tile, sym, one)
            assert same(CPP.quantize_dynamic_by_tile(v, list(tile), 8.0, sym, one, torch.int8), want), (tile, sym, one)


@cases(VALUES)
def test_minmax_and_running_minmax(dtype, layout):
    v = layout.make(data(dtype, 4))
    c = v.clone()
    for tile in TILES.values():
        want = ops.minmax_by_tile(c, tile)
        assert same(ops.minmax_by_tile(v, tile), want), tile
        n = want[0].numel()
        results = []
        for operand in (v, c):
            rmin = torch.full((n,), 0.5, dtype=dtype, device=DEV)
            rmax = torch.full((n,), 0.75, dtype=dtype, device=DEV)
            scale, offset = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
            ops.running_minmax_step(operand, tile, rmin, rmax, None, 8, False, False, scale, offset)
            ops._running_minmax_step(operand, tile, rmin, rmax, None, 8, False, False, scale, offset)  # (the ctypes route, a second step)
            r2min, r2max = torch.full((n,), 0.5, dtype=dtype, device=DEV), torch.full((n,), 0.75, dtype=dtype, device=DEV)
            s2, o2 = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
            codes = ops.running_minmax_quantize(operand, tile, r2min, r2max, None, 8, False, False, s2, o2, torch.int8)
            if codes is None:  # the documented decline: nothing written, the caller takes the two calls
                ops.running_minmax_step(operand, tile, r2min, r2max, None, 8, False, False, s2, o2)
                codes = ops.quantize_by_tile(operand, s2, tile, 8, torch.int8, o2)
            results.append((rmin, rmax, scale, offset, codes, r2min, r2max, s2, o2))
        assert same(results[0], results[1]), tile


@pytest.mark.parametrize("sync_free", [False, True])
@layouts_of(torch.bfloat16)
def test_range_estimation_on_a_view(layout, sync_free):
    x = data(torch.bfloat16, 5)
    got = []
    for operand in (layout.make(x), layout.make(x).clone()):
        q = ff.nn.LinearQuantizer(8, symmetric=False, granularity=ff.PerChannel(0), quantized_dtype=torch.int8, device=DEV)
        with torch.no_grad(), ff.estimate_ranges(q, ff.range_setting.running_minmax, sync_free=sync_free):
            first = q(operand)
            second = q(operand * 0.5)
        got.append((first.raw_data, second.raw_data, q.scale.detach().clone(), q.offset.detach().clone()))
    assert same(got[0], got[1])


@layouts_of(torch.float32, expand=True)
def test_parameters_for_range(layout):
    g = gen(6)
    lo = -torch.rand(8, 16, device=DEV, generator=g) * 4
    hi = torch.rand(8, 16, device=DEV, generator=g) * 4
    lo[0, :3] = torch.tensor([0.0, 0.0, 1.0])
    hi[0, :3] = torch.tensor([0.0, 2.0, 3.0])
    lv, hv = layout.make(lo), layout.make(hi)
    for sym, one in ((False, False), (True, False), (True, True)):
        assert same(ops.parameters_for_range(lv, hv, 8, sym, one), ops.parameters_for_range(lv.clone(), hv.clone(), 8, sym, one))


@cases(VALUES)
def test_quantize_by_tile_backward(dtype, layout):
    x = data(dtype, 7)
    grad = torch.randn(SHAPE, device=DEV, generator=gen(8)).to(dtype)
    v, gv = layout.make(x), layout.make(grad)
    for name, tile in TILES.items():
        scale, offset = params(tile, 9)
        want = ops.quantize_by_tile_backward(v.clone(), gv.clone(), scale, tile, 4, offset)
        assert same(ops.quantize_by_tile_backward(v, gv, scale, tile, 4, offset), want), name
        assert same(CPP.quantize_by_tile_backward(v, gv, scale, list(tile), 4.0, offset), want), name


@cases(VALUES)
def test_grid_sqerror_by_tile(dtype, layout):
    v = layout.make(data(dtype, 10))
    for tile in ((1, 64), (1, 32)):
        n = math.prod(s // t for s, t in zip(SHAPE, tile))
        scales = torch.rand(5, n, device=DEV, generator=gen(11)) * 0.05 + 0.02
        offsets = torch.randint(-3, 4, (5, n), device=DEV, generator=gen(12)).float()
        want = ops.grid_sqerror_by_tile(v.clone(), scales, offsets, tile, 4)
        got = ops.grid_sqerror_by_tile(v, scales, offsets, tile, 4)
        assert same(got, want), tile  # (None for both where the tiling is outside the kernel's range)


@layouts_of(torch.int8)
def test_pack_and_unpack_int4(layout):
    codes = torch.randint(-8, 8, SHAPE, device=DEV, generator=gen(13), dtype=torch.int8)
    v = layout.make(codes)
    packed = ops.pack_int4(v, 32)
    assert same(packed, ops.pack_int4(v.clone(), 32))
    assert same(ops.unpack_int4(packed, SHAPE, torch.int8, 32), codes)
    pv = layout.make(packed.reshape(SHAPE[0], -1))  # the packed bytes viewed the same way
    assert same(ops.unpack_int4(pv, SHAPE, torch.int8, 32), codes)
    assert same(ops.unpack_int4(pv, SHAPE, torch.bfloat16, 32), codes.to(torch.bfloat16))


@cases(VALUES)
def test_quantize_pack_and_unpack_dequantize_int4(dtype, layout):
    v = layout.make(data(dtype, 14))
    for name, tile in (("channel", (1, 64)), ("block32", (1, 32)), ("tensor", SHAPE)):
        scale, offset = params(tile, 15)
        want = ops.quantize_pack_int4(v.clone(), scale, tile, offset, 32)
        packed = ops.quantize_pack_int4(v, scale, tile, offset, 32)
        assert same(packed, want), name
        assert same(packed, ops.pack_int4(ops.quantize_by_tile(v.clone(), scale, tile, 4, torch.int8, offset), 32)), name
        for pl in misaligned(1):
            pv = pl.make(packed)
            for out_dtype in VALUES:
                want_d = ops.unpack_dequantize_int4(packed, scale, SHAPE, tile, offset, 32, out_dtype)
                assert same(ops.unpack_dequantize_int4(pv, scale, SHAPE, tile, offset, 32, out_dtype), want_d), (name, pl.id, out_dtype)


@layouts_of(torch.int8)
def test_gguf_block_writers(layout):
    codes = torch.randint(-8, 8, (40, 32), device=DEV, generator=gen(16), dtype=torch.int8)
    codes8 = torch.randint(-128, 128, (40, 32), device=DEV, generator=gen(17), dtype=torch.int8)
    scales = torch.rand(40, device=DEV, generator=gen(18)) + 0.1
    sv = Layout("offset", 4).make(scales)
    assert same(ops.pack_q4_0_blocks(layout.make(codes), sv), ops.pack_q4_0_blocks(codes, scales))
    assert same(ops.pack_q8_0_blocks(layout.make(codes8), sv), ops.pack_q8_0_blocks(codes8, scales))


@cases(VALUES)
def test_quantize_by_tile_unless_same(dtype, layout):
    v = layout.make(data(dtype, 19))
    s, o = torch.tensor([0.03], device=DEV), torch.tensor([1.0], device=DEV)
    es = torch.tensor([0.05], device=DEV)
    want = ops.quantize_by_tile_unless_same(v.clone(), s, o, 8, es, o)
    assert want is not None and same(want, ops.quantize_by_tile(v.clone(), s, SHAPE, 8, torch.int8, o))
    got = ops.quantize_by_tile_unless_same(v, s, o, 8, es, o)
    assert got is None or same(got, want)  # None: nothing launched, the caller quantizes (documented decline)


@pytest.mark.parametrize("layout", every(2, expand=True), ids=[layout.id for layout in every(2, expand=True)])
def test_codec_on_views_matches_the_oracle(layout, oracle_lib):
    """The route a view takes on the device (generic kernels where misaligned) against the C oracle on the same values."""
    x = data(torch.bfloat16, 20)
    v = layout.make(x)
    tile = (1, 32)
    scale, offset = params(tile, 21)
    q = ops.quantize_by_tile(v, scale, tile, 4, torch.int8, offset)
    d = ops.dequantize_by_tile(Layout("offset", 1).make(q), scale, tile, offset, torch.bfloat16)
    mm = ops.minmax_by_tile(v, tile)
    dyn = ops.quantize_dynamic_by_tile(v, tile, 8, False, False, torch.int8)
    host = v.cpu()
    with use_backend(oracle_lib):
        assert same(q.cpu(), ops.quantize_by_tile(host, scale.cpu(), tile, 4, torch.int8, offset.cpu()))
        assert same(d.cpu(), ops.dequantize_by_tile(q.cpu(), scale.cpu(), tile, offset.cpu(), torch.bfloat16))
        assert same([t.cpu() for t in mm], ops.minmax_by_tile(host, tile))
        assert same([t.cpu() for t in dyn], ops.quantize_dynamic_by_tile(host, tile, 8, False, False, torch.int8))


# ---- fused modules and elementwise ----------------------------------------------------------------------------------------------
ROUTED = ("layer_norm_quantize", "embedding_quantize", "pointwise_quantize", "binary_quantize", "softmax_quantize", "activation_quantize")


@pytest.fixture()
def launches(monkeypatch):
    counts = {name: 0 for name in ROUTED}
    for name in ROUTED:
        real = getattr(ops, name)

        def counted(*a, _real=real, _name=name, **k):
            counts[_name] += 1
            return _real(*a, **k)

        monkeypatch.setattr(ops, name, counted)
    return counts


def on_view_and_clone(fn, make_args, launches, check=same):
    """fn on the views and on their clones, with and without an output quantizer: no exception, the values agree, the codes are A1
    of the value, and both calls took the same route."""
    oq = act_quantizer(-2.0, 2.0)
    got, want, routes = [], [], []
    for clone in (False, True):
        before = dict(launches)
        args, kwargs = make_args(clone)
        with torch.no_grad(), ff.strict_quantization(False):
            value = fn(*args, output_quantizer=None, **kwargs)
            quantized = fn(*args, output_quantizer=oq, **kwargs)
        (want if clone else got).append((value, quantized))
        routes.append({k: launches[k] - before[k] for k in launches})
    (value, quantized), (want_value, want_q) = got[0], want[0]
    check(value, want_value)
    with torch.no_grad():
        assert torch.equal(quantized.raw_data, oq(value).raw_data)
        qv = quantized.dequantize()
    assert routes[0] == routes[1], routes
    if check is same:
        assert torch.equal(quantized.raw_data, want_q.raw_data) and same(qv, want_q.dequantize())
    return routes[0]


def plain_or_codes(x, layout, form):
    """`x` viewed through `layout`, plain or as a QuantizedTensor whose codes are viewed through `layout`."""
    if form == "plain":
        return lambda clone: layout.make(x).clone() if clone else layout.make(x)
    q = act_quantizer(-4.0, 5.0)(x) if form == "int8" else act_quantizer(-4.0, 5.0, container=x.dtype)(x)
    lay = Layout(layout.kind, layout.byte_offset // x.element_size()) if form == "int8" and layout.kind != "expand" else layout

    def make(clone):
        raw = lay.make(q.raw_data)
        return ff.QuantizedTensor(raw.clone() if clone else raw, q.quantization_context)

    return make


FORMS = ("plain", "int8", "container")
UNARY = {
    "relu": lambda x: (F.relu, (x,), {}),
    "silu": lambda x: (F.silu, (x,), {}),
    "sigmoid": lambda x: (F.sigmoid, (x,), {}),
    "gelu": lambda x: (F.gelu, (x,), {}),
    "gelu_tanh": lambda x: (F.gelu, (x,), {"approximate": "tanh"}),
}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("op", list(UNARY))
@layouts_of(torch.bfloat16, expand=True)
def test_pointwise_and_activations(op, form, layout, launches):
    x = data(torch.bfloat16, 22, (9, 40))
    operand = plain_or_codes(x, layout, form)

    def make(clone):
        fn, args, kw = UNARY[op](operand(clone))
        return args, kw

    fn, _, extra = UNARY[op](x)
    route = on_view_and_clone(lambda *a, **k: fn(*a, **k), make, launches)
    assert sum(route.values()) == 2, route  # the fused kernel ran for the view, with and without the output quantizer


@pytest.mark.parametrize("form", FORMS)
@layouts_of(torch.bfloat16, expand=True)
def test_softmax(form, layout, launches):
    operand = plain_or_codes(data(torch.bfloat16, 23, (9, 40)), layout, form)
    route = on_view_and_clone(lambda x, **k: F.softmax(x, -1, **k), lambda clone: ((operand(clone),), {}), launches)
    assert route["softmax_quantize"] == 2


@pytest.mark.parametrize("affine", ["none", "weight_and_bias_views"])
@pytest.mark.parametrize("form", FORMS)
@layouts_of(torch.bfloat16, expand=True)
def test_layer_norm(form, affine, layout, launches):
    x = data(torch.bfloat16, 24, (9, 40))
    operand = plain_or_codes(x, layout, form)
    w = (torch.rand(40, device=DEV, generator=gen(25)) + 0.5).to(torch.bfloat16)
    b = (torch.randn(40, device=DEV, generator=gen(26)) * 0.1).to(torch.bfloat16)

    def make(clone):
        if affine == "none":
            return (operand(clone), (40,)), {}
        wv, bv = Layout("offset", 2).make(w), Layout("offset", 6).make(b)
        return (operand(clone), (40,), wv.clone() if clone else wv, bv.clone() if clone else bv, 1e-5), {}

    route = on_view_and_clone(F.layer_norm, make, launches)
    assert route["layer_norm_quantize"] == 2


BINARY = ("add", "sub", "mul", "div")


@pytest.mark.parametrize("which", ["input", "other", "both", "bias_suffix", "scalar"])
@pytest.mark.parametrize("op", BINARY)
@layouts_of(torch.bfloat16, expand=True)
def test_binary(op, which, layout, launches):
    a = data(torch.bfloat16, 27, (9, 40))
    b = (torch.rand(9, 40, device=DEV, generator=gen(28)) + 0.5).to(torch.bfloat16)
    bias = (torch.rand(40, device=DEV, generator=gen(29)) + 0.5).to(torch.bfloat16)
    av, bv = plain_or_codes(a, layout, "plain"), plain_or_codes(b, layout, "plain")
    bias_lay = Layout("offset", layout.byte_offset) if layout.kind in ("offset",) else Layout("offset", 2)
    fn = getattr(F, op)

    def make(clone):
        fresh_a, fresh_b = a.clone(), b.clone()
        if which == "input":
            return (av(clone), fresh_b), {}
        if which == "other":
            return (fresh_a, bv(clone)), {}
        if which == "both":
            return (av(clone), bv(clone)), {}
        if which == "bias_suffix":
            bb = bias_lay.make(bias)
            return (av(clone), bb.clone() if clone else bb), {}
        return (av(clone), 1.5), {}

    route = on_view_and_clone(fn, make, launches)
    assert route["binary_quantize"] == 2


@pytest.mark.parametrize("op", BINARY)
@pytest.mark.parametrize("layout", misaligned(1), ids=[layout.id for layout in misaligned(1)])
def test_binary_on_int8_codes_at_an_offset(op, layout, launches):
    a = data(torch.bfloat16, 30, (9, 40))
    b = (torch.rand(9, 40, device=DEV, generator=gen(31)) + 0.5).to(torch.bfloat16)
    qa, qb = plain_or_codes(a, Layout("offset", layout.byte_offset * 2), "int8"), plain_or_codes(b, Layout("offset", 2), "int8")
    route = on_view_and_clone(getattr(F, op), lambda clone: ((qa(clone), qb(clone)), {}), launches)
    assert route["binary_quantize"] == 2


@pytest.mark.parametrize("ids_dtype", [torch.int64, torch.int32], ids=["i64", "i32"])
@layouts_of(torch.int8)
def test_embedding(layout, ids_dtype, launches):
    V, D = 50, 96
    table = torch.randn(V, D, device=DEV, generator=gen(32)).to(torch.bfloat16)
    q = ff.nn.LinearQuantizer(8, granularity=ff.PerChannel(0), quantized_dtype=torch.int8, device=DEV)
    q.quantization_range = (table.float().amin(1), table.float().amax(1))
    with torch.no_grad():
        qt = q(table)
    ids = torch.randint(0, V, (3, 14), device=DEV, generator=gen(33)).to(ids_dtype)
    ids_lay = Layout(layout.kind, layout.byte_offset * ids.element_size()) if layout.kind != "expand" else layout

    def make(clone):
        raw, iv = layout.make(qt.raw_data), ids_lay.make(ids)
        if clone:
            raw, iv = raw.clone(), iv.clone()
        return (iv, ff.QuantizedTensor(raw, qt.quantization_context)), {}

    route = on_view_and_clone(F.embedding, make, launches)
    assert route["embedding_quantize"] == 2


@layouts_of(torch.bfloat16)
def test_the_modules_on_views(layout, launches):
    x = data(torch.bfloat16, 34, (9, 40))
    with torch.no_grad(), ff.strict_quantization(False):
        for cls in (ff.nn.QuantizedRelu, ff.nn.QuantizedSilu):
            m = cls()
            m.output_quantizer = act_quantizer(-2.0, 2.0)
            assert same(m(layout.make(x)).raw_data, m(layout.make(x).clone()).raw_data), cls.__name__
        ln = ff.nn.QuantizedLayerNorm(40).to(DEV, torch.bfloat16)
        ln.output_quantizer = act_quantizer(-2.0, 2.0)
        assert same(ln(layout.make(x)).raw_data, ln(layout.make(x).clone()).raw_data)
        emb = ff.nn.QuantizedEmbedding(50, 96).to(DEV, torch.bfloat16)
        emb.weight_quantizer = ff.nn.LinearQuantizer(8, granularity=ff.PerChannel(0), quantized_dtype=torch.int8, device=DEV)
        emb.weight_quantizer.quantization_range = (emb.weight.float().amin(1), emb.weight.float().amax(1))
        emb.output_quantizer = act_quantizer(-2.0, 2.0)
        ids = torch.randint(0, 50, (9, 40), device=DEV, generator=gen(35)).to(torch.int32)
        iv = Layout(layout.kind, layout.byte_offset * 2).make(ids)
        assert same(emb(iv).raw_data, emb(iv.clone()).raw_data)
    assert launches["pointwise_quantize"] == 4 and launches["layer_norm_quantize"] == 2 and launches["embedding_quantize"] == 2


def test_contracts_against_the_reference_chain_on_an_offset_view(launches):
    """The offset view's fused values against the reference chain under the existing contracts (the fused call must run)."""
    x = Layout("offset", 2).make(data(torch.bfloat16, 36, (9, 40)))
    with torch.no_grad(), ff.strict_quantization(False):
        ln, sm = F.layer_norm(x, (40,)), F.softmax(x, -1)
        assert launches["layer_norm_quantize"] == 1 and launches["softmax_quantize"] == 1
        with chain_off():
            check_layer_norm_contract(ln, F.layer_norm(x, (40,)))
            check_softmax_contract(sm, F.softmax(x, -1))
            assert launches["layer_norm_quantize"] == 1 and launches["softmax_quantize"] == 1


@contextlib.contextmanager
def chain_off():
    """The dispatcher without this package's module / elementwise kernels: the reference chain runs."""
    from fastforward_amd import fused_elementwise, fused_modules  # noqa: F401

    saved = {}
    for op in ("layer_norm", "embedding", "relu", "silu", "add", "sub", "mul", "div", "softmax", "sigmoid", "gelu"):
        saved[op] = dispatcher._DISPATCHER[op]
        dispatcher._DISPATCHER[op] = [it for it in saved[op] if getattr(it.fn, "__self__", None) not in (fused_elementwise.KERNELS, fused_modules.KERNELS)]
    try:
        yield
    finally:
        dispatcher._DISPATCHER.update(saved)


# ---- zero-size operands -----------------------------------------------------------------------------------------------------------
ZERO = {
    "relu": lambda x: F.relu(x, output_quantizer=act_quantizer(-2.0, 2.0)),
    "silu": lambda x: F.silu(x, output_quantizer=act_quantizer(-2.0, 2.0)),
    "sigmoid": lambda x: F.sigmoid(x, output_quantizer=act_quantizer(-2.0, 2.0)),
    "gelu": lambda x: F.gelu(x, output_quantizer=act_quantizer(-2.0, 2.0)),
    "softmax": lambda x: F.softmax(x, -1, output_quantizer=act_quantizer(-2.0, 2.0)),
    "layer_norm": lambda x: F.layer_norm(x, (x.shape[-1],), output_quantizer=act_quantizer(-2.0, 2.0)),
    "add": lambda x: F.add(x, x, output_quantizer=act_quantizer(-2.0, 2.0)),
    "mul_scalar": lambda x: F.mul(x, 2.0, output_quantizer=act_quantizer(-2.0, 2.0)),
    "div": lambda x: F.div(x, x, output_quantizer=act_quantizer(-2.0, 2.0)),
    "embedding": lambda x: F.embedding(torch.zeros(x.shape[:-1], dtype=torch.int64, device=DEV), act_quantizer(-4.0, 4.0)(
        torch.randn(5, 40, device=DEV).to(torch.bfloat16)), output_quantizer=act_quantizer(-2.0, 2.0)),
}
ZERO_CASES = [(op, shape) for op in ZERO for shape in ((0, 40), (3, 0, 40), (0,)) if not (op == "embedding" and len(shape) == 1)]


def _outcome(fn, x):
    try:
        with torch.no_grad(), ff.strict_quantization(False):
            r = fn(x)
    except Exception as e:  # noqa: BLE001
        return type(e)
    return r


@pytest.mark.parametrize("op,shape", ZERO_CASES, ids=[f"{op}-{shape}" for op, shape in ZERO_CASES])
def test_zero_size_operands_behave_like_the_reference_chain(op, shape):
    x = torch.empty(shape, device=DEV, dtype=torch.bfloat16)
    got = _outcome(ZERO[op], x)
    with chain_off():
        want = _outcome(ZERO[op], x)
    if isinstance(want, type):  # the reference raises: the same type of exception
        assert isinstance(got, type) and issubclass(got, want), (got, want)
        return
    assert not isinstance(got, type), got
    got_t = got.raw_data if isinstance(got, ff.QuantizedTensor) else got
    want_t = want.raw_data if isinstance(want, ff.QuantizedTensor) else want
    assert type(got) is type(want) and got_t.shape == want_t.shape and got_t.numel() == 0 and got_t.dtype == want_t.dtype


# ---- GEMMs --------------------------------------------------------------------------------------------------------------------------
def int8(shape, seed, lo=-128, hi=128):
    return torch.randint(lo, hi, shape, device=DEV, generator=gen(seed), dtype=torch.int8)


W8A8_ROUTES = {"cpp": ops.linear_w8a8, "ctypes": lambda *a: ops._linear_w8a8(*a, torch.bfloat16, None, None, 8.0, None, None)}


@pytest.mark.parametrize("route", list(W8A8_ROUTES))
@pytest.mark.parametrize("operand", ["x", "w", "bias", "all"])
@layouts_of(torch.int8)
def test_linear_w8a8(layout, operand, route):
    if route == "cpp" and not ops.NATIVE_DISPATCH:
        pytest.fail("the C++ dispatch-key extension is not loaded")
    M, N, K = 33, 96, 128
    x, w = int8((M, K), 40), int8((N, K), 41)
    bias = torch.randn(N, device=DEV, generator=gen(42)).to(torch.bfloat16)
    sx, ox, sw = torch.tensor([0.02], device=DEV), torch.tensor([3.0], device=DEV), torch.rand(N, device=DEV, generator=gen(43)) * 0.01 + 0.001
    blay = Layout(layout.kind, layout.byte_offset * 2) if layout.kind in ("offset", "step2") else Layout("offset", 2)  # (the bias is 1-d)
    xv = layout.make(x) if operand in ("x", "all") else x
    wv = layout.make(w) if operand in ("w", "all") else w
    bv = blay.make(bias) if operand in ("bias", "all") else bias
    call = W8A8_ROUTES[route]
    want = call(x, w, sx, ox, sw, None, bias)
    assert same(call(xv, wv, sx, ox, sw, None, bv), want)


@pytest.mark.parametrize("route", ["cpp", "ctypes"])
@layouts_of(torch.int8)
def test_bmm_w8a8(layout, route):
    B, M, N, K = 3, 20, 48, 64
    x, w = int8((B, M, K), 44), int8((B, N, K), 45)
    s, o = torch.tensor([0.02], device=DEV), torch.tensor([1.0], device=DEV)
    call = ops.bmm_w8a8 if route == "cpp" else (lambda *a: ops._bmm_w8a8(*a, torch.bfloat16, None, None, 8.0, None))
    want = call(x, w, s, o, s, None)
    assert same(call(layout.make(x), layout.make(w), s, o, s, None), want)


@layouts_of(torch.int8)
def test_linear_w8a8_multi(layout):
    M, K, rows = 2048, 256, (768, 768, 512)
    x, w = int8((M, K), 46), int8((sum(rows), K), 47)
    sx, sw = torch.tensor([0.02], device=DEV), torch.rand(sum(rows), device=DEV, generator=gen(48)) * 0.01 + 0.001
    want = ops.linear_w8a8_multi(x, w, sx, None, sw, rows)
    assert want is not None
    got = ops.linear_w8a8_multi(layout.make(x), layout.make(w), sx, None, sw, rows)
    assert got is None or same(got, want)  # None: the documented decline, the caller launches the linears one by one
    if got is None:
        pytest.fail(f"linear_w8a8_multi declined a {layout.id} view that its aligned clone takes")


def wq_operands(N, K, group, seed):
    w = torch.randint(-8, 8, (N, K), device=DEV, generator=gen(seed), dtype=torch.int8)
    scale = torch.rand(N, K // group, device=DEV, generator=gen(seed + 1)) * 0.02 + 0.005
    offset = torch.randint(-2, 3, (N, K // group), device=DEV, generator=gen(seed + 2)).float()
    return w, scale, offset


WQ_ROUTES = {"cpp": ops.linear_wq, "ctypes": lambda x, w, s, o, g, pack_block=0: ops._linear_wq(x, w, s, o, g, None, torch.bfloat16, pack_block, -1, 0)}


WQ_VIEWS = [(o, layout) for o in ("x", "w", "both") for layout in misaligned(2) + [Layout("step2", 0)]] + [("w", Layout("offset", 1))]


@pytest.mark.parametrize("route", list(WQ_ROUTES))
@pytest.mark.parametrize("packed", [False, True], ids=["int8_codes", "nibbles"])
@pytest.mark.parametrize("operand,layout", WQ_VIEWS, ids=[f"{o}-{layout.id}" for o, layout in WQ_VIEWS])
def test_linear_wq(layout, operand, packed, route):
    M, N, K, group = 7, 256, 256, 64
    x = (torch.randn(M, K, device=DEV, generator=gen(50)) * 0.5).to(torch.bfloat16)
    w, scale, offset = wq_operands(N, K, group, 51)
    wk = ops.pack_int4(w, 32) if packed else w
    xv = layout.make(x) if operand in ("x", "both") else x
    wv = layout.make(wk) if operand in ("w", "both") else wk
    call = WQ_ROUTES[route]
    want = call(x, wk, scale, offset, group, pack_block=32 if packed else 0)
    assert want is not None
    got = call(xv, wv, scale, offset, group, pack_block=32 if packed else 0)
    if got is None:
        pytest.fail("linear_wq declined a view its aligned clone takes")
    assert same(got, want)
    wq_within_bound(x, w, scale, offset, group, got)


@pytest.mark.parametrize("layout", misaligned(2), ids=lambda layout: layout.id)
def test_linear_wq_multi_and_mlp_gate_up_wq(layout):
    M, K, group = 5, 256, 64
    x = (torch.randn(M, K, device=DEV, generator=gen(52)) * 0.5).to(torch.bfloat16)
    mats = [wq_operands(n, K, group, 53 + 3 * i) for i, n in enumerate((256, 256, 128))]
    codes = [m[0] for m in mats]
    cv = [Layout("offset", layout.byte_offset // 2 or 1).make(c) for c in codes]
    want = ops.linear_wq_multi(x, codes, [m[1] for m in mats], [m[2] for m in mats], group)
    assert want is not None
    got = ops.linear_wq_multi(layout.make(x), cv, [m[1] for m in mats], [m[2] for m in mats], group)
    assert got is not None and same(got, want)
    (g, gs, go), (u, us, uo) = mats[0], mats[1]
    want = ops.mlp_gate_up_wq(x, g, u, gs, go, us, uo, group)
    assert want is not None
    got = ops.mlp_gate_up_wq(layout.make(x), cv[0], cv[1], gs, go, us, uo, group)
    assert got is not None and same(got, want)


# ---- conv and SDPA ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", misaligned(1) + [Layout("channels_last", 0), Layout("channels_last", 1), Layout("channels_last", 8),
                                                    Layout("transposed", 0)], ids=lambda layout: layout.id)
def test_conv2d_on_codes_at_an_offset(layout):
    B, C, OC, H, W = 2, 16, 24, 9, 11
    x, w = int8((B, C, H, W), 60, -20, 20), int8((OC, C, 3, 3), 61, -20, 20)
    one, zero = torch.ones(1, device=DEV), torch.zeros(1, device=DEV)
    xv = layout.make(x)
    got = ops.conv2d_w8a8(xv, w, one, zero, one, None, None, 1, 1, 1, torch.float32)
    want = accumulator64(x, w, (1, 1), (1, 1), (1, 1))
    assert torch.equal(got.double(), want)
    assert same(got, ops.conv2d_w8a8(xv.clone(), w, one, zero, one, None, None, 1, 1, 1, torch.float32))
    wv = Layout("offset", 1).make(w)
    assert same(ops.conv2d_w8a8(xv, wv, one, zero, one, None, None, 1, 1, 1, torch.float32), got)


@pytest.mark.parametrize("layout", misaligned(2) + [Layout("step2", 0), Layout("step2", 2)], ids=lambda layout: layout.id)
def test_sdpa_on_views_gives_the_math_path(layout):
    g = torch.Generator().manual_seed(62)
    q, k, v = [(torch.randint(-8, 9, (1, 2, 33, 64), generator=g) * 2.0**-3).to(torch.bfloat16).to(DEV) for _ in range(3)]
    qv, kv, vv = layout.make(q), layout.make(k), layout.make(v)
    aligned = layout.kind == "offset" and layout.byte_offset % 16 == 0  # (16-byte aligned rows: the fused kernel takes the view)
    with torch.no_grad():
        got = F.scaled_dot_product_attention(qv, kv, vv, strict_quantization=False)
        if aligned:
            want = F.scaled_dot_product_attention(q, k, v, strict_quantization=False)
        else:
            want = scaled_dot_product_attention_math(qv, kv, vv, strict_quantization=False)
    assert torch.equal(got, want)
