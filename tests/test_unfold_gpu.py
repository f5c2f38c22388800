"""The one-pass unfold kernel (csrc/ffq_unfold.hip) on the MI355X.

unfold only moves data, so nothing is tolerated anywhere: value and codes equal the device reference chain's (dequantize,
``torch.nn.functional.unfold``, the output quantizer) bit for bit — compared as integer patterns, so the sign of a zero counts —
with this package's registration taken out of the dispatcher. The shapes are the smallest at which each branch of the kernel can go
wrong (``test_unfold_cpu.GEOMETRIES``).

Every test counts the calls of ``ops.unfold_quantize``, so a silent fallback fails it."""

import contextlib

import pytest
import torch

import fastforward_amd as ff
import guards

from fastforward_amd import dispatcher, fused_unfold, ops
from fastforward_amd.nn import functional as F
from layouts import every
from test_modules_gpu import act_quantizer
from test_unfold_cpu import CASES as G30_CASES, GEOMETRIES, geometry_id, run_g30, same_as_recorded

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture()
def launches(monkeypatch):
    """{"unfold_quantize": number of calls} of the ops entry point."""
    counts = {"unfold_quantize": 0}
    real = ops.unfold_quantize

    def counted(*a, **k):
        counts["unfold_quantize"] += 1
        return real(*a, **k)

    monkeypatch.setattr(ops, "unfold_quantize", counted)
    return counts


@pytest.fixture()
def chain(monkeypatch):
    """A context in which the dispatcher has no unfold kernel of this package: the reference chain runs."""

    @contextlib.contextmanager
    def off():
        with monkeypatch.context() as m:
            kept = [it for it in dispatcher._DISPATCHER.get("unfold", []) if getattr(it.fn, "__self__", None) is not fused_unfold.KERNELS]
            m.setitem(dispatcher._DISPATCHER, "unfold", kept)
            yield

    return off


def bits(t):
    return t.contiguous().view(torch.int16)


def same_tensor(got, want, contiguous=True):
    assert type(got) is type(want) and got.shape == want.shape and got.dtype == want.dtype
    assert not contiguous or got.is_contiguous()
    assert torch.equal(bits(got), bits(want)), f"{int((bits(got) != bits(want)).sum())} of {got.numel()} elements differ"


def same_quantized(got, want):
    assert isinstance(got, ff.QuantizedTensor) and isinstance(want, ff.QuantizedTensor)
    assert got.raw_data.shape == want.raw_data.shape and got.raw_data.dtype == want.raw_data.dtype and got.raw_data.is_contiguous()
    assert torch.equal(got.raw_data, want.raw_data), f"{int((got.raw_data != want.raw_data).sum())} of {got.numel()} codes differ"
    assert torch.equal(bits(got.dequantize()), bits(want.dequantize()))


def compare(call, quantizers, chain):
    """`call(output_quantizer)` fused and through the chain: the value (None: not compared) and the codes of every output quantizer."""
    with torch.no_grad(), ff.strict_quantization(False):
        value = call(None) if None in quantizers else None
        coded = [call(q) for q in quantizers if q is not None]
        with chain():
            want = call(None) if None in quantizers else None
            want_coded = [call(q) for q in quantizers if q is not None]
    if want is not None:
        same_tensor(value, want)
    for got, exp in zip(coded, want_coded):
        same_quantized(got, exp)
    return value, coded


def out_quantizers(count=2):
    return [act_quantizer(lo, hi) for lo, hi in ((-6.0, 7.0), (-2.0, 9.0), (-9.0, 1.5))[:count]]


def operand(x, form, lo=-4.0, hi=5.0, bits_=8, channel=False):
    """`x` plain, or as codes of `bits_` in an int8 or value-dtype container, per tensor or per channel (dim 1; dim 0 unbatched)."""
    if form == "plain":
        return x
    container = torch.int8 if form == "int8" else x.dtype
    with torch.no_grad():
        if channel:
            axis = x.dim() - 3
            per = x.float().movedim(axis, 0).reshape(x.shape[axis], -1)
            return act_quantizer(per.amin(-1).clamp(max=-0.5), per.amax(-1).clamp(min=0.5), granularity=ff.PerChannel(axis), container=container, bits=bits_)(x)
        return act_quantizer(lo, hi, container=container, bits=bits_)(x)


def unfold(x, geometry, **k):
    _, kernel, dilation, padding, stride = geometry
    return F.unfold(x, kernel, dilation, padding, stride, **k)


# ---- 1. the chain's bits on every geometry, input form and granularity -----------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=[geometry_id(g) for g in GEOMETRIES])
def test_unfold_equals_the_chain(geometry, dtype, launches, chain):
    torch.manual_seed(sum(geometry[0]))
    x = (torch.randn(geometry[0], device=DEV) * 2).to(dtype)
    q = out_quantizers(1)[0]
    compare(lambda oq: unfold(x, geometry, output_quantizer=oq), [q], chain)                       # plain + quantizer
    for form in ("int8", "container"):
        for channel in (False, True):                                                            # per tensor, PerChannel(1)
            qx = operand(x, form, channel=channel)
            compare(lambda oq: unfold(qx, geometry, output_quantizer=oq), [None, q], chain)       # without and with an output quantizer
    assert launches["unfold_quantize"] == 1 + 2 * 2 * 2


# ---- 2. the padding, the sign of a zero, offsets beyond int8, the clamps ---------------------------------------------------------
# group form (L = 64; L = 256 with groups wholly in the padding left and right of the image, and shifts of up to 7 elements), element forms
PADDED = [((1, 2, 8, 8), 3, 1, 1, 1), ((1, 2, 8, 16), 3, 1, (1, 9), 1), ((1, 3, 4, 4), 1, 1, 2, 1), ((2, 3, 5, 7), (3, 2), (1, 2), (2, 1), (2, 1))]


def negative_zero(q):
    """`q` (value-dtype codes) with codes -0.0 under an offset that rounds to -0.0: A2 gives (-0.0 + -0.0) * s = -0.0."""
    codes = q.raw_data.clone()
    codes.view(-1)[::3] = -0.0
    return ff.QuantizedTensor(codes, q.quantization_context.with_changes(offset=torch.tensor([-0.25], device=DEV)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geometry", PADDED, ids=[geometry_id(g) for g in PADDED])
def test_padding_is_the_value_zero_and_zeros_keep_their_sign(geometry, dtype, launches, chain):
    torch.manual_seed(2)
    shape = geometry[0]
    x = (torch.randn(shape, device=DEV) * 2).to(dtype)
    x.view(-1)[::5] = -0.0
    q = act_quantizer(-6.0, 7.0)
    assert float(q.offset.detach()) != round(float(q.offset.detach()))                                             # asymmetric, and not an integer
    inside = torch.nn.functional.unfold(torch.ones(shape, device=DEV, dtype=dtype), *geometry[1:]) != 0   # where a window is in the image
    assert bool(inside.any()) and not bool(inside.all())
    with torch.no_grad():
        code_of_zero = q(torch.zeros(1, device=DEV, dtype=dtype)).raw_data
    assert int(code_of_zero) not in (0, -128, 127)
    # rne(offset) beyond int8: (40, 49) puts it near -1260
    far = operand(x, "container", 40.0, 49.0)
    assert abs(float(far.quantization_context.quantization_params.offset.detach())) > 1000
    for t in (x, negative_zero(operand(x, "container")), operand(x, "int8"), far):
        quantizers = [q] if t is x else [None, q]
        value, (coded,) = compare(lambda oq: unfold(t, geometry, output_quantizer=oq), quantizers, chain)
        assert bool((coded.raw_data[~inside] == code_of_zero).all())                             # A1(0.0), not code 0
        if value is not None:
            assert bool((bits(value)[~inside] == 0).all())                                       # +0.0
    with torch.no_grad(), ff.strict_quantization(False):
        for t in (operand(x, "int8", channel=True), negative_zero(operand(x, "container"))):
            value = unfold(t, geometry)
            assert bool((bits(value)[~inside] == 0).all())
        zeros = unfold(negative_zero(operand(x, "container")), geometry)
        assert bool(((zeros == 0) & torch.signbit(zeros) & inside).any())                         # the -0.0 of A2 keeps its sign
        plain = ops.unfold_quantize(x, *geometry[1:])[0]                                          # (a plain input without a quantizer: the ops level)
        same_tensor(plain, unfold(x, geometry))
        assert bool(((plain == 0) & torch.signbit(plain) & inside).any()) and bool((bits(plain)[~inside] == 0).all())
    assert launches["unfold_quantize"] == 1 + 3 * 2 + 3 + 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("num_bits,lo,hi", [(4, -8, 7), (8, -128, 127)])
def test_output_quantizers_of_4_and_8_bits_reach_both_clamps(num_bits, lo, hi, dtype, launches, chain):
    torch.manual_seed(3)
    geometry = ((2, 3, 8, 8), 3, 1, 1, 1)
    x = (torch.randn(geometry[0], device=DEV) * 2).to(dtype)
    q = act_quantizer(-1.0, 0.75, bits=num_bits)
    for t in (x, operand(x, "int8"), operand(x, "container", channel=True)):
        _, (coded,) = compare(lambda oq: unfold(t, geometry, output_quantizer=oq), [q], chain)
        assert int(coded.raw_data.min()) == lo and int(coded.raw_data.max()) == hi
    assert launches["unfold_quantize"] == 3


# ---- 3. two quantizers from one launch, no value ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geometry", [GEOMETRIES[1], GEOMETRIES[2], GEOMETRIES[14]], ids=[geometry_id(g) for g in (GEOMETRIES[1], GEOMETRIES[2], GEOMETRIES[14])])
def test_one_launch_feeds_two_quantizers_without_a_value(geometry, dtype, launches):
    torch.manual_seed(4)
    qx = operand((torch.randn(geometry[0], device=DEV) * 2).to(dtype), "int8", channel=True)
    q1, q2 = out_quantizers(2)
    k = fused_unfold.KERNELS
    with torch.no_grad():
        x, dequant = k._dequant(qx)
        args = dict(dtype=dtype, dequant=dequant, per_channel=True)
        value, both = ops.unfold_quantize(x, *geometry[1:], quantizers=[(q1.scale, q1.offset), (q2.scale, q2.offset)], want_value=False, **args)
        _, first = ops.unfold_quantize(x, *geometry[1:], quantizers=[(q1.scale, q1.offset)], want_value=False, **args)
        _, second = ops.unfold_quantize(x, *geometry[1:], quantizers=[(q2.scale, q2.offset)], want_value=False, **args)
        want = torch.nn.functional.unfold(qx.dequantize(), *geometry[1:])
    assert value is None and len(both) == 2 and both[0].is_contiguous() and both[0].shape == want.shape
    assert torch.equal(both[0], first[0]) and torch.equal(both[1], second[0])
    assert torch.equal(both[0], q1(want).raw_data) and torch.equal(both[1], q2(want).raw_data)
    assert launches["unfold_quantize"] == 3


# ---- 4. G30 on the device -----------------------------------------------------------------------------------------------------------
G30_BF16 = [c for c in G30_CASES if c["dtype"] == "torch.bfloat16"]


@pytest.mark.parametrize("index", range(len(G30_BF16)), ids=[c["name"] for c in G30_BF16])
def test_the_fixture_on_the_device(index, launches):
    case = G30_BF16[index]
    plain, quantized = run_g30(case, DEV)
    same_as_recorded(plain, case["plain"])
    same_as_recorded(quantized, case["quantized"])
    assert plain.is_cuda and quantized.is_cuda
    assert launches["unfold_quantize"] == (1 if case["slot"] is None else 2)  # (a plain input without a quantizer: ATen's im2col alone)


# ---- 5. views of the input -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", every(2, channels_last=True), ids=[layout.id for layout in every(2, channels_last=True)])
def test_views_of_the_input_equal_the_contiguous_call(layout, launches, chain):
    torch.manual_seed(5)
    geometry = ((2, 6, 5, 8), 3, 1, 1, (2, 1))
    x = (torch.randn(geometry[0], device=DEV) * 2).bfloat16()
    q = out_quantizers(1)[0]
    viewed = lambda t: ff.QuantizedTensor(layout.make(t.raw_data), t.quantization_context)  # noqa: E731  (the codes in the view)
    with torch.no_grad(), ff.strict_quantization(False):
        same_quantized(unfold(layout.make(x), geometry, output_quantizer=q), unfold(x, geometry, output_quantizer=q))
        for qx in (operand(x, "int8"), operand(x, "container", channel=True)):
            view = viewed(qx)
            same_tensor(unfold(view, geometry), unfold(qx, geometry))
            same_quantized(unfold(view, geometry, output_quantizer=q), unfold(qx, geometry, output_quantizer=q))
            compare(lambda oq: unfold(view, geometry, output_quantizer=oq), [None, q], chain)
    assert launches["unfold_quantize"] == 2 + 2 * 6


# ---- 6. declines ----------------------------------------------------------------------------------------------------------------------
def _declines(call, launches, chain):
    """`call(output_quantizer)` takes the chain: no launch, and the chain's result (or its error)."""
    q = out_quantizers(1)[0]
    with ff.strict_quantization(False):
        try:
            with chain():
                want = call(q)
        except Exception as e:  # noqa: BLE001  (what ATen refuses, it refuses on both routes)
            with pytest.raises(type(e)):
                call(q)
        else:
            got = call(q)
            same_quantized(got, want) if isinstance(want, ff.QuantizedTensor) else same_tensor(got, want, contiguous=False)
    assert launches["unfold_quantize"] == 0


def test_unfold_declines(launches, chain):
    torch.manual_seed(6)
    x = (torch.randn(2, 3, 5, 8, device=DEV) * 2).bfloat16()
    with torch.no_grad():
        _declines(lambda q: F.unfold(x.float(), 3, output_quantizer=q), launches, chain)                                      # fp32
        _declines(lambda q: F.unfold(x, 3, padding=1), launches, chain)                                                      # plain, no quantizer
        per_batch = act_quantizer(torch.tensor([-4.0, -3.0]), torch.tensor([5.0, 4.0]), granularity=ff.PerChannel(0))(x)
        _declines(lambda q: F.unfold(per_batch, 3, output_quantizer=q), launches, chain)                                     # PerChannel(0), batched
        _declines(lambda q: torch.nn.functional.unfold(operand(x, "int8"), 3), launches, chain)                              # not ff.nn.functional
        _declines(lambda q: F.unfold(operand(x, "int8"), 6, output_quantizer=q), launches, chain)                            # does not fit: ATen's error
        _declines(lambda q: F.unfold(operand(x, "int8"), 3, padding=1.0, output_quantizer=q), launches, chain)               # float geometry
    leaf = x.clone().requires_grad_()
    _declines(lambda q: F.unfold(leaf, 3, output_quantizer=q), launches, chain)                                               # a gradient is needed
    with ff.strict_quantization(False):
        F.unfold(leaf, 3).float().sum().backward()
    assert leaf.grad is not None and launches["unfold_quantize"] == 0
    with pytest.raises(RuntimeError), torch.no_grad(), ff.strict_quantization(False):                                         # the chain's error, as it words it
        F.unfold(operand(x, "int8"), 6, output_quantizer=out_quantizers(1)[0])


# ---- 7. guard bands ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", [GEOMETRIES[2], GEOMETRIES[3], ((2, 3, 9, 16), 3, 1, 1, 1), PADDED[1], GEOMETRIES[1], GEOMETRIES[5], GEOMETRIES[15]],
                         ids=["group-2-rows", "group-3-rows", "group-one-load", "group-wide-padding", "element", "element-L9", "element-L1"])
def test_guard_bands_around_the_value_and_the_codes(geometry, launches):
    """`out` and both code buffers are carved from an arena (tests/guards.py) whose guards and fresh bodies hold a poison byte; two
    runs with two poisons: every guard keeps its poison (no stray write), and the runs agree with each other and with an unguarded
    run on every output byte (none left unwritten)."""
    g = torch.Generator().manual_seed(7)
    shape = geometry[0]
    x = torch.randint(-128, 128, shape, generator=g, dtype=torch.int8).to(DEV)
    xs, xo = (torch.rand(shape[1], generator=g) * 0.05 + 0.01).to(DEV), torch.full((shape[1],), 2.5, device=DEV)
    pairs = [(q.scale.detach(), q.offset.detach()) for q in out_quantizers(2)]

    def run():
        return ops.unfold_quantize(x, *geometry[1:], quantizers=pairs, dtype=torch.bfloat16, dequant=(xs, xo), per_channel=True)

    results = []
    for poison in (guards.POISON_A, guards.POISON_B):
        arena = guards.Arena(poison)
        with guards.capture(arena):
            value, codes = run()
        torch.cuda.synchronize()
        assert all(arena.find(t.data_ptr()) is not None for t in (value, *codes)), "the outputs were not allocated inside the arena"
        assert not arena.touched_guards(), arena.touched_guards()
        results.append([t.clone() for t in (value, *codes)])
    value, codes = run()
    for a, b, plain in zip(results[0], results[1], (value, *codes)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)) and torch.equal(a.view(torch.uint8), plain.view(torch.uint8))
    assert launches["unfold_quantize"] == 3


# ---- 8. im2col + GEMM, captured ------------------------------------------------------------------------------------------------------------
def test_im2col_and_gemm_is_an_exact_convolution_and_replays(launches):
    """Per-tensor codes with unit scales and no offset: unfold under an 8-bit quantizer with the same parameters (a symmetric
    quantizer, whose offset buffer holds zero) returns the input's codes in place and code 0 in the padding, and the matmul of
    [OC, C * taps] weight codes with it is the float64 conv2d of the codes. Codes in [-16, 15] and 16 weights of +-1 per row keep
    every sum within +-256, which bf16 holds exactly."""
    g = torch.Generator().manual_seed(8)
    B, C, H, W, OC, k = 2, 16, 6, 6, 8, 3
    one = torch.tensor([1.0], device=DEV)
    codes = torch.randint(-16, 16, (B, C, H, W), generator=g)
    weight = torch.zeros(OC, C * k * k)
    for row in weight:
        at = torch.randperm(C * k * k, generator=g)[:16]
        row[at] = torch.randint(0, 2, (16,), generator=g).float() * 2 - 1
    xq = ff.quantization.affine.quantize_per_tensor(codes.to(DEV, torch.bfloat16), one, None, 8, output_dtype=torch.int8)
    wq = ff.quantization.affine.quantize_per_tensor(weight.to(DEV, torch.bfloat16), one, None, 8, output_dtype=torch.int8)
    assert xq.quantization_context.quantization_params.offset is None and torch.equal(xq.raw_data.cpu(), codes.to(torch.int8))
    oq = ff.nn.LinearQuantizer(8, symmetric=True, quantized_dtype=torch.int8, device=DEV)
    oq.quantization_range = (torch.tensor(-128.0, device=DEV), torch.tensor(127.0, device=DEV))
    with torch.no_grad():
        oq.scale.fill_(1.0)

    def step():
        with torch.no_grad(), ff.strict_quantization(False):
            cols = F.unfold(xq, k, padding=1, output_quantizer=oq)
            return cols, F.matmul(wq, cols)

    def check(cols, y, codes):
        assert isinstance(cols, ff.QuantizedTensor) and cols.raw_data.dtype == torch.int8
        want_cols = torch.nn.functional.unfold(codes.double(), k, padding=1)                       # the codes in place, code 0 in the padding
        assert torch.equal(cols.raw_data.cpu().double(), want_cols)
        exact = torch.nn.functional.conv2d(codes.double(), weight.double().reshape(OC, C, k, k), padding=1).reshape(B, OC, H * W)
        assert float(exact.abs().max()) <= 256
        y = y.dequantize() if isinstance(y, ff.QuantizedTensor) else y
        assert torch.equal(y.cpu().double(), exact)

    cols, y = step()  # (the first call outside the capture)
    check(cols, y, codes)
    assert launches["unfold_quantize"] == 1
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
        cols_g, y_g = step()
    torch.cuda.current_stream().wait_stream(side)
    fresh = codes.flip(0).roll(1, -1)  # fresh contents in the captured input
    xq.raw_data.copy_(fresh.to(torch.int8))
    cols, y = step()
    check(cols, y, fresh)
    eager_cols, eager_y = cols.raw_data.clone(), (y.dequantize() if isinstance(y, ff.QuantizedTensor) else y).clone()
    for _ in range(2):
        cols_g.raw_data.zero_()
        graph.replay()
        torch.cuda.synchronize()
        replayed = y_g.dequantize() if isinstance(y_g, ff.QuantizedTensor) else y_g
        assert torch.equal(cols_g.raw_data, eager_cols) and torch.equal(bits(replayed), bits(eager_y)) and bool(eager_cols.any())
    assert launches["unfold_quantize"] == 3
