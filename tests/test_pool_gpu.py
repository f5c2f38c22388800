"""The one-pass avg_pool1d / avg_pool2d / max_pool2d and nearest interpolate kernels (csrc/ffq_pool.hip) on the MI355X, against the
device reference chain — dequantize the input, the ATen op, the output quantizer — that the generated fallbacks run (reference
_gen/fallback.py), with this package's registrations taken out of the dispatcher.

Every operator: the value is bit for bit the chain's (max and nearest are selections; the average keeps ATen's one fp32 accumulator,
its rows-outer / columns-inner order, its one division by the window's size and its one rounding), NaN exactly where ATen has NaN,
and the codes are the output quantizer applied to that value. Every test counts the calls of the two ``ops`` entry points, so a
silent fallback fails it."""

import contextlib
import random

import pytest
import torch

import fastforward_amd as ff

from fastforward_amd import dispatcher, fused_pool, ops
from fastforward_amd.nn import functional as F
from layouts import Layout, every
from test_elementwise_gpu import compare_with_chain, operand
from test_modules_gpu import act_quantizer

pytestmark = pytest.mark.gpu
DEV = "cuda"
OPS = ("pool2d_quantize", "upsample_nearest_quantize")
NAMES = ("avg_pool1d", "avg_pool2d", "max_pool2d", "interpolate")
POOL_FORMS = ("plain", "int8_tensor", "container_tensor", "int8_channel", "container_channel")
DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture()
def launches(monkeypatch):
    """{op name: number of calls} of the two ops entry points."""
    counts = {name: 0 for name in OPS}
    for name in OPS:
        real = getattr(ops, name)

        def counted(*a, _real=real, _name=name, **k):
            counts[_name] += 1
            return _real(*a, **k)

        monkeypatch.setattr(ops, name, counted)
    return counts


@pytest.fixture()
def chain(monkeypatch):
    """A context in which the dispatcher has none of this package's pool kernels: the reference chain runs."""

    @contextlib.contextmanager
    def off():
        with monkeypatch.context() as m:
            for op in NAMES:
                kept = [it for it in dispatcher._DISPATCHER.get(op, []) if getattr(it.fn, "__self__", None) is not fused_pool.KERNELS]
                m.setitem(dispatcher._DISPATCHER, op, kept)
            yield

    return off


def pool_operand(x, form):
    """`x` [B, C, ...] plain, or as codes with per-tensor or per-channel parameters in an int8 or value-dtype container."""
    if not form.endswith("_channel"):
        return operand(x, form)
    per = x.float().transpose(0, 1).reshape(x.shape[1], -1)
    lo, hi = per.amin(-1).clamp(max=-0.5), per.amax(-1).clamp(min=0.5)
    container = torch.int8 if form.startswith("int8") else x.dtype
    return act_quantizer(lo, hi, granularity=ff.PerChannel(1), container=container)(x)


def quantizers(count):
    """One to three output quantizers with their own ranges (each its own launch of the public operator)."""
    return [act_quantizer(lo, hi) for lo, hi in ((-3.0, 3.5), (-1.0, 6.0), (-5.0, 0.5))[:count]]


# ---- the named cases ------------------------------------------------------------------------------------------------------------------
CASES = [
    ("avg_pool2d", (4, 6, 14, 14), dict(kernel_size=2, stride=2)),
    ("avg_pool2d", (4, 6, 14, 14), dict(kernel_size=3, stride=2, padding=1)),
    ("avg_pool2d", (4, 6, 14, 14), dict(kernel_size=3, stride=2, padding=1, count_include_pad=False)),
    ("avg_pool2d", (3, 5, 13, 11), dict(kernel_size=2, stride=2, ceil_mode=True)),
    ("avg_pool2d", (3, 5, 13, 11), dict(kernel_size=(3, 2), stride=(2, 1), padding=(1, 0))),
    ("avg_pool2d", (8, 64, 7, 7), dict(kernel_size=7, stride=7)),
    ("avg_pool1d", (4, 6, 64), dict(kernel_size=4, stride=4)),
    ("avg_pool1d", (4, 6, 61), dict(kernel_size=3, stride=1, padding=1)),
    ("max_pool2d", (4, 6, 28, 28), dict(kernel_size=3, stride=2, padding=1)),
    ("max_pool2d", (4, 6, 14, 14), dict(kernel_size=2)),
    ("max_pool2d", (3, 5, 13, 11), dict(kernel_size=3, stride=1, padding=1, dilation=2)),
    ("max_pool2d", (3, 5, 13, 11), dict(kernel_size=3, stride=2, ceil_mode=True)),
    ("interpolate", (4, 6, 10, 10), dict(scale_factor=2)),
    ("interpolate", (3, 5, 13, 11), dict(scale_factor=1.5)),
    ("interpolate", (4, 6, 10, 10), dict(size=(13, 9))),
    ("interpolate", (3, 5, 13, 11), dict(scale_factor=(1.7, 0.6), mode="nearest-exact")),
    ("interpolate", (3, 5, 13, 11), dict(size=(7, 29), mode="nearest-exact")),
    ("interpolate", (4, 6, 61), dict(scale_factor=2.5)),
    ("interpolate", (4, 6, 61), dict(size=17)),
]


def entry(name):
    return "upsample_nearest_quantize" if name == "interpolate" else "pool2d_quantize"


@pytest.mark.parametrize("case", range(len(CASES)), ids=[f"{n}-{'x'.join(map(str, s))}-{i}" for i, (n, s, _) in enumerate(CASES)])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", POOL_FORMS)
def test_equals_the_reference_chain(case, dtype, form, launches, chain):
    name, shape, kwargs = CASES[case]
    torch.manual_seed(40 + case)
    x = (torch.randn(shape, device=DEV) * 2).to(dtype)
    compare_with_chain(getattr(F, name), (pool_operand(x, form),), kwargs, act_quantizer(-3.0, 3.5), chain)
    assert launches[entry(name)] == 2 and sum(launches.values()) == 2


# ---- a seeded sweep of the geometry: every draw is valid by construction, so none is skipped -------------------------------------------
def draw(rng, name):
    """(shape, kwargs) of one call of `name` ATen accepts: padding <= kernel // 2, the map at least the dilated kernel less the padding."""
    n = 1 if name == "avg_pool1d" else 2
    k = [rng.randint(1, 7) for _ in range(n)]
    s = [rng.randint(1, 4) for _ in range(n)]
    p = [rng.randint(0, ki // 2) for ki in k]
    d = [rng.randint(1, 3) if name == "max_pool2d" else 1 for _ in range(n)]
    sizes = [rng.randint(max(1, di * (ki - 1) + 1 - 2 * pi), 57) for ki, pi, di in zip(k, p, d)]
    shape = (rng.randint(1, 3), rng.randint(1, 5), *sizes)
    one = lambda v: v[0] if n == 1 or (v[0] == v[1] and rng.random() < 0.5) else tuple(v)  # noqa: E731  an int or a tuple
    kwargs = dict(kernel_size=one(k), stride=one(s), padding=one(p), ceil_mode=rng.random() < 0.5)
    if name == "max_pool2d":
        kwargs["dilation"] = one(d)
        if rng.random() < 0.2:
            kwargs["stride"] = None
    else:
        kwargs["count_include_pad"] = rng.random() < 0.5
    return shape, kwargs


def draw_interpolate(rng):
    n = rng.choice((1, 2))
    shape = (rng.randint(1, 3), rng.randint(1, 5), *[rng.randint(1, 57) for _ in range(n)])
    mode = rng.choice(("nearest", "nearest-exact"))
    while True:
        if rng.random() < 0.5:
            size = tuple(rng.randint(1, 90) for _ in range(n))
            kwargs = dict(size=size if n == 2 or rng.random() < 0.5 else size[0], mode=mode)
            out = size
        else:
            factors = tuple(rng.choice((2, 3, 0.5, 1.5, 2.5)) if rng.random() < 0.5 else round(rng.uniform(0.3, 3.2), 3) for _ in range(n))
            kwargs = dict(scale_factor=factors if n == 2 and rng.random() < 0.7 else factors[0], mode=mode)
            used = factors if isinstance(kwargs["scale_factor"], tuple) else (factors[0],) * n
            out = tuple(int(extent * float(f)) for extent, f in zip(shape[2:], used))
        if min(out) >= 1 and out != shape[2:]:  # (an output of the input's size is ATen's copy: the predicate declines it)
            return shape, kwargs


@pytest.mark.parametrize("name", NAMES)
def test_seeded_geometry_sweep(name, launches, chain):
    rng = random.Random(f"pool-{name}")
    draws, ran = 72, 0
    for i in range(draws):
        shape, kwargs = draw_interpolate(rng) if name == "interpolate" else draw(rng, name)
        dtype, form, count = DTYPES[i % 2], POOL_FORMS[i % len(POOL_FORMS)], 1 + i % 3
        torch.manual_seed(1000 + i)
        x = pool_operand((torch.randn(shape, device=DEV) * 2).to(dtype), form)
        for oq in quantizers(count):
            compare_with_chain(getattr(F, name), (x,), kwargs, oq, chain)
        ran += 1
    assert ran == draws
    assert launches[entry(name)] == 2 * sum(1 + i % 3 for i in range(draws))


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_launch_feeds_three_output_quantizers(dtype, launches):
    torch.manual_seed(41)
    x = (torch.randn(3, 5, 13, 11, device=DEV) * 2).to(dtype)
    qs = quantizers(3)
    pairs = [(q.scale, q.offset) for q in qs]
    with torch.no_grad():
        value, codes = ops.pool2d_quantize("avg", x, (3, 3), (2, 2), (1, 1), quantizers=pairs)
        up, up_codes = ops.upsample_nearest_quantize(x, (20, 17), None, quantizers=pairs)
        assert torch.equal(value, torch.nn.functional.avg_pool2d(x, 3, 2, 1)) and torch.equal(up, torch.nn.functional.interpolate(x, size=(20, 17)))
        for q, c, u in zip(qs, codes, up_codes):
            assert torch.equal(c, q(value).raw_data) and torch.equal(u, q(up).raw_data)
    assert launches == {"pool2d_quantize": 1, "upsample_nearest_quantize": 1}


@pytest.mark.parametrize("form", ["plain", "int8_channel"])
def test_eight_outputs_per_lane_with_a_tail(form, launches, chain):
    """More than 2^20 outputs take the kernels' 8-outputs-per-lane form; a result whose size is no multiple of 8 ends in a partial group."""
    torch.manual_seed(50)
    x = pool_operand((torch.randn(1, 33, 181, 179, device=DEV) * 2).to(torch.bfloat16), form)
    calls = [("max_pool2d", dict(kernel_size=1)), ("avg_pool2d", dict(kernel_size=3, stride=1, padding=1)), ("interpolate", dict(size=(180, 181)))]
    for name, kwargs in calls:
        value = compare_with_chain(getattr(F, name), (x,), kwargs, act_quantizer(-3.0, 3.5), chain)
        assert value.numel() >= 2**20 and value.numel() % 8
    assert sum(launches.values()) == 2 * len(calls)


# ---- specials ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,kwargs", [("max_pool2d", dict(kernel_size=3, stride=2, padding=1)), ("max_pool2d", dict(kernel_size=2, stride=1, dilation=2)),
                                         ("avg_pool2d", dict(kernel_size=3, stride=2, padding=1)), ("interpolate", dict(scale_factor=1.5))])
def test_nan_inf_and_signed_zero_planes(dtype, name, kwargs, launches, chain):
    torch.manual_seed(42)
    x = (torch.randn(2, 8, 9, 11, device=DEV) * 2).to(dtype)
    x[0, 0], x[0, 1], x[0, 2], x[0, 3], x[0, 4] = float("nan"), float("inf"), float("-inf"), -0.0, 0.0
    x[1, 0, 4, 5], x[1, 1, 0, 0], x[1, 2, 8, 10], x[1, 3, 2, 2], x[1, 4, ::2, ::2] = float("nan"), float("inf"), float("-inf"), -0.0, -0.0
    # a window whose only finite values sit next to the padding: the rest of the plane is -inf
    x[1, 5] = float("-inf")
    x[1, 5, 0, :], x[1, 5, :, 0] = 1.5, -2.5
    value = compare_with_chain(getattr(F, name), (x,), kwargs, act_quantizer(-3.0, 3.5), chain)
    assert torch.isnan(value[0, 0]).all()
    assert launches[entry(name)] == 2


@pytest.mark.parametrize("dtype", DTYPES)
def test_negative_zero_codes_under_an_offset_that_rounds_to_negative_zero(dtype, launches, chain):
    """A float container holds -0.0 codes, and an offset in (-0.5, 0] rounds to -0.0: A2 gives (-0.0 + -0.0) * s = -0.0, which a
    multiply fused with the fp16 conversion loses (hipcc's v_fma_mixlo_f16 adds +0)."""
    torch.manual_seed(49)
    q = pool_operand((torch.randn(2, 4, 9, 11, device=DEV) * 2).to(dtype), "container_tensor")
    codes = q.raw_data.clone()
    codes[..., ::3] = -0.0
    codes[0, 0] = -0.0
    moved = ff.QuantizedTensor(codes, q.quantization_context.with_changes(offset=torch.tensor([-0.25], device=DEV)))
    calls = [("max_pool2d", dict(kernel_size=1)), ("max_pool2d", dict(kernel_size=3, stride=2, padding=1)), ("avg_pool2d", dict(kernel_size=2, stride=2)),
             ("interpolate", dict(scale_factor=1.5)), ("interpolate", dict(size=(5, 7), mode="nearest-exact"))]
    for name, kwargs in calls:
        value = compare_with_chain(getattr(F, name), (moved,), kwargs, act_quantizer(-3.0, 3.5), chain)
        if name != "avg_pool2d":
            assert bool(((value == 0) & torch.signbit(value)).any())
    assert sum(launches.values()) == 2 * len(calls)


@pytest.mark.parametrize("form", ["int8_tensor", "container_tensor", "int8_channel"])
def test_max_over_codes_whose_values_round_alike(form, launches, chain):
    """Neighbouring codes dequantize to one bf16 value when the offset is large: the selection on the codes gives the chain's value.
    A negative scale turns the order round, a NaN scale gives NaN: both compare the dequantized values, as the chain does."""
    torch.manual_seed(43)
    x = (torch.randn(2, 4, 15, 15, device=DEV) * 0.05 + 3.0).to(torch.bfloat16)  # codes near 255 * 3 / 3.2 above the offset -128 - ...
    compare_with_chain(F.max_pool2d, (pool_operand(x, form),), dict(kernel_size=3, stride=2, padding=1), act_quantizer(0.0, 4.0), chain)
    q = operand((torch.randn(2, 4, 15, 15, device=DEV) * 2).to(torch.bfloat16), "int8_tensor")
    for scale in (-0.03, float("nan"), 0.0, float("inf"), 1e-30):
        moved = ff.QuantizedTensor(q.raw_data, q.quantization_context.with_changes(scale=torch.tensor([scale], device=DEV)))
        compare_with_chain(F.max_pool2d, (moved,), dict(kernel_size=3, stride=2, padding=1), act_quantizer(-4.0, 4.0), chain)
    assert launches["pool2d_quantize"] == 12


# ---- layouts: offset, strided and misaligned views reach the kernels as aligned copies; channels-last is ATen's ----------------------
CALLS = {"avg_pool2d": lambda v, oq: F.avg_pool2d(v, 3, 2, 1, output_quantizer=oq), "max_pool2d": lambda v, oq: F.max_pool2d(v, 3, 2, 1, output_quantizer=oq),
         "interpolate": lambda v, oq: F.interpolate(v, scale_factor=1.5, output_quantizer=oq)}


@pytest.mark.parametrize("layout", every(2), ids=[layout.id for layout in every(2)])
@pytest.mark.parametrize("name", list(CALLS))
def test_views(name, layout, launches):
    torch.manual_seed(44)
    view = layout.make(torch.randn(3, 4, 9, 14, device=DEV).to(torch.bfloat16))
    oq = act_quantizer(-4.0, 4.0)
    with torch.no_grad(), ff.strict_quantization(False):
        got, want = CALLS[name](view, oq), CALLS[name](view.clone(memory_format=torch.contiguous_format), oq)
    assert torch.equal(got.raw_data, want.raw_data) and got.raw_data.is_contiguous()
    assert sum(launches.values()) == 2


@pytest.mark.parametrize("layout", [Layout("channels_last", 0), Layout("channels_last", 2)], ids=lambda layout: layout.id)
@pytest.mark.parametrize("name", list(CALLS))
def test_channels_last_input_keeps_atens_strides(name, layout, launches, chain):
    torch.manual_seed(45)
    view = layout.make(torch.randn(3, 4, 9, 14, device=DEV).to(torch.bfloat16))
    with torch.no_grad(), ff.strict_quantization(False):
        got = CALLS[name](view, None)
        with chain():
            want = CALLS[name](view, None)
    assert torch.equal(got, want) and got.stride() == want.stride() and got.is_contiguous(memory_format=torch.channels_last)
    assert launches == {name: 0 for name in OPS}


# ---- the predicate declines: the reference chain runs, unchanged -------------------------------------------------------------------
def test_fallbacks_when_the_predicate_declines(launches, chain):
    torch.manual_seed(46)
    x = (torch.randn(2, 4, 12, 12, device=DEV) * 2).to(torch.bfloat16)
    qx = operand(x, "int8_tensor")
    oq = act_quantizer(-3.0, 3.0)
    with torch.no_grad():
        assert not fused_pool.max_pool2d_predicate(input=qx, kernel_size=2, output_quantizer=oq)  # no strict_quantization keyword
        assert fused_pool.max_pool2d_predicate(input=qx, kernel_size=2, output_quantizer=oq, strict_quantization=False)
    declined = [
        (F.max_pool2d, (x[0], 2), {}),                                           # unbatched
        (F.avg_pool2d, (x[0], 2, 2), {}),
        (F.avg_pool1d, (x[0, 0], 2, 2), {}),
        (F.interpolate, (qx,), dict(scale_factor=2, mode="bilinear")),           # another mode
        (F.interpolate, (qx,), dict(scale_factor=2, mode="bilinear", antialias=True)),
        (F.interpolate, (qx,), dict(scale_factor=1.5, recompute_scale_factor=True)),
        (F.interpolate, (qx,), dict(size=(12, 12))),                             # the input's size: ATen copies
        (F.avg_pool2d, (x.float(), 2, 2), {}),                                   # fp32 values
        (F.max_pool2d, (operand(x, "int8_row"), 2), {}),                         # parameters per row of the last dim
    ]
    for fn, args, kwargs in declined:
        with torch.no_grad(), ff.strict_quantization(False):
            got = fn(*args, **kwargs, output_quantizer=oq)
            with chain():
                want = fn(*args, **kwargs, output_quantizer=oq)
        assert torch.equal(got.raw_data, want.raw_data), fn
    # geometry ATen refuses raises ATen's error
    for fn, args, kwargs in ((F.max_pool2d, (qx, 2), dict(padding=2)), (F.avg_pool2d, (qx, 3, 2), dict(padding=2)), (F.max_pool2d, (qx, 7), dict(dilation=3))):
        with pytest.raises(RuntimeError) as got, ff.strict_quantization(False):
            fn(*args, **kwargs)
        with pytest.raises(RuntimeError) as want, ff.strict_quantization(False):
            getattr(torch.nn.functional, fn.__name__)(qx.dequantize(), *args[1:], **kwargs)
        assert str(got.value) == str(want.value)
    xg = x.clone().requires_grad_()  # grad mode with an operand that needs a gradient
    for fn, args in ((F.max_pool2d, (xg, 2)), (F.avg_pool2d, (xg, 2, 2)), (F.interpolate, (xg, None, 2))):
        with ff.strict_quantization(False):
            got = fn(*args, output_quantizer=oq)
            with chain():
                want = fn(*args, output_quantizer=oq)
        assert torch.equal(got.raw_data, want.raw_data)
    assert F.max_pool2d(x.cpu(), 2, strict_quantization=False).device.type == "cpu"  # not on the device
    assert launches == {name: 0 for name in OPS}


# ---- hipGraph -----------------------------------------------------------------------------------------------------------------------
GRAPHED = {
    "max_pool2d": ((4, 8, 28, 28), "int8_tensor", lambda q, oq: F.max_pool2d(q, 3, 2, 1, output_quantizer=oq)),
    "avg_pool2d": ((4, 8, 28, 28), "int8_channel", lambda q, oq: F.avg_pool2d(q, 2, 2, output_quantizer=oq)),
    "avg_pool1d": ((4, 8, 250), "int8_tensor", lambda q, oq: F.avg_pool1d(q, 4, 4, output_quantizer=oq)),
    "interpolate": ((4, 8, 28, 28), "int8_channel", lambda q, oq: F.interpolate(q, scale_factor=2, output_quantizer=oq)),
}


@pytest.mark.parametrize("name", list(GRAPHED))
def test_fused_pool_calls_capture_and_replay(name, launches):
    """One capture per operator, replayed on fresh input contents: the launches read nothing on the host."""
    torch.manual_seed(47)
    shape, form, call = GRAPHED[name]
    x = (torch.randn(shape, device=DEV) * 2).to(torch.bfloat16)
    q, oq = pool_operand(x, form), act_quantizer(-3.0, 3.0)

    def step():
        with torch.no_grad(), ff.strict_quantization(False):
            return call(q, oq)

    step()  # (the first call outside the capture)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side), torch.cuda.graph(g, stream=side):
        out = step()
    torch.cuda.current_stream().wait_stream(side)
    q.raw_data.copy_(q.raw_data.flip(-1).neg().clamp(max=127))  # fresh contents in the captured input
    eager = step().raw_data.clone()
    out.raw_data.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.raw_data, eager) and bool(eager.any())
    assert launches[entry(name)] == 3 and sum(launches.values()) == 3


# ---- full size (the timing table's shapes) ----------------------------------------------------------------------------------------
FULL = [("max_pool2d", (64, 64, 112, 112), dict(kernel_size=3, stride=2, padding=1)), ("avg_pool2d", (64, 128, 56, 56), dict(kernel_size=2, stride=2)),
        ("avg_pool2d", (64, 2048, 7, 7), dict(kernel_size=7, stride=7)), ("avg_pool1d", (64, 512, 4096), dict(kernel_size=4, stride=4)),
        ("interpolate", (64, 256, 40, 40), dict(scale_factor=2))]


@pytest.mark.parametrize("name,shape,kwargs", FULL, ids=[f"{n}-{'x'.join(map(str, s))}" for n, s, _ in FULL])
def test_full_size_shapes(name, shape, kwargs, launches, chain):
    torch.manual_seed(48)
    x = (torch.randn(shape, device=DEV) * 2).to(torch.bfloat16)
    oq = act_quantizer(-4.0, 4.0)
    for arg in (x, act_quantizer(-4.0, 5.0)(x)):  # bf16 -> int8 and int8 -> int8
        with torch.no_grad(), ff.strict_quantization(False):
            got = getattr(F, name)(arg, **kwargs, output_quantizer=oq).raw_data
            with chain():
                want = getattr(F, name)(arg, **kwargs, output_quantizer=oq).raw_data
        assert torch.equal(got, want)
        del got, want
    assert launches[entry(name)] == 2
