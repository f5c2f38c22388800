"""The one-pass cat and pad kernels (csrc/ffq_concat.hip) on the MI355X, against the device reference chain — dequantize every
quantized input, ``torch.cat`` / ``F.pad``, the output quantizer — that the generated fallbacks run (reference _gen/fallback.py),
with this package's registrations for ``cat`` / ``pad`` taken out of the dispatcher.

Both operators only move data, so nothing is tolerated: the value's bits, shape, dtype and strides and the codes under a fused
output quantizer equal the chain's. Every test counts the calls of the two ``ops`` entry points, so a silent fallback fails it."""

import contextlib
import random

import pytest
import torch

import fastforward_amd as ff

from conftest import golden
from fastforward_amd import dispatcher, fused_concat, ops
from fastforward_amd.nn import functional as F
from fastforward_amd.quantization import _linear_quantized_ops as code_level
from layouts import every
from test_modules_gpu import act_quantizer

pytestmark = pytest.mark.gpu
DEV = "cuda"
OPS = ("cat_quantize", "pad_quantize")
DTYPES = [torch.bfloat16, torch.float16]
FORMS = ("plain", "int8", "container")
FILLS = (None, 0, -1.5, 65504, 1.00390625 + 2**-30, float("inf"), float("nan"))


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
    """A context in which the dispatcher has none of this package's fused cat / pad kernels: the reference chain runs (the
    concatenation of codes is the reference's own registration and stays)."""

    @contextlib.contextmanager
    def off():
        with monkeypatch.context() as m:
            for op in ("cat", "pad"):
                kept = [it for it in dispatcher._DISPATCHER.get(op, []) if getattr(it.fn, "__self__", None) is not fused_concat.KERNELS]
                m.setitem(dispatcher._DISPATCHER, op, kept)
            yield

    return off


def bits(t):
    return t.contiguous().view(torch.int16)


def same_tensor(got, want):
    assert type(got) is type(want) and got.shape == want.shape and got.dtype == want.dtype and got.stride() == want.stride()
    assert torch.equal(bits(got), bits(want)), f"{int((bits(got) != bits(want)).sum())} of {got.numel()} elements differ"


def same_quantized(got, want):
    assert isinstance(got, ff.QuantizedTensor) and isinstance(want, ff.QuantizedTensor)
    assert got.raw_data.shape == want.raw_data.shape and got.raw_data.dtype == want.raw_data.dtype and got.raw_data.stride() == want.raw_data.stride()
    assert torch.equal(got.raw_data, want.raw_data), f"{int((got.raw_data != want.raw_data).sum())} of {got.numel()} codes differ"
    assert torch.equal(bits(got.dequantize()), bits(want.dequantize()))


def compare(call, quantizers, chain):
    """`call(output_quantizer)` fused and through the chain: the value, and the codes of every output quantizer."""
    with torch.no_grad(), ff.strict_quantization(False):
        value = call(None)
        coded = [call(q) for q in quantizers]
        with chain():
            want = call(None)
            want_coded = [call(q) for q in quantizers]
    (same_quantized if isinstance(want, ff.QuantizedTensor) else same_tensor)(value, want)
    for got, exp in zip(coded, want_coded):
        same_quantized(got, exp)
    return value


def quantizers(count):
    return [act_quantizer(lo, hi) for lo, hi in ((-3.0, 3.5), (-1.0, 6.0), (-5.0, 0.5))[:count]]


def operand(x, form, lo=-4.0, hi=5.0, num_bits=8, channel=False):
    """`x` plain, or as codes of `num_bits` in an int8 or value-dtype container, per tensor or per channel (dim 1)."""
    if form == "plain":
        return x
    container = torch.int8 if form == "int8" else x.dtype
    if channel:
        per = x.float().transpose(0, 1).reshape(x.shape[1], -1)
        return act_quantizer(per.amin(-1).clamp(max=-0.5), per.amax(-1).clamp(min=0.5), granularity=ff.PerChannel(1), container=container, bits=num_bits)(x)
    return act_quantizer(lo, hi, container=container, bits=num_bits)(x)


def negative_zero(q):
    """`q` (value-dtype codes) with codes -0.0 under an offset that rounds to -0.0: A2 gives (-0.0 + -0.0) * s = -0.0."""
    codes = q.raw_data.clone()
    codes.view(-1)[::3] = -0.0
    return ff.QuantizedTensor(codes, q.quantization_context.with_changes(offset=torch.tensor([-0.25], device=DEV)))


# ---- 1. fused == chain: the fixture's shapes ---------------------------------------------------------------------------------------
G25 = [c for c in golden("g25_cat_pad.pt") if c["dtype"] == "torch.bfloat16"]


def device_quantizer(spec):
    num_bits, symmetric, gran, lo, hi = spec
    granularity = ff.PerTensor() if gran == "tensor" else ff.PerChannel(gran[1])
    q = ff.nn.LinearQuantizer(num_bits, symmetric=symmetric, granularity=granularity, quantized_dtype=torch.int8, device=DEV)
    q.quantization_range = (torch.as_tensor(lo, dtype=torch.float32, device=DEV), torch.as_tensor(hi, dtype=torch.float32, device=DEV))
    return q


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("index", range(len(G25)), ids=[c["name"] for c in G25])
def test_the_fixture_shapes_equal_the_reference_chain(index, dtype, launches, chain):
    case = G25[index]
    shared = device_quantizer(case["slots"][0]) if case["share"] else None
    with torch.no_grad():
        args = []
        for x, slot in zip(case["inputs"], case["slots"]):
            q = shared if case["share"] else (None if slot is None else device_quantizer(slot))
            x = x.to(DEV, dtype)
            args.append(x if q is None else q(x))
    kwargs = case["kwargs"]
    oq = device_quantizer(case["out_slot"])
    same_parameters = "same parameters" in case["name"]
    if case["through_torch"]:
        with torch.no_grad(), ff.strict_quantization(False):
            got = torch.cat(args, **kwargs)
        assert isinstance(got, ff.QuantizedTensor) and torch.equal(got.raw_data, torch.cat([a.raw_data for a in args], **kwargs))
        assert sum(launches.values()) == 0
        return
    call = (lambda q: F.cat(args, **kwargs, output_quantizer=q)) if case["op"] == "cat" else (lambda q: F.pad(args[0], **kwargs, output_quantizer=q))
    if same_parameters:  # without an output quantizer the codes are concatenated: the reference's kernel, here and in the "chain"
        with torch.no_grad(), ff.strict_quantization(False):
            kept = call(None)
            got = call(oq)
            with chain():
                want = call(oq)
        assert isinstance(kept, ff.QuantizedTensor) and torch.equal(kept.raw_data, torch.cat([a.raw_data for a in args], **kwargs))
        same_quantized(got, want)
        assert launches["cat_quantize"] == 1
        return
    compare(call, [oq], chain)
    # (per-channel parameters under a pad that reaches the channel dimension are the chain's)
    declined = case["op"] == "pad" and "per-channel" in case["name"] and args[0].dim() - len(kwargs["pad"]) // 2 < 2
    assert launches[f"{case['op']}_quantize"] == (0 if declined else 2) and sum(launches.values()) == (0 if declined else 2)


# ---- 1. fused == chain: seeded sweeps -------------------------------------------------------------------------------------------------
def draw_cat(rng, i):
    rank = 1 + i % 5
    dim = rng.randrange(rank)
    count = 1 + (i * 7) % 20
    shape = [rng.randint(1, 4) for _ in range(rank)]
    if rank > 1 and dim != rank - 1 and rng.random() < 0.6:
        shape[-1] = rng.choice((8, 16, 24))  # rows of a multiple of 8 ...
    extents = [rng.choice((8, 16)) if dim == rank - 1 and shape[-1] % 8 == 0 and rng.random() < 0.5 else rng.randint(1, 9) for _ in range(count)]
    if i % 4 == 0:  # ... and whole launches of them: the 8-elements-per-lane form
        shape[-1] = 8
        extents = [rng.choice((1, 2, 3)) * (8 if dim == rank - 1 else 1) for _ in range(count)]
    return rank, dim if rng.random() < 0.5 else dim - rank, shape, extents


def test_seeded_cat_sweep(launches, chain):
    rng = random.Random("cat")
    draws, expected = 72, 0
    for i in range(draws):
        rank, dim, shape, extents = draw_cat(rng, i)
        dtype, count = DTYPES[i % 2], 1 + i % 3
        torch.manual_seed(2000 + i)
        tensors = []
        for j, extent in enumerate(extents):
            s = list(shape)
            s[dim] = extent
            form = FORMS[(i + j) % 3]  # every form in every position over the sweep
            x = (torch.randn(s, device=DEV) * (6 if (i + j) % 5 == 0 else 2)).to(dtype)  # (x 6: codes at both clamps)
            t = operand(x, form, lo=-4.0 + 0.25 * j, hi=5.0 - 0.125 * j, num_bits=2 + (i + j) % 7)
            if form == "container" and (i + j) % 2:
                t = negative_zero(t)
            tensors.append(t)
        with torch.no_grad():  # (one quantized input alone is the concatenation of codes: no launch for it)
            as_codes = code_level.cat_predicate(tensors, dim, output_quantizer=None, strict_quantization=False)
        value = compare(lambda q: F.cat(tensors, dim, output_quantizer=q), quantizers(count), chain)
        assert value.shape[dim] == sum(extents)
        expected += count + (0 if as_codes else 1)
    assert launches["cat_quantize"] == expected and launches["pad_quantize"] == 0


def test_cat_keeps_negative_zero_and_the_clamps(launches, chain):
    torch.manual_seed(5)
    for dtype in DTYPES:
        x = (torch.randn(3, 4, 16, device=DEV) * 8).to(dtype)
        q = operand(x, "int8", num_bits=4)
        assert int(q.raw_data.min()) == -8 and int(q.raw_data.max()) == 7
        z = negative_zero(operand(x, "container"))
        narrow = operand(x[..., :5].contiguous(), "int8", num_bits=4)
        for tensors, dim in (([q, z, x], 1), ([z, narrow, x[..., :3]], -1)):
            value = compare(lambda oq: F.cat(tensors, dim, output_quantizer=oq), quantizers(1), chain)
            assert bool(((value == 0) & torch.signbit(value)).any())
    assert launches["cat_quantize"] == 8


def draw_pad(rng, i):
    mode = ("constant", "reflect", "replicate")[i % 3]
    k = 1 + (i // 3) % 3
    if mode == "constant":
        rank = rng.randint(k, 5)
    else:
        rank = k + rng.choice((1, 2))
    shape = [rng.randint(1, 4) for _ in range(rank - k)] + [rng.randint(2, 12) for _ in range(k)]
    if i % 2 == 0:
        shape[-1] = rng.choice((8, 16))
    pad = []
    for d in range(k):
        extent = shape[-1 - d]
        if mode == "constant":
            lo = -((extent - 1) // 2)
            pair = [rng.randint(lo, 6), rng.randint(lo, 6)]
        elif mode == "reflect":
            pair = [rng.randint(0, extent - 1), rng.randint(0, extent - 1)]
        else:
            pair = [rng.randint(0, 6), rng.randint(0, 6)]
        pad += pair
    if i % 4 == 0:  # a result row of a multiple of 8: the 8-elements-per-lane form
        pad[0], pad[1] = (8, 0) if i % 8 == 0 else (3, 5)
        if mode == "reflect" and shape[-1] <= 8:
            shape[-1] = 16
    if mode == "constant" and max(pad) <= 0:
        pad[0] = 2
    return mode, shape, tuple(pad)


def test_seeded_pad_sweep(launches, chain):
    rng = random.Random("pad")
    draws, expected = 90, 0
    for i in range(draws):
        mode, shape, pad = draw_pad(rng, i)
        dtype, count = DTYPES[i % 2], 1 + i % 3
        form = FORMS[(i // 3) % 3]
        channel = form != "plain" and len(shape) - len(pad) // 2 >= 2 and i % 2 == 1
        torch.manual_seed(3000 + i)
        x = (torch.randn(shape, device=DEV) * (6 if i % 5 == 0 else 2)).to(dtype)
        t = operand(x, form, num_bits=2 + i % 7, channel=channel)
        if form == "container" and not channel and i % 2 == 0:
            t = negative_zero(t)
        value = FILLS[i % len(FILLS)] if mode == "constant" else None
        got = compare(lambda q: F.pad(t, pad, mode, value, output_quantizer=q), quantizers(count), chain)
        assert got.shape == ops.concat.padded_shape(shape, pad)
        expected += 1 + count
    assert launches["pad_quantize"] == expected and launches["cat_quantize"] == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_fill_of_a_constant_pad_has_the_chains_bits(dtype, launches, chain):
    """Every fill of the issue on a plain and on a quantized input: a padded element is the fill, not A2 of a code."""
    torch.manual_seed(6)
    x = (torch.randn(2, 3, 5, 8, device=DEV) * 2).to(dtype)
    for t in (x, operand(x, "int8"), operand(x, "container", channel=True)):
        for value in FILLS + (0.1, -0.0, 1e-8):
            got = compare(lambda q: F.pad(t, (3, 5, 1, 0), "constant", value, output_quantizer=q), quantizers(1), chain)
            want = torch.full((), 0.0 if value is None else value, dtype=dtype, device=DEV)
            assert torch.equal(bits(got[..., 0, :]), bits(want.expand(2, 3, 16))) and torch.equal(bits(got[..., 1:, :3]), bits(want.expand(2, 3, 5, 3)))
    assert launches["pad_quantize"] == 3 * 10 * 2
    assert ops.concat.fill_bits(1.00390625 + 2**-30, torch.bfloat16) == 0x3F80  # two roundings: the tie goes to even


def test_one_launch_feeds_three_output_quantizers(launches):
    torch.manual_seed(7)
    x, y = (torch.randn(3, 5, 13, device=DEV) * 2).to(torch.bfloat16), (torch.randn(3, 2, 13, device=DEV) * 2).to(torch.bfloat16)
    qs = quantizers(3)
    pairs = [(q.scale, q.offset) for q in qs]
    with torch.no_grad():
        value, codes = ops.cat_quantize([x, y], 1, quantizers=pairs)
        padded, pad_codes = ops.pad_quantize(x, (2, 1, 0, 3), "reflect", quantizers=pairs)
        same_tensor(value, torch.cat([x, y], 1))
        same_tensor(padded, torch.nn.functional.pad(x, (2, 1, 0, 3), "reflect"))
        for q, c, p in zip(qs, codes, pad_codes):
            assert torch.equal(c, q(value).raw_data) and torch.equal(p, q(padded).raw_data)
        none, only = ops.cat_quantize([x, y], 1, quantizers=pairs[:1], want_value=False)
        assert none is None and torch.equal(only[0], codes[0])
    assert launches == {"cat_quantize": 2, "pad_quantize": 1}


# ---- 2. the code-level cat --------------------------------------------------------------------------------------------------------------
def test_the_code_level_cat_concatenates_codes_and_launches_nothing(launches, monkeypatch):
    compared = []
    real = code_level._values_equal
    monkeypatch.setattr(code_level, "_values_equal", lambda a, b: compared.append(1) or real(a, b))
    torch.manual_seed(8)
    x, y = (torch.randn(2, 3, 16, device=DEV) * 2).to(torch.bfloat16), (torch.randn(2, 5, 16, device=DEV) * 2).to(torch.bfloat16)
    q = act_quantizer(-4.0, 5.0)
    with torch.no_grad(), ff.strict_quantization(False):
        a, b = q(x), q(y)
        for got in (F.cat([a, b], 1), torch.cat([a, b], 1), torch.cat([a, b], dim=-2)):
            assert isinstance(got, ff.QuantizedTensor) and torch.equal(got.raw_data, torch.cat([a.raw_data, b.raw_data], 1))
            assert got.quant_args().scale is a.quant_args().scale
            assert torch.equal(got.dequantize(), torch.cat([a.dequantize(), b.dequantize()], 1))
        assert not compared  # one parameter object: no look at device memory
        other = act_quantizer(-4.0, 5.0)(y)  # equal values in other tensors: compared as the reference compares them
        assert isinstance(F.cat([a, other], 1), ff.QuantizedTensor) and compared
        different = act_quantizer(-2.0, 2.0)(y)
        assert sum(launches.values()) == 0
        assert type(F.cat([a, different], 1)) is torch.Tensor  # other parameters: the fused kernel's value
    assert launches == {"cat_quantize": 1, "pad_quantize": 0}


# ---- 3. range estimation sees the value -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["cat", "pad"])
def test_range_estimation_sees_the_real_value(op, launches, chain):
    torch.manual_seed(9)
    x, y = (torch.randn(2, 4, 9, 16, device=DEV) * 2).to(torch.bfloat16), (torch.randn(2, 3, 9, 16, device=DEV) * 3).to(torch.bfloat16)
    qx, qy = operand(x, "int8"), operand(y, "container", lo=-6.0, hi=6.0)
    call = (lambda q: F.cat([qx, y, qy], 1, output_quantizer=q)) if op == "cat" else (lambda q: F.pad(qy, (2, 2, 1, 1), "constant", 7.5, output_quantizer=q))

    def estimate():
        q = ff.nn.LinearQuantizer(8, symmetric=False, quantized_dtype=torch.int8, device=DEV)
        with torch.no_grad(), ff.strict_quantization(False), ff.estimate_ranges(q, ff.range_setting.running_minmax):
            out = call(q)
        return q, out

    q, out = estimate()
    with chain():
        want_q, want = estimate()
    assert torch.equal(q.scale, want_q.scale) and torch.equal(q.offset, want_q.offset)
    same_quantized(out, want)
    assert launches[f"{op}_quantize"] == 1


# ---- 4. hipGraph: a quantized decoder step ----------------------------------------------------------------------------------------------
class DecoderStep(torch.nn.Module):
    """interpolate (nearest x2) -> cat with the skip tensor -> reflect pad 1 -> a 3x3 convolution: one U-Net join."""

    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(16, 16, 3)
        self.up_quantizer = ff.nn.QuantizerStub()
        self.cat_quantizer = ff.nn.QuantizerStub()
        self.pad_quantizer = ff.nn.QuantizerStub()

    def forward(self, low, skip):
        up = F.interpolate(low, scale_factor=2, output_quantizer=self.up_quantizer)
        joined = F.cat([up, skip], 1, output_quantizer=self.cat_quantizer)
        return self.conv(F.pad(joined, (1, 1, 1, 1), "reflect", output_quantizer=self.pad_quantizer))


def test_a_decoder_step_captures_and_replays(launches):
    torch.manual_seed(10)
    conv = ff.nn.quantized_conv_modules()
    model = DecoderStep().to(DEV, torch.bfloat16)
    model = ff.quantize_model(model, extra_conversion={**conv, **ff.nn.surrogate_quantized_modules(model, extra_conversion=conv)})
    assert type(model.conv) is ff.nn.QuantizedConv2d
    act = lambda: ff.nn.LinearQuantizer(8, symmetric=False, quantized_dtype=torch.int8, device=DEV)  # noqa: E731
    model.up_quantizer, model.cat_quantizer, model.pad_quantizer, model.conv.output_quantizer = act(), act(), act(), act()
    model.conv.weight_quantizer = ff.nn.LinearQuantizer(8, granularity=ff.PerChannel(0), quantized_dtype=torch.int8, device=DEV)
    low, skip = torch.randn(2, 8, 8, 8, device=DEV, dtype=torch.bfloat16), torch.randn(2, 8, 16, 16, device=DEV, dtype=torch.bfloat16)
    skip_quantizer = act_quantizer(-4.0, 4.0)

    def step():
        with torch.no_grad(), ff.strict_quantization(False):
            return model(low, skip_quantizer(skip))

    with torch.no_grad(), ff.strict_quantization(False), ff.estimate_ranges(model, ff.range_setting.running_minmax):
        model(low, skip_quantizer(skip))
    before = dict(launches)
    step()  # (the first call outside the capture)
    assert {k: launches[k] - before[k] for k in OPS} == {"cat_quantize": 1, "pad_quantize": 1}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side), torch.cuda.graph(g, stream=side):
        out = step()
    torch.cuda.current_stream().wait_stream(side)
    low.copy_(low.flip(-1) * 0.5)  # fresh contents in the captured inputs
    skip.copy_(skip.flip(0))
    eager = step().raw_data.clone()
    out.raw_data.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.raw_data, eager) and bool(eager.any())
    assert {k: launches[k] - before[k] for k in OPS} == {"cat_quantize": 3, "pad_quantize": 3}


# ---- 5. layouts: offset, strided, permuted and odd-sized views reach the kernels as aligned copies -------------------------------------
@pytest.mark.parametrize("layout", every(2), ids=[layout.id for layout in every(2)])
@pytest.mark.parametrize("op", ["cat", "pad_constant", "pad_reflect"])
def test_views(op, layout, launches):
    torch.manual_seed(11)
    base = torch.randn(3, 4, 9, 14, device=DEV).to(torch.bfloat16)
    view = layout.make(base)
    other = operand(base[:, :3].contiguous(), "int8")
    oq = act_quantizer(-4.0, 4.0)
    calls = {"cat": lambda v: F.cat([v, other, v], 1, output_quantizer=oq), "pad_constant": lambda v: F.pad(v, (3, 2, 1, 0), "constant", -1.5, output_quantizer=oq),
             "pad_reflect": lambda v: F.pad(v, (3, 3, 2, 2), "reflect", output_quantizer=oq)}
    with torch.no_grad(), ff.strict_quantization(False):
        got, want = calls[op](view), calls[op](view.clone(memory_format=torch.contiguous_format))
    assert torch.equal(got.raw_data, want.raw_data) and got.raw_data.is_contiguous()
    assert sum(launches.values()) == 2


def test_channels_last_inputs_keep_atens_strides(launches, chain):
    torch.manual_seed(12)
    x = torch.randn(3, 4, 9, 14, device=DEV).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    with torch.no_grad(), ff.strict_quantization(False):
        for call in (lambda: F.cat([x, x], 1), lambda: F.pad(x, (1, 1), "constant", 0.5), lambda: F.pad(x, (1, 1, 2, 2), "reflect")):
            got = call()
            with chain():
                want = call()
            same_tensor(got, want)
        assert F.cat([x, x], 1).is_contiguous(memory_format=torch.channels_last)
        mixed = F.cat([x, x.contiguous()], 1)  # one channels-last input is not enough: ATen answers contiguous, and so does the kernel
        with chain():
            same_tensor(mixed, F.cat([x, x.contiguous()], 1))
    assert launches == {"cat_quantize": 1, "pad_quantize": 0}


# ---- 6. full size (the timing table's shapes) --------------------------------------------------------------------------------------------
FULL_CAT = [((8, 64, 256, 256), (8, 64, 256, 256), 1), ((8, 512, 32, 32), (8, 512, 32, 32), 1), ((8, 8, 2047, 128), (8, 8, 1, 128), 2)]
FULL_PAD = [((32, 3, 224, 224), (3, 3, 3, 3), "reflect"), ((32, 3, 224, 224), (3, 3, 3, 3), "constant"), ((8, 2048, 4096), (0, 0, 1, 0), "constant")]


def full_size(call, args, launches, chain):
    oq = act_quantizer(-4.0, 4.0)
    with torch.no_grad(), ff.strict_quantization(False):
        got = call(args, oq).raw_data
        with chain():
            want = call(args, oq).raw_data
    assert got.shape == want.shape and got.stride() == want.stride() and torch.equal(got, want)


@pytest.mark.parametrize("a,b,dim", FULL_CAT, ids=[f"{'x'.join(map(str, a))}+{'x'.join(map(str, b))}" for a, b, _ in FULL_CAT])
def test_full_size_cat(a, b, dim, launches, chain):
    torch.manual_seed(13)
    x, y = (torch.randn(a, device=DEV) * 2).to(torch.bfloat16), (torch.randn(b, device=DEV) * 2).to(torch.bfloat16)
    for args in ([x, y], [act_quantizer(-4.0, 5.0)(x), act_quantizer(-3.0, 4.0)(y)]):  # bf16 -> int8 and int8 -> int8
        full_size(lambda t, oq: F.cat(t, dim, output_quantizer=oq), args, launches, chain)
    assert launches["cat_quantize"] == 2


@pytest.mark.parametrize("shape,pad,mode", FULL_PAD, ids=[f"{'x'.join(map(str, s))}-{m}" for s, _, m in FULL_PAD])
def test_full_size_pad(shape, pad, mode, launches, chain):
    torch.manual_seed(14)
    x = (torch.randn(shape, device=DEV) * 2).to(torch.bfloat16)
    for arg in (x, act_quantizer(-4.0, 5.0)(x)):
        full_size(lambda t, oq: F.pad(t, pad, mode, output_quantizer=oq), arg, launches, chain)
    assert launches["pad_quantize"] == 2


# ---- 7. the predicate declines: the reference chain runs, unchanged ---------------------------------------------------------------------
def test_fallbacks_when_the_predicate_declines(launches, chain):
    torch.manual_seed(15)
    x, y = (torch.randn(2, 4, 12, 12, device=DEV) * 2).to(torch.bfloat16), (torch.randn(2, 3, 12, 12, device=DEV) * 2).to(torch.bfloat16)
    qx, qc = operand(x, "int8"), operand(y, "int8", channel=True)
    oq = act_quantizer(-3.0, 3.0)
    with torch.no_grad():
        assert not fused_concat.cat_predicate(tensors=[qx, y], dim=1, output_quantizer=oq)  # no strict_quantization keyword
        assert fused_concat.cat_predicate(tensors=[qx, y], dim=1, output_quantizer=oq, strict_quantization=False)
        assert fused_concat.pad_predicate(input=qc, pad=(1, 1), mode="constant", value=None, output_quantizer=oq, strict_quantization=False)
    declined = [
        (F.cat, ([qx, qc], 1), {}),                                   # a per-channel cat input
        (F.cat, ([x.float(), y.float()], 1), {}),                     # fp32 values
        (F.cat, ([x, y.half()], 1), {}),                              # mixed dtypes: ATen promotes
        (F.cat, ([x, torch.zeros(0, device=DEV, dtype=torch.bfloat16)], 1), {}),  # ATen skips a [0] tensor
        (F.pad, (qx, (1, 1, 1, 1), "circular"), {}),
        (F.pad, (qx, (-1, -2, 0, 0), "constant"), {}),                # a pure crop
        (F.pad, (qx, (-1, 2, 1, 1), "reflect"), {}),                  # ATen takes negative reflect pads; the kernel does not
        (F.pad, (operand(x, "int8").dequantize().float(), (1, 1), "constant", 2.0), {}),
    ]
    for fn, args, kwargs in declined:
        with torch.no_grad(), ff.strict_quantization(False):
            got = fn(*args, **kwargs, output_quantizer=oq)
            with chain():
                want = fn(*args, **kwargs, output_quantizer=oq)
        same_quantized(got, want)
    # grad mode with learnable quantizer parameters: the chain, with its autograd graph
    with ff.strict_quantization(False):
        got = F.cat([qx, y], 1, output_quantizer=oq)
        with chain():
            want = F.cat([qx, y], 1, output_quantizer=oq)
        assert torch.equal(got.raw_data, want.raw_data)
        padded = F.pad(qx, (1, 1), "constant", output_quantizer=oq)
        with chain():
            assert torch.equal(padded.raw_data, F.pad(qx, (1, 1), "constant", output_quantizer=oq).raw_data)
    # geometry ATen refuses raises ATen's error
    for args in ((qx, (12, 0, 0, 0), "reflect"), (qx, (1, 1), "reflect"), (qx, (1, 1, 1), "constant"), (qx, (1, 1))):
        with pytest.raises((RuntimeError, NotImplementedError)) as got, torch.no_grad(), ff.strict_quantization(False):
            F.pad(*args)
        with pytest.raises((RuntimeError, NotImplementedError)) as want, torch.no_grad():
            torch.nn.functional.pad(qx.dequantize(), *args[1:]) if len(args) > 2 else torch.nn.functional.pad(qx.dequantize(), args[1], "...")
        assert str(got.value) == str(want.value)
    with pytest.raises(RuntimeError) as got, torch.no_grad(), ff.strict_quantization(False):
        F.cat([x, y], 0)
    with pytest.raises(RuntimeError) as want:
        torch.cat([x, y], 0)
    assert str(got.value) == str(want.value)
    assert F.cat([x.cpu(), y.cpu()], 1, strict_quantization=False).device.type == "cpu"  # not on the device
    assert launches == {name: 0 for name in OPS}
