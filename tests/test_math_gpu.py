"""The one-pass rms_norm, pow, exp, sin, cos, sum and cumsum kernels (csrc/ffq_math.hip) on the MI355X, against the device reference
chain — dequantize the input, the ATen op, the output quantizer — that the generated fallbacks run (reference _gen/fallback.py),
with this package's registrations taken out of the dispatcher.

exp, sin, cos and pow by a number: the value is bit for bit the chain's on every bf16 / fp16 input (ATen's formulas, each pow branch
included; fp16 sizes are multiples of 65536, see test_elementwise_gpu.py), the codes are the output quantizer applied to it.
rms_norm and sum: the value is within 1 ulp of ATen's with fewer than 1 % of the elements differing (a result of fewer than 100
elements may have one) — the fp32 sum is the kernel's own summation order; NaN exactly where ATen has NaN; the codes are exactly A1
of the value the call produced.
cumsum: ATen's device kernel keeps its running sum in the data dtype (measured on the MI355X: 83 % of the prefixes of a bf16
[16, 4096] row scan differ from the fp32 scan, by up to 1.9 in absolute value against the exact scan), so it is no reference for the
value. The kernels keep an fp32 running sum, as ATen's CPU kernel, and the bound is that of any fp32 summation order: the value is
within one ulp of the data dtype plus l * 2^-24 * sum(|v|) of the float64 scan of the same dequantized input (l: the prefix
length), fewer than 1 % of the values differ from that scan rounded to the data dtype, and the codes are exactly A1 of the value. Every test counts the calls of the ``ops`` entry points, so a silent fallback fails it."""

import contextlib
import math

import pytest
import torch

import fastforward_amd as ff

from fastforward_amd import dispatcher, fused_math, ops
from fastforward_amd.exceptions import QuantizationError
from fastforward_amd.nn import functional as F
from layouts import every
from test_elementwise_gpu import FORMS, SHAPE, compare_with_chain, operand, run, specials
from test_modules_gpu import act_quantizer, ordered

pytestmark = pytest.mark.gpu
DEV = "cuda"
OPS = ("rms_norm_quantize", "unary_quantize", "sum_quantize", "cumsum_quantize")
NAMES = ("rms_norm", "pow", "exp", "sin", "cos", "sum", "cumsum")
EXPONENTS = (2, 3, 0.5, -0.5, -1, -2, 1.7, 0, 1, 2.001, -3, 4)
KERNELS = fused_math.KERNELS  # its sum / cumsum called directly: the column forms the predicates decline (slower than the route)


def columns(shape, dim):
    """A reduction or scan over a dim before the last: the column kernels, which ff.nn.functional declines."""
    return dim is not None and math.prod(shape[dim % len(shape) + 1:]) > 1


@pytest.fixture()
def launches(monkeypatch):
    """{op name: number of calls} of the four ops entry points."""
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
    """A context in which the dispatcher has none of this package's math kernels: the reference chain runs."""

    @contextlib.contextmanager
    def off():
        with monkeypatch.context() as m:
            for op in NAMES:
                kept = [it for it in dispatcher._DISPATCHER.get(op, []) if getattr(it.fn, "__self__", None) is not fused_math.KERNELS]
                m.setitem(dispatcher._DISPATCHER, op, kept)
            yield

    return off


def check_contract(got, want):
    """NaN where `want` has NaN; elsewhere at most 1 ulp with fewer than 1 % of the elements differing (one, below 100)."""
    nan_g, nan_w = torch.isnan(got), torch.isnan(want)
    assert torch.equal(nan_g, nan_w)
    g, w = got[~nan_g], want[~nan_w]
    if not g.numel():
        return
    ulps = (ordered(g) - ordered(w)).abs()
    assert int(ulps.max()) <= 1, int(ulps.max())
    differ = int((ulps != 0).sum())
    assert differ <= 1 if g.numel() < 100 else differ < 0.01 * g.numel(), (differ, g.numel())


def against_chain(fn, args, kwargs, oq, chain, public=None):
    """The contract against the chain's value (of `public`, the ff.nn.functional op, when `fn` is a kernel called directly), the
    codes exactly A1 of the value."""
    value, quantized = run(fn, *args, oq=oq, **kwargs)
    with chain():
        want, _ = run(public or fn, *args, oq=oq, **kwargs)
    assert value.dtype == want.dtype and value.shape == want.shape
    check_contract(value, want)
    with torch.no_grad():
        assert torch.equal(quantized.raw_data, oq(value).raw_data)  # exactly A1 of the value this call produced
    return value


def _dequantized(x):
    return x.dequantize() if isinstance(x, ff.QuantizedTensor) else x


def cumsum_against_exact(x, dim, oq, fn=F.cumsum):
    """The cumsum contract: each value within one ulp of the data dtype of the float64 scan of the same dequantized input, plus
    the bound of any fp32 summation order (l * 2^-24 * sum |v| at prefix length l); fewer than 1 % of the values differ from the
    float64 scan rounded to the data dtype; the codes exactly A1 of the value."""
    value, quantized = run(fn, x, dim, oq=oq)
    v = _dequantized(x)
    exact = torch.cumsum(v.double(), dim)
    shape = [1] * v.dim()
    shape[dim] = v.shape[dim]
    count = torch.arange(1, v.shape[dim] + 1, device=DEV, dtype=torch.float64).view(shape)
    slack = count * 2.0**-24 * torch.cumsum(v.double().abs(), dim)
    bits, emin = (7, -126) if v.dtype == torch.bfloat16 else (10, -14)
    ulp = torch.exp2(torch.floor(torch.log2(exact.abs().clamp(min=2.0**emin))) - bits)
    assert value.dtype == v.dtype and value.shape == v.shape
    assert bool(((value.double() - exact).abs() <= ulp + slack).all())
    assert float((value != exact.to(v.dtype)).float().mean()) < 0.01
    with torch.no_grad():
        assert torch.equal(quantized.raw_data, oq(value).raw_data)


# ---- exp / sin / cos / pow by a number ---------------------------------------------------------------------------------------------
UNARY = [("exp", {}), ("sin", {}), ("cos", {})] + [("pow", dict(exponent=e)) for e in EXPONENTS]


@pytest.mark.parametrize("op", range(len(UNARY)), ids=[f"{n}{k.get('exponent', '')}" for n, k in UNARY])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("form", FORMS)
def test_unary_equals_the_reference_chain(op, dtype, form, launches, chain):
    torch.manual_seed(30 + op)
    x = (torch.randn(SHAPE[dtype], device=DEV) * 3).to(dtype)
    if form == "plain":
        specials(x)
    name, kwargs = UNARY[op]
    compare_with_chain(getattr(F, name), (operand(x, form),), kwargs, act_quantizer(-2.0, 6.0), chain)
    assert launches["unary_quantize"] == 2


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_unary_on_every_16_bit_pattern(dtype, launches, chain):
    x = torch.arange(-32768, 32768, dtype=torch.int32, device=DEV).to(torch.int16).view(dtype).view(-1, 256)
    for name, kwargs in UNARY:
        compare_with_chain(getattr(F, name), (x,), kwargs, act_quantizer(-2.0, 2.0), chain)
    assert launches["unary_quantize"] == 2 * len(UNARY)


# ---- rms_norm -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("cols", [8, 64, 512, 520, 4096, 16384])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("weight", ["none", "plain", "int8"])
def test_rms_norm_meets_the_contract(dtype, cols, form, weight, launches, chain):
    torch.manual_seed(cols + 7)
    x = (torch.randn(37, cols, device=DEV) * 2).to(dtype)
    w = (torch.randn(cols, device=DEV) * 0.5 + 1).to(dtype)
    w = {"none": None, "plain": w, "int8": act_quantizer(-2.0, 2.5)(w) if weight == "int8" else None}[weight]
    eps = None if cols % 1024 else 1e-6
    against_chain(F.rms_norm, (operand(x, form), (cols,), w, eps), {}, act_quantizer(-3.0, 3.0), chain)
    assert launches["rms_norm_quantize"] == 2


def test_rms_norm_with_nan_and_inf_rows(launches, chain):
    x = torch.randn(8, 256, device=DEV).to(torch.bfloat16)
    x[1, 5], x[2, 7], x[3] = float("nan"), float("inf"), 0.0
    value = against_chain(F.rms_norm, (x, (256,)), {}, act_quantizer(-3.0, 3.0), chain)
    assert torch.isnan(value[1]).all() and not value[3].any()
    assert launches["rms_norm_quantize"] == 2


# ---- sum / cumsum -------------------------------------------------------------------------------------------------------------------
REDUCTIONS = [((37, 264), None), ((37, 264), 0), ((37, 264), 1), ((37, 264), -1), ((6, 40, 64), 1), ((6, 40, 64), 0),
              ((2048, 512), 0), ((16, 8, 4096), 1), ((3, 200008), -1), ((1 << 21,), 0), ((4, 4, 8), None)]


SUM_CASES = [(s, d, f) for s, d in REDUCTIONS for f in FORMS if not (f == "int8_row" and len(s) == 1)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape,dim,form", SUM_CASES, ids=[f"{s}-{d}-{f}" for s, d, f in SUM_CASES])
def test_sum_meets_the_contract(dtype, shape, dim, form, launches, chain):
    torch.manual_seed(11)
    x = torch.randn(shape, device=DEV).to(dtype)
    kwargs = {} if dim is None else dict(dim=dim)
    fn = KERNELS.sum if columns(shape, dim) else F.sum
    value = against_chain(fn, (operand(x, form),), kwargs, act_quantizer(-40.0, 40.0), chain, public=F.sum)
    assert value.shape == (torch.sum(x) if dim is None else torch.sum(x, dim)).shape
    assert launches["sum_quantize"] == 2


SCANS = [((37, 264), 0), ((37, 264), 1), ((3, 4104), -1), ((6, 40, 64), 1), ((6, 40, 64), 0), ((2, 16, 24), 2), ((1, 65536), 1)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape,dim", SCANS, ids=[f"{s}-{d}" for s, d in SCANS])
@pytest.mark.parametrize("form", FORMS)
def test_cumsum_meets_the_contract(dtype, shape, dim, form, launches, chain):
    torch.manual_seed(12)
    x = torch.randn(shape, device=DEV).to(dtype)
    cumsum_against_exact(operand(x, form), dim, act_quantizer(-40.0, 40.0), KERNELS.cumsum if columns(shape, dim) else F.cumsum)
    assert launches["cumsum_quantize"] == 2


def test_sum_is_deterministic(launches):
    x = torch.randn(64, 2048, device=DEV).to(torch.bfloat16)
    calls = [lambda: F.sum(x), lambda: KERNELS.sum(x, 0), lambda: F.sum(x, 1)]  # the whole tensor, columns, rows
    with torch.no_grad(), ff.strict_quantization(False):
        first = [call() for call in calls]
        for _ in range(3):
            assert all(torch.equal(a, call()) for a, call in zip(first, calls))
    assert launches["sum_quantize"] == 12


# ---- layouts: offset, strided and misaligned views reach the kernels as aligned copies -------------------------------------------
@pytest.mark.parametrize("layout", every(2), ids=[layout.id for layout in every(2)])
@pytest.mark.parametrize("name", ["rms_norm", "exp", "pow", "sum", "cumsum"])
def test_views(name, layout, launches):
    torch.manual_seed(14)
    t = torch.randn(24, 64, device=DEV).to(torch.bfloat16)
    view = layout.make(t)
    call = {"rms_norm": lambda v: F.rms_norm(v, (64,), output_quantizer=oq), "exp": lambda v: F.exp(v, output_quantizer=oq),
            "pow": lambda v: F.pow(v, 3, output_quantizer=oq), "sum": lambda v: F.sum(v, -1, output_quantizer=oq),
            "cumsum": lambda v: F.cumsum(v, -1, output_quantizer=oq)}[name]
    oq = act_quantizer(-4.0, 4.0)
    with torch.no_grad(), ff.strict_quantization(False):
        got, want = call(view), call(view.clone())
    assert torch.equal(got.raw_data, want.raw_data)
    assert sum(launches.values()) == 2


# ---- the predicate declines: the reference chain runs, unchanged -------------------------------------------------------------------
def test_fallbacks_when_the_predicate_declines(launches, chain):
    torch.manual_seed(15)
    x = torch.randn(16, 64, device=DEV).to(torch.bfloat16)
    qx = operand(x, "int8_tensor")
    oq = act_quantizer(-3.0, 3.0)
    with torch.no_grad():
        assert not fused_math.unary_predicate(input=qx, output_quantizer=oq)  # no strict_quantization keyword
        assert fused_math.unary_predicate(input=qx, output_quantizer=oq, strict_quantization=False)
    declined = [
        (F.pow, (qx, torch.full((16, 64), 2.0, device=DEV).to(torch.bfloat16)), {}),       # a tensor exponent
        (F.pow, (qx, torch.tensor(2.0, device=DEV)), {}),                                  # a 0-dim tensor exponent
        (F.rms_norm, (torch.randn(2, 16392, device=DEV).to(torch.bfloat16), (16392,)), {}),  # cols > 16384
        (F.rms_norm, (qx, (16, 64)), {}),                                                  # not the last dim alone
        (F.rms_norm, (x.view(4, 4, 64), (4, 64)), {}),
        (F.sum, (torch.randn(8, 4, 6, device=DEV).to(torch.bfloat16), 1), {}),              # 6 elements after dim
        (F.cumsum, (torch.randn(4, 36, device=DEV).to(torch.bfloat16), -1), {}),            # 36 % 8
        (F.sum, (qx, 0), {}),                                                              # a dim before the last: the
        (F.cumsum, (qx, 0), {}),                                                           # column kernels are slower
        (F.exp, (x[:3, :3],), {}),                                                         # 9 elements
        (F.sin, (x.float(),), {}),                                                         # fp32 values
    ]
    for fn, args, kwargs in declined:
        with torch.no_grad(), ff.strict_quantization(False):
            got = fn(*args, **kwargs, output_quantizer=oq)
            with chain():
                want = fn(*args, **kwargs, output_quantizer=oq)
        assert torch.equal(got.raw_data, want.raw_data), fn
    assert F.exp(x.cpu(), output_quantizer=None, strict_quantization=False).device.type == "cpu"  # not on the device
    # grad mode with an operand that needs a gradient
    xg = x.clone().requires_grad_()
    for fn, args in ((F.exp, (xg,)), (F.sum, (xg, 0)), (F.rms_norm, (xg, (64,)))):
        with ff.strict_quantization(False):
            got = fn(*args, output_quantizer=oq)
            with chain():
                want = fn(*args, output_quantizer=oq)
        assert torch.equal(got.raw_data, want.raw_data)
    # strict mode: the calls the fallback rejects still raise its errors
    for fn, args in ((F.exp, (x,)), (F.sum, (x,)), (F.pow, (qx, torch.ones(16, 64, device=DEV))), (F.rms_norm, (qx, (64,), x[0]))):
        with pytest.raises(QuantizationError):
            fn(*args, output_quantizer=oq, strict_quantization=True)
    assert launches == {name: 0 for name in OPS}


def test_the_torch_function_route_launches_nothing_new(launches):
    x = torch.randn(16, 64, device=DEV).to(torch.bfloat16)
    qa = operand(x, "int8_tensor")
    da = qa.dequantize()
    with ff.strict_quantization(False):
        got = [torch.exp(qa), torch.sin(qa), torch.cos(qa), torch.pow(qa, 2), torch.sum(qa, 0), torch.cumsum(qa, 1)]
    want = [torch.exp(da), torch.sin(da), torch.cos(da), torch.pow(da, 2), torch.sum(da, 0), torch.cumsum(da, 1)]
    for g, w in zip(got, want):
        assert type(g) is torch.Tensor and torch.equal(g, w)
    assert launches == {name: 0 for name in OPS}


# ---- hipGraph -----------------------------------------------------------------------------------------------------------------------
def test_fused_math_calls_capture_and_replay(launches):
    torch.manual_seed(16)
    x = torch.randn(64, 1024, device=DEV).to(torch.bfloat16)
    qa, qr = operand(x, "int8_tensor"), operand(x.flip(0), "int8_row")
    w = (torch.randn(1024, device=DEV) * 0.5 + 1).to(torch.bfloat16)
    oq, wide = act_quantizer(-3.0, 3.0), act_quantizer(-60.0, 60.0)

    def step():
        with torch.no_grad(), ff.strict_quantization(False):
            return (F.rms_norm(qa, (1024,), w, output_quantizer=oq), F.exp(qr, output_quantizer=oq), F.pow(qa, 2, output_quantizer=oq),
                    KERNELS.sum(qr, 0, output_quantizer=wide), F.sum(qa, output_quantizer=wide), F.cumsum(qa, -1, output_quantizer=wide),
                    KERNELS.cumsum(qr, 0, output_quantizer=wide))

    eager = [t.raw_data.clone() for t in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side), torch.cuda.graph(g, stream=side):
        outs = step()
    torch.cuda.current_stream().wait_stream(side)
    for t in outs:
        t.raw_data.zero_()
    g.replay()
    torch.cuda.synchronize()
    for t, e in zip(outs, eager):
        assert torch.equal(t.raw_data, e)
    assert launches == {"rms_norm_quantize": 2, "unary_quantize": 4, "sum_quantize": 4, "cumsum_quantize": 4}


# ---- full size (the timing table's shapes) ----------------------------------------------------------------------------------------
def test_full_size_shapes(launches, chain):
    torch.manual_seed(17)
    oq = act_quantizer(-4.0, 4.0)
    h = torch.randn(16384, 4096, device=DEV).to(torch.bfloat16)
    w = (torch.randn(4096, device=DEV) * 0.5 + 1).to(torch.bfloat16)
    # rms_norm [16384, 4096] bf16 -> int8 and int8 -> int8
    against_chain(F.rms_norm, (h, (4096,), w), {}, oq, chain)
    against_chain(F.rms_norm, (act_quantizer(-4.0, 4.0)(h), (4096,), w), {}, oq, chain)
    # sum(-1) and sum(0) of [16384, 4096]
    against_chain(F.sum, (h, -1), {}, act_quantizer(-300.0, 300.0), chain)
    against_chain(KERNELS.sum, (h, 0), {}, act_quantizer(-600.0, 600.0), chain, public=F.sum)
    del h
    # cumsum(-1) of [4096, 4096]
    c = torch.randn(4096, 4096, device=DEV).to(torch.bfloat16)
    cumsum_against_exact(c, -1, act_quantizer(-200.0, 200.0))
    del c
    # exp / sin / cos / pow(2) [16384, 16384] bf16 -> int8: bit for bit
    y = (torch.randn(16384, 16384, device=DEV) * 2).to(torch.bfloat16)
    for fn, args in ((F.exp, (y,)), (F.sin, (y,)), (F.cos, (y,)), (F.pow, (y, 2))):
        with torch.no_grad(), ff.strict_quantization(False):
            got = fn(*args, output_quantizer=oq).raw_data
            with chain():
                want = fn(*args, output_quantizer=oq).raw_data
        assert torch.equal(got, want), fn
        del got, want
    assert launches == {"rms_norm_quantize": 4, "unary_quantize": 4, "sum_quantize": 4, "cumsum_quantize": 2}
