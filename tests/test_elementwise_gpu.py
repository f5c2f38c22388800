"""The one-pass add / sub / mul / div, softmax, sigmoid and GELU kernels (csrc/ffq_elementwise.hip) on the MI355X, against the device
reference chain — dequantize each operand, the ATen op, the output quantizer — that the generated fallbacks run (reference
_gen/fallback.py), with this package's registrations taken out of the dispatcher.

Binary ops, sigmoid and GELU: the value is bit for bit the chain's (ATen's fp32 formula, one rounding), the codes are the output
quantizer applied to it. ATen's own fp16 kernels compute that value only on their vectorized path: elements of a broadcast
operand, and the tail of a tensor whose size is not a multiple of the vectorized block's work, go through ATen's unrolled path, whose
fp16 results differ from its vectorized ones (negative zeros become positive zeros, and some values move by an ulp). The fp16 cases
therefore use sizes that are multiples of 65536 and compare broadcasts with the chain on the expanded operand. Softmax: the value is within 1 ulp of ATen's F.softmax on the same dequantized operand with fewer than 1 % of
the elements differing — the fp32 sum of the exponentials is the kernel's own summation order, and one ulp of the sum moves the
quotient by at most one ulp of the data dtype; NaN exactly where ATen has NaN; the codes are exactly A1 of the value the call
produced. Every test counts the calls of the ``ops`` entry points, so a silent fallback fails it."""

import contextlib

import pytest
import torch

import fastforward_amd as ff

from fastforward_amd import dispatcher, fused_elementwise, ops
from fastforward_amd.exceptions import QuantizationError
from fastforward_amd.nn import functional as F
from helpers import mismatch_report, same_with_nan
from test_modules_gpu import act_quantizer, ordered

pytestmark = pytest.mark.gpu
DEV = "cuda"
OPS = ("binary_quantize", "softmax_quantize", "activation_quantize")
NAMES = ("add", "sub", "mul", "div", "softmax", "sigmoid", "gelu")
FORMS = ("plain", "int8_tensor", "int8_row", "container_tensor")
SHAPE = {torch.bfloat16: (37, 264), torch.float16: (64, 1024)}  # fp16: ATen's vectorized path throughout (module docstring)


@pytest.fixture()
def launches(monkeypatch):
    """{op name: number of calls} of the three ops entry points."""
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
    """A context in which the dispatcher has none of this package's elementwise kernels: the reference chain runs (the
    reference's own rescale for mul by a number stays registered)."""

    @contextlib.contextmanager
    def off():
        with monkeypatch.context() as m:
            for op in NAMES:
                kept = [it for it in dispatcher._DISPATCHER[op] if getattr(it.fn, "__self__", None) is not fused_elementwise.KERNELS]
                m.setitem(dispatcher._DISPATCHER, op, kept)
            yield

    return off


def operand(x, form, lo=-4.0, hi=5.0):
    """`x` in one of the forms the kernels take."""
    if form == "plain":
        return x
    if form == "int8_tensor":
        return act_quantizer(lo, hi)(x)
    if form == "int8_row":
        rows = x.float().reshape(-1, x.shape[-1])
        lo_r, hi_r = rows.amin(-1).clamp(max=-0.5), rows.amax(-1).clamp(min=0.5)
        return act_quantizer(lo_r, hi_r, granularity=ff.PerChannel(tuple(range(x.dim() - 1))))(x)
    if form == "container_tensor":
        return act_quantizer(lo, hi, container=x.dtype)(x)
    raise ValueError(form)


def run(fn, *args, oq, **kwargs):
    with torch.no_grad(), ff.strict_quantization(False):
        value = fn(*args, output_quantizer=None, **kwargs)
        quantized = fn(*args, output_quantizer=oq, **kwargs)
    return value, quantized


def compare_with_chain(fn, args, kwargs, oq, chain, chain_args=None):
    value, quantized = run(fn, *args, oq=oq, **kwargs)
    with chain():
        want_value, want_q = run(fn, *(chain_args or args), oq=oq, **kwargs)
    assert value.dtype == want_value.dtype and same_with_nan(value, want_value), mismatch_report(value, want_value)
    assert isinstance(quantized, ff.QuantizedTensor) and torch.equal(quantized.raw_data, want_q.raw_data)
    assert torch.equal(quantized.dequantize(), want_q.dequantize())
    return value


def specials(x, zeros=False, at=0):
    """NaN, +-inf, signed zeros (and zeros to divide by) in a plain operand, from element `at` on."""
    flat = x.view(-1)[at:]
    flat[:6] = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0, 0.0, -1e-30], device=x.device).to(x.dtype)
    if zeros:
        flat[100:140] = 0.0
        flat[140:150] = -0.0
    return x


# ---- add / sub / mul / div -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["add", "sub", "mul", "div"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("a_form", FORMS)
@pytest.mark.parametrize("b_form", FORMS)
def test_binary_equals_the_reference_chain(op, dtype, a_form, b_form, launches, chain):
    torch.manual_seed(3)
    a = (torch.randn(SHAPE[dtype], device=DEV) * 2).to(dtype)
    b = (torch.randn(SHAPE[dtype], device=DEV) * 1.5 + 0.25).to(dtype)
    if a_form == "plain":
        specials(a)
    if b_form == "plain":
        specials(b, zeros=True, at=3)  # NaN / inf against a's NaN / inf / zeros
    # different scales on the two operands; quantized zeros in `other` divide by zero as well
    args = (operand(a, a_form), operand(b, b_form, lo=-3.0, hi=2.0))
    oq = act_quantizer(-4.0, 6.0)
    compare_with_chain(getattr(F, op), args, {}, oq, chain)
    assert launches["binary_quantize"] == 2


@pytest.mark.parametrize("op", ["add", "sub"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("alpha", [1, 2, -0.5, 0.3])
@pytest.mark.parametrize("other", ["tensor", "scalar", "bias"])
def test_alpha(op, dtype, alpha, other, launches, chain):
    torch.manual_seed(5)
    shape = (16, 6, 64) if dtype == torch.bfloat16 else (16, 64, 64)
    a = operand((torch.randn(shape, device=DEV) * 2).to(dtype), "int8_row")
    b = {"tensor": lambda: operand((torch.randn(shape, device=DEV)).to(dtype), "int8_tensor"), "scalar": lambda: 0.1,
         "bias": lambda: (torch.randn(64, device=DEV)).to(dtype)}[other]()
    chain_args = (a, b.expand(shape).contiguous()) if other == "bias" and dtype == torch.float16 else None
    compare_with_chain(getattr(F, op), (a, b), dict(alpha=alpha), act_quantizer(-5.0, 5.0), chain, chain_args)
    assert launches["binary_quantize"] == 2


@pytest.mark.parametrize("op", ["add", "sub", "mul", "div"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("other", [0.1, -3, 2.5, 0.0, 1e-3, float("inf")])
@pytest.mark.parametrize("a_form", ["plain", "int8_row"])
def test_scalar_other(op, dtype, other, a_form, launches, chain):
    torch.manual_seed(6)
    a = (torch.randn(SHAPE[dtype], device=DEV) * 2).to(dtype)
    if a_form == "plain":
        specials(a)
    compare_with_chain(getattr(F, op), (operand(a, a_form), other), {}, act_quantizer(-4.0, 4.0), chain)
    assert launches["binary_quantize"] == 2


SUFFIXES = [(shape, form) for shape in [(64,), (1, 64), (6, 64), (1, 6, 64)] for form in FORMS if not (form == "int8_row" and len(shape) == 1)]


@pytest.mark.parametrize("op", ["add", "mul", "div"])
@pytest.mark.parametrize("b_shape,b_form", SUFFIXES)
def test_suffix_broadcast(op, b_shape, b_form, launches, chain):
    torch.manual_seed(7)
    a = operand((torch.randn(5, 6, 64, device=DEV) * 2).to(torch.bfloat16), "int8_tensor")
    b = operand((torch.randn(b_shape, device=DEV) + 0.5).to(torch.bfloat16), b_form, lo=-2.0, hi=3.0)
    value = compare_with_chain(getattr(F, op), (a, b), {}, act_quantizer(-6.0, 6.0), chain)
    assert value.shape == (5, 6, 64)
    assert launches["binary_quantize"] == 2


def test_mul_by_a_number_without_an_output_quantizer_is_the_rescale(launches):
    qa = operand(torch.randn(16, 64, device=DEV).to(torch.bfloat16), "int8_tensor")
    got = F.mul(qa, 2.5, strict_quantization=False)
    assert isinstance(got, ff.QuantizedTensor) and torch.equal(got.raw_data, qa.raw_data)
    assert torch.equal(got.quant_args().scale, qa.quant_args().scale * 2.5)
    assert launches["binary_quantize"] == 0


# ---- sigmoid / GELU -------------------------------------------------------------------------------------------------------------------
ACTIVATIONS = [(F.sigmoid, {}), (F.gelu, {}), (F.gelu, dict(approximate="tanh"))]


@pytest.mark.parametrize("act", range(3), ids=["sigmoid", "gelu", "gelu_tanh"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("form", FORMS)
def test_activation_equals_the_reference_chain(act, dtype, form, launches, chain):
    torch.manual_seed(8)
    x = (torch.randn(SHAPE[dtype], device=DEV) * 3).to(dtype)
    if form == "plain":
        specials(x)
    fn, kwargs = ACTIVATIONS[act]
    compare_with_chain(fn, (operand(x, form),), kwargs, act_quantizer(-1.0, 2.5), chain)
    assert launches["activation_quantize"] == 2


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_activations_on_every_16_bit_pattern(dtype, launches, chain):
    x = torch.arange(-32768, 32768, dtype=torch.int32, device=DEV).to(torch.int16).view(dtype).view(-1, 256)
    for fn, kwargs in ACTIVATIONS:
        compare_with_chain(fn, (x,), kwargs, act_quantizer(-2.0, 2.0), chain)
    assert launches["activation_quantize"] == 6


# ---- softmax ----------------------------------------------------------------------------------------------------------------------------
def check_softmax_contract(got, want):
    """NaN where ATen has NaN; elsewhere at most 1 ulp with fewer than 1 % of the elements differing."""
    nan_g, nan_w = torch.isnan(got), torch.isnan(want)
    assert torch.equal(nan_g, nan_w)
    g, w = got[~nan_g], want[~nan_w]
    if not g.numel():
        return
    ulps = (ordered(g) - ordered(w)).abs()
    assert int(ulps.max()) <= 1
    assert float((ulps != 0).float().mean()) < 0.01


def softmax_against_chain(inp, oq, chain, **kwargs):
    value, quantized = run(F.softmax, inp, -1, oq=oq, **kwargs)
    with chain():
        want_value, want_q = run(F.softmax, inp, -1, oq=oq, **kwargs)
    assert value.dtype == want_value.dtype
    check_softmax_contract(value, want_value)
    with torch.no_grad():
        assert torch.equal(quantized.raw_data, oq(value).raw_data)  # exactly A1 of the value this call produced
    same = value == want_value
    assert torch.equal(quantized.raw_data[same], want_q.raw_data[same])
    return value


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("cols", [8, 64, 512, 520, 4096, 16384])
@pytest.mark.parametrize("form", FORMS)
def test_softmax_meets_the_contract(dtype, cols, form, launches, chain):
    torch.manual_seed(cols)
    x = (torch.randn(37, cols, device=DEV) * 2.5).to(dtype)
    softmax_against_chain(operand(x, form), act_quantizer(0.0, 0.5), chain)
    assert launches["softmax_quantize"] == 2


def test_softmax_rows_of_minus_inf_and_nan(launches, chain):
    x = torch.randn(6, 4, 128, device=DEV).to(torch.bfloat16)
    x[0, 0] = float("-inf")           # all -inf: NaN
    x[1, 2, :100] = float("-inf")     # masked positions: exact zeros
    x[2, 1, 7] = float("nan")         # NaN anywhere: the row is NaN
    x[3, 3, 5] = float("inf")         # +inf: NaN as well (inf - inf)
    value = softmax_against_chain(x, act_quantizer(0.0, 1.0), chain, dtype=torch.bfloat16)
    assert torch.isnan(value[0, 0]).all() and torch.isnan(value[2, 1]).all()
    assert not value[1, 2, :100].any() and not torch.isnan(value[1, 2]).any()
    assert launches["softmax_quantize"] == 2


# ---- the output quantizer: fused, or called on the value ------------------------------------------------------------------------------
def test_range_estimation_sees_the_value(launches, chain):
    torch.manual_seed(9)
    a = operand(torch.randn(64, 512, device=DEV).to(torch.bfloat16), "int8_tensor")
    b = operand(torch.randn(64, 512, device=DEV).to(torch.bfloat16), "int8_row")
    cases = [(F.add, (a, b), {}), (F.softmax, (a, -1), {}), (F.gelu, (b,), {})]
    for fn, args, kwargs in cases:
        got_q, want_q = [ff.nn.LinearQuantizer(8, symmetric=False, quantized_dtype=torch.int8, device=DEV) for _ in range(2)]
        with torch.no_grad(), ff.strict_quantization(False):
            with ff.estimate_ranges(got_q, ff.range_setting.running_minmax):
                got = fn(*args, **kwargs, output_quantizer=got_q)
            with chain(), ff.estimate_ranges(want_q, ff.range_setting.running_minmax):
                want = fn(*args, **kwargs, output_quantizer=want_q)
        if fn is not F.softmax:
            assert torch.equal(got.dequantize(), want.dequantize())
            assert torch.equal(got_q.scale, want_q.scale) and torch.equal(got_q.offset, want_q.offset)
        assert not got_q.has_uninitialized_params
    assert launches == {"binary_quantize": 1, "softmax_quantize": 1, "activation_quantize": 1}


# ---- the predicate declines: the reference chain runs, unchanged -------------------------------------------------------------------
def test_fallbacks_when_the_predicate_declines(launches, chain):
    torch.manual_seed(10)
    x = torch.randn(16, 64, device=DEV).to(torch.bfloat16)
    y = torch.randn(16, 64, device=DEV).to(torch.bfloat16)
    qx = operand(x, "int8_tensor")
    oq = act_quantizer(-3.0, 3.0)
    # a call without the strict_quantization keyword (the torch-function route's form)
    with torch.no_grad():
        assert not fused_elementwise.add_predicate(input=qx, other=y, alpha=1, output_quantizer=oq)
        assert fused_elementwise.add_predicate(input=qx, other=y, alpha=1, output_quantizer=oq, strict_quantization=False)
    tile = act_quantizer(torch.full((16,), -3.0, device=DEV), torch.full((16,), 3.0, device=DEV), granularity=ff.PerTile((4, 16)))
    with torch.no_grad(), ff.strict_quantization(False):                  # not on the device
        assert torch.equal(F.add(x.cpu(), y.cpu()), x.cpu() + y.cpu())
    declined = [
        (F.add, (x, y.half()), {}),                                        # value dtypes differ (ATen promotes)
        (F.add, (qx, torch.tensor(2.0, device=DEV)), {}),                  # a 0-dim other
        (F.add, (y[0], qx), {}),                                           # input is the broadcast side
        (F.mul, (x, y[:, :1]), {}),                                        # not a suffix broadcast
        (F.add, (x[:3, :3], y[:3, :3]), {}),                               # 9 elements
        (F.sigmoid, (tile(x),), {}),                                       # an input tiling the kernels do not take
        (F.mul, (qx, True), {}),                                           # a bool is not a number here
        (F.softmax, (qx, 0), {}),                                          # not the last dim
        (F.softmax, (qx, -1), dict(dtype=torch.float32)),                  # another dtype
        (F.softmax, (torch.randn(4, 36, device=DEV).to(torch.bfloat16), -1), {}),      # cols % 8
        (F.softmax, (torch.randn(2, 16392, device=DEV).to(torch.bfloat16), -1), {}),   # cols > 16384
        (F.gelu, (x.float(),), {}),                                        # fp32 values
    ]
    for fn, args, kwargs in declined:
        with torch.no_grad(), ff.strict_quantization(False):
            got = fn(*args, **kwargs, output_quantizer=oq)
            with chain():
                want = fn(*args, **kwargs, output_quantizer=oq)
        assert torch.equal(got.raw_data, want.raw_data), fn
    # grad mode with an operand that needs a gradient
    xg = x.clone().requires_grad_()
    with ff.strict_quantization(False):
        got = F.add(xg, y, output_quantizer=oq)
        with chain():
            want = F.add(xg, y, output_quantizer=oq)
    assert torch.equal(got.raw_data, want.raw_data)
    # strict mode: the calls the fallback rejects still raise its errors
    for fn, args in ((F.add, (x, y)), (F.add, (qx, y)), (F.softmax, (x, -1)), (F.sigmoid, (x,))):
        with pytest.raises(QuantizationError):
            fn(*args, output_quantizer=oq, strict_quantization=True)
    assert launches == {name: 0 for name in OPS}


def test_the_torch_function_route_launches_nothing_new(launches):
    x = torch.randn(16, 64, device=DEV).to(torch.bfloat16)
    qa, qb = operand(x, "int8_tensor"), operand(x.flip(0), "int8_tensor", lo=-2.0, hi=2.0)
    with ff.strict_quantization(False):
        got = [qa + qb, qa - qb, qa * qb, qa / qb, qa * 2, torch.softmax(qa, -1), torch.sigmoid(qa), torch.nn.functional.gelu(qa)]
    da, db = qa.dequantize(), qb.dequantize()
    want = [da + db, da - db, da * db, da / db, da * 2, torch.softmax(da, -1), torch.sigmoid(da), torch.nn.functional.gelu(da)]
    for g, w in zip(got, want):
        assert type(g) is torch.Tensor and same_with_nan(g, w)
    with ff.strict_quantization(True):
        for fn in (lambda: qa + qb, lambda: qa * 2, lambda: torch.softmax(qa, -1), lambda: torch.sigmoid(qa)):
            with pytest.raises(QuantizationError):
                fn()
    assert launches == {name: 0 for name in OPS}


# ---- hipGraph -----------------------------------------------------------------------------------------------------------------------
def test_fused_elementwise_calls_capture_and_replay(launches):
    torch.manual_seed(12)
    x = torch.randn(64, 1024, device=DEV).to(torch.bfloat16)
    qa, qb = operand(x, "int8_tensor"), operand(x.flip(0), "int8_row")
    bias = torch.randn(1024, device=DEV).to(torch.bfloat16)
    oq = act_quantizer(-3.0, 3.0)

    def step():
        with torch.no_grad(), ff.strict_quantization(False):
            r = F.add(qa, qb, output_quantizer=oq)
            s = F.softmax(F.add(r.dequantize(), bias, alpha=0.5), -1, output_quantizer=oq)
            return r, s, F.gelu(qb, "tanh", output_quantizer=oq)

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
    assert launches == {"binary_quantize": 4, "softmax_quantize": 2, "activation_quantize": 2}


# ---- full size ---------------------------------------------------------------------------------------------------------------------
def test_full_size_shapes(launches, chain):
    torch.manual_seed(13)
    oq = act_quantizer(-4.0, 4.0)

    def codes(fn, *args, **kwargs):
        with torch.no_grad(), ff.strict_quantization(False):
            got = fn(*args, output_quantizer=oq, **kwargs).raw_data
            with chain():
                want = fn(*args, output_quantizer=oq, **kwargs).raw_data
        assert torch.equal(got, want), fn
        return got

    # residual add of int8 codes with different scales -> int8
    h = torch.randn(16384, 4096, device=DEV).to(torch.bfloat16)
    ra, rb = act_quantizer(-4.0, 4.0)(h), act_quantizer(-2.0, 3.0)(h.flip(1))
    codes(F.add, ra, rb)
    del ra, rb
    # bias add [16384, 4096] + [4096] bf16 -> int8
    codes(F.add, h, torch.randn(4096, device=DEV).to(torch.bfloat16))
    del h
    # sigmoid and GELU [16384, 16384] bf16 -> int8
    y = (torch.randn(16384, 16384, device=DEV) * 3).to(torch.bfloat16)
    for fn, kwargs in ACTIVATIONS:
        codes(fn, y, **kwargs)
    del y
    # softmax [32768, 2048] bf16 -> int8: the contract
    s = (torch.randn(32768, 2048, device=DEV) * 3).to(torch.bfloat16)
    softmax_against_chain(s, act_quantizer(0.0, 0.25), chain)
    assert launches == {"binary_quantize": 2, "softmax_quantize": 2, "activation_quantize": 3}
