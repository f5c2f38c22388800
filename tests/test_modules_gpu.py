"""The one-pass LayerNorm / Embedding / ReLU / SiLU kernels (csrc/ffq_modules.hip) on the MI355X, against the device reference
chain — dequantize, the ATen op, the output quantizer — that the generated fallbacks run (reference _gen/fallback.py).

ReLU, SiLU and Embedding: the value is bit for bit the chain's, the codes are the output quantizer applied to it. LayerNorm: the
value is within 2 ulp of ATen's F.layer_norm on the same dequantized operands with fewer than 1 % of the elements differing (the
fp32 summation order is the kernel's own); the codes are exactly A1 of the value the call produced. Every test counts the calls of
the ``ops`` entry points, so a silent fallback fails it."""

import pytest
import torch

import fastforward_amd as ff

from conftest import golden
from fastforward_amd import dispatcher, ops
from fastforward_amd.nn import functional as F
from helpers import same_with_nan
from test_modules_cpu import install_quantizers, quantize_tiny, run_g19_case, tiny_opt

pytestmark = pytest.mark.gpu
DEV = "cuda"
OPS = ("layer_norm_quantize", "embedding_quantize", "pointwise_quantize")


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
def no_fused_modules(monkeypatch):
    """A context in which the dispatcher has no kernel for the four ops: the reference chain runs."""
    import contextlib

    @contextlib.contextmanager
    def off():
        with monkeypatch.context() as m:
            for op in ("layer_norm", "embedding", "relu", "silu"):
                m.setitem(dispatcher._DISPATCHER, op, [])
            yield

    return off


def act_quantizer(lo, hi, granularity=None, container=torch.int8, bits=8):
    q = ff.nn.LinearQuantizer(bits, symmetric=False, granularity=granularity or ff.PerTensor(), quantized_dtype=container, device=DEV)
    q.quantization_range = (torch.as_tensor(lo, dtype=torch.float32, device=DEV), torch.as_tensor(hi, dtype=torch.float32, device=DEV))
    return q


def quantized_input(x, form):
    """The operand in one of the forms the kernels take."""
    if form == "plain":
        return x
    if form == "int8_tensor":
        return act_quantizer(-4.0, 5.0)(x)
    if form == "int8_row":
        lo, hi = x.float().amin(-1).clamp(max=-0.5).reshape(-1), x.float().amax(-1).clamp(min=0.5).reshape(-1)
        return act_quantizer(lo, hi, granularity=ff.PerChannel(tuple(range(x.dim() - 1))))(x)  # one pair per row of the last dim
    if form == "container_tensor":
        return act_quantizer(-4.0, 5.0, container=x.dtype)(x)
    raise ValueError(form)


def ordered(t):
    """16-bit patterns as integers ordered like the values (ulp distances across zero)."""
    i = t.contiguous().view(torch.int16).int()
    return torch.where(i < 0, -(i & 0x7FFF), i)


def check_layer_norm_contract(got, want):
    """NaN where ATen has NaN; elsewhere at most 2 ulp with fewer than 1 % of the elements differing. Values below 2^-6 come out
    of a cancellation (weight * normalised + bias with terms of order 1 here): one fp32 ulp of the mean or rstd is many bf16 ulps
    of such a value, so there the bound is 2^-14 absolute."""
    nan_g, nan_w = torch.isnan(got), torch.isnan(want)
    assert torch.equal(nan_g, nan_w)
    g, w = got[~nan_g], want[~nan_w]
    if not g.numel():
        return
    ulps = (ordered(g) - ordered(w)).abs()
    small = w.float().abs() < 2.0**-6
    assert int(ulps[~small].max()) <= 2 if bool((~small).any()) else True
    assert float((g.float() - w.float())[small].abs().max()) <= 2.0**-14 if bool(small.any()) else True
    assert float((ulps != 0).float().mean()) < 0.01


def run(fn, *args, oq, **kwargs):
    with torch.no_grad(), ff.strict_quantization(False):
        value = fn(*args, output_quantizer=None, **kwargs)
        quantized = fn(*args, output_quantizer=oq, **kwargs)
    return value, quantized


# ---- ReLU / SiLU --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["relu", "silu"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("form", ["plain", "int8_tensor", "int8_row", "container_tensor"])
@pytest.mark.parametrize("shape", [(37, 264), (3, 5, 8)])
def test_pointwise_equals_the_reference_chain(op, dtype, form, shape, launches, no_fused_modules):
    torch.manual_seed(7)
    x = (torch.randn(shape, device=DEV) * 3).to(dtype)
    if form == "plain":
        flat = x.view(-1)
        flat[:6] = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0, 0.0, -1e-30], device=DEV).to(dtype)
    inp = quantized_input(x, form)
    oq = act_quantizer(-1.0, 2.5)  # values above 2.5 clamp
    fn = getattr(F, op)
    value, quantized = run(fn, inp, oq=oq)
    assert launches["pointwise_quantize"] == 2
    with no_fused_modules():
        want_value, want_q = run(fn, inp, oq=oq)
    assert launches["pointwise_quantize"] == 2
    assert value.dtype == dtype and same_with_nan(value, want_value)
    assert isinstance(quantized, ff.QuantizedTensor) and torch.equal(quantized.raw_data, want_q.raw_data)
    assert torch.equal(quantized.dequantize(), want_q.dequantize())


def test_silu_on_every_bf16_pattern_and_the_table_form(launches, no_fused_modules):
    """All 65536 bf16 values, repeated until the launch takes the LDS-table kernel (>= 1M chunks)."""
    patterns = torch.arange(-32768, 32768, dtype=torch.int32, device=DEV).to(torch.int16).view(torch.bfloat16)
    for reps in (1, 130):
        x = patterns.repeat(reps).view(-1, 256)
        oq = act_quantizer(-4.0, 4.0)
        value, quantized = run(F.silu, x, oq=oq)
        with no_fused_modules():
            want_value, want_q = run(F.silu, x, oq=oq)
        assert same_with_nan(value, want_value) and torch.equal(quantized.raw_data, want_q.raw_data)
    assert launches["pointwise_quantize"] == 4


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("cols", [8, 40, 520, 2056, 4096, 16384])
@pytest.mark.parametrize("form", ["plain", "int8_tensor", "int8_row", "container_tensor"])
@pytest.mark.parametrize("affine", ["none", "both", "quantized_weight"])
def test_layer_norm_meets_the_contract(dtype, cols, form, affine, launches, no_fused_modules):
    torch.manual_seed(cols)
    rows = 37
    x = (torch.randn(rows, cols, device=DEV) * 1.5 + 0.25).to(dtype)
    inp = quantized_input(x, form)
    weight = bias = None
    if affine != "none":
        weight = (torch.rand(cols, device=DEV) + 0.5).to(dtype)
        bias = (torch.randn(cols, device=DEV) * 0.1).to(dtype)
    if affine == "quantized_weight":
        wq = ff.nn.LinearQuantizer(8, quantized_dtype=torch.int8, device=DEV)
        wq.quantization_range = (torch.tensor(-1.6, device=DEV), torch.tensor(1.6, device=DEV))
        weight = wq(weight)
    oq = act_quantizer(-2.0, 2.0)
    value, quantized = run(F.layer_norm, inp, (cols,), weight, bias, 1e-5, oq=oq)
    assert launches["layer_norm_quantize"] == 2
    with no_fused_modules():
        want_value, want_q = run(F.layer_norm, inp, (cols,), weight, bias, 1e-5, oq=oq)
    assert launches["layer_norm_quantize"] == 2
    assert value.dtype == dtype
    check_layer_norm_contract(value, want_value)
    with torch.no_grad():
        assert torch.equal(quantized.raw_data, oq(value).raw_data)  # exactly A1 of the value this call produced
    same = value == want_value
    assert torch.equal(quantized.raw_data[same], want_q.raw_data[same])


def test_layer_norm_over_several_dims_and_rows_with_nan_or_inf(launches, no_fused_modules):
    x = torch.randn(4, 6, 8, 16, device=DEV).to(torch.bfloat16)
    x[0, 1, 2, 3] = float("nan")
    x[1, 2, 0, 0] = float("inf")
    x[2, 3, 4, 5] = float("-inf")
    oq = act_quantizer(-2.0, 2.0)
    value, quantized = run(F.layer_norm, x, (8, 16), oq=oq)
    with no_fused_modules():
        want_value, _ = run(F.layer_norm, x, (8, 16), oq=oq)
    check_layer_norm_contract(value, want_value)
    assert launches["layer_norm_quantize"] == 2


# ---- Embedding ---------------------------------------------------------------------------------------------------------------------
GRANULARITIES = {"tensor": ff.PerTensor(), "row": ff.PerChannel(0), "column": ff.PerChannel(1), "group32": ff.PerBlock(1, 32, 0)}


def quantized_table(V, D, dtype, gran, container, seed=5):
    """A [V, D] table quantized by a symmetric 8-bit quantizer whose range is the table's own min / max per parameter tile."""
    gen = torch.Generator(DEV).manual_seed(seed)
    table = torch.randn(V, D, device=DEV, generator=gen).to(dtype)
    t = table.float()
    lo, hi = {
        "tensor": lambda: (t.amin(), t.amax()),
        "row": lambda: (t.amin(1), t.amax(1)),
        "column": lambda: (t.amin(0), t.amax(0)),
        "group32": lambda: (t.view(V, D // 32, 32).amin(-1).reshape(-1), t.view(V, D // 32, 32).amax(-1).reshape(-1)),
    }[gran]()
    del t
    q = ff.nn.LinearQuantizer(8, granularity=GRANULARITIES[gran], quantized_dtype=container or dtype, device=DEV)
    q.quantization_range = (lo, hi)
    with torch.no_grad():
        return q(table)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("gran", list(GRANULARITIES))
@pytest.mark.parametrize("container", [torch.int8, None])
@pytest.mark.parametrize("ids_dtype", [torch.int64, torch.int32])
def test_embedding_equals_the_reference_chain(dtype, gran, container, ids_dtype, launches, no_fused_modules):
    table = quantized_table(50, 96, dtype, gran, container)
    ids = torch.randint(0, 50, (3, 7, 5), device=DEV, dtype=ids_dtype)
    oq = act_quantizer(-1.5, 1.5)
    value, quantized = run(F.embedding, ids, table, oq=oq)
    assert launches["embedding_quantize"] == 2
    with no_fused_modules():
        want_value, want_q = run(F.embedding, ids, table, oq=oq)
    assert value.shape == (3, 7, 5, 96) and value.dtype == dtype and same_with_nan(value, want_value)
    assert torch.equal(quantized.raw_data, want_q.raw_data)


def test_embedding_flags_the_first_id_out_of_range():
    table = quantized_table(20, 64, torch.bfloat16, "row", torch.int8)
    p = table.quantization_context.quantization_params
    ids = torch.randint(0, 20, (16,), device=DEV)
    ids[5], ids[9] = 20, -1
    value, codes, bad = ops.embedding_quantize(ids, table.raw_data, p.scale, p.offset, True, 64, torch.bfloat16,
                                               [(torch.ones(1, device=DEV), None)])
    assert int(bad.item()) == 5
    assert not value[5].any() and not value[9].any() and not codes[0][5].any()
    good = torch.ones(16, dtype=torch.bool, device=DEV)
    good[5] = good[9] = False
    assert torch.equal(value[good], torch.nn.functional.embedding(ids[good], table.dequantize()))


# ---- the predicate declines: the reference chain runs, unchanged -------------------------------------------------------------------
def test_fallbacks_when_the_predicate_declines(launches, no_fused_modules):
    x = (torch.randn(16, 64, device=DEV)).to(torch.bfloat16)
    oq = act_quantizer(-2.0, 2.0)
    # grad mode with a quantizer whose parameters need gradients
    xq = act_quantizer(-4.0, 5.0)
    with ff.strict_quantization(False):
        got = F.relu(xq(x), output_quantizer=oq)
        with no_fused_modules():
            want = F.relu(xq(x), output_quantizer=oq)
    assert torch.equal(got.raw_data, want.raw_data)
    # max_norm on an embedding (it rewrites the table): the chain
    table = quantized_table(20, 64, torch.bfloat16, "row", torch.int8)
    ids = torch.randint(0, 20, (9,), device=DEV)
    with torch.no_grad(), ff.strict_quantization(False):
        got = F.embedding(ids, table, max_norm=1.0, output_quantizer=oq)
        with no_fused_modules():
            want = F.embedding(ids, table, max_norm=1.0, output_quantizer=oq)
    assert torch.equal(got.raw_data, want.raw_data)
    # an input tiling the kernels do not take (PerTile)
    tq = act_quantizer(torch.full((16,), -3.0, device=DEV), torch.full((16,), 3.0, device=DEV), granularity=ff.PerTile((4, 16)))
    with torch.no_grad(), ff.strict_quantization(False):
        got = F.layer_norm(tq(x), (64,), output_quantizer=oq)
        with no_fused_modules():
            want = F.layer_norm(tq(x), (64,), output_quantizer=oq)
    assert torch.equal(got.raw_data, want.raw_data)
    assert launches == {name: 0 for name in OPS}


# ---- hipGraph ----------------------------------------------------------------------------------------------------------------------
def test_a_fused_layer_norm_captures_and_replays(launches):
    torch.manual_seed(3)
    x = torch.randn(64, 1024, device=DEV).to(torch.bfloat16)
    xq = act_quantizer(-4.0, 4.0)(x)
    w = (torch.rand(1024, device=DEV) + 0.5).to(torch.bfloat16)
    oq = act_quantizer(-2.0, 2.0)

    def step():
        with torch.no_grad(), ff.strict_quantization(False):
            return F.layer_norm(xq, (1024,), w, None, 1e-5, output_quantizer=oq)

    eager = step().raw_data.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side), torch.cuda.graph(g, stream=side):
        out = step()
    torch.cuda.current_stream().wait_stream(side)
    out.raw_data.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.raw_data, eager)
    assert launches["layer_norm_quantize"] == 2


# ---- fixture G19 on the device -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(8))
def test_g19_on_the_device(index, launches):
    case = golden("g19_modules.pt")[index]
    value, quantized = run_g19_case(case, DEV)
    want = case["value"].to(DEV)
    if case["dtype"] != str(torch.bfloat16):
        return  # fp32 activations take the reference chain on the device (the kernels are built for bf16 / fp16)
    assert sum(launches.values()) == 2
    if case["op"] in ("relu", "embedding"):
        assert same_with_nan(value, want) and torch.equal(quantized.raw_data, case["codes"].to(DEV))
    else:  # silu against the host's ATen, layer_norm: the contract
        check_layer_norm_contract(value, want)
        same = value == want
        assert torch.equal(quantized.raw_data[same], case["codes"].to(DEV)[same])


# ---- full size ---------------------------------------------------------------------------------------------------------------------
def test_full_size_shapes(launches, no_fused_modules):
    torch.manual_seed(11)
    oq = act_quantizer(-2.0, 2.0)
    x = torch.randn(16384, 4096, device=DEV).to(torch.bfloat16)
    xq = act_quantizer(-4.0, 4.0)(x)
    w = (torch.rand(4096, device=DEV) + 0.5).to(torch.bfloat16)
    b = (torch.randn(4096, device=DEV) * 0.1).to(torch.bfloat16)
    value, quantized = run(F.layer_norm, xq, (4096,), w, b, 1e-5, oq=oq)
    with no_fused_modules():
        want_value, _ = run(F.layer_norm, xq, (4096,), w, b, 1e-5, oq=oq)
    check_layer_norm_contract(value, want_value)
    with torch.no_grad():
        assert torch.equal(quantized.raw_data, oq(value).raw_data)
    del x, xq, value, quantized, want_value
    y = (torch.randn(16384, 16384, device=DEV) * 3).to(torch.bfloat16)
    for fn in (F.relu, F.silu):
        with torch.no_grad(), ff.strict_quantization(False):
            got = fn(y, output_quantizer=oq).raw_data
            with no_fused_modules():
                want = fn(y, output_quantizer=oq).raw_data
        assert torch.equal(got, want)
        del got, want
    del y
    table = quantized_table(128256, 4096, torch.bfloat16, "row", torch.int8)
    ids = torch.randint(0, 128256, (16384,), device=DEV)
    with torch.no_grad(), ff.strict_quantization(False):
        got = F.embedding(ids, table, output_quantizer=oq).raw_data
        with no_fused_modules():
            want = F.embedding(ids, table, output_quantizer=oq).raw_data
    assert torch.equal(got, want)
    assert launches == {"layer_norm_quantize": 2, "embedding_quantize": 1, "pointwise_quantize": 2}


# ---- the tiny OPT-like model, end to end ---------------------------------------------------------------------------------------------
def test_tiny_opt_model_end_to_end(launches, no_fused_modules):
    model = quantize_tiny(tiny_opt(DEV, torch.bfloat16))
    install_quantizers(model, DEV)
    ids = torch.randint(0, 96, (4, 24), device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    with torch.no_grad(), ff.strict_quantization(False):
        with ff.estimate_ranges(model, ff.range_setting.running_minmax):
            model(ids)
        calibration = dict(launches)
        got = model(ids)
        with no_fused_modules():
            want = model(ids)
    forward = {k: launches[k] - calibration[k] for k in OPS}
    assert forward == {"layer_norm_quantize": 3, "embedding_quantize": 1, "pointwise_quantize": 3}
    assert isinstance(got, ff.QuantizedTensor) and got.raw_data.dtype == torch.int8
    g, w = got.dequantize().float(), want.dequantize().float()
    step = float(model.act.output_quantizer.scale)
    assert float((g - w).abs().max()) <= 4 * step
    assert float((got.raw_data != want.raw_data).float().mean()) < 0.02
