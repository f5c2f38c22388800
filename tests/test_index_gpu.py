"""The one-pass index_add and permute kernels (csrc/ffq_index.hip) on the MI355X.

permute only moves data, so nothing is tolerated: value and codes equal the device reference chain's (dequantize, ``torch.permute``,
the output quantizer) bit for bit, with this package's registrations taken out of the dispatcher. index_add is held to its contract
(include/ffq_index.h): on operands whose fp32 partial sums are exact the value is the rounded float64 sum; with indices that are all
different value and codes are the chain's bit for bit; with repeated indices the value is within the fp32 left-to-right bound of the
float64 sum — for a row with m addends ``|got - exact| <= ulp_T(exact) / 2 + m * 2^-24 * (|in| + sum |addend_j|)`` — the fused codes
are A1 of the launch's own value, and two launches agree in every bit. No test passes an index out of range.

Every test counts the calls of the two ``ops`` entry points, so a silent fallback fails it."""

import contextlib
import ctypes

import pytest
import torch

import fastforward_amd as ff

from conftest import golden
from fastforward_amd import dispatcher, fused_index, ops
from fastforward_amd._cabi import DType, FanOut, Status
from fastforward_amd.nn import functional as F
from layouts import Layout, every
from test_index_cpu import g29_quantizer, run_code_level, run_g29
from test_modules_gpu import act_quantizer

pytestmark = pytest.mark.gpu
DEV = "cuda"
OPS = ("index_add_quantize", "permute_quantize")
DTYPES = [torch.bfloat16, torch.float16]
MANTISSA = {torch.bfloat16: 7, torch.float16: 10}
MARGIN = 4096


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
    """A context in which the dispatcher has none of this package's index_add / permute kernels: the reference chain runs."""

    @contextlib.contextmanager
    def off():
        with monkeypatch.context() as m:
            for op in ("index_add", "permute"):
                kept = [it for it in dispatcher._DISPATCHER.get(op, []) if getattr(it.fn, "__self__", None) is not fused_index.KERNELS]
                m.setitem(dispatcher._DISPATCHER, op, kept)
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
    return value


def out_quantizers(count=2):
    return [act_quantizer(lo, hi) for lo, hi in ((-6.0, 7.0), (-2.0, 9.0), (-9.0, 1.5))[:count]]


def operand(x, form, lo=-4.0, hi=5.0, bits_=8, axis=None):
    """`x` plain, or as codes of `bits_` in an int8 or value-dtype container, per tensor or per channel along `axis`."""
    if form == "plain":
        return x
    container = torch.int8 if form == "int8" else x.dtype
    with torch.no_grad():
        if axis is not None:
            per = x.float().movedim(axis, 0).reshape(x.shape[axis], -1)
            return act_quantizer(per.amin(-1).clamp(max=-0.5), per.amax(-1).clamp(min=0.5), granularity=ff.PerChannel(axis), container=container, bits=bits_)(x)
        return act_quantizer(lo, hi, container=container, bits=bits_)(x)


def shaped(outer, R, inner):
    """(shape, dim) of a tensor whose view along `dim` is [outer, R, inner]: dim first, last or in the middle."""
    if outer == 1 and inner == 1:
        return (R,), 0
    if outer == 1:
        return (R, inner), 0
    if inner == 1:
        return (outer, R), -1
    return (outer, R, inner), 1


def with_rows(shape, dim, n):
    out = list(shape)
    out[dim] = n
    return tuple(out)


# ---- index_add 1. the exact form ---------------------------------------------------------------------------------------------------
# (outer, R, inner, n, index dtype, how the index is drawn)
EXACT = [
    (1, 5, 8, 13, torch.int64, "random"), (3, 70, 264, 300, torch.int32, "random"), (3, 5, 7, 13, torch.int32, "random"),
    (1, 70, 9, 300, torch.int64, "random"), (3, 70, 1, 300, torch.int64, "random"), (1, 1, 8, 1, torch.int32, "random"),
    (3, 1, 264, 13, torch.int64, "random"), (1, 5, 1, 0, torch.int64, "random"), (3, 5, 9, 1, torch.int64, "random"),
    (1, 70, 8, 300, torch.int32, "one row"), (3, 70, 7, 300, torch.int64, "one row"), (3, 5, 264, 0, torch.int32, "random"),
    (1, 70, 264, 13, torch.int64, "few rows"), (3, 70, 8, 13, torch.int32, "few rows"), (1, 70, 1, 300, torch.int32, "random"),
    (3, 1, 1, 300, torch.int64, "random"), (1, 5, 7, 300, torch.int64, "random"), (3, 70, 9, 1, torch.int32, "random"),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", EXACT, ids=[f"{o}x{r}x{i}-n{n}-{str(t)[6:]}-{k.replace(' ', '_')}" for o, r, i, n, t, k in EXACT])
def test_exact_operands_give_the_rounded_float64_sum(case, dtype, launches):
    outer, R, inner, n, index_dtype, kind = case
    g = torch.Generator().manual_seed(outer * 1000 + R * 10 + inner + n)
    shape, dim = shaped(outer, R, inner)
    # small integers times 2^-2: every product by alpha = 0.5 and every fp32 partial sum (|sum| <= 301 * 8) is exact
    x = (torch.randint(-32, 33, shape, generator=g) * 0.25).to(dtype)
    src = (torch.randint(-32, 33, with_rows(shape, dim, n), generator=g) * 0.25).to(dtype)
    if kind == "one row":
        index = torch.full((n,), R // 2)
    elif kind == "few rows":
        index = torch.randint(0, R, (3,), generator=g)[torch.randint(0, 3, (n,), generator=g)]
    else:
        index = torch.randint(0, R, (n,), generator=g)
    if kind != "random" and R > 3:
        assert index.unique().numel() < R  # rows with no source
    for alpha in (1, 0.5):
        exact = torch.index_add(x.double(), dim, index, src.double(), alpha=alpha)
        want = exact.float().to(dtype)
        with torch.no_grad():
            got = F.index_add(x.to(DEV), dim, index.to(DEV, index_dtype), src.to(DEV), alpha, strict_quantization=False)
        same_tensor(got.cpu(), want)
    assert launches["index_add_quantize"] == 2


# ---- index_add 2. indices that are all different: the chain's bits -----------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("alpha", [1, 0.5, -2])
@pytest.mark.parametrize("shape,dim,n,forms", [((3, 70, 264), 1, 70, ("int8", "int8")), ((70, 9), 0, 40, ("plain", "container")),
                                               ((3, 70), -1, 33, ("int8", "plain")), ((5, 8), 0, 5, ("plain", "plain"))])
def test_unique_indices_equal_the_chain(shape, dim, n, forms, alpha, dtype, launches, chain):
    torch.manual_seed(n)
    x = operand((torch.randn(shape, device=DEV) * 2).to(dtype), forms[0])
    src = operand((torch.randn(with_rows(shape, dim, n), device=DEV) * 2).to(dtype), forms[1], -3.0, 3.0, 6)
    index = torch.randperm(shape[dim], device=DEV)[:n]  # a permutation (n == rows), or a part of one
    compare(lambda q: F.index_add(x, dim, index, src, alpha, output_quantizer=q), [None] + out_quantizers(2), chain)
    assert launches["index_add_quantize"] == 3


# ---- index_add 3. repeated indices: the bound, the codes, determinism --------------------------------------------------------------
def exact_and_bound(x, dim, index, src, alpha, dtype):
    """(float64 sum, the contract's bound) from the dequantized operands (host tensors of `dtype`)."""
    a = torch.tensor(float(alpha), dtype=torch.float32).to(dtype)
    addend = (src.float() * a.float()).to(dtype)  # (the fp32 product of two values of T is exact: one rounding, as the kernel's)
    exact = torch.index_add(x.double(), dim, index, addend.double())
    mass = torch.index_add(x.double().abs(), dim, index, addend.double().abs())
    m = torch.bincount(index, minlength=x.shape[dim]).double()
    m = m.reshape([-1 if d == dim % x.dim() else 1 for d in range(x.dim())])
    half_ulp = torch.where(exact == 0, torch.zeros_like(exact), torch.ldexp(torch.ones_like(exact), torch.frexp(exact).exponent - 1 - MANTISSA[dtype] - 1))
    return exact, half_ulp + m * 2.0**-24 * mass


def within_bound(got, x, dim, index, src, alpha, dtype, what=""):
    exact, bound = exact_and_bound(x, dim, index, src, alpha, dtype)
    err = (got.double() - exact).abs()
    print(f"{what} max err / bound {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} of {err.numel()} elements beyond the bound"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,dim,n,alpha,forms", [((3, 70, 264), 1, 300, 0.5, ("int8", "int8")), ((70, 9), 0, 300, -2, ("plain", "container")),
                                                     ((3, 70), -1, 300, 1, ("int8", "plain")), ((24, 64), 0, 48, 1, ("plain", "int8"))])
def test_repeated_indices_stay_within_the_fp32_bound(shape, dim, n, alpha, forms, dtype, launches):
    torch.manual_seed(n + len(shape))
    x = operand((torch.randn(shape, device=DEV) * 2).to(dtype), forms[0])
    src = operand((torch.randn(with_rows(shape, dim, n), device=DEV) * 2).to(dtype), forms[1], -3.0, 3.0, 6)
    index = torch.randint(0, shape[dim], (n,), device=DEV)
    index[: n // 3] = shape[dim] // 2  # a long row
    q1, q2 = out_quantizers(2)
    with torch.no_grad(), ff.strict_quantization(False):
        value = F.index_add(x, dim, index, src, alpha)
        again = F.index_add(x, dim, index, src, alpha)
        coded = F.index_add(x, dim, index, src, alpha, output_quantizer=q1)
        (xd, x_deq), (sd, s_deq) = fused_index.KERNELS._dequant(x), fused_index.KERNELS._dequant(src)
        _, both = ops.index_add_quantize(xd, dim, index, sd, alpha, quantizers=[(q1.scale, q1.offset), (q2.scale, q2.offset)], dtype=dtype,
                                         dequant=x_deq, source_dequant=s_deq, want_value=False)
        assert torch.equal(bits(value), bits(again))  # two launches, the same bits
        same_quantized(coded, q1(value))               # the fused codes are A1 of the launch's own value
        assert torch.equal(both[0], q1(value).raw_data) and torch.equal(both[1], q2(value).raw_data)  # two quantizers, one launch
        deq = [t.dequantize() if isinstance(t, ff.QuantizedTensor) else t for t in (x, src)]
    within_bound(value.cpu(), deq[0].cpu(), dim, index.cpu(), deq[1].cpu(), alpha, dtype, f"{shape} n={n}")
    assert launches["index_add_quantize"] == 4


# ---- index_add / permute / code-level 4. G29 on the device ---------------------------------------------------------------------------
G29 = golden("g29_index.pt")
G29_BF16 = [c for c in G29["cases"] if c["dtype"] == "torch.bfloat16"]
SHARES = {"codes": 0, "differ from the reference": 0, "reference differs from float64": 0, "kernel differs from float64": 0}


def same_as_recorded(got, want):
    if want["type"] == "Tensor":
        same_tensor(got.cpu(), want["value"], contiguous=False)
    else:
        assert isinstance(got, ff.QuantizedTensor) and torch.equal(got.raw_data.cpu(), want["codes"])
        assert torch.equal(bits(got.dequantize().cpu()), bits(want["dequantized"]))


@pytest.mark.parametrize("index", range(len(G29_BF16)), ids=[c["name"] for c in G29_BF16])
def test_the_fixture_on_the_device(index, launches):
    case = G29_BF16[index]
    plain, quantized = run_g29(case, DEV)
    if case["op"] == "permute":
        same_as_recorded(plain, case["plain"])
        same_as_recorded(quantized, case["quantized"])
        assert launches["permute_quantize"] == 1 and launches["index_add_quantize"] == 0  # (without a quantizer: a view, the fallback's)
        return
    assert launches["index_add_quantize"] == 2
    if " unique " in case["name"]:
        same_as_recorded(plain, case["plain"])
        same_as_recorded(quantized, case["quantized"])
        return
    # repeated indices: the reference rounds to bf16 after every addend, the kernel once
    host_plain, _ = run_g29(case)  # the host path restates the reference bit for bit (tests/test_index_cpu.py)
    assert torch.equal(bits(host_plain), bits(case["plain"]["value"]))
    with torch.no_grad():
        deq = [x if slot is None else g29_quantizer(slot, got)(x).dequantize() for x, slot, got in zip(case["inputs"], case["slots"], case["params"])]
    dim, alpha = case["kwargs"]["dim"], case["kwargs"]["alpha"]
    within_bound(plain.cpu(), deq[0], dim, case["index"], deq[1], alpha, torch.bfloat16, case["name"])
    exact, _ = exact_and_bound(deq[0], dim, case["index"], deq[1], alpha, torch.bfloat16)
    with torch.no_grad():
        ideal = g29_quantizer(case["out_slot"], case["out_params"])(exact.float()).raw_data
    SHARES["codes"] += ideal.numel()
    SHARES["differ from the reference"] += int((quantized.raw_data.cpu() != case["quantized"]["codes"]).sum())
    SHARES["reference differs from float64"] += int((case["quantized"]["codes"] != ideal).sum())
    SHARES["kernel differs from float64"] += int((quantized.raw_data.cpu() != ideal).sum())
    print("G29 repeated-index codes so far:", SHARES)
    # inside the output quantizer's range (-6, 7) half a bf16 ulp is at most 2^-6, a third of its step 13 / 255, and beyond it both
    # codes clamp: a value within the bound moves a code by one step at most
    assert int((quantized.raw_data.cpu().int() - ideal.int()).abs().max()) <= 1


@pytest.mark.parametrize("index", range(len(G29["code_level"])), ids=[c["name"] for c in G29["code_level"]])
def test_the_code_level_fixture_on_the_device(index):
    case = G29["code_level"][index]
    dtype = torch.bfloat16 if case["dtype"] == "torch.bfloat16" else torch.float32
    with ff.strict_quantization(True):
        q, got, raw = run_code_level(case, DEV, dtype)
    values = got.values if isinstance(got, torch.return_types.topk) else got
    assert isinstance(values, ff.QuantizedTensor) and values.quantization_context is q.quantization_context and values.is_cuda
    assert torch.equal(values.raw_data.cpu(), case["result"]["codes"])
    if case["indices"] is not None:
        assert torch.equal(got.indices.cpu(), case["indices"])


# ---- index_add 5. layouts and parameters -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", every(2), ids=[layout.id for layout in every(2)])
@pytest.mark.parametrize("which", ["input", "source", "both"])
def test_views_of_the_operands(which, layout, launches, chain):
    torch.manual_seed(5)
    x, src = (torch.randn(6, 10, 16, device=DEV) * 2).bfloat16(), (torch.randn(6, 7, 16, device=DEV) * 2).bfloat16()
    qx, qs = operand(x, "int8"), operand(src, "container", 40.0, 49.0)  # (|rne(offset)| is about 1260: beyond int8)
    viewed = lambda q: ff.QuantizedTensor(layout.make(q.raw_data), q.quantization_context)  # noqa: E731  (the codes in the view)
    if which in ("input", "both"):
        x, qx = layout.make(x), viewed(qx)
    if which in ("source", "both"):
        src, qs = layout.make(src), viewed(qs)
    index = torch.randperm(10, device=DEV)[:7]
    for a, b in ((qx, qs), (x, qs), (qx, src)):
        compare(lambda q: F.index_add(a, 1, index, b, 0.5, output_quantizer=q), [None] + out_quantizers(1), chain)
    assert launches["index_add_quantize"] == 6


@pytest.mark.parametrize("kind", ["offset", "strided"])
@pytest.mark.parametrize("index_dtype", [torch.int32, torch.int64])
def test_views_of_the_index(index_dtype, kind, launches, chain):
    torch.manual_seed(6)
    x, src = operand((torch.randn(12, 24, device=DEV) * 2).bfloat16(), "int8"), (torch.randn(7, 24, device=DEV) * 2).bfloat16()
    perm = torch.randperm(12, device=DEV)[:7].to(index_dtype)
    if kind == "offset":
        index = Layout("offset", index_dtype.itemsize).make(perm)
    else:
        index = torch.stack([perm, perm.flip(0)], 1)[:, 0]
        assert index.stride(0) == 2
    compare(lambda q: F.index_add(x, 0, index, src, -2, output_quantizer=q), [None] + out_quantizers(1), chain)
    assert launches["index_add_quantize"] == 2


# ---- index_add 6. declines -----------------------------------------------------------------------------------------------------------
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
    assert launches == {name: 0 for name in OPS}


def test_index_add_declines(launches, chain):
    torch.manual_seed(7)
    x, src = (torch.randn(4, 6, 8, device=DEV) * 2).bfloat16(), (torch.randn(4, 3, 8, device=DEV) * 2).bfloat16()
    index = torch.tensor([5, 0, 2], device=DEV)
    with torch.no_grad():
        _declines(lambda q: F.index_add(operand(x, "int8", axis=1), 1, index, src, output_quantizer=q), launches, chain)       # per channel
        _declines(lambda q: F.index_add(x, 1, index.reshape(1, 3), src, output_quantizer=q), launches, chain)                  # a 2-D index
        _declines(lambda q: F.index_add(x, 1, index, src, torch.tensor(2.0), output_quantizer=q), launches, chain)             # a tensor alpha
        _declines(lambda q: F.index_add(x.float(), 1, index, src.float(), output_quantizer=q), launches, chain)                # fp32
        _declines(lambda q: torch.index_add(operand(x, "int8"), 1, index, src), launches, chain)                               # not ff.nn.functional
    leaf = x.clone().requires_grad_()
    _declines(lambda q: F.index_add(leaf, 1, index, src, output_quantizer=q), launches, chain)                                  # a gradient is needed
    with ff.strict_quantization(False):
        F.index_add(leaf, 1, index, src).float().sum().backward()
    assert leaf.grad is not None and launches == {name: 0 for name in OPS}


# ---- index_add 7. guard bands ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inner", [264, 9, 1])
def test_index_add_guard_bands(inner, launches):
    """`out` and the codes sit inside larger buffers filled with a poison byte; two runs with two poisons: the margins keep their
    poison (no stray write), and the runs agree on every output byte (none left unwritten)."""
    outer, R, n = 3, 70, 300
    g = torch.Generator().manual_seed(8)
    x = (torch.randn(outer, R, inner, generator=g) * 2).bfloat16().to(DEV)
    src = torch.randint(-128, 128, (outer, n, inner), generator=g, dtype=torch.int8).to(DEV)
    ss, so = torch.tensor([0.02], device=DEV), torch.tensor([3.0], device=DEV)
    index = torch.randint(0, R, (n,), generator=g).to(DEV)
    qs = torch.tensor([0.05], device=DEV)
    numel = outer * R * inner
    lib = ops._native.library()
    stream = torch.cuda.current_stream().cuda_stream
    results = []
    for poison in (0x5A, 0xA5):
        out_buf = torch.full((MARGIN + 2 * numel + MARGIN,), poison, dtype=torch.uint8, device=DEV)
        code_buf = torch.full((MARGIN + numel + MARGIN,), poison, dtype=torch.uint8, device=DEV)
        fan = FanOut.make(8.0, [qs.data_ptr()], [None], [code_buf.data_ptr() + MARGIN])
        rc = lib.ffq_index_add_quantize(x.data_ptr(), int(DType.BF16), None, None, index.data_ptr(), int(DType.I64), n, src.data_ptr(), int(DType.I8),
                                        ss.data_ptr(), so.data_ptr(), 0.5, int(DType.BF16), outer, R, inner, out_buf.data_ptr() + MARGIN, fan, stream)
        assert rc == Status.OK, lib.ffq_last_error()
        torch.cuda.synchronize()
        for buf, size in ((out_buf, 2 * numel), (code_buf, numel)):
            assert bool((buf[:MARGIN] == poison).all()) and bool((buf[MARGIN + size:] == poison).all())
        results.append((out_buf[MARGIN:MARGIN + 2 * numel].clone(), code_buf[MARGIN:MARGIN + numel].clone()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    value, codes = ops.index_add_quantize(x, 1, index, src, 0.5, quantizers=[(qs, None)], dtype=torch.bfloat16, source_dequant=(ss, so))
    assert torch.equal(results[0][0], value.reshape(-1).view(torch.uint8)) and torch.equal(results[0][1], codes[0].reshape(-1).view(torch.uint8))
    assert launches["index_add_quantize"] == 1


# ---- permute 1. the chain's bits -------------------------------------------------------------------------------------------------------
PERMUTES = [
    ((1, 1), (1, 0)), ((31, 33), (1, 0)), ((65, 64), (1, 0)), ((2, 5, 7), (2, 1, 0)), ((2, 3, 5, 7), (0, 2, 3, 1)), ((2, 5, 7, 3), (0, 3, 1, 2)),
    ((2, 3, 4, 9), (0, 2, 1, 3)), ((2, 3, 4, 8), (0, 2, 1, 3)), ((3, 2, 5, 40), (2, 0, 1, 3)), ((2, 3, 2, 4, 5), (0, 2, 3, 4, 1)),
    ((2, 3, 2, 2, 3, 5), (5, 0, 3, 1, 4, 2)), ((2, 3, 2, 2, 3, 8), (4, 1, 0, 3, 2, 5)), ((2, 3, 5, 7), (0, 1, 2, 3)), ((70, 130), (1, 0)),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["int8", "container", "plain"])
@pytest.mark.parametrize("shape,dims", PERMUTES, ids=[f"{s}->{d}".replace(" ", "") for s, d in PERMUTES])
def test_permute_equals_the_chain(shape, dims, form, dtype, launches, chain):
    torch.manual_seed(len(shape) + shape[-1])
    x = (torch.randn(shape, device=DEV) * 2).to(dtype)
    inputs = [operand(x, form)] + ([operand(x, form, axis=a) for a in range(len(shape))] if form != "plain" else [])
    for qx in inputs:  # per tensor, then PerChannel on each axis
        compare(lambda q: F.permute(qx, dims, output_quantizer=q), out_quantizers(1), chain)
    assert launches["permute_quantize"] == len(inputs)


@pytest.mark.parametrize("shape,dims,axis", [((2, 3, 5, 7), (0, 2, 3, 1), 1), ((2, 3, 4, 8), (0, 2, 1, 3), None), ((65, 64), (1, 0), 0)])
def test_permute_feeds_two_quantizers_from_one_launch(shape, dims, axis, launches):
    torch.manual_seed(9)
    qx = operand((torch.randn(shape, device=DEV) * 2).bfloat16(), "int8", axis=axis)
    q1, q2 = out_quantizers(2)
    k = fused_index.KERNELS
    with torch.no_grad():
        x, dequant = k._dequant(qx)
        value, codes = ops.permute_quantize(x, dims, quantizers=[(q1.scale, q1.offset), (q2.scale, q2.offset)], dtype=torch.bfloat16, dequant=dequant,
                                            param_axis=axis)
        want = qx.dequantize().permute(dims)
        same_tensor(value, want.contiguous())
        assert torch.equal(codes[0], q1(want).raw_data) and torch.equal(codes[1], q2(want).raw_data) and codes[0].is_contiguous()
    assert launches["permute_quantize"] == 1


@pytest.mark.parametrize("layout", every(2, channels_last=True), ids=[layout.id for layout in every(2, channels_last=True)])
def test_permute_of_views(layout, launches, chain):
    torch.manual_seed(10)
    x = layout.make((torch.randn(2, 6, 5, 8, device=DEV) * 2).bfloat16())
    for qx in (operand(x, "int8"), operand(x, "container", axis=1)):
        compare(lambda q: F.permute(qx, (0, 2, 3, 1), output_quantizer=q), out_quantizers(1), chain)
    assert launches["permute_quantize"] == 2


def test_permute_declines(launches, chain):
    torch.manual_seed(11)
    x = (torch.randn(2, 3, 5, 8, device=DEV) * 2).bfloat16()
    with torch.no_grad(), ff.strict_quantization(False):
        view = F.permute(operand(x, "int8"), (0, 2, 3, 1))                                                        # no output quantizer: a view
        assert not view.is_contiguous() and torch.equal(view, operand(x, "int8").dequantize().permute(0, 2, 3, 1))
        seven = operand((torch.randn(2, 1, 2, 3, 2, 1, 4, device=DEV)).bfloat16(), "int8")
        _declines(lambda q: F.permute(seven, (6, 5, 4, 3, 2, 1, 0), output_quantizer=q), launches, chain)         # rank 7
        _declines(lambda q: F.permute(x.float(), (0, 2, 3, 1), output_quantizer=q), launches, chain)              # fp32
        _declines(lambda q: operand(x, "int8").permute(0, 2, 3, 1), launches, chain)                              # not ff.nn.functional
    assert launches == {name: 0 for name in OPS}


@pytest.mark.parametrize("shape,dims", [((2, 3, 4, 8), (0, 2, 1, 3)), ((2, 3, 4, 9), (0, 2, 1, 3)), ((3, 65, 70), (0, 2, 1))])
def test_permute_guard_bands(shape, dims, launches):
    g = torch.Generator().manual_seed(12)
    x = torch.randint(-128, 128, shape, generator=g, dtype=torch.int8).to(DEV)
    xs, xo, qs = torch.rand(shape[1], generator=g).to(DEV) * 0.05 + 0.01, torch.full((shape[1],), 2.0, device=DEV), torch.tensor([0.05], device=DEV)
    numel = x.numel()
    lib = ops._native.library()
    stream = torch.cuda.current_stream().cuda_stream
    rank = len(shape)
    results = []
    for poison in (0x5A, 0xA5):
        out_buf = torch.full((MARGIN + 2 * numel + MARGIN,), poison, dtype=torch.uint8, device=DEV)
        code_buf = torch.full((MARGIN + numel + MARGIN,), poison, dtype=torch.uint8, device=DEV)
        fan = FanOut.make(8.0, [qs.data_ptr()], [None], [code_buf.data_ptr() + MARGIN])
        rc = lib.ffq_permute_quantize(x.data_ptr(), int(DType.I8), xs.data_ptr(), xo.data_ptr(), 1, int(DType.BF16), rank, (ctypes.c_int64 * rank)(*shape),
                                      (ctypes.c_int64 * rank)(*dims), out_buf.data_ptr() + MARGIN, fan, stream)
        assert rc == Status.OK, lib.ffq_last_error()
        torch.cuda.synchronize()
        for buf, size in ((out_buf, 2 * numel), (code_buf, numel)):
            assert bool((buf[:MARGIN] == poison).all()) and bool((buf[MARGIN + size:] == poison).all())
        results.append((out_buf[MARGIN:MARGIN + 2 * numel].clone(), code_buf[MARGIN:MARGIN + numel].clone()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    value, codes = ops.permute_quantize(x, dims, quantizers=[(qs, None)], dtype=torch.bfloat16, dequant=(xs, xo), param_axis=1)
    assert torch.equal(results[0][0], value.reshape(-1).view(torch.uint8)) and torch.equal(results[0][1], codes[0].reshape(-1).view(torch.uint8))
    assert launches["permute_quantize"] == 1


# ---- together: a sparse mixture-of-experts block under a graph ----------------------------------------------------------------------------
class MoE(torch.nn.Module):
    """4 experts, top-2: quantized router logits -> topk -> take_along_dim -> expert linears -> mul by the routing weight ->
    index_add combine. Every expert sees every token (static shapes: capturable); a token's weight is zero off its top-2."""

    def __init__(self, hidden=64, experts=4):
        super().__init__()
        self.router = torch.nn.Linear(hidden, experts, bias=False)
        self.experts = torch.nn.ModuleList(torch.nn.Linear(hidden, hidden, bias=False) for _ in range(experts))

    def forward(self, x, want_value=False):
        tokens, hidden = x.shape
        logits = self.router(x)                                                       # quantized [tokens, experts]
        probs = F.softmax(logits, -1, output_quantizer=self.prob_quantizer)
        top = torch.topk(logits, 2, dim=-1)                                           # on the codes
        assert isinstance(top.values, ff.QuantizedTensor)
        chosen = torch.take_along_dim(probs, top.indices, dim=1)                      # on the codes
        assert isinstance(chosen, ff.QuantizedTensor)
        weights = torch.zeros(tokens, len(self.experts), dtype=x.dtype, device=x.device).scatter(1, top.indices, chosen.dequantize())
        parts = []
        for e, expert in enumerate(self.experts):
            w = weights[:, e:e + 1].expand(tokens, hidden).contiguous()
            parts.append(F.mul(expert(x), w, output_quantizer=self.mul_quantizer))
        source = F.cat(parts, 0, output_quantizer=self.cat_quantizer)
        index = torch.arange(tokens, device=x.device).repeat(len(self.experts))
        zeros = torch.zeros(tokens, hidden, dtype=x.dtype, device=x.device)
        if want_value:
            return F.index_add(zeros, 0, index, source), source, index
        return F.index_add(zeros, 0, index, source, output_quantizer=self.out_quantizer)


def test_a_moe_block_captures_and_replays(launches):
    torch.manual_seed(13)
    model = MoE().to(DEV, torch.bfloat16)
    model = ff.quantize_model(model, extra_conversion=ff.nn.surrogate_quantized_modules(model))
    act = lambda: ff.nn.LinearQuantizer(8, symmetric=False, quantized_dtype=torch.int8, device=DEV)  # noqa: E731
    for layer in [model.router, *model.experts]:
        assert type(layer) is ff.nn.QuantizedLinear
        layer.input_quantizer, layer.output_quantizer = act(), act()
        layer.weight_quantizer = ff.nn.LinearQuantizer(8, granularity=ff.PerChannel(0), quantized_dtype=torch.int8, device=DEV)
    model.prob_quantizer, model.mul_quantizer, model.cat_quantizer, model.out_quantizer = act(), act(), act(), act()
    x = torch.randn(24, 64, device=DEV, dtype=torch.bfloat16)

    def step(**k):
        with torch.no_grad(), ff.strict_quantization(False):
            return model(x, **k)

    with torch.no_grad(), ff.strict_quantization(False), ff.estimate_ranges(model, ff.range_setting.running_minmax):
        model(x)
    before = launches["index_add_quantize"]
    step()  # (the first call outside the capture)
    assert launches["index_add_quantize"] - before == 1
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side), torch.cuda.graph(g, stream=side):
        out = step()
    torch.cuda.current_stream().wait_stream(side)
    x.copy_(x.flip(0) * 0.5)  # fresh contents in the captured input
    eager = step().raw_data.clone()
    for _ in range(2):
        out.raw_data.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.raw_data, eager) and bool(eager.any())
    # the combine against float64: 4 addends per token row (two of them zero)
    value, source, index = step(want_value=True)
    within_bound(value.cpu(), torch.zeros(24, 64, dtype=torch.bfloat16), 0, index.cpu(), source.dequantize().detach().cpu(), 1, torch.bfloat16, "moe combine")
    assert launches["index_add_quantize"] - before == 4
