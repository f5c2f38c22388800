"""The quantized joining operators (cat, pad) without a GPU: the public names and the reference's signatures, the host path against
the reference's outputs (fixture G25), the reference's strict-mode errors, what the predicates decline, the code-level cat and how it
decides that parameters are equal, the two C-ABI entry points (exported by the HIP library, absent from the oracle, argument checks
before any device call) and what hipcc emitted for their kernels."""

import ctypes
import inspect
import sys

import pytest
import torch

import fastforward_amd as ff

from conftest import HIP_SO, ROOT, golden, load_oracle
from fastforward_amd import _cabi, fused_concat, fused_math
from fastforward_amd._cabi import CatInputs, DType, FanOut, FFQLibrary, Status
from fastforward_amd.exceptions import BackendError, QuantizationError
from fastforward_amd.quantization import _linear_quantized_ops as code_level

sys.path.insert(0, str(ROOT / "tools"))

import kernel_resources  # noqa: E402

F = ff.nn.functional
ENTRY_POINTS = ("ffq_cat_quantize", "ffq_pad_quantize")
OUTPUT_MSG = "'output_quantizer' must be provided if strict_quantization=True"
INPUT_MSG = "Expected 'input' to be an instance of 'QuantizedTensor' because strict_quantization=True."
ELEM_MSG = "Expected 'elem__' to be an instance of 'QuantizedTensor' because strict_quantization=True."
# the reference's signatures (_gen/operators.py:1290, 1383), as `str(inspect.signature(...))` of its functions with annotations dropped
REFERENCE_SIGNATURES = {
    "cat": "(tensors, dim=0, *, output_quantizer=None, strict_quantization=None)",
    "pad": "(input, pad, mode='...', value=None, *, output_quantizer=None, strict_quantization=None)",
}


def quantizer(spec):
    bits, symmetric, gran, lo, hi = spec
    granularity = ff.PerTensor() if gran == "tensor" else ff.PerChannel(gran[1])
    q = ff.nn.LinearQuantizer(bits, symmetric=symmetric, granularity=granularity, quantized_dtype=torch.int8)
    q.quantization_range = (torch.as_tensor(lo, dtype=torch.float32), torch.as_tensor(hi, dtype=torch.float32))
    return q


def _with_params(q, got):
    with torch.no_grad():
        q.scale.copy_(got["scale"])
        if got["offset"] is not None:
            q.offset.copy_(got["offset"])
    return q


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _unannotated(fn):
    sig = inspect.signature(fn)
    return str(sig.replace(parameters=[p.replace(annotation=inspect.Parameter.empty) for p in sig.parameters.values()],
                           return_annotation=inspect.Signature.empty))


# ---- 1. the names and the signatures ------------------------------------------------------------------------------------------------
def test_the_new_operators_are_public_with_the_reference_signatures():
    assert {"cat", "pad"} <= set(F.__all__) and callable(F.cat) and callable(F.pad)
    assert {"cat_quantize", "pad_quantize"} <= set(ff.ops.__all__)
    for name, want in REFERENCE_SIGNATURES.items():
        assert _unannotated(getattr(F, name)) == want
        params = inspect.signature(getattr(F, name)).parameters
        assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("output_quantizer", "strict_quantization"))


def test_pad_without_a_mode_raises_atens_error_as_in_the_reference():
    x = torch.randn(2, 3, 4)
    with pytest.raises(NotImplementedError) as got, ff.strict_quantization(False):
        F.pad(x, (1, 1))
    with pytest.raises(NotImplementedError) as want:
        torch.nn.functional.pad(x, (1, 1), mode="...")
    assert str(got.value) == str(want.value)


# ---- 2. the host path against the reference (G25) -----------------------------------------------------------------------------------
G25 = golden("g25_cat_pad.pt")


def _same(got, want, name):
    if want["type"] == "Tensor":
        assert type(got) is torch.Tensor, name
        value = want["value"]
        assert got.dtype == value.dtype and got.shape == value.shape and torch.equal(_bits(got), _bits(value)), name
        return
    assert isinstance(got, ff.QuantizedTensor), name
    assert got.raw_data.dtype == want["codes"].dtype and torch.equal(got.raw_data, want["codes"]), name
    assert torch.equal(_bits(got.dequantize()), _bits(want["dequantized"])), name
    p = got.quant_args()
    assert torch.equal(torch.as_tensor(p.scale).reshape(want["scale"].shape), want["scale"]), name
    assert (p.offset is None) == (want["offset"] is None), name
    if want["offset"] is not None:
        assert torch.equal(torch.as_tensor(p.offset).reshape(want["offset"].shape), want["offset"]), name


@pytest.mark.parametrize("index", range(len(G25)), ids=[c["name"] for c in G25])
def test_host_path_equals_the_reference_bit_for_bit(index):
    case = G25[index]
    shared = _with_params(quantizer(case["slots"][0]), case["params"][0]) if case["share"] else None
    args = []
    with torch.no_grad():
        for x, slot, got in zip(case["inputs"], case["slots"], case["params"]):
            q = shared if case["share"] else (None if slot is None else _with_params(quantizer(slot), got))
            args.append(x if q is None else q(x))
    oq = _with_params(quantizer(case["out_slot"]), case["out_params"])
    kwargs = case["kwargs"]
    with torch.no_grad(), ff.strict_quantization(False):
        if case["through_torch"]:
            _same(torch.cat(args, **kwargs), case["plain"], case["name"])
            return
        call = (lambda **k: F.cat(args, **kwargs, **k)) if case["op"] == "cat" else (lambda **k: F.pad(args[0], **kwargs, **k))
        _same(call(), case["plain"], case["name"])
        _same(call(output_quantizer=oq), case["quantized"], case["name"])


# ---- 3. the fixture ------------------------------------------------------------------------------------------------------------------
def test_the_fixture_covers_what_the_issue_lists():
    names = " ".join(c["name"] for c in G25)
    for needle in ("cat dim 0", "cat dim 1", "cat dim -1", "two inputs", "three inputs", "nine inputs", "all quantized", "mixed plain and quantized",
                   "same parameters", "torch.cat dim", "pad constant default value", "pad constant value -1.5", "negative pads", "1-D", "2-D", "3-D",
                   "reflect 1-D on 2-D", "reflect 1-D on 3-D", "reflect 2-D on 3-D", "reflect 2-D on 4-D", "reflect 3-D on 4-D", "reflect 3-D on 5-D",
                   "replicate 1-D on 2-D", "replicate 1-D on 3-D", "replicate 2-D on 3-D", "replicate 2-D on 4-D", "replicate 3-D on 4-D",
                   "replicate 3-D on 5-D", " plain ", " q ", " per-channel q "):
        assert needle in names, needle
    assert {c["dtype"] for c in G25} == {"torch.float32", "torch.bfloat16"}
    assert all(x.shape[-1] <= 16 for c in G25 for x in c["inputs"])
    same = [c for c in G25 if "same parameters" in c["name"]]
    # same parameters: the reference keeps codes without an output quantizer (also through torch.cat), and quantizes with one
    assert same and all(c["plain"]["type"] == "QuantizedTensor" for c in same)
    assert all(c["quantized"]["type"] == "QuantizedTensor" for c in same if not c["through_torch"])
    assert any(c["through_torch"] for c in same) and any(not c["share"] for c in same)
    mixed = [c for c in G25 if "mixed" in c["name"] or "all quantized" in c["name"]]
    assert mixed and all(c["plain"]["type"] == "Tensor" for c in mixed)
    assert any(len(c["inputs"]) == 9 for c in G25)


# ---- 4. strict quantization: the reference's messages (_gen/fallback.py) -------------------------------------------------------------
def _q(x):
    return quantizer((8, False, "tensor", -3.0, 3.0))(x)


def test_strict_mode_errors_match_the_reference():
    x, y = torch.randn(2, 3, 8), torch.randn(2, 3, 8)
    stub = ff.nn.QuantizerStub(output_quantizer=True)
    with pytest.raises(QuantizationError) as e:
        F.cat([x, y], 1, strict_quantization=True)
    assert str(e.value) == OUTPUT_MSG
    with pytest.raises(QuantizationError) as e:  # the output quantizer is checked first, as in the reference
        F.cat([_q(x), y], 1, strict_quantization=True)
    assert str(e.value) == OUTPUT_MSG
    with pytest.raises(QuantizationError) as e:
        F.cat([_q(x), y], 1, output_quantizer=stub, strict_quantization=True)
    assert str(e.value) == ELEM_MSG
    assert F.cat([_q(x), _q(y)], 1, output_quantizer=stub, strict_quantization=True) is not None
    with pytest.raises(QuantizationError) as e:
        F.pad(x, (1, 1), "constant", strict_quantization=True)
    assert str(e.value) == OUTPUT_MSG
    with pytest.raises(QuantizationError) as e:
        F.pad(x, (1, 1), "constant", output_quantizer=stub, strict_quantization=True)
    assert str(e.value) == INPUT_MSG
    assert F.pad(_q(x), (1, 1), "reflect", output_quantizer=stub, strict_quantization=True) is not None
    with ff.strict_quantization(True):  # the global flag is what None means
        with pytest.raises(QuantizationError) as e:
            F.cat([x, y])
        assert str(e.value) == OUTPUT_MSG


# ---- 5. the predicates ---------------------------------------------------------------------------------------------------------------
P = fused_concat


def _kw(**k):
    return dict(output_quantizer=None, strict_quantization=False, **k)


def test_the_predicates_decline_host_tensors_and_any_call_shape():
    x = torch.randn(2, 3, 8, 8, dtype=torch.bfloat16)
    assert not P.cat_predicate(tensors=[x, x], dim=1, **_kw())
    assert not P.pad_predicate(input=x, pad=(1, 1), mode="constant", value=None, **_kw())
    for pred in (P.cat_predicate, P.pad_predicate):
        assert not pred(x, x, 1, 2, 3, 4, out=x)  # any call signature, without raising
        assert not pred()
        assert not pred(x)


@pytest.fixture()
def on_device(monkeypatch):
    """The predicates' device check answered yes for host tensors: what else they decline is what they test."""
    for module in (fused_concat, fused_math):
        monkeypatch.setattr(module, "_on_device", lambda *t: True)


def test_what_the_cat_predicate_accepts_and_declines(on_device):
    cat = P.cat_predicate
    x, y = torch.randn(2, 3, 9, 14, dtype=torch.bfloat16), torch.randn(2, 5, 9, 14, dtype=torch.bfloat16)
    with torch.no_grad():
        qx, qy = _q(x), quantizer((8, False, "tensor", -2.0, 2.0))(y)
        qc = quantizer((8, False, ("channel", 1), torch.full((3,), -3.0), torch.full((3,), 3.0)))(x)
        assert cat(tensors=[x, y], dim=1, **_kw()) and cat(tensors=(qx, y, qy), dim=-3, **_kw()) and cat(tensors=[qx], dim=0, output_quantizer=quantizer((8, False, "tensor", -1.0, 1.0)),
                                                                                                         strict_quantization=False)
        assert cat(tensors=[x, x[..., :5]], dim=-1, **_kw())  # odd widths
        assert cat(tensors=[qx, qy] * 10, dim=1, **_kw())     # 20 inputs: three launches
        # calls without the strict_quantization keyword (torch.cat through __torch_function__)
        assert not cat(tensors=[qx, qy], dim=1, output_quantizer=None) and not cat([qx, qy], 1)
        # fp32, mixed dtypes, per-channel inputs, a [0] input, unequal ranks, sizes that disagree off dim, dim out of range or no int
        assert not cat(tensors=[x.float(), y.float()], dim=1, **_kw())
        assert not cat(tensors=[x, y.half()], dim=1, **_kw()) and not cat(tensors=[x, y.float()], dim=1, **_kw())
        assert not cat(tensors=[qc, y], dim=1, **_kw()) and not cat(tensors=[y, qc], dim=1, **_kw())
        assert not cat(tensors=[x, torch.zeros(0, dtype=torch.bfloat16)], dim=1, **_kw()) and not cat(tensors=[x, y[:, :0]], dim=1, **_kw())
        assert not cat(tensors=[x, y[0]], dim=1, **_kw()) and not cat(tensors=[x, y], dim=0, **_kw())
        assert not cat(tensors=[x, y], dim=4, **_kw()) and not cat(tensors=[x, y], dim=1.0, **_kw()) and not cat(tensors=[x, y], dim=True, **_kw())
        assert not cat(tensors=[], dim=0, **_kw()) and not cat(tensors=x, dim=0, **_kw()) and not cat(tensors=[x, None], dim=0, **_kw())
        # every input channels-last: ATen answers in channels-last. One of them is not enough
        cl = lambda t: t.contiguous(memory_format=torch.channels_last)  # noqa: E731
        assert not cat(tensors=[cl(x), cl(y)], dim=1, **_kw()) and cat(tensors=[cl(x), y], dim=1, **_kw())
        assert cat(tensors=[x.transpose(-1, -2), y.transpose(-1, -2)], dim=1, **_kw())  # other views
        # strict mode: only calls the fallback accepts
        oq = quantizer((8, False, "tensor", -1.0, 1.0))
        assert not cat(tensors=[qx, y], dim=1, output_quantizer=oq, strict_quantization=True)
        assert not cat(tensors=[qx, qy], dim=1, output_quantizer=None, strict_quantization=True)
        assert cat(tensors=[qx, qy], dim=1, output_quantizer=oq, strict_quantization=True)
    # grad mode with an operand that needs a gradient (a quantizer's parameters do)
    xg = x.clone().requires_grad_()
    assert not cat(tensors=[xg, y], dim=1, **_kw()) and not cat(tensors=[qx, y], dim=1, **_kw())
    with torch.no_grad():
        assert cat(tensors=[xg, y], dim=1, **_kw())


def test_what_the_pad_predicate_accepts_and_declines(on_device):
    pad = P.pad_predicate
    x = torch.randn(2, 3, 9, 14, dtype=torch.bfloat16)
    row, vol = torch.randn(2, 3, 14, dtype=torch.float16), torch.randn(1, 2, 3, 4, 6, dtype=torch.bfloat16)
    with torch.no_grad():
        qt = _q(x)
        qc = quantizer((8, False, ("channel", 1), torch.full((3,), -3.0), torch.full((3,), 3.0)))(x)
        for t in (x, qt, qc):
            assert pad(input=t, pad=(1, 2), mode="constant", value=None, **_kw()) and pad(input=t, pad=[3, 0, 1, 1], mode="constant", value=-1.5, **_kw())
            assert pad(input=t, pad=(-2, 3, 1, -1), mode="constant", value=float("inf"), **_kw()) and pad(input=t, pad=(1, 1), mode="constant", value=float("nan"), **_kw())
            assert pad(input=t, pad=(3, 2, 1, 4), mode="reflect", value=None, **_kw()) and pad(input=t, pad=(0, 3, 2, 1), mode="replicate", value=0.0, **_kw())
        assert pad(input=x, pad=(1, 1, 1, 1, 1, 1), mode="constant", value=2, **_kw()) and pad(input=qt, pad=(1, 1, 1, 1, 1, 1), mode="reflect", value=None, **_kw())
        assert not pad(input=qc, pad=(1, 1, 1, 1, 1, 1), mode="constant", value=None, **_kw())  # the channel dimension is padded
        assert pad(input=row, pad=(2, 2), mode="reflect", value=None, **_kw()) and pad(input=row[0], pad=(2, 2), mode="replicate", value=None, **_kw())
        assert pad(input=vol, pad=(2, 1, 3, 0, 1, 2), mode="reflect", value=None, **_kw()) and pad(input=vol[0], pad=(1, 1, 1, 1, 1, 1), mode="replicate", value=None, **_kw())
        # without the strict_quantization keyword (F.pad through __torch_function__)
        assert not pad(input=qt, pad=(1, 1), mode="constant", value=None, output_quantizer=None)
        # circular, the reference's default mode, anything else
        assert not pad(input=x, pad=(1, 1), mode="circular", value=None, **_kw()) and not pad(input=x, pad=(1, 1), mode="...", value=None, **_kw())
        assert not pad(input=x, pad=(1, 1), mode=None, value=None, **_kw())
        # reflect pad >= extent, negative pads outside constant mode, a value outside constant mode, ranks ATen refuses
        assert not pad(input=row, pad=(14, 0), mode="reflect", value=None, **_kw()) and not pad(input=x, pad=(0, 0, 9, 0), mode="reflect", value=None, **_kw())
        assert pad(input=row, pad=(13, 13), mode="reflect", value=None, **_kw()) and pad(input=row, pad=(20, 0), mode="replicate", value=None, **_kw())
        assert not pad(input=row, pad=(-1, 2), mode="reflect", value=None, **_kw()) and not pad(input=x, pad=(2, -1, 0, 0), mode="replicate", value=None, **_kw())
        assert not pad(input=row, pad=(1, 1), mode="reflect", value=1.0, **_kw())
        assert not pad(input=x, pad=(1, 1), mode="reflect", value=None, **_kw()) and not pad(input=row, pad=(1, 1, 1, 1, 1, 1), mode="replicate", value=None, **_kw())
        assert not pad(input=row[0, 0], pad=(1, 1), mode="reflect", value=None, **_kw())
        # pads that are no pairs of ints, more pairs than dims or than three, nothing padded, nothing left
        assert not pad(input=x, pad=(1,), mode="constant", value=None, **_kw()) and not pad(input=x, pad=(1, 1.0), mode="constant", value=None, **_kw())
        assert not pad(input=x, pad=(1, True), mode="constant", value=None, **_kw()) and not pad(input=x, pad=3, mode="constant", value=None, **_kw())
        assert not pad(input=x, pad=(1,) * 8, mode="constant", value=None, **_kw()) and not pad(input=row[0, 0], pad=(1, 1, 1, 1), mode="constant", value=None, **_kw())
        assert not pad(input=x, pad=(0, 0), mode="constant", value=None, **_kw()) and not pad(input=x, pad=(-1, 0, 0, -2), mode="constant", value=None, **_kw())
        assert not pad(input=x, pad=(-7, -7), mode="constant", value=None, **_kw()) and not pad(input=x, pad=(1, 1, -5, -5), mode="constant", value=None, **_kw())
        # a fill the dtype cannot hold (ATen refuses it), a fill that is no number
        assert not pad(input=row, pad=(1, 1), mode="constant", value=1e10, **_kw()) and not pad(input=x, pad=(1, 1), mode="constant", value="0", **_kw())
        assert pad(input=x, pad=(1, 1), mode="constant", value=1e10, **_kw())  # (bf16 holds it)
        # fp32 values, an empty tensor, parameters per row of the last dim, channels-last
        assert not pad(input=x.float(), pad=(1, 1), mode="constant", value=None, **_kw()) and not pad(input=x[:0], pad=(1, 1), mode="constant", value=None, **_kw())
        qr = quantizer((8, False, ("channel", (0, 1, 2)), torch.full((54,), -3.0), torch.full((54,), 3.0)))(x)
        assert not pad(input=qr, pad=(1, 1), mode="constant", value=None, **_kw())
        assert not pad(input=x.contiguous(memory_format=torch.channels_last), pad=(1, 1), mode="constant", value=None, **_kw())
        assert not pad(input=vol.contiguous(memory_format=torch.channels_last_3d), pad=(1, 1), mode="replicate", value=None, **_kw())
        assert pad(input=x.transpose(-1, -2), pad=(1, 1, 1, 1), mode="reflect", value=None, **_kw()) and pad(input=x[..., ::2], pad=(1, 1), mode="constant", value=None, **_kw())
        # strict mode: only calls the fallback accepts
        oq = quantizer((8, False, "tensor", -1.0, 1.0))
        assert not pad(input=x, pad=(1, 1), mode="constant", value=None, output_quantizer=oq, strict_quantization=True)
        assert not pad(input=qt, pad=(1, 1), mode="constant", value=None, output_quantizer=None, strict_quantization=True)
        assert pad(input=qt, pad=(1, 1), mode="constant", value=None, output_quantizer=oq, strict_quantization=True)
    xg = x.clone().requires_grad_()
    assert not pad(input=xg, pad=(1, 1), mode="constant", value=None, **_kw()) and not pad(input=qt, pad=(1, 1), mode="constant", value=None, **_kw())


def test_the_fill_is_what_atens_fill_writes():
    """Scalar -> fp32 -> dtype: two roundings. 1.00390625 is the tie between 1.0 and 1.0078125 in bf16; the 2**-30 that would break it
    upwards in one rounding from double does not survive the fp32 step, so the tie goes to even."""
    fill = ff.ops.concat.fill_bits
    assert fill(1.00390625 + 2**-30, torch.bfloat16) == 0x3F80 and fill(None, torch.bfloat16) == 0 and fill(-1.5, torch.float16) == 0xBE00
    assert fill(float("inf"), torch.float16) == 0x7C00 and fill(65504, torch.float16) == 0x7BFF and fill(float("nan"), torch.bfloat16) == 0x7FC0
    for value in (1.00390625 + 2**-30, 0.1, -1.5, 65504.0, float("inf"), float("nan"), 1e-8, -0.0, 3):
        for dtype in (torch.bfloat16, torch.float16):
            want = torch.tensor(value, dtype=torch.float64).to(torch.float32).to(dtype)  # the two roundings, spelled out
            assert fill(value, dtype) == int(want.view(torch.int16)) & 0xFFFF
    with pytest.raises(RuntimeError) as got:
        fill(1e10, torch.float16)
    with pytest.raises(RuntimeError) as want:
        torch.nn.functional.pad(torch.zeros(1, dtype=torch.float16), (1, 0), "constant", 1e10)
    assert str(got.value) == str(want.value)


# ---- 6. the code-level cat -----------------------------------------------------------------------------------------------------------
def test_the_code_level_cat_wins_and_compares_no_values_for_shared_parameters(on_device, monkeypatch):
    compared = []
    real = code_level._values_equal
    monkeypatch.setattr(code_level, "_values_equal", lambda a, b: compared.append(1) or real(a, b))
    x, y = torch.randn(2, 3, 8, dtype=torch.bfloat16), torch.randn(2, 5, 8, dtype=torch.bfloat16)
    q = quantizer((8, False, "tensor", -3.0, 3.0))
    with torch.no_grad(), ff.strict_quantization(False):
        a, b = q(x), q(y)
        assert a.quant_args().scale is b.quant_args().scale
        # the same parameter objects: equal without a comparison; the code-level kernel is what the dispatcher finds, not the fused one
        assert code_level.cat_predicate(tensors=[a, b], dim=1, **_kw()) and not P.cat_predicate(tensors=[a, b], dim=1, **_kw())
        assert ff.dispatcher.dispatch("cat", tensors=[a, b], dim=1, **_kw()) is code_level.cat
        out = F.cat([a, b], 1)
        assert isinstance(out, ff.QuantizedTensor) and torch.equal(out.raw_data, torch.cat([a.raw_data, b.raw_data], 1))
        assert out.quant_args().scale is a.quant_args().scale
        through_torch = torch.cat([a, b], 1)
        assert isinstance(through_torch, ff.QuantizedTensor) and torch.equal(through_torch.raw_data, out.raw_data)
        # one view of one storage is equal as well
        view = ff.QuantizedTensor(b.raw_data, b.quantization_context.with_changes(scale=b.quant_args().scale.view(-1), offset=b.quant_args().offset.view(-1)))
        assert code_level.cat_predicate(tensors=[a, view], dim=1, **_kw())
        assert not compared
        # equal values in other tensors: compared as the reference compares them, and equal
        other = quantizer((8, False, "tensor", -3.0, 3.0))(y)
        assert code_level.cat_predicate(tensors=[a, other], dim=1, **_kw()) and compared
        assert ff.dispatcher.dispatch("cat", tensors=[a, other], dim=1, **_kw()) is code_level.cat
        # other parameters, an output quantizer, a plain element, a per-channel element: not the code-level kernel
        c = quantizer((8, False, "tensor", -2.0, 2.0))(y)
        assert not code_level.cat_predicate(tensors=[a, c], dim=1, **_kw()) and P.cat_predicate(tensors=[a, c], dim=1, **_kw())
        oq = quantizer((8, False, "tensor", -1.0, 1.0))
        assert not code_level.cat_predicate(tensors=[a, b], dim=1, output_quantizer=oq, strict_quantization=False)
        assert P.cat_predicate(tensors=[a, b], dim=1, output_quantizer=oq, strict_quantization=False)
        assert not code_level.cat_predicate(tensors=[a, y], dim=1, **_kw()) and not code_level.cat_predicate(tensors=[], dim=1, **_kw())
        qc = quantizer((8, False, ("channel", 1), torch.full((3,), -3.0), torch.full((3,), 3.0)))
        assert not code_level.cat_predicate(tensors=[qc(x), qc(x)], dim=0, **_kw())
        with ff.strict_quantization(True):  # codes stay codes: no implicit dequantization to refuse
            assert isinstance(torch.cat([a, b], 1), ff.QuantizedTensor)


# ---- 7. the ctypes wrappers and the C ABI --------------------------------------------------------------------------------------------
def test_the_wrappers_reject_bad_arguments_before_a_launch():
    x = torch.randn(2, 3, 8, 8, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="non-empty list"):
        ff.ops.cat_quantize([])
    with pytest.raises(RuntimeError, match="out of range"):
        ff.ops.cat_quantize([x, x], 4)
    with pytest.raises(RuntimeError, match="agree off dim"):
        ff.ops.cat_quantize([x, x[:, :, :4]], 1)
    with pytest.raises(RuntimeError, match="agree off dim"):
        ff.ops.cat_quantize([x, x[:, :0]], 1)
    with pytest.raises(RuntimeError, match="value dtype"):
        ff.ops.cat_quantize([x, x.float()], 1)
    with pytest.raises(RuntimeError, match="parameters are one pair"):
        ff.ops.cat_quantize([x, x.to(torch.int8)], 1, dtype=torch.bfloat16, dequant=[None, (torch.ones(3), None)])
    with pytest.raises(RuntimeError, match="mode is one of"):
        ff.ops.pad_quantize(x, (1, 1), "circular")
    with pytest.raises(RuntimeError, match="pairs of ints"):
        ff.ops.pad_quantize(x, (1, 1, 1))
    with pytest.raises(RuntimeError, match="takes no value"):
        ff.ops.pad_quantize(x, (1, 1), "reflect", 1.0)
    with pytest.raises(RuntimeError, match="not empty"):
        ff.ops.pad_quantize(x, (-4, -4), "constant")
    with pytest.raises(RuntimeError, match="channel dimension"):
        ff.ops.pad_quantize(x.to(torch.int8), (1, 1, 1, 1, 1, 1), "constant", dtype=torch.bfloat16, dequant=(torch.ones(3), None))
    with pytest.raises(BackendError):  # a host tensor: there is no CPU implementation
        ff.ops.cat_quantize([x, x], 1)
    with pytest.raises(BackendError):
        ff.ops.pad_quantize(x, (1, 1), "constant")


def test_the_hip_library_exports_the_entry_points():
    dll = ctypes.CDLL(str(HIP_SO))
    lib = FFQLibrary(HIP_SO)
    for name in ENTRY_POINTS:
        assert hasattr(dll, name) and name in _cabi.SIGNATURES and name in _cabi.DEVICE_ONLY
        assert getattr(lib, name) is not None


def test_the_oracle_loads_without_them():
    lib = load_oracle()
    assert not lib.is_device
    for name in ENTRY_POINTS:
        assert getattr(lib, name) is None


FAKE = 1 << 20  # never dereferenced: every call below returns from the argument checks


def _fan(count=1, bits=8.0, codes=FAKE):
    return FanOut.make(bits, [FAKE] * count, [None] * count, [codes] * count)


def _cat(lib, n=2, data=FAKE, tag=DType.I8, scale=FAKE, run=16, dt=DType.BF16, outer=4, out_run=None, col0=0, out=FAKE, fan=None, inputs=True):
    f = _fan() if fan is None else fan
    c = CatInputs.make([(data, tag, scale, None, run)] * n)
    out_run = n * run if out_run is None else out_run
    return lib.ffq_cat_quantize(ctypes.byref(c) if inputs else None, dt, outer, out_run, col0, out, ctypes.byref(f), None)


def _pad(lib, mode=0, x=FAKE, x_dt=DType.I8, scale=FAKE, channels=0, inner=0, dt=DType.BF16, outer=6, D=(1, 9, 14), pads=(1, 2, 3, 0, 0, 0), fill=0,
         out=FAKE, fan=None):
    f = _fan() if fan is None else fan
    return lib.ffq_pad_quantize(mode, x, x_dt, scale, None, channels, inner, dt, outer, *D, (ctypes.c_int64 * 6)(*pads), fill, out, ctypes.byref(f), None)


@pytest.mark.parametrize(
    "call,status",
    [
        (lambda lib: _cat(lib, dt=DType.F32), Status.ERR_DTYPE),
        (lambda lib: _cat(lib, dt=DType.F32, data=None), Status.ERR_DTYPE),    # the dtype first, before any buffer is looked at
        (lambda lib: _cat(lib, scale=None), Status.ERR_DTYPE),                 # int8 codes without a scale
        (lambda lib: _cat(lib, tag=DType.F16), Status.ERR_DTYPE),              # codes of another value dtype
        (lambda lib: _cat(lib, inputs=False), Status.ERR_ARG),
        (lambda lib: _cat(lib, n=9), Status.ERR_ARG),                          # more than 8 inputs in one launch
        (lambda lib: _cat(lib, n=0), Status.ERR_ARG),
        (lambda lib: _cat(lib, run=0), Status.ERR_ARG),
        (lambda lib: _cat(lib, out_run=24), Status.ERR_ARG),                   # 2 x 16 columns in a row of 24
        (lambda lib: _cat(lib, out_run=40, col0=16), Status.ERR_ARG),
        (lambda lib: _cat(lib, outer=-1), Status.ERR_ARG),
        (lambda lib: _cat(lib, outer=1 << 20, run=1 << 10), Status.ERR_DTYPE),  # 2^31 elements
        (lambda lib: _cat(lib, data=None), Status.ERR_ARG),
        (lambda lib: _cat(lib, data=FAKE + 8), Status.ERR_ARG),                # misaligned
        (lambda lib: _cat(lib, out=FAKE + 2), Status.ERR_ARG),
        (lambda lib: _cat(lib, fan=_fan(bits=9.0)), Status.ERR_PRECISION),
        (lambda lib: _cat(lib, fan=_fan(codes=None)), Status.ERR_ARG),
        (lambda lib: _cat(lib, fan=_fan(count=3, codes=FAKE + 4)), Status.ERR_ARG),
        (lambda lib: _cat(lib, outer=0), Status.OK),
        (lambda lib: _pad(lib, mode=3), Status.ERR_ARG),                       # circular has no number
        (lambda lib: _pad(lib, mode=-1), Status.ERR_ARG),
        (lambda lib: _pad(lib, dt=DType.F32), Status.ERR_DTYPE),
        (lambda lib: _pad(lib, dt=DType.F32, x=None), Status.ERR_DTYPE),
        (lambda lib: _pad(lib, scale=None), Status.ERR_DTYPE),
        (lambda lib: _pad(lib, x_dt=DType.BF16, scale=None, channels=3, inner=1), Status.ERR_DTYPE),  # a plain input has no parameters
        (lambda lib: _pad(lib, channels=4, inner=1), Status.ERR_ARG),          # 6 rows are not images of 4 channels
        (lambda lib: _pad(lib, channels=3, inner=0), Status.ERR_ARG),
        (lambda lib: _pad(lib, D=(1, 0, 14)), Status.ERR_ARG),
        (lambda lib: _pad(lib, mode=1, pads=(14, 0, 0, 0, 0, 0)), Status.ERR_ARG),  # reflect pad >= extent
        (lambda lib: _pad(lib, mode=1, pads=(-1, 2, 0, 0, 0, 0)), Status.ERR_ARG),  # negative pads crop in constant mode only
        (lambda lib: _pad(lib, mode=2, pads=(1, 1, 0, -1, 0, 0)), Status.ERR_ARG),
        (lambda lib: _pad(lib, pads=(-7, -7, 0, 0, 0, 0)), Status.ERR_ARG),     # nothing left
        (lambda lib: _pad(lib, fill=1 << 16), Status.ERR_ARG),
        (lambda lib: _pad(lib, outer=1 << 16, D=(1, 256, 256)), Status.ERR_DTYPE),  # 2^32 elements
        (lambda lib: _pad(lib, outer=1 << 10, D=(1, 1024, 1024), pads=(1024, 0, 0, 0, 0, 0)), Status.ERR_DTYPE),  # 2^31 outputs
        (lambda lib: _pad(lib, x=FAKE + 8), Status.ERR_ARG),
        (lambda lib: _pad(lib, x=None), Status.ERR_ARG),
        (lambda lib: _pad(lib, out=FAKE + 2), Status.ERR_ARG),
        (lambda lib: _pad(lib, fan=_fan(bits=9.0)), Status.ERR_PRECISION),
        (lambda lib: _pad(lib, fan=_fan(codes=None)), Status.ERR_ARG),
        (lambda lib: _pad(lib, outer=0), Status.OK),
    ],
)
def test_argument_checks_need_no_device(call, status):
    lib = FFQLibrary(HIP_SO)
    assert call(lib) == status
    if status != Status.OK:
        assert lib.ffq_last_error()


# ---- 8. what hipcc emitted ------------------------------------------------------------------------------------------------------------
KERNELS = {  # kernel: instances
    "cat_quantize_kernel": 4,    # 2 value dtypes x (groups of 8 | elements); the input's form is a uniform branch
    "pad_quantize_kernel": 12,   # 2 value dtypes x 3 input forms x (groups of 8 | elements)
}


def test_the_new_kernels_spill_nothing_and_use_no_scratch():
    """No scratch, no spills and no LDS; at most 64 VGPRs per lane, i.e. 8 waves per SIMD: the loads of these memory-bound kernels
    have the whole machine's waves to hide behind."""
    if kernel_resources.readelf() is None or not kernel_resources.DEFAULT_LIBRARY.exists():
        pytest.skip("llvm-readelf or the built library is missing")
    rows = [k for k in kernel_resources.kernel_resources() if any(n in str(k["name"]) for n in KERNELS)]
    for needle, count in KERNELS.items():
        assert sum(needle in str(k["name"]) for k in rows) == count, needle
    bad = {str(k["name"]): k for k in rows if k["vgpr_spill_count"] or k["sgpr_spill_count"] or k["private_segment_fixed_size"]}
    assert not bad, bad
    assert all(k["group_segment_fixed_size"] == 0 for k in rows)
    assert all(k["vgpr_count"] <= 64 for k in rows), max(k["vgpr_count"] for k in rows)
