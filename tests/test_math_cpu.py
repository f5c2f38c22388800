"""The quantized math operators (rms_norm, pow, exp, sin, cos, sum, cumsum) without a GPU: the public names, the host path against the
reference's outputs (fixture G23), the reference's strict-mode errors, what the predicates decline, the four C-ABI entry points and
the workspace query (exported by the HIP library, absent from the oracle, argument checks before any device call) and what hipcc
emitted for their kernels."""

import ctypes
import sys

import pytest
import torch

import fastforward_amd as ff

from conftest import HIP_SO, ROOT, golden, load_oracle
from fastforward_amd import _cabi, fused_elementwise, fused_math
from fastforward_amd._cabi import DType, FanOut, FFQLibrary, Status
from fastforward_amd.exceptions import QuantizationError

sys.path.insert(0, str(ROOT / "tools"))

import kernel_resources  # noqa: E402

F = ff.nn.functional
NAMES = ("rms_norm", "pow", "exp", "sin", "cos", "sum", "cumsum")
ENTRY_POINTS = ("ffq_rms_norm_quantize", "ffq_unary_quantize", "ffq_sum_quantize_workspace_bytes", "ffq_sum_quantize", "ffq_cumsum_quantize")
OUTPUT_MSG = "'output_quantizer' must be provided if strict_quantization=True"


def _expected(name):
    return f"Expected '{name}' to be an instance of 'QuantizedTensor' because strict_quantization=True."


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


def test_the_new_operators_are_public():
    assert set(NAMES) <= set(F.__all__)
    assert all(callable(getattr(F, name)) for name in NAMES)
    assert {"rms_norm_quantize", "unary_quantize", "sum_quantize", "cumsum_quantize"} <= set(ff.ops.__all__)


# ---- the host path against the reference (G23) -----------------------------------------------------------------------------------
G23 = golden("g23_math.pt")


@pytest.mark.parametrize("index", range(len(G23)), ids=[c["name"] for c in G23])
def test_host_path_equals_the_reference_bit_for_bit(index):
    case = G23[index]
    args = {}
    for name, v in case["inputs"].items():
        if name in case["slots"]:
            q = _with_params(quantizer(case["slots"][name]), case["params"][name])
            with torch.no_grad():
                v = q(v)
        args[name] = v
    oq = _with_params(quantizer(case["out_slot"]), case["out_params"])
    fn = getattr(F, case["op"])
    with torch.no_grad(), ff.strict_quantization(False):
        value = fn(**args, **case["kwargs"])
        quantized = fn(**args, **case["kwargs"], output_quantizer=oq)
    want = case["value"]
    assert value.dtype == want.dtype and value.shape == want.shape and torch.equal(_bits(value), _bits(want)), case["name"]
    assert isinstance(quantized, ff.QuantizedTensor)
    assert torch.equal(quantized.raw_data, case["codes"]), case["name"]
    assert torch.equal(quantized.dequantize(), case["dequantized"]), case["name"]


def test_the_fixture_covers_what_the_issue_lists():
    names = " ".join(c["name"] for c in G23)
    for needle in ("eps=None", "q weight", "per-row", "pow 2 ", "pow 3 ", "pow 0.5 ", "pow -1 ", "pow 1.7 ", "sum dim=0", "sum dim=1",
                   "sum dim=-1", "sum dim=None", "cumsum dim=0", "cumsum dim=1", "cumsum dim=-1", "exp", "sin", "cos"):
        assert needle in names, needle
    assert {c["dtype"] for c in G23} == {"torch.float32", "torch.bfloat16"}
    assert [c["value"].dim() for c in G23 if c["name"].startswith("sum dim=None")] == [0] * 4


# ---- strict quantization: the reference's messages (_gen/fallback.py) ------------------------------------------------------------
def _q(x):
    return quantizer((8, False, "tensor", -3.0, 3.0))(x)


def test_strict_mode_errors_match_the_reference():
    x = torch.randn(4, 16)
    stub = ff.nn.QuantizerStub(output_quantizer=True)
    calls = [(F.exp, {}), (F.sin, {}), (F.cos, {}), (F.pow, dict(exponent=2.0)), (F.sum, {}), (F.sum, dict(dim=0)),
             (F.cumsum, dict(dim=1)), (F.rms_norm, dict(normalized_shape=(16,)))]
    for fn, kwargs in calls:
        with pytest.raises(QuantizationError) as e:
            fn(x, **kwargs, strict_quantization=True)
        assert str(e.value) == OUTPUT_MSG
        with pytest.raises(QuantizationError) as e:
            fn(x, **kwargs, output_quantizer=stub, strict_quantization=True)
        assert str(e.value) == _expected("input")
        assert fn(_q(x), **kwargs, output_quantizer=stub, strict_quantization=True) is not None
    # rms_norm's weight and pow's tensor exponent
    with pytest.raises(QuantizationError) as e:
        F.rms_norm(_q(x), (16,), torch.ones(16), output_quantizer=stub, strict_quantization=True)
    assert str(e.value) == _expected("weight")
    assert F.rms_norm(_q(x), (16,), _q(torch.ones(16)), output_quantizer=stub, strict_quantization=True) is not None
    with pytest.raises(QuantizationError) as e:
        F.pow(_q(x), torch.full((4, 16), 2.0), output_quantizer=stub, strict_quantization=True)
    assert str(e.value) == _expected("exponent")
    assert F.pow(_q(x), _q(torch.full((4, 16), 2.0)), output_quantizer=stub, strict_quantization=True) is not None


def test_signatures_follow_the_reference():
    x = torch.randn(4, 16).bfloat16()
    w = torch.randn(16).bfloat16()
    with ff.strict_quantization(False):
        assert torch.equal(F.rms_norm(x, (16,), w, 1e-6), torch.nn.functional.rms_norm(x, (16,), w, 1e-6))
        assert torch.equal(F.rms_norm(x, [16]), torch.nn.functional.rms_norm(x, [16]))
        assert torch.equal(F.pow(x, 3), torch.pow(x, 3))
        assert torch.equal(F.pow(x.abs(), x.float()), torch.pow(x.abs(), x.float()))
        assert F.sum(x).dim() == 0 and torch.equal(F.sum(x), torch.sum(x))
        assert torch.equal(F.sum(x, -1), torch.sum(x, -1)) and torch.equal(F.cumsum(x, 0), torch.cumsum(x, 0))
        for name in ("exp", "sin", "cos"):
            assert torch.equal(getattr(F, name)(x), getattr(torch, name)(x))


# ---- the predicates ---------------------------------------------------------------------------------------------------------------
P = fused_math


def test_the_predicates_decline_host_tensors_and_calls_without_the_strict_keyword():
    x = torch.randn(4, 16, dtype=torch.bfloat16)
    assert not P.rms_norm_predicate(input=x, normalized_shape=(16,), weight=None, eps=None, output_quantizer=None, strict_quantization=False)
    assert not P.pow_predicate(input=x, exponent=2.0, output_quantizer=None, strict_quantization=False)
    assert not P.unary_predicate(input=x, output_quantizer=None, strict_quantization=False)
    assert not P.sum_predicate(input=x, dim=None, output_quantizer=None, strict_quantization=False)
    assert not P.cumsum_predicate(input=x, dim=0, output_quantizer=None, strict_quantization=False)
    for pred in (P.rms_norm_predicate, P.pow_predicate, P.unary_predicate, P.sum_predicate, P.cumsum_predicate):
        assert not pred(x, x, 1, 2, out=x)  # any call signature, without raising
        assert not pred()
        assert not pred(x)


@pytest.fixture()
def on_device(monkeypatch):
    """The predicates' device check answered yes for host tensors: what else they decline is what they test."""
    for module in (fused_math, fused_elementwise):
        monkeypatch.setattr(module, "_on_device", lambda *t: True)


def _kw(**k):
    return dict(output_quantizer=None, strict_quantization=False, **k)


def test_what_the_predicates_accept_and_decline(on_device):
    x = torch.randn(4, 64, dtype=torch.bfloat16)
    w = torch.randn(64, dtype=torch.bfloat16)
    # accepted (the device check aside)
    assert P.rms_norm_predicate(input=x, normalized_shape=(64,), weight=w, eps=None, **_kw())
    assert P.rms_norm_predicate(input=x, normalized_shape=64, weight=None, eps=1e-6, **_kw())
    assert P.pow_predicate(input=x, exponent=-0.5, **_kw()) and P.unary_predicate(input=x, **_kw())
    assert all(P.sum_predicate(input=x, dim=d, **_kw()) for d in (None, 1, -1))
    assert all(P.cumsum_predicate(input=x, dim=d, **_kw()) for d in (1, -1))
    assert P.sum_predicate(input=x.view(4, 64, 1), dim=1, **_kw())  # dims of size 1 after it
    # a dim before the last: the column kernels measured slower than the route
    assert not any(P.sum_predicate(input=x, dim=d, **_kw()) or P.cumsum_predicate(input=x, dim=d, **_kw()) for d in (0, -2))
    # calls without the strict_quantization keyword (the torch-function route)
    assert not P.unary_predicate(input=x, output_quantizer=None)
    assert not P.sum_predicate(input=x, dim=0, output_quantizer=None)
    # tensor and other non-number exponents, exponents ATen cannot convert
    for e in (torch.tensor(2.0), torch.full((4, 64), 2.0), True, None, "2", float("nan"), float("inf"), 1e6):
        assert not P.pow_predicate(input=x, exponent=e, **_kw()), e
    # rms_norm: not the last dim alone, cols > 16384 or % 8, a weight of another dtype / shape, eps not a number
    big = torch.randn(2, 16392, dtype=torch.bfloat16)
    assert not P.rms_norm_predicate(input=big, normalized_shape=(16392,), weight=None, eps=None, **_kw())
    assert not P.rms_norm_predicate(input=x, normalized_shape=(4, 64), weight=None, eps=None, **_kw())
    assert not P.rms_norm_predicate(input=x, normalized_shape=(64,), weight=w.float(), eps=None, **_kw())
    assert not P.rms_norm_predicate(input=x, normalized_shape=(64,), weight=w[:32], eps=None, **_kw())
    assert not P.rms_norm_predicate(input=x, normalized_shape=(64,), weight=None, eps="1e-6", **_kw())
    odd = torch.randn(4, 36, dtype=torch.bfloat16)
    assert not P.rms_norm_predicate(input=odd, normalized_shape=(36,), weight=None, eps=None, **_kw())
    # sum / cumsum: axes the kernels do not tile, dims that are not one int
    x3 = torch.randn(8, 4, 6, dtype=torch.bfloat16)
    assert not P.sum_predicate(input=x3, dim=-1, **_kw()) and not P.cumsum_predicate(input=x3, dim=-1, **_kw())  # 6 % 8
    assert not P.cumsum_predicate(input=x3, dim=-1, **_kw()) and not P.cumsum_predicate(input=x, dim=None, **_kw())
    assert not P.sum_predicate(input=x, dim=(0, 1), **_kw()) and not P.sum_predicate(input=x, dim=2, **_kw())
    assert not P.sum_predicate(input=x, dim=True, **_kw())
    # fp32 values, 9 elements, an empty tensor
    assert not P.unary_predicate(input=x.float(), **_kw())
    assert not P.unary_predicate(input=x[:3, :3], **_kw()) and not P.unary_predicate(input=x[:0], **_kw())
    # grad mode with an operand that needs a gradient (not under no_grad)
    xg = x.clone().requires_grad_()
    assert not P.unary_predicate(input=xg, **_kw()) and not P.sum_predicate(input=xg, dim=0, **_kw())
    assert not P.rms_norm_predicate(input=x, normalized_shape=(64,), weight=w.clone().requires_grad_(), eps=None, **_kw())
    with torch.no_grad():
        assert P.unary_predicate(input=xg, **_kw())
    # strict mode: only calls the fallback accepts
    assert not P.unary_predicate(input=x, output_quantizer=None, strict_quantization=True)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
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


def test_the_workspace_query():
    lib = FFQLibrary(HIP_SO)
    ws = lib.ffq_sum_quantize_workspace_bytes
    assert ws(16384, 4096, 1) == 0                 # row sums: none
    assert ws(1, 16384 * 4096, 1) == 1024 * 4      # the whole tensor: one fp32 partial per first-stage block
    assert ws(1, 16384, 4096) == 256 * 4096 * 4    # sum(0) of [16384, 4096]: 256 segments of 64 rows
    assert ws(1, 64, 4096) == 0                    # one segment: no partials
    assert ws(0, 8, 8) == 0 and ws(-1, 8, 8) == 0


FAKE = 1 << 20  # never dereferenced: every call below returns from the argument checks


def _fan(count=1, bits=8.0, codes=FAKE):
    return FanOut.make(bits, [FAKE] * count, [None] * count, [codes] * count)


def _rms(lib, x=FAKE, x_dt=DType.I8, scale=FAKE, per_row=0, weight=None, dt=DType.BF16, rows=4, cols=64, fan=None):
    f = _fan() if fan is None else fan
    return lib.ffq_rms_norm_quantize(x, x_dt, scale, None, per_row, weight, dt, rows, cols, 1e-6, None, ctypes.byref(f), None)


def _un(lib, op=3, x=FAKE, x_dt=DType.I8, scale=FAKE, run=0, exponent=2.0, dt=DType.BF16, numel=64, fan=None):
    f = _fan() if fan is None else fan
    return lib.ffq_unary_quantize(op, x, x_dt, scale, None, run, exponent, dt, numel, None, ctypes.byref(f), None)


def _sum(lib, x=FAKE, x_dt=DType.BF16, scale=None, run=0, dt=DType.BF16, outer=4, length=64, inner=1, ws=None, ws_bytes=0, fan=None):
    f = _fan() if fan is None else fan
    return lib.ffq_sum_quantize(x, x_dt, scale, None, run, dt, outer, length, inner, None, ctypes.byref(f), ws, ws_bytes, None)


def _cs(lib, x=FAKE, x_dt=DType.BF16, scale=None, run=0, dt=DType.BF16, outer=4, length=64, inner=1, fan=None):
    f = _fan() if fan is None else fan
    return lib.ffq_cumsum_quantize(x, x_dt, scale, None, run, dt, outer, length, inner, None, ctypes.byref(f), None)


@pytest.mark.parametrize(
    "call,status",
    [
        (lambda lib: _rms(lib, rows=-1), Status.ERR_ARG),
        (lambda lib: _rms(lib, dt=DType.F32), Status.ERR_DTYPE),
        (lambda lib: _rms(lib, scale=None), Status.ERR_DTYPE),              # int8 codes without a scale
        (lambda lib: _rms(lib, cols=36), Status.ERR_DTYPE),
        (lambda lib: _rms(lib, cols=16392), Status.ERR_DTYPE),
        (lambda lib: _rms(lib, cols=0), Status.ERR_EMPTY),
        (lambda lib: _rms(lib, weight=FAKE + 4), Status.ERR_ARG),           # misaligned
        (lambda lib: _rms(lib, x=None), Status.ERR_ARG),
        (lambda lib: _rms(lib, fan=_fan(bits=9.0)), Status.ERR_PRECISION),
        (lambda lib: _rms(lib, rows=0), Status.OK),
        (lambda lib: _un(lib, op=4), Status.ERR_ARG),
        (lambda lib: _un(lib, op=0, exponent=2.0), Status.ERR_ARG),         # the exponent belongs to pow
        (lambda lib: _un(lib, exponent=float("nan")), Status.ERR_ARG),
        (lambda lib: _un(lib, exponent=1e6), Status.ERR_ARG),
        (lambda lib: _un(lib, dt=DType.F16, x_dt=DType.BF16), Status.ERR_DTYPE),
        (lambda lib: _un(lib, numel=60), Status.ERR_DTYPE),
        (lambda lib: _un(lib, run=24), Status.ERR_DTYPE),
        (lambda lib: _un(lib, x=FAKE + 8), Status.ERR_ARG),
        (lambda lib: _un(lib, numel=0), Status.OK),
        (lambda lib: _sum(lib, outer=-1), Status.ERR_ARG),
        (lambda lib: _sum(lib, length=60), Status.ERR_DTYPE),               # 8 | len for a row sum
        (lambda lib: _sum(lib, outer=1, length=60, inner=12), Status.ERR_DTYPE),  # 8 | inner otherwise
        (lambda lib: _sum(lib, x_dt=DType.I8), Status.ERR_DTYPE),
        (lambda lib: _sum(lib, dt=DType.F32, x_dt=DType.F32), Status.ERR_DTYPE),
        (lambda lib: _sum(lib, length=0, inner=8), Status.ERR_EMPTY),
        (lambda lib: _sum(lib, outer=1, inner=1), Status.ERR_WORKSPACE),    # the whole tensor needs partials
        (lambda lib: _sum(lib, outer=1, length=16384, inner=4096, ws=FAKE, ws_bytes=1024), Status.ERR_WORKSPACE),
        (lambda lib: _sum(lib, x=None), Status.ERR_ARG),
        (lambda lib: _sum(lib, outer=0), Status.OK),
        (lambda lib: _cs(lib, length=12), Status.ERR_DTYPE),
        (lambda lib: _cs(lib, inner=4), Status.ERR_DTYPE),
        (lambda lib: _cs(lib, scale=FAKE, x_dt=DType.I16), Status.ERR_DTYPE),
        (lambda lib: _cs(lib, x=FAKE + 2), Status.ERR_ARG),
        (lambda lib: _cs(lib, fan=_fan(codes=None)), Status.ERR_ARG),
        (lambda lib: _cs(lib, outer=0), Status.OK),
    ],
)
def test_argument_checks_need_no_device(call, status):
    lib = FFQLibrary(HIP_SO)
    assert call(lib) == status
    if status != Status.OK:
        assert lib.ffq_last_error()


KERNELS = {  # kernel: instances (2 value dtypes x 3 input forms x ...)
    "rms_norm_quantize_kernel": 30,     # x 5 row geometries
    "unary_quantize_kernel": 72,        # x 12 device forms
    "reduce_rows_kernel": 12,           # x 2 row geometries
    "reduce_cols_kernel": 12,           # x finishing or leaving partials
    "reduce_cols_finish_kernel": 2,
    "reduce_all_kernel": 6,
    "reduce_all_finish_kernel": 2,
    "scan_rows_kernel": 6,
    "scan_cols_kernel": 6,
}


def test_the_new_kernels_spill_nothing_and_use_no_scratch():
    if kernel_resources.readelf() is None or not kernel_resources.DEFAULT_LIBRARY.exists():
        pytest.skip("llvm-readelf or the built library is missing")
    rows = [k for k in kernel_resources.kernel_resources() if any(n in str(k["name"]) for n in KERNELS)]
    for needle, count in KERNELS.items():
        assert sum(needle in str(k["name"]) for k in rows) == count, needle
    for k in rows:  # the substrings other resource tests count stay theirs
        assert not any(n in str(k["name"]) for n in ("pointwise_quantize_kernel", "layer_norm_quantize_kernel", "embedding_quantize_kernel",
                                                      "activation_quantize_kernel", "softmax_quantize_kernel", "binary_quantize_kernel"))
    bad = {str(k["name"]): k for k in rows if k["vgpr_spill_count"] or k["sgpr_spill_count"] or k["private_segment_fixed_size"]}
    assert not bad, bad
    assert all(k["group_segment_fixed_size"] <= 16384 for k in rows)
