"""The quantized elementwise operators (add / sub / mul / div, softmax, sigmoid, GELU) without a GPU: the public names, the host path
against the reference's outputs (fixture G21), the reference's strict-mode errors, the reference's rescale for mul by a number and
its gradient, the unchanged ``__torch_function__`` route, the three C-ABI entry points (exported by the HIP library, absent from the
oracle, argument checks before any device call) and what hipcc emitted for their kernels."""

import ctypes
import sys

import pytest
import torch

import fastforward_amd as ff

from conftest import HIP_SO, ROOT, golden, load_oracle
from fastforward_amd import _cabi, fused_elementwise
from fastforward_amd._cabi import DType, FanOut, FFQLibrary, Status
from fastforward_amd.exceptions import QuantizationError
from fastforward_amd.quantization._linear_quantized_ops import _ScaleGradient

sys.path.insert(0, str(ROOT / "tools"))

import kernel_resources  # noqa: E402

F = ff.nn.functional
NAMES = ("add", "sub", "mul", "div", "softmax", "sigmoid", "gelu")
ENTRY_POINTS = ("ffq_binary_quantize", "ffq_softmax_quantize", "ffq_activation_quantize")
KERNELS = ("binary_quantize_kernel", "softmax_quantize_kernel", "activation_quantize_kernel")
OUTPUT_MSG = "'output_quantizer' must be provided if strict_quantization=True"


def _expected(name):
    return f"Expected '{name}' to be an instance of 'QuantizedTensor' because strict_quantization=True."


def quantizer(spec, device="cpu"):
    bits, symmetric, gran, lo, hi = spec
    granularity = ff.PerTensor() if gran == "tensor" else ff.PerChannel(gran[1])
    q = ff.nn.LinearQuantizer(bits, symmetric=symmetric, granularity=granularity, quantized_dtype=torch.int8, device=device)
    q.quantization_range = (torch.as_tensor(lo, dtype=torch.float32, device=device), torch.as_tensor(hi, dtype=torch.float32, device=device))
    return q


def _with_params(q, got):
    with torch.no_grad():
        q.scale.copy_(got["scale"])
        if got["offset"] is not None:
            q.offset.copy_(got["offset"])
    return q


def g21_operands(case, device="cpu"):
    """The case's keyword arguments with its quantized operands rebuilt (the reference's scale / offset copied in)."""
    args = {}
    for name, v in case["inputs"].items():
        v = v.to(device) if isinstance(v, torch.Tensor) else v
        if name in case["slots"]:
            q = _with_params(quantizer(case["slots"][name], device), case["params"][name])
            with torch.no_grad():
                v = q(v)
        args[name] = v
    return args


def run_g21_case(case, device="cpu"):
    """(value without an output quantizer, output QuantizedTensor) of the case's operator."""
    args = g21_operands(case, device)
    fn = getattr(F, case["op"])
    oq = _with_params(quantizer(case["out_slot"], device), case["out_params"])
    with torch.no_grad(), ff.strict_quantization(False):
        value = fn(**args, **case["kwargs"])
        quantized = fn(**args, **case["kwargs"], output_quantizer=oq)
    return value, quantized


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def test_the_new_operators_are_public():
    assert set(NAMES) <= set(F.__all__)
    assert all(callable(getattr(F, name)) for name in NAMES)
    assert {"binary_quantize", "softmax_quantize", "activation_quantize"} <= set(ff.ops.__all__)


# ---- the host path against the reference (G21) -----------------------------------------------------------------------------------
G21 = golden("g21_elementwise.pt")


@pytest.mark.parametrize("index", range(len(G21)), ids=[c["name"] for c in G21])
def test_host_path_equals_the_reference_bit_for_bit(index):
    case = G21[index]
    if case["op"] == "scalar_multiply":
        args = g21_operands(case)
        with torch.no_grad():
            got = F.mul(args["input"], args["other"], strict_quantization=False)
        assert isinstance(got, ff.QuantizedTensor)
        assert torch.equal(got.raw_data, case["codes"]) and torch.equal(got.quant_args().scale, case["scale"])
        assert torch.equal(got.dequantize(), case["dequantized"])
        return
    value, quantized = run_g21_case(case)
    if case["value_rescaled"]:
        assert isinstance(value, ff.QuantizedTensor)
        value = value.dequantize()
    assert value.dtype == case["value"].dtype and torch.equal(_bits(value), _bits(case["value"])), case["name"]
    assert isinstance(quantized, ff.QuantizedTensor)
    assert torch.equal(quantized.raw_data, case["codes"]), case["name"]
    assert torch.equal(quantized.dequantize(), case["dequantized"]), case["name"]


# ---- strict quantization: the reference's messages (_gen/fallback.py) ------------------------------------------------------------
def _q(x):
    return quantizer((8, False, "tensor", -3.0, 3.0))(x)


def test_strict_mode_errors_match_the_reference():
    x, y = torch.randn(4, 16), torch.randn(4, 16)
    stub = ff.nn.QuantizerStub(output_quantizer=True)
    for fn in (F.add, F.sub, F.mul, F.div):
        with pytest.raises(QuantizationError) as e:
            fn(x, y, strict_quantization=True)
        assert str(e.value) == OUTPUT_MSG
        with pytest.raises(QuantizationError) as e:
            fn(x, y, output_quantizer=stub, strict_quantization=True)
        assert str(e.value) == _expected("input")
        with pytest.raises(QuantizationError) as e:
            fn(_q(x), y, output_quantizer=stub, strict_quantization=True)
        assert str(e.value) == _expected("other")
        # a number `other` is not a strict-mode error; a quantized one is not either
        assert fn(_q(x), 2.0, output_quantizer=stub, strict_quantization=True).shape == (4, 16)
        assert fn(_q(x), _q(y), output_quantizer=stub, strict_quantization=True).shape == (4, 16)
    for fn, kwargs in ((F.softmax, dict(dim=-1)), (F.sigmoid, {}), (F.gelu, {}), (F.gelu, dict(approximate="tanh"))):
        with pytest.raises(QuantizationError) as e:
            fn(x, **kwargs, strict_quantization=True)
        assert str(e.value) == OUTPUT_MSG
        with pytest.raises(QuantizationError) as e:
            fn(x, **kwargs, output_quantizer=stub, strict_quantization=True)
        assert str(e.value) == _expected("input")


def test_alpha_and_the_keyword_signatures_follow_the_reference():
    x, y = torch.randn(4, 16), torch.randn(4, 16)
    with ff.strict_quantization(False):
        assert torch.equal(F.add(x, y, 2), torch.add(x, y, alpha=2))
        assert torch.equal(F.sub(x, y, alpha=-0.5), torch.sub(x, y, alpha=-0.5))
        assert torch.equal(F.softmax(x, 0), torch.softmax(x, 0))
        assert F.softmax(x.bfloat16(), -1, torch.float32).dtype == torch.float32
        assert torch.equal(F.gelu(x, "tanh"), torch.nn.functional.gelu(x, approximate="tanh"))
        assert torch.equal(F.div(x, 0.0), x / 0.0)


# ---- mul by a number: the reference's rescale ---------------------------------------------------------------------------------------
def test_scalar_multiply_rescales_the_scale_and_keeps_the_codes():
    x = torch.randn(4, 16)
    qx = _q(x)
    for strict in (True, False):
        got = F.mul(qx, -2.5, strict_quantization=strict)  # no output quantizer needed: the rescale is selected first
        assert isinstance(got, ff.QuantizedTensor) and got.raw_data is not None
        assert torch.equal(got.raw_data, qx.raw_data)
        assert torch.equal(got.quant_args().scale, qx.quant_args().scale * -2.5)
        assert torch.equal(got.quant_args().offset, qx.quant_args().offset)
    stub = ff.nn.QuantizerStub(output_quantizer=True)
    assert isinstance(F.mul(qx, 3, output_quantizer=stub), ff.QuantizedTensor)
    # not the rescale: a tensor other, a bool, a per-channel input, a real output quantizer
    with ff.strict_quantization(False):
        assert type(F.mul(qx, torch.tensor(2.0))) is torch.Tensor
        assert type(F.mul(qx, True)) is torch.Tensor
        qrow = quantizer((8, False, ("channel", 0), torch.full((4,), -3.0), torch.full((4,), 3.0)))(x)
        assert type(F.mul(qrow, 2.0)) is torch.Tensor
        oq = quantizer((8, False, "tensor", -6.0, 6.0))
        out = F.mul(qx, 2.0, output_quantizer=oq)
        assert torch.equal(out.raw_data, oq(qx.dequantize() * 2.0).raw_data)


def test_scalar_multiply_scales_the_gradient_of_the_raw_data():
    codes = torch.randint(-100, 100, (4, 16)).float().requires_grad_()
    qx = _q(torch.randn(4, 16)).quantization_context.attach(codes)
    got = F.mul(qx, 2.5)
    got.raw_data.sum().backward()
    assert torch.equal(codes.grad, torch.full_like(codes, 2.5))
    v = torch.randn(8, requires_grad=True)
    _ScaleGradient.apply(v, -3.0).sum().backward()
    assert torch.equal(v.grad, torch.full_like(v, -3.0))


# ---- the torch-function route is unchanged ------------------------------------------------------------------------------------------
def test_operators_and_torch_functions_on_quantized_tensors_keep_the_dequantizing_route():
    x, y = torch.randn(4, 16), torch.randn(4, 16)
    qx, qy = _q(x), _q(y)
    dx, dy = qx.dequantize(), qy.dequantize()
    with ff.strict_quantization(False):
        cases = [(lambda: qx + qy, dx + dy), (lambda: qx - qy, dx - dy), (lambda: qx * 2, dx * 2), (lambda: qx / qy, dx / dy),
                 (lambda: torch.add(qx, qy, alpha=2), torch.add(dx, dy, alpha=2)), (lambda: torch.mul(qx, 3.0), dx * 3.0),
                 (lambda: torch.softmax(qx, -1), torch.softmax(dx, -1)), (lambda: torch.sigmoid(qx), torch.sigmoid(dx)),
                 (lambda: torch.nn.functional.gelu(qx), torch.nn.functional.gelu(dx))]
        for fn, want in cases:
            got = fn()
            assert type(got) is torch.Tensor and torch.equal(got, want)
    with ff.strict_quantization(True):
        for fn, _ in cases:
            with pytest.raises(QuantizationError):
                fn()


def test_the_predicates_decline_host_tensors_and_calls_without_the_strict_keyword():
    x = torch.randn(4, 16, dtype=torch.bfloat16)
    P = fused_elementwise
    assert not P.add_predicate(input=x, other=x, alpha=1, output_quantizer=None, strict_quantization=False)
    assert not P.mul_predicate(input=x, other=2.0, output_quantizer=None, strict_quantization=False)
    assert not P.div_predicate(input=x, other=x, output_quantizer=None, strict_quantization=False)
    assert not P.softmax_predicate(input=x, dim=-1, dtype=None, output_quantizer=None, strict_quantization=False)
    assert not P.activation_predicate(input=x, output_quantizer=None, strict_quantization=False)
    # any call signature, without raising (the torch-function route passes positional arguments and out=)
    for pred in (P.add_predicate, P.mul_predicate, P.div_predicate, P.softmax_predicate, P.activation_predicate):
        assert not pred(x, x, 1, 2, out=x)
        assert not pred()
        assert not pred(x)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_the_hip_library_exports_the_three_entry_points():
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


def _bin(lib, op=0, a=FAKE, a_dt=DType.I8, a_scale=FAKE, a_run=0, b=FAKE, b_dt=DType.BF16, b_scale=None, b_run=0, b_numel=64,
         scalar=0.0, alpha=1.0, dt=DType.BF16, numel=256, fan=None):
    f = _fan() if fan is None else fan
    return lib.ffq_binary_quantize(op, a, a_dt, a_scale, None, a_run, b, b_dt, b_scale, None, b_run, b_numel, scalar, alpha, dt, numel,
                                   None, ctypes.byref(f), None)


def _sm(lib, x=FAKE, x_dt=DType.BF16, scale=None, per_row=0, dt=DType.BF16, rows=4, cols=64, fan=None):
    f = _fan() if fan is None else fan
    return lib.ffq_softmax_quantize(x, x_dt, scale, None, per_row, dt, rows, cols, None, ctypes.byref(f), None)


def _act(lib, op=0, x=FAKE, x_dt=DType.I8, scale=FAKE, run=0, dt=DType.BF16, numel=64, fan=None):
    f = _fan() if fan is None else fan
    return lib.ffq_activation_quantize(op, x, x_dt, scale, None, run, dt, numel, None, ctypes.byref(f), None)


@pytest.mark.parametrize(
    "call,status",
    [
        (lambda lib: _bin(lib, op=4), Status.ERR_ARG),
        (lambda lib: _bin(lib, op=-1), Status.ERR_ARG),
        (lambda lib: _bin(lib, op=2, alpha=2.0), Status.ERR_ARG),              # alpha belongs to add / sub
        (lambda lib: _bin(lib, numel=-8), Status.ERR_ARG),
        (lambda lib: _bin(lib, dt=DType.F32), Status.ERR_DTYPE),
        (lambda lib: _bin(lib, a_dt=DType.I16), Status.ERR_DTYPE),
        (lambda lib: _bin(lib, a_scale=None), Status.ERR_DTYPE),              # int8 codes without a scale
        (lambda lib: _bin(lib, b_dt=DType.F16), Status.ERR_DTYPE),            # plain other of another dtype
        (lambda lib: _bin(lib, numel=260), Status.ERR_DTYPE),
        (lambda lib: _bin(lib, b_numel=12, numel=24), Status.ERR_DTYPE),
        (lambda lib: _bin(lib, b_numel=48), Status.ERR_TILE_DIVIDE),          # 48 does not divide 256
        (lambda lib: _bin(lib, a_run=24), Status.ERR_DTYPE),
        (lambda lib: _bin(lib, a_run=48), Status.ERR_DTYPE),                  # 48 does not divide numel
        (lambda lib: _bin(lib, b=None, b_numel=64), Status.ERR_ARG),          # a scalar other has no extent
        (lambda lib: _bin(lib, fan=_fan(bits=9.0)), Status.ERR_PRECISION),
        (lambda lib: _bin(lib, fan=_fan(codes=None)), Status.ERR_ARG),
        (lambda lib: _bin(lib, a=None), Status.ERR_ARG),
        (lambda lib: _bin(lib, a=FAKE + 8), Status.ERR_ARG),                  # misaligned
        (lambda lib: _bin(lib, b=FAKE + 4), Status.ERR_ARG),
        (lambda lib: _bin(lib, numel=0), Status.OK),
        (lambda lib: _bin(lib, numel=0, b=None, b_numel=0), Status.OK),
        (lambda lib: _sm(lib, rows=-1), Status.ERR_ARG),
        (lambda lib: _sm(lib, dt=DType.F32, x_dt=DType.F32), Status.ERR_DTYPE),
        (lambda lib: _sm(lib, x_dt=DType.I8), Status.ERR_DTYPE),              # codes without a scale
        (lambda lib: _sm(lib, cols=36), Status.ERR_DTYPE),
        (lambda lib: _sm(lib, cols=16392), Status.ERR_DTYPE),
        (lambda lib: _sm(lib, x=None), Status.ERR_ARG),
        (lambda lib: _sm(lib, x=FAKE + 8), Status.ERR_ARG),
        (lambda lib: _sm(lib, rows=0), Status.OK),
        (lambda lib: _sm(lib, cols=0), Status.OK),
        (lambda lib: _act(lib, op=3), Status.ERR_ARG),
        (lambda lib: _act(lib, dt=DType.F32), Status.ERR_DTYPE),
        (lambda lib: _act(lib, numel=60), Status.ERR_DTYPE),
        (lambda lib: _act(lib, run=24), Status.ERR_DTYPE),
        (lambda lib: _act(lib, scale=None), Status.ERR_DTYPE),
        (lambda lib: _act(lib, x=None), Status.ERR_ARG),
        (lambda lib: _act(lib, numel=0), Status.OK),
    ],
)
def test_argument_checks_need_no_device(call, status):
    lib = FFQLibrary(HIP_SO)
    assert call(lib) == status
    if status != Status.OK:
        assert lib.ffq_last_error()


def test_the_new_kernels_spill_nothing_and_use_no_scratch():
    if kernel_resources.readelf() is None or not kernel_resources.DEFAULT_LIBRARY.exists():
        pytest.skip("llvm-readelf or the built library is missing")
    rows = [k for k in kernel_resources.kernel_resources() if any(n in str(k["name"]) for n in KERNELS)]
    # binary: 2 value dtypes x 3 input forms x 4 other forms; softmax: x 3 forms x 5 row geometries; activation: x 3 forms x 3 ops
    for needle, count in zip(KERNELS, (24, 30, 18)):
        assert sum(needle in str(k["name"]) for k in rows) == count, needle
    for k in rows:  # the substrings other resource tests count stay theirs
        assert not any(n in str(k["name"]) for n in ("pointwise_quantize_kernel", "layer_norm_quantize_kernel", "embedding_quantize_kernel",
                                                      "conv_w8a8_kernel", "wq_mid_kernel"))
    bad = {str(k["name"]): k for k in rows if k["vgpr_spill_count"] or k["sgpr_spill_count"] or k["private_segment_fixed_size"]}
    assert not bad, bad
    assert all(k["group_segment_fixed_size"] <= 16384 for k in rows)
