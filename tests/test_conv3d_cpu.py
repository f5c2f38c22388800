"""Quantized conv3d / avg_pool3d without a GPU: the functional surface and the reference's strict-mode errors, the host path against
the reference's outputs (fixture G27), ``QuantizedConv3d`` (conversion only on request), the predicates on what they decline, the
second header ``include/ffq_3d.h`` against ``_cabi.SIGNATURES_3D`` (exported by the HIP library, absent from the oracle, ``ffq.h``
and ``SIGNATURES`` untouched), every argument error of the three entry points in the documented order before any device call, the
workspace formula, and what hipcc emitted for the new kernels."""

import ctypes
import re
import sys

import pytest
import torch

import fastforward_amd as ff

from conftest import HIP_SO, ROOT, golden, load_oracle
from fastforward_amd import _cabi, fused_conv3d, fused_pool
from fastforward_amd._cabi import DType, FFQLibrary, Status
from fastforward_amd.exceptions import BackendError, QuantizationError

sys.path.insert(0, str(ROOT / "tools"))

import kernel_resources  # noqa: E402

ENTRY_POINTS = ("ffq_conv3d_w8a8_workspace_bytes", "ffq_conv3d_w8a8", "ffq_pool3d_quantize")
CONV3D = ff.nn.quantized_conv3d_modules()
F = ff.nn.functional


# ---- the functional surface --------------------------------------------------------------------------------------------------------
def test_functional_surface():
    assert {"conv3d", "avg_pool3d"} <= set(F.__all__)
    x = torch.randn(2, 4, 5, 6, 7)
    w = torch.randn(3, 4, 3, 2, 3)
    b = torch.randn(3)
    for stride, padding, dilation in ((1, 0, 1), (2, 1, 1), ((1, 2, 3), (1, 0, 2), (1, 2, 1)), (1, "same", (1, 1, 1)), (1, "valid", 1)):
        out = F.conv3d(x, w, b, stride, padding, dilation, strict_quantization=False)
        assert torch.equal(out, torch.nn.functional.conv3d(x, w, b, stride, padding, dilation))
    grouped = F.conv3d(x, torch.randn(6, 2, 1, 1, 1), None, groups=2, strict_quantization=False)
    assert grouped.shape == (2, 6, 5, 6, 7)
    for kwargs in (dict(kernel_size=2, stride=2), dict(kernel_size=3, stride=2, padding=1, count_include_pad=False),
                   dict(kernel_size=(1, 3, 2), stride=(1, 2, 1), ceil_mode=True)):
        assert torch.equal(F.avg_pool3d(x, **kwargs, strict_quantization=False), torch.nn.functional.avg_pool3d(x, **kwargs))


# ---- strict quantization: the reference's messages (_gen/fallback.py:218-265, 579-612), in its order -----------------------------------
OUTPUT_MSG = "'output_quantizer' must be provided if strict_quantization=True"


def _expected(name):
    return f"Expected '{name}' to be an instance of 'QuantizedTensor' because strict_quantization=True."


def _input_quantizer():
    q = ff.nn.LinearQuantizer(8, symmetric=False)
    q.quantization_range = (torch.tensor(-3.0), torch.tensor(3.0))
    return q


def test_strict_mode_errors_match_the_reference():
    x, w = torch.randn(1, 4, 5, 6, 6), torch.randn(3, 4, 3, 3, 3)
    stub = ff.nn.QuantizerStub(output_quantizer=True)
    with pytest.raises(QuantizationError) as e:
        F.conv3d(x, w, strict_quantization=True)
    assert str(e.value) == OUTPUT_MSG
    with pytest.raises(QuantizationError) as e:
        F.conv3d(x, w, output_quantizer=stub, strict_quantization=True)
    assert str(e.value) == _expected("input")
    with pytest.raises(QuantizationError) as e:
        F.conv3d(_input_quantizer()(x), w, output_quantizer=stub, strict_quantization=True)
    assert str(e.value) == _expected("weight")
    with pytest.raises(QuantizationError) as e:
        F.avg_pool3d(x, 2, 2, strict_quantization=True)
    assert str(e.value) == OUTPUT_MSG
    with pytest.raises(QuantizationError) as e:
        F.avg_pool3d(x, 2, 2, output_quantizer=stub, strict_quantization=True)
    assert str(e.value) == _expected("input")
    # the module default is strict: a stub input quantizer leaves a plain tensor
    model = ff.quantize_model(torch.nn.Sequential(torch.nn.Conv3d(4, 3, 3)), extra_conversion=CONV3D)
    with pytest.raises(QuantizationError) as e:
        model(x)
    assert str(e.value) == _expected("input")


# ---- the host path against the reference (G27) -----------------------------------------------------------------------------------
def g27_quantizer(spec, got, device="cpu"):
    bits, symmetric, gran, lo, hi = spec
    granularity = ff.PerTensor() if gran == "tensor" else ff.PerChannel(gran[1])
    q = ff.nn.LinearQuantizer(bits, symmetric=symmetric, granularity=granularity, quantized_dtype=torch.int8)
    q.quantization_range = (torch.as_tensor(lo, dtype=torch.float32), torch.as_tensor(hi, dtype=torch.float32))
    with torch.no_grad():
        q.scale.copy_(got["scale"])
        if got["offset"] is not None:
            q.offset.copy_(got["offset"])
    return q.to(device)


def run_g27_conv(case, device="cpu"):
    """(value without an output quantizer, output QuantizedTensor) of the case's conv3d call (shared with the GPU tests)."""
    qs = {name: g27_quantizer(spec, case["params"][name], device) for name, spec in case["slots"].items()}
    with torch.no_grad(), ff.strict_quantization(False):
        xq = qs["input_quantizer"](case["x"].to(device))
        wq = qs["weight_quantizer"](case["weight"].to(device))
        bias = None if case["bias"] is None else case["bias"].to(device)
        if case["bias_kind"] == "quantized":
            bias = qs["bias_quantizer"](bias)
        args = (xq, wq, bias, case["stride"], case["padding"], case["dilation"], 1)
        return F.conv3d(*args), F.conv3d(*args, output_quantizer=qs["output_quantizer"])


def run_g27_pool(case, device="cpu", dtype=None):
    """(value, output QuantizedTensor) of the case's avg_pool3d call; `dtype` casts the float input first (the GPU tests)."""
    x = case["x"].to(device)
    x = x if dtype is None else x.to(dtype)
    with torch.no_grad(), ff.strict_quantization(False):
        if case["slots"]:
            x = g27_quantizer(case["slots"]["input"], case["params"]["input"], device)(x)
        oq = g27_quantizer(case["out_slot"], case["out_params"], device)
        return F.avg_pool3d(x, **case["kwargs"]), F.avg_pool3d(x, **case["kwargs"], output_quantizer=oq)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("index", range(16))
def test_conv3d_host_path_equals_the_reference_bit_for_bit(index):
    case = golden("g27_conv3d.pt")["conv"][index]
    value, quantized = run_g27_conv(case)
    assert value.dtype == case["value"].dtype and value.shape == case["value"].shape
    assert torch.equal(_bits(value), _bits(case["value"])), (index, case["dtype"])
    assert isinstance(quantized, ff.QuantizedTensor)
    assert torch.equal(quantized.raw_data, case["codes"])
    assert torch.equal(quantized.dequantize(), case["dequantized"])


@pytest.mark.parametrize("index", range(18))
def test_avg_pool3d_host_path_equals_the_reference_bit_for_bit(index):
    case = golden("g27_conv3d.pt")["pool"][index]
    value, quantized = run_g27_pool(case)
    assert value.dtype == case["value"].dtype and torch.equal(_bits(value), _bits(case["value"])), (index, case["form"])
    assert isinstance(quantized, ff.QuantizedTensor)
    assert torch.equal(quantized.raw_data, case["codes"]) and torch.equal(quantized.dequantize(), case["dequantized"])


def test_the_fixture_covers_what_it_names():
    data = golden("g27_conv3d.pt")
    conv, pool = data["conv"], data["pool"]
    assert len(conv) == 16 and {c["dtype"] for c in conv} == {"torch.float32", "torch.bfloat16"}
    assert {c["bias_kind"] for c in conv} == {None, "plain", "quantized"}
    assert {c["w_kind"] for c in conv} == {"tensor", "tensor-asym", "channel", "channel-asym"}
    assert any(c["padding"] == "same" for c in conv) and any(c["weight"].shape[2:] == (2, 14, 14) and c["stride"] == (2, 14, 14) for c in conv)
    assert any(c["weight"].shape[:2] == (130, 20) and c["dilation"] == (2, 1, 2) for c in conv)
    assert len(pool) == 18 and {c["form"] for c in pool} == {"plain", "q", "per-channel q"}
    assert any(c["kwargs"].get("ceil_mode") for c in pool) and any(c["kwargs"].get("count_include_pad") is False for c in pool)
    assert any(c["kwargs"].get("padding") for c in pool) and any(c["kwargs"]["kernel_size"] == (1, 3, 2) for c in pool)
    assert (ROOT / "tests" / "golden" / "g27_conv3d.pt").stat().st_size <= 1 << 20


# ---- the module --------------------------------------------------------------------------------------------------------------------
TAGS = {"input_quantizer": "activation/input", "weight_quantizer": "parameter/weight", "bias_quantizer": "parameter/bias",
        "output_quantizer": "activation/output"}


def test_conversion_needs_the_opt_in_mapping():
    cls = torch.nn.Conv3d
    assert cls not in ff.nn.quantized_module_map() and cls not in ff.nn.quantized_conv_modules()
    assert cls not in ff.nn.quantized_conv_transpose_modules()
    for extra in (None, ff.nn.quantized_conv_modules()):
        with pytest.raises(QuantizationError, match="no quantized version"):
            ff.quantize_model(torch.nn.Sequential(cls(4, 6, 3)), extra_conversion=extra)
    conv = ff.quantize_model(torch.nn.Sequential(cls(4, 6, 3)), extra_conversion=CONV3D)[0]
    assert type(conv) is ff.nn.QuantizedConv3d and isinstance(conv, cls) and CONV3D[cls] is type(conv)
    for name, tag in TAGS.items():
        stub = getattr(conv, name)
        assert isinstance(stub, ff.nn.QuantizerStub) and tag in stub.quant_metadata, name
    assert tuple(conv.weight_quantizer.quant_metadata.shape) == (6, 4, 3, 3, 3)
    assert set(CONV3D) == {cls} and CONV3D is not ff.nn.quantized_conv3d_modules()
    no_bias = ff.quantize_model(torch.nn.Sequential(cls(4, 6, 3, bias=False)), extra_conversion=CONV3D)[0]
    assert no_bias.bias_quantizer is None


def test_module_forward_on_the_host():
    torch.manual_seed(0)
    plain = torch.nn.Conv3d(4, 5, 3, stride=(1, 2, 1), padding=1, dilation=(1, 1, 2))
    x = torch.randn(2, 4, 5, 6, 7)
    want = plain(x)
    module = ff.quantize_model(torch.nn.Sequential(plain), extra_conversion=CONV3D)[0]
    with ff.strict_quantization(False):
        assert torch.equal(module(x), want)


# ---- the predicates ----------------------------------------------------------------------------------------------------------------
def _codes(shape, lo=-3.0, hi=3.0, granularity=None, symmetric=False, lo_hi_shape=None):
    q = ff.nn.LinearQuantizer(8, symmetric=symmetric, granularity=granularity or ff.PerTensor(), quantized_dtype=torch.int8)
    if lo_hi_shape is None:
        q.quantization_range = (torch.tensor(lo), torch.tensor(hi))
    else:
        q.quantization_range = (torch.full((lo_hi_shape,), lo), torch.full((lo_hi_shape,), hi))
    return q(torch.randn(shape))


def test_the_predicates_decline(monkeypatch):
    conv, pool = fused_conv3d.conv3d_predicate, fused_pool.avg_pool3d_predicate
    x, w = _codes((1, 16, 4, 6, 6)), _codes((8, 16, 3, 3, 3), -1.0, 1.0, symmetric=True)
    common = dict(output_quantizer=None, strict_quantization=False)
    # host tensors: nothing here is on the device
    assert not conv(input=x, weight=w, **common)
    assert not pool(input=x, kernel_size=2, stride=2, **common)
    assert not pool(input=torch.randn(1, 2, 4, 4, 4).bfloat16(), kernel_size=2, stride=2, **common)
    # ... and with the device check out of the way, each rule on its own (the geometry and operand rules read no memory)
    monkeypatch.setattr("fastforward_amd.fused_conv._on_device", lambda *t: True)

    def ok(**k):  # inference, as the models run: under grad mode the quantizers' learnable parameters decline every call
        with torch.no_grad():
            return fused_conv3d.KERNELS.supported(3, **{**dict(input=x, weight=w), **common, **k})

    assert ok()
    assert ok(padding="same") and ok(padding="valid") and ok(padding=(1, 0, 2), stride=(1, 2, 3), dilation=(2, 1, 1))
    assert not ok(groups=2, weight=_codes((8, 8, 3, 3, 3), -1.0, 1.0, symmetric=True))
    assert not ok(groups=2)
    x_pc = _codes((1, 16, 4, 6, 6), granularity=ff.PerChannel(1), lo_hi_shape=16)
    assert not ok(input=x_pc)                                             # per-channel activations
    assert not ok(input=_codes((16, 4, 6, 6)))                            # an unbatched 4-D input
    assert not ok(input=_codes((1, 16, 6, 6)), weight=_codes((8, 16, 3, 3), -1.0, 1.0, symmetric=True))  # conv2d's operands
    assert not ok(padding="same", weight=_codes((8, 16, 2, 3, 3), -1.0, 1.0, symmetric=True))   # 'same' with an even kernel: asymmetric
    assert not ok(padding="same", stride=2) and not ok(padding=(1, 1)) and not ok(padding=-1) and not ok(stride=0) and not ok(dilation=1.0)
    assert not ok(padding="circular")
    assert not ok(weight=_codes((8, 16, 5, 7, 7), -1.0, 1.0, symmetric=True))   # the filter exceeds the input
    w_in = _codes((8, 16, 3, 3, 3), -1.0, 1.0, symmetric=True, granularity=ff.PerChannel(1), lo_hi_shape=16)
    assert not ok(weight=w_in)                                            # per-input-channel weights
    assert ok(weight=_codes((8, 16, 3, 3, 3), -1.0, 1.0, symmetric=True, granularity=ff.PerChannel(0), lo_hi_shape=8))
    assert not ok(bias=torch.randn(8).bfloat16()) and ok(bias=torch.randn(8))   # the bias has the data dtype
    assert not ok(strict_quantization=True)                               # strict without an output quantizer: the fallback raises
    big = _codes((1, 4860, 3, 3, 3))                                      # 4860 * 27 = 131220 > 131071
    assert not ok(input=big, weight=_codes((2, 4860, 3, 3, 3), -1.0, 1.0, symmetric=True))
    with torch.enable_grad():
        assert not fused_conv3d.KERNELS.supported(3, input=x, weight=w, **common)   # a gradient is needed: no autograd formula


def test_the_wrappers_say_not_covered_on_a_library_without_the_symbols(oracle_backend):
    one = torch.ones(1)
    with pytest.raises(BackendError, match="not covered"):
        ff.ops.conv3d_w8a8(torch.zeros(1, 16, 3, 3, 3, dtype=torch.int8), torch.zeros(4, 16, 1, 1, 1, dtype=torch.int8), one, None, one, None)
    with pytest.raises(BackendError, match="not covered"):
        ff.ops.pool3d_quantize("avg", torch.zeros(1, 2, 4, 4, 4, dtype=torch.bfloat16), (2, 2, 2), (2, 2, 2))
    assert {"conv3d_w8a8", "pool3d_quantize"} <= set(ff.ops.__all__)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def _declared(header):
    text = (ROOT / "include" / header).read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(ffq_[a-z0-9_]+)\s*\(", text))


def test_the_second_header_and_its_table_agree():
    assert _declared("ffq_3d.h") == set(_cabi.SIGNATURES_3D) == set(ENTRY_POINTS)
    assert '#include "ffq.h"' in (ROOT / "include" / "ffq_3d.h").read_text()


def test_the_first_header_and_its_table_are_untouched():
    assert _declared("ffq.h") == set(_cabi.SIGNATURES)
    assert not set(_cabi.SIGNATURES) & set(_cabi.SIGNATURES_3D) and not set(_cabi.SIGNATURES_3D) & _cabi.DEVICE_ONLY
    assert _cabi.FFQ_ABI_VERSION == 9 and "#define FFQ_ABI_VERSION 9" in (ROOT / "include" / "ffq.h").read_text()


def test_the_hip_library_exports_them():
    dll = ctypes.CDLL(str(HIP_SO))
    lib = FFQLibrary(HIP_SO)
    for name in ENTRY_POINTS:
        assert hasattr(dll, name) and getattr(lib, name) is not None, name


def test_the_oracle_loads_without_them():
    lib = load_oracle()
    assert not lib.is_device
    for name in ENTRY_POINTS:
        assert getattr(lib, name) is None


FAKE = 1 << 20  # never dereferenced: every call below returns from the argument checks


def _conv(lib, x=FAKE, ndhwc=0, w=FAKE, xs=FAKE, ws=FAKE, bias=None, bias_dt=0, out=FAKE, out_dt=DType.BF16, out_scale=None, bits=8.0,
          y_dt=0, B=2, C=16, D=4, H=8, W=8, OC=32, K=(3, 3, 3), s=(1, 1, 1), p=(1, 1, 1), d=(1, 1, 1), workspace=FAKE, nbytes=None):
    if nbytes is None:
        nbytes = lib.ffq_conv3d_w8a8_workspace_bytes(B, C, D, H, W, OC, *K, ndhwc)
    return lib.ffq_conv3d_w8a8(x, ndhwc, w, xs, None, ws, None, 0, bias, bias_dt, out, out_dt, out_scale, None, bits, y_dt, B, C, D, H, W, OC,
                               *K, *s, *p, *d, workspace, nbytes, None)


# in the documented order: each call fails the named check and passes every check ahead of it; the `then` calls fail TWO checks and
# must report the earlier one
CONV_ERRORS = [
    (lambda lib: _conv(lib, B=-1, C=0), Status.ERR_ARG),                                   # negative extent, before the empty filter
    (lambda lib: _conv(lib, D=-1), Status.ERR_ARG),
    (lambda lib: _conv(lib, C=0, s=(0, 1, 1)), Status.ERR_EMPTY),                          # empty filter, before the stride
    (lambda lib: _conv(lib, K=(0, 3, 3)), Status.ERR_EMPTY),
    (lambda lib: _conv(lib, s=(0, 1, 1), K=(1 << 25, 3, 3)), Status.ERR_ARG),              # stride
    (lambda lib: _conv(lib, d=(1, 1, 0)), Status.ERR_ARG),
    (lambda lib: _conv(lib, p=(0, -1, 0)), Status.ERR_ARG),
    (lambda lib: _conv(lib, D=(1 << 24) + 1, C=1 << 20), Status.ERR_ARG),                  # above 2^24, before the reduction bound
    (lambda lib: _conv(lib, s=(1, (1 << 24) + 1, 1)), Status.ERR_ARG),
    (lambda lib: _conv(lib, C=4855, K=(3, 3, 3), ndhwc=1), Status.ERR_DTYPE),              # 131085 > 131071
    (lambda lib: _conv(lib, C=1 << 40, K=(1 << 24, 1 << 24, 1 << 24), p=(1 << 24,) * 3), Status.ERR_DTYPE),  # no int64 overflow on the way
    (lambda lib: _conv(lib, ndhwc=1, C=24, K=(9, 3, 3), p=(0, 0, 0)), Status.ERR_DTYPE),   # channels-last needs C % 16 == 0; before the filter size
    (lambda lib: _conv(lib, K=(7, 3, 3), bias=FAKE, bias_dt=DType.I8), Status.ERR_ARG),    # the filter exceeds the padded input; before the bias
    (lambda lib: _conv(lib, D=0), Status.ERR_ARG),
    (lambda lib: _conv(lib, B=1 << 30, bias=FAKE, bias_dt=DType.I8), Status.ERR_ARG),      # B * OD * OH * OW >= 2^31; before the bias
    (lambda lib: _conv(lib, bias=FAKE, bias_dt=DType.I8, out_dt=DType.I8), Status.ERR_DTYPE),
    (lambda lib: _conv(lib, out_dt=DType.I8, x=None), Status.ERR_DTYPE),                   # codes out without an output quantizer; before NULL
    (lambda lib: _conv(lib, out_scale=FAKE, out_dt=DType.BF16, y_dt=DType.BF16, bits=11.0), Status.ERR_DTYPE),
    (lambda lib: _conv(lib, out_scale=FAKE, out_dt=DType.I8, y_dt=DType.I8, bits=11.0), Status.ERR_PRECISION),
    (lambda lib: _conv(lib, out_scale=FAKE, out_dt=DType.I8, y_dt=DType.I8, x=None), Status.ERR_DTYPE),
    (lambda lib: _conv(lib, x=None, workspace=None), Status.ERR_ARG),
    (lambda lib: _conv(lib, xs=None), Status.ERR_ARG),
    (lambda lib: _conv(lib, out=None), Status.ERR_ARG),
    (lambda lib: _conv(lib, ndhwc=1, x=FAKE + 8, workspace=None), Status.ERR_ARG),         # misaligned channels-last codes; before the workspace
    (lambda lib: _conv(lib, workspace=None), Status.ERR_WORKSPACE),
    (lambda lib: _conv(lib, workspace=FAKE + 4), Status.ERR_WORKSPACE),
    (lambda lib: _conv(lib, nbytes=1024), Status.ERR_WORKSPACE),
    (lambda lib: _conv(lib, B=0, x=None, workspace=None), Status.OK),
    (lambda lib: _conv(lib, OC=0, x=None, workspace=None), Status.OK),
    (lambda lib: _conv(lib, B=0, out_dt=DType.I8), Status.ERR_DTYPE),                      # ... but the dtype checks come first
]


@pytest.mark.parametrize("index", range(len(CONV_ERRORS)))
def test_conv3d_argument_checks_need_no_device(index):
    call, status = CONV_ERRORS[index]
    lib = FFQLibrary(HIP_SO)
    assert call(lib) == status
    if status != Status.OK:
        assert lib.ffq_last_error()


def _pool(lib, mode=0, x=FAKE, x_dt=DType.BF16, xs=None, xo=None, channels=0, dt=DType.BF16, planes=6, size=(6, 7, 8), k=(3, 3, 3),
          s=(2, 2, 2), p=(1, 1, 1), ceil=0, out_size=(3, 4, 4), out=FAKE, fan=None):
    return lib.ffq_pool3d_quantize(mode, x, x_dt, xs, xo, channels, dt, planes, *size, *k, *s, *p, ceil, *out_size, out, fan, None)


def _fan(count=1, bits=8.0, codes=FAKE):
    return ctypes.byref(_cabi.FanOut.make(bits, [FAKE] * count, [None] * count, [codes] * count))


POOL_ERRORS = [
    (lambda lib: _pool(lib, mode=2, dt=DType.F32), Status.ERR_ARG),                        # no max pool here; the mode comes first
    (lambda lib: _pool(lib, mode=-1), Status.ERR_ARG),
    (lambda lib: _pool(lib, dt=DType.F32, x_dt=DType.F32, k=(0, 3, 3)), Status.ERR_DTYPE),  # dt, before the geometry
    (lambda lib: _pool(lib, x_dt=DType.I8, k=(0, 3, 3)), Status.ERR_DTYPE),                # codes without a scale
    (lambda lib: _pool(lib, xo=FAKE), Status.ERR_DTYPE),                                   # an offset without a scale
    (lambda lib: _pool(lib, channels=3), Status.ERR_DTYPE),                                # per-channel parameters without a scale
    (lambda lib: _pool(lib, k=(0, 3, 3), p=(2, 1, 1)), Status.ERR_ARG),
    (lambda lib: _pool(lib, s=(2, 0, 2)), Status.ERR_ARG),
    (lambda lib: _pool(lib, p=(1, 1, -1)), Status.ERR_ARG),
    (lambda lib: _pool(lib, k=((1 << 20) + 1, 3, 3)), Status.ERR_ARG),
    (lambda lib: _pool(lib, p=(2, 1, 1), out_size=(9, 9, 9)), Status.ERR_ARG),             # pad above half the kernel; before the output size
    (lambda lib: _pool(lib, out_size=(3, 4, 5), planes=-1), Status.ERR_ARG),               # not ATen's output size
    (lambda lib: _pool(lib, ceil=1, out_size=(3, 4, 4)), Status.ERR_ARG),                  # ceil_mode: [4, 4, 5]
    (lambda lib: _pool(lib, planes=-1), Status.ERR_ARG),
    (lambda lib: _pool(lib, xs=FAKE, x_dt=DType.I8, channels=4), Status.ERR_ARG),          # 6 planes are no whole volumes of 4 channels
    (lambda lib: _pool(lib, size=(6, 0, 8)), Status.ERR_ARG),
    (lambda lib: _pool(lib, size=(1, 1, 1), k=(2, 2, 2), s=(1, 1, 1), p=(0, 0, 0), out_size=(0, 0, 0)), Status.ERR_ARG),
    (lambda lib: _pool(lib, planes=1 << 24, fan=_fan(1, bits=11.0)), Status.ERR_DTYPE),    # 2^24 * 336 inputs; before the fan-out
    (lambda lib: _pool(lib, fan=_fan(1, bits=11.0), x=None), Status.ERR_PRECISION),        # the fan-out; before the buffers
    (lambda lib: _pool(lib, fan=_fan(1, codes=FAKE + 8), x=None), Status.ERR_ARG),
    (lambda lib: _pool(lib, x=None), Status.ERR_ARG),
    (lambda lib: _pool(lib, x=FAKE + 2), Status.ERR_ARG),
    (lambda lib: _pool(lib, out=FAKE + 8), Status.ERR_ARG),
    (lambda lib: _pool(lib, planes=0, x=None, out=None), Status.OK),
    (lambda lib: _pool(lib, planes=0, ceil=1), Status.ERR_ARG),                            # ... but the geometry is checked first
]


@pytest.mark.parametrize("index", range(len(POOL_ERRORS)))
def test_pool3d_argument_checks_need_no_device(index):
    call, status = POOL_ERRORS[index]
    lib = FFQLibrary(HIP_SO)
    assert call(lib) == status
    if status != Status.OK:
        assert lib.ffq_last_error()


def test_workspace_bytes():
    lib = FFQLibrary(HIP_SO)
    q = lib.ffq_conv3d_w8a8_workspace_bytes
    # NDHWC input [2, 4, 8, 8, 16] + weight [32, 3, 3, 3, 16] + (tap sums 32 * 27 + totals 32) int32, each rounded up to 256 bytes
    assert q(2, 3, 4, 8, 8, 32, 3, 3, 3, 0) == 8192 + 13824 + 3584
    assert q(2, 16, 4, 8, 8, 32, 3, 3, 3, 1) == 13824 + 3584
    # the patch embedding: [32, 4, 28, 28, 16] + [64, 2, 14, 14, 16] + (64 * 392 + 64) * 4
    assert q(32, 16, 4, 28, 28, 64, 2, 14, 14, 0) == 1605632 + 401408 + 100608
    assert q(2, 0, 4, 8, 8, 32, 3, 3, 3, 0) == 0 and q(2, 3, 4, 8, 8, 32, 3, 0, 3, 0) == 0 and q(-1, 3, 4, 8, 8, 32, 3, 3, 3, 0) == 0
    assert q(1 << 20, 16, 1 << 24, 1 << 24, 1 << 24, 32, 3, 3, 3, 0) == 0   # no launch takes it; no overflow into a small number


def test_the_new_kernels_spill_nothing_and_use_no_scratch():
    if kernel_resources.readelf() is None:
        pytest.skip("llvm-readelf is missing")
    assert kernel_resources.DEFAULT_LIBRARY.exists(), "build() leaves the HIP library in the tree"
    needles = {"conv3d_layout_kernel": 1, "conv3d_w8a8_kernel": 4, "pool3d_quantize_kernel": 24}
    rows = [k for k in kernel_resources.kernel_resources() if any(n in str(k["name"]) for n in needles)]
    for needle, count in needles.items():
        assert sum(needle in str(k["name"]) for k in rows) == count, needle
    bad = {str(k["name"]): k for k in rows if k["vgpr_spill_count"] or k["sgpr_spill_count"] or k["private_segment_fixed_size"]}
    assert not bad, bad
    gemm = [k for k in rows if "conv3d_w8a8_kernel" in str(k["name"])]
    assert all(k["group_segment_fixed_size"] <= 33280 and k["vgpr_count"] + k["agpr_count"] <= 256 for k in gemm), gemm
