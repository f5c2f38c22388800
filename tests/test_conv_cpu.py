"""Quantized Conv1d / Conv2d without a GPU: conversion by ``quantize_model`` on request (alone and in a tiny CNN; the global
module map still has no convolution), the reference's quantizer
tags and strict-mode errors, the host path against the reference's outputs (fixture G20), range estimation, the predicates on
host tensors, the C-ABI entry points (exported by the HIP library, absent from the oracle, argument checks before any device
call) and what hipcc emitted for the new kernels."""

import ctypes
import sys

import pytest
import torch

import fastforward_amd as ff

from conftest import HIP_SO, ROOT, golden, load_oracle
from fastforward_amd import _cabi, fused_conv
from fastforward_amd._cabi import DType, FFQLibrary, Status
from fastforward_amd.exceptions import QuantizationError

sys.path.insert(0, str(ROOT / "tools"))

import kernel_resources  # noqa: E402

ENTRY_POINTS = ("ffq_conv2d_w8a8", "ffq_conv2d_w8a8_workspace_bytes")
KERNELS = ("conv_layout_kernel", "conv_w8a8_kernel")


# ---- a tiny CNN built from torch.nn parts (shared with tests/test_conv_gpu.py) ---------------------------------------------------
def _plain(t):
    return t.dequantize() if isinstance(t, ff.QuantizedTensor) else t


class TinyCNN(torch.nn.Module):
    """Conv2d 3x3 -> ReLU -> Conv2d 3x3 stride 2 -> flatten -> Linear."""

    def __init__(self, c_in: int = 3, width: int = 16, size: int = 8, classes: int = 10) -> None:
        super().__init__()
        self.conv1 = torch.nn.Conv2d(c_in, width, 3, padding=1)
        self.act = torch.nn.ReLU()
        self.conv2 = torch.nn.Conv2d(width, 2 * width, 3, stride=2, padding=1)
        self.fc = torch.nn.Linear(2 * width * (size // 2) ** 2, classes)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        h = self.conv2(self.act(self.conv1(x)))
        return self.fc(torch.flatten(_plain(h), 1))


def tiny_cnn(device="cpu", dtype=torch.float32, seed=0) -> TinyCNN:
    torch.manual_seed(seed)
    return TinyCNN().to(device, dtype)


CONV = ff.nn.quantized_conv_modules()


def quantize_cnn(model: TinyCNN) -> TinyCNN:
    surrogates = ff.nn.surrogate_quantized_modules(model, extra_conversion=CONV)
    return ff.quantize_model(model, extra_conversion={**CONV, **surrogates})


def install_quantizers(model: torch.nn.Module, device="cpu") -> None:
    """W8A8: per-tensor asymmetric int8 activations (each quantized once: conv1's input, the ReLU's output — conv2's input —
    conv2's output and the linear's input), per-channel symmetric int8 weights."""
    act = lambda: ff.nn.LinearQuantizer(8, symmetric=False, quantized_dtype=torch.int8, device=device)  # noqa: E731
    model.conv1.input_quantizer = act()
    model.act.input_quantizer = act()
    model.act.output_quantizer = act()
    model.conv2.output_quantizer = act()
    model.fc.input_quantizer = act()
    for m in (model.conv1, model.conv2, model.fc):
        m.weight_quantizer = ff.nn.LinearQuantizer(8, granularity=ff.PerChannel(0), quantized_dtype=torch.int8, device=device)


# ---- conversion and tags ---------------------------------------------------------------------------------------------------------
TAGS = {"input_quantizer": "activation/input", "weight_quantizer": "parameter/weight", "bias_quantizer": "parameter/bias",
        "output_quantizer": "activation/output"}


@pytest.mark.parametrize("cls,qcls,shape", [(torch.nn.Conv2d, "QuantizedConv2d", (6, 4, 3, 3)), (torch.nn.Conv1d, "QuantizedConv1d", (6, 4, 3))])
def test_quantize_model_converts_conv_with_the_reference_tags(cls, qcls, shape):
    model = ff.quantize_model(torch.nn.Sequential(cls(4, 6, 3)), extra_conversion=CONV)
    conv = model[0]
    assert type(conv) is getattr(ff.nn, qcls) and isinstance(conv, cls)
    assert CONV[cls] is getattr(ff.nn, qcls)
    for name, tag in TAGS.items():
        stub = getattr(conv, name)
        assert isinstance(stub, ff.nn.QuantizerStub) and tag in stub.quant_metadata, name
    assert tuple(conv.weight_quantizer.quant_metadata.shape) == shape
    assert tuple(conv.bias_quantizer.quant_metadata.shape) == (6,)


def test_a_conv_without_bias_has_no_bias_quantizer():
    for cls in (torch.nn.Conv2d, torch.nn.Conv1d):
        model = ff.quantize_model(torch.nn.Sequential(cls(4, 6, 3, bias=False)), extra_conversion=CONV)
        assert model[0].bias_quantizer is None
        assert isinstance(model[0].weight_quantizer, ff.nn.QuantizerStub)


def test_the_global_module_map_has_no_convolution():
    """Conversion is asked for: without it quantize_model raises on a convolution, as before these classes existed."""
    mapping = ff.nn.quantized_module_map()
    for cls in (torch.nn.Conv1d, torch.nn.Conv2d):
        assert cls not in mapping
        with pytest.raises(QuantizationError, match="no quantized version"):
            ff.quantize_model(torch.nn.Sequential(cls(1, 1, 1)))
    assert set(CONV) == {torch.nn.Conv1d, torch.nn.Conv2d} and CONV is not ff.nn.quantized_conv_modules()


def test_quantize_model_converts_the_tiny_cnn():
    model = quantize_cnn(tiny_cnn())
    assert type(model.conv1) is ff.nn.QuantizedConv2d and type(model.conv2) is ff.nn.QuantizedConv2d
    assert type(model.act) is ff.nn.QuantizedRelu and type(model.fc) is ff.nn.QuantizedLinear
    assert model.conv2.stride == (2, 2)


def test_functional_surface():
    assert {"conv1d", "conv2d"} <= set(ff.nn.functional.__all__)
    x = torch.randn(2, 4, 9, 9)
    w = torch.randn(5, 4, 3, 3)
    for padding in (1, (1, 2), "same", "valid"):
        out = ff.nn.functional.conv2d(x, w, None, 1, padding, 1, 1, strict_quantization=False)
        assert torch.equal(out, torch.nn.functional.conv2d(x, w, None, 1, padding))
    out = ff.nn.functional.conv1d(x[:, :, 0], w[:, :, 0], None, 2, 1, strict_quantization=False)
    assert torch.equal(out, torch.nn.functional.conv1d(x[:, :, 0], w[:, :, 0], None, 2, 1))


# ---- strict quantization: the reference's messages (_gen/fallback.py:116-214) ---------------------------------------------------
OUTPUT_MSG = "'output_quantizer' must be provided if strict_quantization=True"


def _expected(name):
    return f"Expected '{name}' to be an instance of 'QuantizedTensor' because strict_quantization=True."


@pytest.mark.parametrize("op,x,w", [("conv2d", torch.randn(1, 4, 6, 6), torch.randn(3, 4, 3, 3)), ("conv1d", torch.randn(1, 4, 6), torch.randn(3, 4, 3))])
def test_strict_mode_errors_match_the_reference(op, x, w):
    fn = getattr(ff.nn.functional, op)
    stub = ff.nn.QuantizerStub(output_quantizer=True)
    with pytest.raises(QuantizationError) as e:
        fn(x, w, strict_quantization=True)
    assert str(e.value) == OUTPUT_MSG
    with pytest.raises(QuantizationError) as e:
        fn(x, w, output_quantizer=stub, strict_quantization=True)
    assert str(e.value) == _expected("input")
    q = ff.nn.LinearQuantizer(8, symmetric=False)
    q.quantization_range = (torch.tensor(-3.0), torch.tensor(3.0))
    with pytest.raises(QuantizationError) as e:
        fn(q(x), w, output_quantizer=stub, strict_quantization=True)
    assert str(e.value) == _expected("weight")
    # the module default is strict, as in the reference: a stub input quantizer leaves a plain tensor
    model = ff.quantize_model(torch.nn.Sequential(torch.nn.Conv2d(4, 3, 3)), extra_conversion=CONV)
    with pytest.raises(QuantizationError) as e:
        model(torch.randn(1, 4, 6, 6))
    assert str(e.value) == _expected("input")


# ---- the host path against the reference (G20) -----------------------------------------------------------------------------------
def _set(module, name, spec, got):
    bits, symmetric, gran, lo, hi = spec
    granularity = ff.PerTensor() if gran == "tensor" else ff.PerChannel(gran[1])
    q = ff.nn.LinearQuantizer(bits, symmetric=symmetric, granularity=granularity, quantized_dtype=torch.int8)
    q.quantization_range = (torch.as_tensor(lo, dtype=torch.float32), torch.as_tensor(hi, dtype=torch.float32))
    with torch.no_grad():
        q.scale.copy_(got["scale"])
        if got["offset"] is not None:
            q.offset.copy_(got["offset"])
    setattr(module, name, q)


def build_g20_module(case, device="cpu"):
    """The case's module, converted, with its quantizers; returns (module, input)."""
    cls = torch.nn.Conv2d if case["kind"] == "conv2d" else torch.nn.Conv1d
    module = cls(case["in_channels"], case["out_channels"], case["kernel_size"], stride=case["stride"], padding=case["padding"],
                 dilation=case["dilation"], bias=case["bias"] is not None, padding_mode=case["padding_mode"]).to(case["x"].dtype)
    with torch.no_grad():
        module.weight.copy_(case["weight"])
        if case["bias"] is not None:
            module.bias.copy_(case["bias"])
    ff.quantize_model(module, extra_conversion=CONV)
    for name, spec in case["slots"].items():
        _set(module, name, spec, case["params"][name])
    module.to(device)
    return module, case["x"].to(device)


def run_g20_case(case, device="cpu"):
    """(value with a stub output quantizer, output QuantizedTensor) of the case's module."""
    module, x = build_g20_module(case, device)
    out_q = module.output_quantizer
    with torch.no_grad(), ff.strict_quantization(False):
        module.output_quantizer = ff.nn.QuantizerStub(output_quantizer=True)
        value = module(x)
        module.output_quantizer = out_q
        quantized = module(x)
    return value, quantized


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("index", range(14))
def test_host_path_equals_the_reference_bit_for_bit(index):
    case = golden("g20_conv.pt")[index]
    value, quantized = run_g20_case(case)
    assert value.dtype == case["value"].dtype and value.shape == case["value"].shape
    assert torch.equal(_bits(value), _bits(case["value"])), (case["kind"], case["dtype"])
    assert isinstance(quantized, ff.QuantizedTensor)
    assert torch.equal(quantized.raw_data, case["codes"])
    assert torch.equal(quantized.dequantize(), case["dequantized"])


def test_the_fixture_pins_the_ignored_padding_mode():
    case = next(c for c in golden("g20_conv.pt") if c["padding_mode"] == "reflect")
    x, w, b = case["x"].float(), case["weight"].float(), case["bias"].float()
    zero_padded = torch.nn.functional.conv2d(x, w, b, padding=1)
    reflected = torch.nn.functional.conv2d(torch.nn.functional.pad(x, (1, 1, 1, 1), mode="reflect"), w, b)
    got = case["value"].float()
    assert (got - zero_padded).abs().max() < (got - reflected).abs().max()


def test_estimate_ranges_calibrates_the_tiny_cnn():
    model = quantize_cnn(tiny_cnn())
    install_quantizers(model)
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(3))
    with ff.strict_quantization(False):
        with ff.estimate_ranges(model, ff.range_setting.running_minmax):
            model(x)
        out = model(x)
    assert all(not q.has_uninitialized_params for _, q in ff.nn.named_quantizers(model))
    assert out.shape == (2, 10) and torch.isfinite(_plain(out)).all()


def test_the_predicates_decline_host_tensors():
    q = ff.nn.LinearQuantizer(8, symmetric=False, quantized_dtype=torch.int8)
    q.quantization_range = (torch.tensor(-3.0), torch.tensor(3.0))
    wq = ff.nn.LinearQuantizer(8, quantized_dtype=torch.int8)
    wq.quantization_range = (torch.tensor(-1.0), torch.tensor(1.0))
    x, w = q(torch.randn(1, 16, 6, 6)), wq(torch.randn(8, 16, 3, 3))
    assert not fused_conv.conv2d_predicate(input=x, weight=w, output_quantizer=None, strict_quantization=False)
    assert not fused_conv.conv1d_predicate(input=q(torch.randn(1, 16, 6)), weight=wq(torch.randn(8, 16, 3)), output_quantizer=None,
                                           strict_quantization=False)


def test_geometry():
    g = fused_conv.geometry
    assert g(2, (8, 8), (3, 3), 1, 1, 1) == ((1, 1), (1, 1), (1, 1))
    assert g(2, (8, 8), (3, 5), 1, "same", 1) == ((1, 1), (1, 2), (1, 1))
    assert g(2, (8, 8), (4, 4), 1, "same", 1) is None       # asymmetric implied padding
    assert g(2, (8, 8), (3, 3), 2, "same", 1) is None       # F.conv2d raises
    assert g(2, (8, 8), (3, 3), 1, "valid", (2, 1)) == ((1, 1), (0, 0), (2, 1))
    assert g(2, (2, 2), (3, 3), 1, 0, 1) is None            # filter larger than the input
    assert g(1, (13,), (3,), 2, 1, 1) == ((1, 2), (0, 1), (1, 1))
    assert g(2, (8, 8), (3, 3), 1, "circular", 1) is None


# ---- the wrappers' shared validation ------------------------------------------------------------------------------------------------
OC = 4
WRAPPERS = {  # name -> (input shape, weight shape), OC output channels each: a few dozen elements
    "conv2d_w8a8": ((1, 2, 4, 4), (OC, 2, 3, 3)),
    "depthwise_conv2d_w8a8": ((1, 2, 4, 4), (OC, 1, 3, 3)),
    "conv_transpose2d_w8a8": ((1, 2, 4, 4), (2, OC, 3, 3)),
    "conv3d_w8a8": ((1, 2, 3, 4, 4), (OC, 2, 2, 3, 3)),
}


def _wrapper_error(name, **change):
    """The exception `name` raises on otherwise valid operands with `change` applied (these checks run before any library is touched)."""
    x_shape, w_shape = WRAPPERS[name]
    one = torch.ones(1)
    call = dict(x_codes=torch.zeros(x_shape, dtype=torch.int8), w_codes=torch.zeros(w_shape, dtype=torch.int8), x_scale=one, x_offset=None,
                w_scale=one, w_offset=None)
    call.update(change)
    with pytest.raises((TypeError, RuntimeError)) as caught:
        getattr(ff.ops, name)(**call)
    return type(caught.value), str(caught.value).replace(name, "<op>")


@pytest.mark.parametrize(
    "change,kind,text",
    [
        (dict(x_codes=torch.zeros(1, 2, 4, 4)), TypeError, "<op> expects int8 codes"),
        (dict(x_scale=torch.ones(2)), RuntimeError, "<op>: the input has one parameter pair (per-tensor)"),
        (dict(w_scale=torch.ones(OC + 1)), RuntimeError, "<op>: the weight has 1 or 4 parameter pairs, got 5"),
        (dict(bias=torch.zeros(OC - 1)), RuntimeError, "<op>: the bias is [4] of f32, bf16 or f16"),
        (dict(out_dtype=torch.int8), RuntimeError, "<op>: a real-valued output is f32, bf16 or f16, got torch.int8"),
    ],
)
def test_the_four_wrappers_check_their_operands_alike(change, kind, text):
    errors = {name: _wrapper_error(name, **change) for name in WRAPPERS}
    assert set(errors.values()) == {(kind, text)}, errors   # one type, and one message but for the op's name


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_the_hip_library_exports_both_symbols():
    dll = ctypes.CDLL(str(HIP_SO))
    lib = FFQLibrary(HIP_SO)
    for name in ENTRY_POINTS:
        assert hasattr(dll, name) and name in _cabi.SIGNATURES and name in _cabi.DEVICE_ONLY
        assert getattr(lib, name) is not None
    assert "conv2d_w8a8" in ff.ops.__all__ and ff.ops.conv2d_w8a8


def test_the_oracle_loads_without_them():
    lib = load_oracle()
    assert not lib.is_device
    for name in ENTRY_POINTS:
        assert getattr(lib, name) is None


FAKE = 1 << 20  # never dereferenced: every call below returns from the argument checks


def _conv(lib, x=FAKE, nhwc=0, w=FAKE, xs=FAKE, ws=FAKE, bias=None, bias_dt=0, out=FAKE, out_dt=DType.BF16, out_scale=None, bits=8.0,
          y_dt=0, B=2, C=16, H=8, W=8, OC=32, KH=3, KW=3, s=(1, 1), p=(1, 1), d=(1, 1), workspace=FAKE, nbytes=None):
    if nbytes is None:
        nbytes = lib.ffq_conv2d_w8a8_workspace_bytes(B, C, H, W, OC, KH, KW, nhwc) if C > 0 and KH > 0 and KW > 0 else 0
    return lib.ffq_conv2d_w8a8(x, nhwc, w, xs, None, ws, None, 0, bias, bias_dt, out, out_dt, out_scale, None, bits, y_dt, B, C, H, W, OC, KH,
                               KW, s[0], s[1], p[0], p[1], d[0], d[1], workspace, nbytes, None)


@pytest.mark.parametrize(
    "call,status",
    [
        (lambda lib: _conv(lib, B=-1), Status.ERR_ARG),
        (lambda lib: _conv(lib, C=0), Status.ERR_EMPTY),
        (lambda lib: _conv(lib, s=(0, 1)), Status.ERR_ARG),
        (lambda lib: _conv(lib, d=(1, 0)), Status.ERR_ARG),
        (lambda lib: _conv(lib, p=(-1, 0)), Status.ERR_ARG),
        (lambda lib: _conv(lib, C=16385, KH=3, KW=3), Status.ERR_DTYPE),      # C * KH * KW >= 131072
        (lambda lib: _conv(lib, C=1 << 62, KH=2, KW=2), Status.ERR_DTYPE),     # ... and no int64 overflow on the way: 2^64 wraps to 0
        (lambda lib: _conv(lib, C=1 << 40, KH=1 << 24, KW=1 << 24, p=(1 << 24, 1 << 24)), Status.ERR_DTYPE),
        (lambda lib: _conv(lib, nhwc=1, C=24), Status.ERR_DTYPE),             # channels-last needs C % 16 == 0
        (lambda lib: _conv(lib, H=2, p=(0, 0)), Status.ERR_ARG),              # filter larger than the padded input
        (lambda lib: _conv(lib, bias=FAKE, bias_dt=DType.I8), Status.ERR_DTYPE),
        (lambda lib: _conv(lib, out_dt=DType.I8), Status.ERR_DTYPE),          # codes out without an output quantizer
        (lambda lib: _conv(lib, out_scale=FAKE, out_dt=DType.BF16, y_dt=DType.BF16), Status.ERR_DTYPE),
        (lambda lib: _conv(lib, out_scale=FAKE, out_dt=DType.I8, y_dt=DType.BF16, bits=11.0), Status.ERR_PRECISION),
        (lambda lib: _conv(lib, out_scale=FAKE, out_dt=DType.I8, y_dt=DType.I8), Status.ERR_DTYPE),
        (lambda lib: _conv(lib, x=None), Status.ERR_ARG),
        (lambda lib: _conv(lib, xs=None), Status.ERR_ARG),
        (lambda lib: _conv(lib, nhwc=1, x=FAKE + 8), Status.ERR_ARG),         # misaligned channels-last codes
        (lambda lib: _conv(lib, workspace=None), Status.ERR_WORKSPACE),
        (lambda lib: _conv(lib, nbytes=1024), Status.ERR_WORKSPACE),
        (lambda lib: _conv(lib, B=0), Status.OK),
        (lambda lib: _conv(lib, OC=0), Status.OK),
    ],
)
def test_argument_checks_need_no_device(call, status):
    lib = FFQLibrary(HIP_SO)
    assert call(lib) == status
    if status != Status.OK:
        assert lib.ffq_last_error()


def test_workspace_bytes():
    lib = FFQLibrary(HIP_SO)
    # NHWC input [2, 8, 8, 16] + weight [32, 3, 3, 16] + tap sums (32 * 9 + 32) int32, each rounded up to 256 bytes
    assert lib.ffq_conv2d_w8a8_workspace_bytes(2, 3, 8, 8, 32, 3, 3, 0) == 2048 + 4608 + 1280
    assert lib.ffq_conv2d_w8a8_workspace_bytes(2, 16, 8, 8, 32, 3, 3, 1) == 4608 + 1280
    assert lib.ffq_conv2d_w8a8_workspace_bytes(1 << 20, 16, 1 << 24, 1 << 24, 32, 3, 3, 0) == 0   # no launch takes it; no overflow into a small number


def test_the_new_kernels_spill_nothing_and_use_no_scratch():
    if kernel_resources.readelf() is None or not kernel_resources.DEFAULT_LIBRARY.exists():
        pytest.skip("llvm-readelf or the built library is missing")
    rows = [k for k in kernel_resources.kernel_resources() if any(n in str(k["name"]) for n in KERNELS)]
    for needle, count in zip(KERNELS, (1, 4)):
        assert sum(needle in str(k["name"]) for k in rows) == count, needle
    bad = {str(k["name"]): k for k in rows if k["vgpr_spill_count"] or k["sgpr_spill_count"] or k["private_segment_fixed_size"]}
    assert not bad, bad
    assert all(k["group_segment_fixed_size"] <= 33280 for k in rows)
