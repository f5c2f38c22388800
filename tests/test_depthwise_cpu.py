"""The quantized depthwise conv1d / conv2d without a GPU: the host path against the reference's outputs (fixture G28), the predicate
on what it accepts and declines, the third header ``include/ffq_depthwise.h`` against ``_cabi.SIGNATURES_DEPTHWISE`` (exported by the
HIP library, absent from the oracle, the other two tables untouched), every argument error of the entry point in the documented
order before any device call, and what hipcc emitted for the new kernels."""

import ctypes
import re
import sys

import pytest
import torch

import fastforward_amd as ff

from conftest import HIP_SO, ROOT, golden, load_oracle
from fastforward_amd import _cabi, fused_conv, fused_depthwise
from fastforward_amd._cabi import DType, FFQLibrary, Status
from fastforward_amd.exceptions import BackendError

sys.path.insert(0, str(ROOT / "tools"))

import kernel_resources  # noqa: E402

ENTRY = "ffq_depthwise_conv2d_w8a8"
F = ff.nn.functional
N_CASES = 22


# ---- the host path against the reference (G28) -----------------------------------------------------------------------------------
def g28_quantizer(spec, got, device="cpu"):
    bits, symmetric, gran, lo, hi = spec
    granularity = ff.PerTensor() if gran == "tensor" else ff.PerChannel(gran[1])
    q = ff.nn.LinearQuantizer(bits, symmetric=symmetric, granularity=granularity, quantized_dtype=torch.int8)
    q.quantization_range = (torch.as_tensor(lo, dtype=torch.float32), torch.as_tensor(hi, dtype=torch.float32))
    with torch.no_grad():
        q.scale.copy_(got["scale"])
        if got["offset"] is not None:
            q.offset.copy_(got["offset"])
    return q.to(device)


def run_g28(case, device="cpu"):
    """(value without an output quantizer, output QuantizedTensor) of the case's conv call (shared with the GPU tests)."""
    qs = {name: g28_quantizer(spec, case["params"][name], device) for name, spec in case["slots"].items()}
    op = F.conv1d if case["dims"] == 1 else F.conv2d
    with torch.no_grad(), ff.strict_quantization(False):
        xq = qs["input_quantizer"](case["x"].to(device))
        wq = qs["weight_quantizer"](case["weight"].to(device))
        bias = None if case["bias"] is None else case["bias"].to(device)
        if case["bias_kind"] == "quantized":
            bias = qs["bias_quantizer"](bias)
        args = (xq, wq, bias, case["stride"], case["padding"], case["dilation"], case["groups"])
        return op(*args), op(*args, output_quantizer=qs["output_quantizer"])


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("index", range(N_CASES))
def test_host_path_equals_the_reference_bit_for_bit(index):
    case = golden("g28_depthwise.pt")["conv"][index]
    value, quantized = run_g28(case)
    assert value.dtype == case["value"].dtype and value.shape == case["value"].shape
    assert torch.equal(_bits(value), _bits(case["value"])), (index, case["dtype"])
    assert isinstance(quantized, ff.QuantizedTensor)
    assert torch.equal(quantized.raw_data, case["codes"])
    assert torch.equal(quantized.dequantize(), case["dequantized"])


def test_the_fixture_covers_what_it_names():
    conv = golden("g28_depthwise.pt")["conv"]
    assert len(conv) == N_CASES and {c["dtype"] for c in conv} == {"torch.float32", "torch.bfloat16"}
    assert all(c["groups"] == c["x"].shape[1] and c["weight"].shape[1] == 1 for c in conv)
    assert {c["groups"] for c in conv} == {3, 5, 8} and {c["multiplier"] for c in conv} == {1, 2, 3}
    assert {c["bias_kind"] for c in conv} == {None, "plain", "quantized"}
    assert {c["w_kind"] for c in conv} == {"tensor", "tensor-asym", "channel", "channel-asym"}
    kernels = {tuple(c["weight"].shape[2:]) for c in conv}
    assert {(3, 3), (5, 5), (7, 7), (1, 1), (31,), (4,), (1, 5)} <= kernels
    assert any(c["padding"] == "same" and c["dilation"] == 2 for c in conv) and any(c["stride"] == 2 and c["x"].shape[2] % 2 for c in conv)
    assert (ROOT / "tests" / "golden" / "g28_depthwise.pt").stat().st_size <= 1 << 20


# ---- the predicate -----------------------------------------------------------------------------------------------------------------
def _codes(shape, lo=-3.0, hi=3.0, granularity=None, symmetric=False, lo_hi_shape=None, dtype=torch.float32):
    q = ff.nn.LinearQuantizer(8, symmetric=symmetric, granularity=granularity or ff.PerTensor(), quantized_dtype=torch.int8)
    if lo_hi_shape is None:
        q.quantization_range = (torch.tensor(lo), torch.tensor(hi))
    else:
        q.quantization_range = (torch.full((lo_hi_shape,), lo), torch.full((lo_hi_shape,), hi))
    return q(torch.randn(shape).to(dtype))


def _w(shape, **k):
    return _codes(shape, -1.0, 1.0, symmetric=True, **k)


def test_the_predicate_accepts_and_declines(monkeypatch):
    x, w = _codes((2, 16, 9, 10)), _w((16, 1, 3, 3))
    common = dict(output_quantizer=None, strict_quantization=False)
    # host tensors: nothing here is on the device
    assert not fused_depthwise.conv2d_predicate(input=x, weight=w, groups=16, **common)
    assert not fused_depthwise.conv1d_predicate(input=_codes((2, 16, 40)), weight=_w((16, 1, 4)), groups=16, **common)
    # ... and with the device check out of the way, each rule on its own (the geometry and operand rules read no memory)
    monkeypatch.setattr("fastforward_amd.fused_conv._on_device", lambda *t: True)

    def ok(dims=2, **k):  # inference, as the models run: under grad mode the quantizers' learnable parameters decline every call
        with torch.no_grad():
            return fused_depthwise.KERNELS.supported(dims, **{**dict(input=x, weight=w, groups=16), **common, **k})

    assert ok()
    assert ok(padding="same") and ok(padding="valid") and ok(padding=(1, 0), stride=(1, 2), dilation=(2, 1))
    assert ok(weight=_w((48, 1, 3, 3))) and ok(weight=_w((32, 1, 3, 3)), bias=torch.randn(32))          # channel multipliers 3 and 2
    assert ok(1, input=_codes((2, 16, 40)), weight=_w((16, 1, 31)), padding=15)                           # conv1d
    assert ok(weight=_w((16, 1, 3, 3), granularity=ff.PerChannel(0), lo_hi_shape=16))
    # groups
    assert not ok(groups=2, weight=_w((16, 8, 3, 3))) and not ok(groups=2) and not ok(groups=1) and not ok(groups=8, weight=_w((16, 2, 3, 3)))
    assert not fused_conv.KERNELS.supported(2, input=x, weight=_w((16, 8, 3, 3)), groups=2, **common)     # ... nor does the GEMM take it
    assert not ok(input=_codes((2, 1, 9, 10)), weight=_w((1, 1, 3, 3)), groups=1)                         # C = 1 is the GEMM's
    assert not ok(input=_codes((2, 1, 9, 10)), weight=_w((4, 1, 3, 3)), groups=1)
    assert not ok(weight=_w((16, 2, 3, 3))) and not ok(weight=_w((24, 1, 3, 3)))                          # weight.shape[1] != 1; OC % C != 0
    assert not ok(groups=True) and not ok(groups=16.0)
    # taps
    big = _codes((1, 2, 40, 45))
    assert ok(input=big, weight=_w((2, 1, 32, 32)), groups=2, padding=0)                                  # 1024 taps
    assert not ok(input=big, weight=_w((2, 1, 25, 41)), groups=2)                                         # 1025 taps
    assert ok(1, input=_codes((1, 2, 1100)), weight=_w((2, 1, 1024)), groups=2) and not ok(1, input=_codes((1, 2, 1100)), weight=_w((2, 1, 1025)), groups=2)
    # operands
    assert not ok(input=_codes((2, 16, 9, 10), granularity=ff.PerChannel(1), lo_hi_shape=16))             # per-channel activations
    assert not ok(weight=_w((16, 1, 3, 3), granularity=ff.PerChannel(1), lo_hi_shape=1))                  # PerChannel(1) weights
    assert not ok(weight=_w((16, 1, 3, 3), granularity=ff.PerChannel(2), lo_hi_shape=3))
    assert not ok(weight=_w((16, 1, 3, 3), dtype=torch.bfloat16))                                         # dtype mismatch
    assert not ok(bias=torch.randn(16).bfloat16()) and ok(bias=torch.randn(16)) and not ok(bias=torch.randn(15))
    assert not ok(input=torch.randn(2, 16, 9, 10)) and not ok(weight=torch.randn(16, 1, 3, 3))            # plain floats
    assert not ok(input=_codes((16, 9, 10))) and not ok(1)                                                # unbatched; conv1d on 4-D operands
    # geometry
    assert not ok(padding="same", weight=_w((16, 1, 2, 3)))                                               # 'same' with an even kernel: asymmetric
    assert not ok(padding="same", stride=2) and not ok(padding=(1, 1, 1)) and not ok(padding=-1) and not ok(stride=0) and not ok(dilation=1.0)
    assert not ok(weight=_w((16, 1, 11, 3)))                                                              # the filter exceeds the input
    assert not ok(strict_quantization=True)                                                               # strict without an output quantizer
    with torch.enable_grad():
        assert not fused_depthwise.KERNELS.supported(2, input=x, weight=w, groups=16, **common)           # a gradient is needed


def test_both_kernels_are_registered_and_the_gemm_predicate_is_untouched(monkeypatch):
    from fastforward_amd import dispatcher, fused_conv3d, fused_conv_transpose

    for op in ("conv1d", "conv2d"):
        fns = [item.fn for item in dispatcher._DISPATCHER[op]]
        assert getattr(fused_depthwise.KERNELS, op) in fns and getattr(fused_conv.KERNELS, op) in fns and len(fns) == 2
    # the depthwise rules do not leak into the other sets, nor theirs into it: with the device check out of the way (as above), the
    # depthwise operands are declined by every groups == 1 predicate, which takes its own groups == 1 call, and the reverse
    monkeypatch.setattr("fastforward_amd.fused_conv._on_device", lambda *t: True)
    common = dict(output_quantizer=None, strict_quantization=False)
    x, x3 = _codes((2, 16, 9, 10)), _codes((2, 16, 6, 9, 10))
    transposed = (fused_conv_transpose.conv_transpose2d_predicate, fused_conv_transpose.KERNELS.supported_conv_transpose2d)
    with torch.no_grad():
        assert fused_depthwise.KERNELS.supported(2, input=x, weight=_w((16, 1, 3, 3)), groups=16, **common)
        assert not fused_conv.conv2d_predicate(input=x, weight=_w((16, 1, 3, 3)), groups=16, **common)
        assert not fused_conv3d.conv3d_predicate(input=x3, weight=_w((16, 1, 3, 3, 3)), groups=16, **common)
        for predicate in transposed:
            assert not predicate(input=x, weight=_w((16, 1, 3, 3)), groups=16, **common)
        assert not fused_conv_transpose.conv_transpose1d_predicate(input=_codes((2, 16, 40)), weight=_w((16, 1, 3)), groups=16, **common)
        assert fused_conv.conv2d_predicate(input=x, weight=_w((16, 16, 3, 3)), groups=1, **common)
        assert fused_conv3d.conv3d_predicate(input=x3, weight=_w((16, 16, 3, 3, 3)), groups=1, **common)
        for predicate in transposed:
            assert predicate(input=x, weight=_w((16, 1, 3, 3)), groups=1, **common)
        assert fused_conv_transpose.conv_transpose1d_predicate(input=_codes((2, 16, 40)), weight=_w((16, 1, 3)), groups=1, **common)
        for weight in (_w((16, 1, 3, 3)), _w((16, 16, 3, 3))):
            assert not fused_depthwise.conv2d_predicate(input=x, weight=weight, groups=1, **common)
            assert not fused_depthwise.KERNELS.supported(2, input=x, weight=weight, groups=1, **common)


def test_the_wrapper_says_not_covered_on_a_library_without_the_symbol(oracle_backend):
    one = torch.ones(1)
    with pytest.raises(BackendError, match="not covered"):
        ff.ops.depthwise_conv2d_w8a8(torch.zeros(1, 4, 5, 5, dtype=torch.int8), torch.zeros(4, 1, 3, 3, dtype=torch.int8), one, None, one, None)
    assert "depthwise_conv2d_w8a8" in ff.ops.__all__


def test_the_wrapper_checks_its_operands():
    one = torch.ones(1)
    x, w = torch.zeros(1, 4, 5, 5, dtype=torch.int8), torch.zeros(4, 1, 3, 3, dtype=torch.int8)
    with pytest.raises(TypeError):
        ff.ops.depthwise_conv2d_w8a8(x.float(), w, one, None, one, None)
    for bad_w in (torch.zeros(4, 2, 3, 3, dtype=torch.int8), torch.zeros(6, 1, 3, 3, dtype=torch.int8)):
        with pytest.raises(RuntimeError, match=r"\[C \* M, 1, KH, KW\]"):
            ff.ops.depthwise_conv2d_w8a8(x, bad_w, one, None, one, None)
    with pytest.raises(RuntimeError, match="parameter pairs"):
        ff.ops.depthwise_conv2d_w8a8(x, w, one, None, torch.ones(3), None)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def _declared(header):
    text = (ROOT / "include" / header).read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(ffq_[a-z0-9_]+)\s*\(", text))


def test_the_third_header_and_its_table_agree():
    assert _declared("ffq_depthwise.h") == set(_cabi.SIGNATURES_DEPTHWISE) == {ENTRY}
    assert '#include "ffq.h"' in (ROOT / "include" / "ffq_depthwise.h").read_text()
    # the prototype's parameters, one ctypes type each
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "ffq_depthwise.h").read_text(), flags=re.S)
    params = re.search(ENTRY + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    want = [ctypes.c_void_p if "*" in p else kinds[p.split()[-2]] for p in params]
    restype, argtypes = _cabi.SIGNATURES_DEPTHWISE[ENTRY]
    assert restype is ctypes.c_int and argtypes == want


def test_the_other_tables_are_untouched_and_disjoint():
    assert _declared("ffq.h") == set(_cabi.SIGNATURES) and _declared("ffq_3d.h") == set(_cabi.SIGNATURES_3D)
    mine = set(_cabi.SIGNATURES_DEPTHWISE)
    assert not mine & set(_cabi.SIGNATURES) and not mine & set(_cabi.SIGNATURES_3D) and not mine & _cabi.DEVICE_ONLY
    assert _cabi.FFQ_ABI_VERSION == 9 and "#define FFQ_ABI_VERSION 9" in (ROOT / "include" / "ffq.h").read_text()


def test_the_hip_library_exports_it_and_the_oracle_loads_without_it():
    assert hasattr(ctypes.CDLL(str(HIP_SO)), ENTRY) and getattr(FFQLibrary(HIP_SO), ENTRY) is not None
    lib = load_oracle()
    assert not lib.is_device and getattr(lib, ENTRY) is None


FAKE = 1 << 20  # never dereferenced: every call below returns from the argument checks


def _conv(lib, x=FAKE, w=FAKE, xs=FAKE, ws=FAKE, bias=None, bias_dt=0, out=FAKE, out_dt=DType.BF16, out_scale=None, bits=8.0, y_dt=0,
          B=2, C=16, M=1, H=8, W=8, K=(3, 3), s=(1, 1), p=(1, 1), d=(1, 1)):
    return getattr(lib, ENTRY)(x, w, xs, None, ws, None, 0, bias, bias_dt, out, out_dt, out_scale, None, bits, y_dt, B, C, M, H, W, *K, *s,
                               *p, *d, None)


# in the documented order: each call fails the named check and passes every check ahead of it; most fail a LATER check too and must
# report the earlier one
ERRORS = [
    (lambda lib: _conv(lib, B=-1, M=0), Status.ERR_ARG),                                   # negative extent, before the empty filter
    (lambda lib: _conv(lib, H=-1), Status.ERR_ARG),
    (lambda lib: _conv(lib, C=-1, K=(0, 3)), Status.ERR_ARG),
    (lambda lib: _conv(lib, M=0, s=(0, 1)), Status.ERR_EMPTY),                             # empty filter, before the stride
    (lambda lib: _conv(lib, K=(0, 3)), Status.ERR_EMPTY),
    (lambda lib: _conv(lib, K=(3, 0), C=0), Status.ERR_EMPTY),                             # ... and before C == 0 returns OK
    (lambda lib: _conv(lib, s=(0, 1), K=(1 << 25, 3)), Status.ERR_ARG),                    # stride
    (lambda lib: _conv(lib, d=(1, 0)), Status.ERR_ARG),
    (lambda lib: _conv(lib, p=(-1, 0)), Status.ERR_ARG),
    (lambda lib: _conv(lib, H=(1 << 24) + 1, K=(33, 32)), Status.ERR_ARG),                 # above 2^24, before the tap bound
    (lambda lib: _conv(lib, s=(1, (1 << 24) + 1)), Status.ERR_ARG),
    (lambda lib: _conv(lib, K=(1 << 24, 1 << 24)), Status.ERR_DTYPE),                      # taps; no int64 overflow on the way
    (lambda lib: _conv(lib, K=(25, 41)), Status.ERR_DTYPE),                                # 1025 taps; before the filter size
    (lambda lib: _conv(lib, K=(1, 1025), p=(0, 600), bias=FAKE, bias_dt=DType.I8), Status.ERR_DTYPE),
    (lambda lib: _conv(lib, K=(11, 3), bias=FAKE, bias_dt=DType.I8), Status.ERR_ARG),      # the filter exceeds the padded input; before the bias
    (lambda lib: _conv(lib, W=0, p=(1, 0)), Status.ERR_ARG),
    (lambda lib: _conv(lib, B=1 << 30, bias=FAKE, bias_dt=DType.I8), Status.ERR_ARG),      # B * OH * OW >= 2^31; before the bias
    (lambda lib: _conv(lib, C=1 << 20, M=1 << 11, bias=FAKE, bias_dt=DType.I8), Status.ERR_ARG),   # C * M >= 2^31
    (lambda lib: _conv(lib, B=1 << 12, C=1 << 12, bias=FAKE, bias_dt=DType.I8), Status.ERR_ARG),   # 2^24 blocks
    (lambda lib: _conv(lib, B=1 << 33, C=0), Status.ERR_ARG),                              # ... also with no channel at all
    (lambda lib: _conv(lib, bias=FAKE, bias_dt=DType.I8, out_dt=DType.I8), Status.ERR_DTYPE),
    (lambda lib: _conv(lib, out_dt=DType.I8, x=None), Status.ERR_DTYPE),                   # codes out without an output quantizer; before NULL
    (lambda lib: _conv(lib, out_scale=FAKE, out_dt=DType.BF16, y_dt=DType.BF16, bits=11.0), Status.ERR_DTYPE),
    (lambda lib: _conv(lib, out_scale=FAKE, out_dt=DType.I8, y_dt=DType.I8, bits=11.0), Status.ERR_PRECISION),
    (lambda lib: _conv(lib, out_scale=FAKE, out_dt=DType.I8, y_dt=DType.I8, x=None), Status.ERR_DTYPE),
    (lambda lib: _conv(lib, x=None), Status.ERR_ARG),
    (lambda lib: _conv(lib, w=None), Status.ERR_ARG),
    (lambda lib: _conv(lib, xs=None), Status.ERR_ARG),
    (lambda lib: _conv(lib, ws=None), Status.ERR_ARG),
    (lambda lib: _conv(lib, out=None), Status.ERR_ARG),
    (lambda lib: _conv(lib, B=0, x=None, out=None), Status.OK),
    (lambda lib: _conv(lib, C=0, x=None, w=None), Status.OK),
    (lambda lib: _conv(lib, B=0, out_dt=DType.I8), Status.ERR_DTYPE),                      # ... but the dtype checks come first
    (lambda lib: _conv(lib, C=0, K=(11, 3)), Status.ERR_ARG),                              # ... and the geometry
]


@pytest.mark.parametrize("index", range(len(ERRORS)))
def test_argument_checks_need_no_device(index):
    call, status = ERRORS[index]
    lib = FFQLibrary(HIP_SO)
    assert call(lib) == status
    if status != Status.OK:
        assert lib.ffq_last_error()


def test_the_new_kernels_spill_nothing_and_use_no_scratch():
    if kernel_resources.readelf() is None:
        pytest.skip("llvm-readelf is missing")
    assert kernel_resources.DEFAULT_LIBRARY.exists(), "build() leaves the HIP library in the tree"
    rows = [k for k in kernel_resources.kernel_resources() if "depthwise_w8a8_kernel" in str(k["name"])]
    assert len(rows) == 12  # {f32, bf16, f16, fused int8 codes} x {dense, strided, direct}
    bad = {str(k["name"]): k for k in rows if k["vgpr_spill_count"] or k["sgpr_spill_count"] or k["private_segment_fixed_size"]}
    assert not bad, bad
    # the taps and the patch are dynamic LDS (at most 48 KiB, set by the launch); the static part is the four wave sums
    assert all(k["group_segment_fixed_size"] <= 64 and k["vgpr_count"] + k["agpr_count"] <= 128 for k in rows), rows
