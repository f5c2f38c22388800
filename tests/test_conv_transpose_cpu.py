"""Quantized conv_transpose1d / conv_transpose2d without a GPU: the functional surface and the reference's strict-mode errors, the
host path against the reference's outputs (fixture G26), the module classes (conversion only on request, ``output_size``), the
predicates on host tensors, ``transposed_geometry``, the phase table by brute force, the C-ABI entry points (exported by the HIP
library, absent from the oracle, argument checks before any device call) and what hipcc emitted for the new kernels."""

import ctypes
import itertools
import sys

import pytest
import torch

import fastforward_amd as ff

from conftest import HIP_SO, ROOT, golden, load_oracle
from fastforward_amd import _cabi, fused_conv_transpose
from fastforward_amd._cabi import DType, FFQLibrary, Status
from fastforward_amd.exceptions import QuantizationError
from fastforward_amd.ops.conv import MAX_PHASES, axis_phases, phase_table

sys.path.insert(0, str(ROOT / "tools"))

import kernel_resources  # noqa: E402

ENTRY_POINTS = ("ffq_conv_transpose2d_w8a8", "ffq_conv_transpose2d_w8a8_workspace_bytes")
KERNELS = ("convt_reorder_kernel", "convt_w8a8_kernel")
CONVT = ff.nn.quantized_conv_transpose_modules()
F = ff.nn.functional


# ---- the functional surface --------------------------------------------------------------------------------------------------------
def test_functional_surface():
    assert {"conv_transpose1d", "conv_transpose2d"} <= set(F.__all__)
    assert "conv_transpose2d" in F.__doc__ and not hasattr(F, "conv_transpose3d")
    x = torch.randn(2, 4, 5, 6)
    w = torch.randn(4, 3, 3, 2)
    b = torch.randn(3)
    for stride, padding, output_padding, dilation in ((1, 0, 0, 1), (2, 1, 1, 1), ((2, 3), (1, 0), (1, 2), (2, 3)), (3, 0, 0, 1)):
        out = F.conv_transpose2d(x, w, b, stride, padding, output_padding, 1, dilation, strict_quantization=False)
        assert torch.equal(out, torch.nn.functional.conv_transpose2d(x, w, b, stride, padding, output_padding, 1, dilation))
    out = F.conv_transpose1d(x[:, :, 0], w[:, :, 0], None, 2, 1, 1, strict_quantization=False)
    assert torch.equal(out, torch.nn.functional.conv_transpose1d(x[:, :, 0], w[:, :, 0], None, 2, 1, 1))
    grouped = F.conv_transpose2d(x, torch.randn(4, 3, 2, 2), None, 2, groups=2, strict_quantization=False)
    assert grouped.shape == (2, 6, 10, 12)


# ---- strict quantization: the reference's messages (_gen/fallback.py:346-449), in its order -------------------------------------------
OUTPUT_MSG = "'output_quantizer' must be provided if strict_quantization=True"


def _expected(name):
    return f"Expected '{name}' to be an instance of 'QuantizedTensor' because strict_quantization=True."


@pytest.mark.parametrize("op,x,w", [("conv_transpose2d", torch.randn(1, 4, 6, 6), torch.randn(4, 3, 3, 3)),
                                    ("conv_transpose1d", torch.randn(1, 4, 6), torch.randn(4, 3, 3))])
def test_strict_mode_errors_match_the_reference(op, x, w):
    fn = getattr(F, op)
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
    # the module default is strict: a stub input quantizer leaves a plain tensor
    cls = torch.nn.ConvTranspose2d if op == "conv_transpose2d" else torch.nn.ConvTranspose1d
    model = ff.quantize_model(torch.nn.Sequential(cls(4, 3, 3)), extra_conversion=CONVT)
    with pytest.raises(QuantizationError) as e:
        model(x)
    assert str(e.value) == _expected("input")


# ---- the host path against the reference (G26) -----------------------------------------------------------------------------------
def g26_quantizer(spec, got, device="cpu"):
    bits, symmetric, gran, lo, hi = spec
    granularity = ff.PerTensor() if gran == "tensor" else ff.PerChannel(gran[1])
    q = ff.nn.LinearQuantizer(bits, symmetric=symmetric, granularity=granularity, quantized_dtype=torch.int8)
    q.quantization_range = (torch.as_tensor(lo, dtype=torch.float32), torch.as_tensor(hi, dtype=torch.float32))
    with torch.no_grad():
        q.scale.copy_(got["scale"])
        if got["offset"] is not None:
            q.offset.copy_(got["offset"])
    return q.to(device)


def run_g26_case(case, device="cpu"):
    """(value without an output quantizer, output QuantizedTensor) of the case's functional call (shared with the GPU tests)."""
    qs = {name: g26_quantizer(spec, case["params"][name], device) for name, spec in case["slots"].items()}
    fn = getattr(F, case["kind"])
    with torch.no_grad(), ff.strict_quantization(False):
        xq = qs["input_quantizer"](case["x"].to(device))
        wq = qs["weight_quantizer"](case["weight"].to(device))
        bias = None if case["bias"] is None else case["bias"].to(device)
        if case["bias_kind"] == "quantized":
            bias = qs["bias_quantizer"](bias)
        args = (xq, wq, bias, case["stride"], case["padding"], case["output_padding"], 1, case["dilation"])
        return fn(*args), fn(*args, output_quantizer=qs["output_quantizer"])


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("index", range(20))
def test_host_path_equals_the_reference_bit_for_bit(index):
    case = golden("g26_conv_transpose.pt")[index]
    value, quantized = run_g26_case(case)
    assert value.dtype == case["value"].dtype and value.shape == case["value"].shape
    assert torch.equal(_bits(value), _bits(case["value"])), (case["kind"], case["dtype"])
    assert isinstance(quantized, ff.QuantizedTensor)
    assert torch.equal(quantized.raw_data, case["codes"])
    assert torch.equal(quantized.dequantize(), case["dequantized"])


def test_the_fixture_covers_what_it_names():
    cases = golden("g26_conv_transpose.pt")
    assert len(cases) == 20 and {c["dtype"] for c in cases} == {"torch.float32", "torch.bfloat16"}
    assert {c["bias_kind"] for c in cases} == {None, "plain", "quantized"}
    assert any(max(c["output_padding"]) > 0 for c in cases) and any(max(c["dilation"]) > 1 for c in cases)
    assert any(c["kind"] == "conv_transpose1d" and c["weight"].shape[2] == 16 and c["stride"] == (8,) and c["padding"] == (4,) for c in cases)
    assert any(s > d * (k - 1) + 1 for c in cases for s, d, k in zip(c["stride"], c["dilation"], c["weight"].shape[2:]))


# ---- the modules ---------------------------------------------------------------------------------------------------------------------
TAGS = {"input_quantizer": "activation/input", "weight_quantizer": "parameter/weight", "bias_quantizer": "parameter/bias",
        "output_quantizer": "activation/output"}


@pytest.mark.parametrize("cls,qcls,shape", [(torch.nn.ConvTranspose2d, "QuantizedConvTranspose2d", (4, 6, 3, 3)),
                                            (torch.nn.ConvTranspose1d, "QuantizedConvTranspose1d", (4, 6, 3))])
def test_conversion_needs_the_new_mapping(cls, qcls, shape):
    assert cls not in ff.nn.quantized_module_map() and cls not in ff.nn.quantized_conv_modules()
    for extra in (None, ff.nn.quantized_conv_modules()):
        with pytest.raises(QuantizationError, match="no quantized version"):
            ff.quantize_model(torch.nn.Sequential(cls(4, 6, 3)), extra_conversion=extra)
    model = ff.quantize_model(torch.nn.Sequential(cls(4, 6, 3)), extra_conversion=CONVT)
    conv = model[0]
    assert type(conv) is getattr(ff.nn, qcls) and isinstance(conv, cls) and CONVT[cls] is type(conv)
    for name, tag in TAGS.items():
        stub = getattr(conv, name)
        assert isinstance(stub, ff.nn.QuantizerStub) and tag in stub.quant_metadata, name
    assert tuple(conv.weight_quantizer.quant_metadata.shape) == shape
    assert set(CONVT) == {torch.nn.ConvTranspose1d, torch.nn.ConvTranspose2d} and CONVT is not ff.nn.quantized_conv_transpose_modules()


def test_a_module_without_bias_has_no_bias_quantizer():
    for cls in (torch.nn.ConvTranspose2d, torch.nn.ConvTranspose1d):
        model = ff.quantize_model(torch.nn.Sequential(cls(4, 6, 3, bias=False)), extra_conversion=CONVT)
        assert model[0].bias_quantizer is None
        assert isinstance(model[0].weight_quantizer, ff.nn.QuantizerStub)


def test_module_forward_and_output_size():
    torch.manual_seed(0)
    plain = torch.nn.ConvTranspose2d(4, 5, 3, stride=2, padding=1)
    x = torch.randn(2, 4, 6, 7)
    want_default, want_sized = plain(x), plain(x, output_size=[12, 14])
    module = ff.quantize_model(torch.nn.Sequential(plain), extra_conversion=CONVT)[0]
    with ff.strict_quantization(False):
        assert torch.equal(module(x), want_default) and want_default.shape[2:] == (11, 13)
        assert torch.equal(module(x, output_size=[12, 14]), want_sized) and want_sized.shape[2:] == (12, 14)
        with pytest.raises(ValueError):
            module(x, output_size=[20, 20])
    one = ff.quantize_model(torch.nn.Sequential(torch.nn.ConvTranspose1d(4, 5, 4, stride=4)), extra_conversion=CONVT)[0]
    with ff.strict_quantization(False):
        assert one(torch.randn(2, 4, 9), output_size=[38]).shape == (2, 5, 38)


# ---- the predicates and the geometry -----------------------------------------------------------------------------------------------
def test_the_predicates_decline_host_tensors():
    q = ff.nn.LinearQuantizer(8, symmetric=False, quantized_dtype=torch.int8)
    q.quantization_range = (torch.tensor(-3.0), torch.tensor(3.0))
    wq = ff.nn.LinearQuantizer(8, quantized_dtype=torch.int8)
    wq.quantization_range = (torch.tensor(-1.0), torch.tensor(1.0))
    x, w = q(torch.randn(1, 16, 6, 6)), wq(torch.randn(16, 8, 3, 3))
    assert not fused_conv_transpose.conv_transpose2d_predicate(input=x, weight=w, output_quantizer=None, strict_quantization=False)
    assert not fused_conv_transpose.conv_transpose1d_predicate(input=q(torch.randn(1, 16, 6)), weight=wq(torch.randn(16, 8, 3)),
                                                               output_quantizer=None, strict_quantization=False)


def test_transposed_geometry():
    g = fused_conv_transpose.transposed_geometry
    assert g(2, (8, 8), (3, 3), 2, 1, 1, 1) == ((2, 2), (1, 1), (1, 1), (1, 1))
    assert g(2, (8, 8), (3, 3), (2, 3), (1, 0), (1, 2), (2, 3)) == ((2, 3), (1, 0), (1, 2), (2, 3))
    assert g(1, (13,), (16,), 8, 4, 0, 1) == ((1, 8), (0, 4), (0, 0), (1, 1))
    assert g(2, (8, 8), (3, 3), 2, 1, 2, 1) is None             # output_padding >= max(stride, dilation): torch raises
    assert g(2, (8, 8), (3, 3), 1, 1, 1, 2) == ((1, 1), (1, 1), (1, 1), (2, 2))  # ... smaller than the dilation: allowed
    assert g(2, (8, 8), (3, 3), 2, 1, -1, 1) is None
    assert g(2, (8, 8), (3, 3), 2, "same", 0, 1) is None         # torch takes no string padding here
    assert g(2, (1, 1), (1, 1), 1, 1, 0, 1) is None              # the padding leaves no output
    assert g(2, (8, 8), (3, 3), (8, 8), 0, 0, 1) == ((8, 8), (0, 0), (0, 0), (1, 1))
    assert g(2, (8, 8), (3, 3), (8, 9), 0, 0, 1) is None         # 72 phases > the table's 64
    assert g(1, (8,), (3,), 64, 0, 0, 1) == ((1, 64), (0, 0), (0, 0), (1, 1)) and g(1, (8,), (3,), 65, 0, 0, 1) is None
    assert g(2, (8, 8), (3, 3), 2.0, 1, 0, 1) is None and g(2, (8, 8), (3, 3), 0, 1, 0, 1) is None
    assert MAX_PHASES == 64


# ---- the phase table, by brute force -------------------------------------------------------------------------------------------------
AXES = [(K, s, p, d, op) for K, s, p, d, op in itertools.product((1, 2, 3, 4, 7), (1, 2, 3, 4, 8), (0, 1, 3), (1, 2, 3), (0, 1, 2))
        if op < max(s, d)]


@pytest.mark.parametrize("n_in", [1, 5])
def test_every_tap_lands_in_exactly_one_phase_and_the_offsets_reproduce_the_input_index(n_in):
    checked = 0
    for K, s, p, d, op in AXES:
        O = (n_in - 1) * s - 2 * p + d * (K - 1) + op + 1
        if O < 1:
            continue
        rows, kstep, ostep = axis_phases(K, s, p, d, O)
        assert len(rows) == s
        taps_seen, outputs = [], []
        for r, (k0, n, off0, extent) in enumerate(rows):
            taps = [k0 + a * kstep for a in range(n)]
            assert taps == [k for k in range(K) if (r + p - k * d) % s == 0], (K, s, p, d, r)
            taps_seen += taps
            mine = list(range(r, O, s))
            assert extent == len(mine)
            outputs += mine
            for i, o in enumerate(mine):
                for a, k in enumerate(taps):
                    assert (o + p - k * d) % s == 0 and off0 + a * ostep + i == (o + p - k * d) // s
        assert sorted(taps_seen) == list(range(K))   # every tap in exactly one phase
        assert sorted(outputs) == list(range(O))     # the phases' positions are the output grid
        checked += 1
    assert checked > 300


@pytest.mark.parametrize("geometry", [((2, 2), (2, 2), (0, 0), (1, 1), (0, 0)), ((4, 4), (2, 2), (1, 1), (1, 1), (0, 0)),
                                      ((2, 2), (3, 3), (0, 0), (1, 1), (0, 0)), ((3, 3), (2, 3), (1, 2), (2, 3), (1, 2)),
                                      ((3, 2), (2, 4), (1, 0), (2, 2), (1, 2)), ((1, 16), (1, 8), (0, 4), (1, 1), (0, 0)),
                                      ((3, 5), (1, 2), (0, 3), (2, 1), (0, 1))])
def test_the_phase_table_evaluates_the_transposed_convolution(geometry):
    """Summing, per phase, its taps at their offsets over its grid is F.conv_transpose2d (float64 on integer data: exact)."""
    k, s, p, d, op = geometry
    B, C, OC, H, W = 3, 2, 3, 5, 6
    g = torch.Generator().manual_seed(7)
    x = torch.randint(-9, 10, (B, C, H, W), generator=g).double()
    w = torch.randint(-9, 10, (C, OC, *k), generator=g).double()
    want = torch.nn.functional.conv_transpose2d(x, w, None, s, p, op, 1, d)
    OH, OW = want.shape[2:]
    table = phase_table(B, k, s, p, d, (OH, OW))
    assert len(table) == s[0] * s[1]
    got = torch.full_like(want, float("nan"))
    tiles = tap = 0
    for ph in table:
        assert ph["tap_begin"] == tap
        tap += len(ph["taps"])
        tiles += -(-B * ph["rows"] * ph["cols"] // 128)
        assert ph["tile_end"] == tiles
        for i in range(ph["rows"]):
            for j in range(ph["cols"]):
                acc = torch.zeros(B, OC, dtype=torch.float64)
                for kh, kw, oh_, ow_ in ph["taps"]:
                    ih, iw = i + oh_, j + ow_
                    if 0 <= ih < H and 0 <= iw < W:
                        acc += x[:, :, ih, iw] @ w[:, :, kh, kw]
                assert torch.isnan(got[:, :, ph["rh"] + s[0] * i, ph["rw"] + s[1] * j]).all()   # written once
                got[:, :, ph["rh"] + s[0] * i, ph["rw"] + s[1] * j] = acc
    assert tap == k[0] * k[1]
    assert torch.equal(got, want)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_the_hip_library_exports_both_symbols():
    dll = ctypes.CDLL(str(HIP_SO))
    lib = FFQLibrary(HIP_SO)
    for name in ENTRY_POINTS:
        assert hasattr(dll, name) and name in _cabi.SIGNATURES and name in _cabi.DEVICE_ONLY
        assert getattr(lib, name) is not None
    assert "conv_transpose2d_w8a8" in ff.ops.__all__ and ff.ops.conv_transpose2d_w8a8


def test_the_oracle_loads_without_them():
    lib = load_oracle()
    assert not lib.is_device
    for name in ENTRY_POINTS:
        assert getattr(lib, name) is None


FAKE = 1 << 20  # never dereferenced: every call below returns from the argument checks


def _convt(lib, x=FAKE, nhwc=0, w=FAKE, xs=FAKE, ws=FAKE, bias=None, bias_dt=0, out=FAKE, out_dt=DType.BF16, out_scale=None, bits=8.0,
           y_dt=0, B=2, C=16, H=8, W=8, OC=32, KH=3, KW=3, s=(2, 2), p=(1, 1), op=(0, 0), d=(1, 1), workspace=FAKE, nbytes=None):
    if nbytes is None:
        nbytes = lib.ffq_conv_transpose2d_w8a8_workspace_bytes(B, C, H, W, OC, KH, KW, nhwc) if C > 0 and KH > 0 and KW > 0 else 0
    return lib.ffq_conv_transpose2d_w8a8(x, nhwc, w, xs, None, ws, None, 0, bias, bias_dt, out, out_dt, out_scale, None, bits, y_dt, B, C, H,
                                         W, OC, KH, KW, s[0], s[1], p[0], p[1], op[0], op[1], d[0], d[1], workspace, nbytes, None)


@pytest.mark.parametrize(
    "call,status",
    [
        (lambda lib: _convt(lib, B=-1), Status.ERR_ARG),
        (lambda lib: _convt(lib, C=0), Status.ERR_EMPTY),
        (lambda lib: _convt(lib, s=(0, 1)), Status.ERR_ARG),
        (lambda lib: _convt(lib, d=(1, 0)), Status.ERR_ARG),
        (lambda lib: _convt(lib, p=(-1, 0)), Status.ERR_ARG),
        (lambda lib: _convt(lib, op=(2, 0)), Status.ERR_ARG),                  # out_pad >= max(stride, dilation)
        (lambda lib: _convt(lib, op=(0, -1)), Status.ERR_ARG),
        (lambda lib: _convt(lib, op=(2, 2), d=(3, 3), nbytes=16), Status.ERR_WORKSPACE),  # below the dilation: that check passes
        (lambda lib: _convt(lib, s=(8, 9)), Status.ERR_ARG),                   # 72 phases
        (lambda lib: _convt(lib, s=(1, 65)), Status.ERR_ARG),
        (lambda lib: _convt(lib, C=16385, KH=3, KW=3), Status.ERR_DTYPE),      # C * KH * KW >= 131072
        (lambda lib: _convt(lib, C=1 << 62, KH=2, KW=2), Status.ERR_DTYPE),     # ... and no int64 overflow on the way: 2^64 wraps to 0
        (lambda lib: _convt(lib, nhwc=1, C=24), Status.ERR_DTYPE),             # channels-last needs C % 16 == 0
        (lambda lib: _convt(lib, H=1, W=1, KH=1, KW=1, s=(1, 1), p=(1, 1)), Status.ERR_ARG),  # OH < 1
        (lambda lib: _convt(lib, H=0), Status.ERR_ARG),
        (lambda lib: _convt(lib, bias=FAKE, bias_dt=DType.I8), Status.ERR_DTYPE),
        (lambda lib: _convt(lib, out_dt=DType.I8), Status.ERR_DTYPE),          # codes out without an output quantizer
        (lambda lib: _convt(lib, out_scale=FAKE, out_dt=DType.BF16, y_dt=DType.BF16), Status.ERR_DTYPE),
        (lambda lib: _convt(lib, out_scale=FAKE, out_dt=DType.I8, y_dt=DType.BF16, bits=11.0), Status.ERR_PRECISION),
        (lambda lib: _convt(lib, out_scale=FAKE, out_dt=DType.I8, y_dt=DType.I8), Status.ERR_DTYPE),
        (lambda lib: _convt(lib, x=None), Status.ERR_ARG),
        (lambda lib: _convt(lib, xs=None), Status.ERR_ARG),
        (lambda lib: _convt(lib, nhwc=1, x=FAKE + 8), Status.ERR_ARG),         # misaligned channels-last codes
        (lambda lib: _convt(lib, workspace=None), Status.ERR_WORKSPACE),
        (lambda lib: _convt(lib, nbytes=1024), Status.ERR_WORKSPACE),
        (lambda lib: _convt(lib, B=0), Status.OK),
        (lambda lib: _convt(lib, OC=0), Status.OK),
    ],
)
def test_argument_checks_need_no_device(call, status):
    lib = FFQLibrary(HIP_SO)
    assert call(lib) == status
    if status != Status.OK:
        assert lib.ffq_last_error()


def test_workspace_bytes():
    lib = FFQLibrary(HIP_SO)
    # NHWC input [2, 8, 8, 16] + weight [32, 3, 3, 16] + (tap sums 32 * 9 + phase totals 32 * 64) int32, each rounded up to 256 bytes
    assert lib.ffq_conv_transpose2d_w8a8_workspace_bytes(2, 3, 8, 8, 32, 3, 3, 0) == 2048 + 4608 + 9472
    assert lib.ffq_conv_transpose2d_w8a8_workspace_bytes(2, 16, 8, 8, 32, 3, 3, 1) == 4608 + 9472
    assert lib.ffq_conv_transpose2d_w8a8_workspace_bytes(2, 0, 8, 8, 32, 3, 3, 0) == 0
    assert lib.ffq_conv_transpose2d_w8a8_workspace_bytes(1 << 20, 16, 1 << 24, 1 << 24, 32, 3, 3, 0) == 0   # no launch takes it; no overflow


def test_the_new_kernels_spill_nothing_and_use_no_scratch():
    if kernel_resources.readelf() is None:
        pytest.skip("llvm-readelf is missing")
    assert kernel_resources.DEFAULT_LIBRARY.exists(), "build() leaves the HIP library in the tree"
    rows = [k for k in kernel_resources.kernel_resources() if any(n in str(k["name"]) for n in KERNELS)]
    for needle, count in zip(KERNELS, (1, 4)):
        assert sum(needle in str(k["name"]) for k in rows) == count, needle
    bad = {str(k["name"]): k for k in rows if k["vgpr_spill_count"] or k["sgpr_spill_count"] or k["private_segment_fixed_size"]}
    assert not bad, bad
    assert all(k["group_segment_fixed_size"] <= 33280 for k in rows)
