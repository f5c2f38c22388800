"""The quantized spatial operators (avg_pool1d, avg_pool2d, max_pool2d, interpolate) without a GPU: the public names and the
reference's signatures, the host path against the reference's outputs (fixture G24), the reference's strict-mode errors, what the
predicates decline, ATen's output sizes, the two C-ABI entry points (exported by the HIP library, absent from the oracle, argument
checks before any device call) and what hipcc emitted for their kernels."""

import ctypes
import inspect
import random
import sys

import pytest
import torch

import fastforward_amd as ff

from conftest import HIP_SO, ROOT, golden, load_oracle
from fastforward_amd import _cabi, fused_math, fused_pool
from fastforward_amd._cabi import DType, FanOut, FFQLibrary, Status
from fastforward_amd.exceptions import BackendError, QuantizationError
from fastforward_amd.ops.pool import pooled_size

sys.path.insert(0, str(ROOT / "tools"))

import kernel_resources  # noqa: E402

F = ff.nn.functional
NAMES = ("avg_pool1d", "avg_pool2d", "max_pool2d", "interpolate")
ENTRY_POINTS = ("ffq_pool2d_quantize", "ffq_upsample_nearest_quantize")
OUTPUT_MSG = "'output_quantizer' must be provided if strict_quantization=True"
INPUT_MSG = "Expected 'input' to be an instance of 'QuantizedTensor' because strict_quantization=True."


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
    assert {"pool2d_quantize", "upsample_nearest_quantize"} <= set(ff.ops.__all__)


# ---- the host path against the reference (G24) -----------------------------------------------------------------------------------
G24 = golden("g24_pool.pt")


@pytest.mark.parametrize("index", range(len(G24)), ids=[c["name"] for c in G24])
def test_host_path_equals_the_reference_bit_for_bit(index):
    case = G24[index]
    x = case["inputs"]["input"]
    if "input" in case["slots"]:
        q = _with_params(quantizer(case["slots"]["input"]), case["params"]["input"])
        with torch.no_grad():
            x = q(x)
    oq = _with_params(quantizer(case["out_slot"]), case["out_params"])
    fn = getattr(F, case["op"])
    with torch.no_grad(), ff.strict_quantization(False):
        value = fn(x, **case["kwargs"])
        quantized = fn(x, **case["kwargs"], output_quantizer=oq)
    want = case["value"]
    assert value.dtype == want.dtype and value.shape == want.shape and torch.equal(_bits(value), _bits(want)), case["name"]
    assert isinstance(quantized, ff.QuantizedTensor)
    assert torch.equal(quantized.raw_data, case["codes"]), case["name"]
    assert torch.equal(_bits(quantized.dequantize()), _bits(case["dequantized"])), case["name"]


def test_the_fixture_covers_what_the_issue_lists():
    names = " ".join(c["name"] for c in G24)
    for needle in ("avg_pool2d k2 s2", "avg_pool2d k3 s2 p1 plain", "count_include_pad=False", "avg_pool2d ceil_mode odd", "avg_pool2d k(3, 2)",
                   "avg_pool2d global 7x7", "avg_pool1d k4 s4", "avg_pool1d k3 s1 p1", "max_pool2d k3 s2 p1", "max_pool2d stride=None",
                   "max_pool2d dilation 2", "max_pool2d ceil_mode", "max_pool2d NaN inf", "interpolate nearest x2", "interpolate nearest x1.5",
                   "interpolate size=(13, 9)", "interpolate nearest-exact", "interpolate 3-D", " plain ", " q ", " per-channel q "):
        assert needle in names, needle
    assert {c["dtype"] for c in G24} == {"torch.float32", "torch.bfloat16"}
    assert all(c["inputs"]["input"].shape[-1] <= 16 for c in G24)


# ---- strict quantization: the reference's messages (_gen/fallback.py) ------------------------------------------------------------
def _q(x):
    return quantizer((8, False, "tensor", -3.0, 3.0))(x)


def test_strict_mode_errors_match_the_reference():
    x, row = torch.randn(2, 3, 8, 8), torch.randn(2, 3, 8)
    stub = ff.nn.QuantizerStub(output_quantizer=True)
    calls = [(F.avg_pool1d, row, dict(kernel_size=2, stride=2)), (F.avg_pool2d, x, dict(kernel_size=2, stride=2)), (F.max_pool2d, x, dict(kernel_size=2)),
             (F.interpolate, x, dict(scale_factor=2)), (F.interpolate, row, dict(size=5, mode="linear"))]
    for fn, t, kwargs in calls:
        with pytest.raises(QuantizationError) as e:
            fn(t, **kwargs, strict_quantization=True)
        assert str(e.value) == OUTPUT_MSG
        with pytest.raises(QuantizationError) as e:
            fn(t, **kwargs, output_quantizer=stub, strict_quantization=True)
        assert str(e.value) == INPUT_MSG
        assert fn(_q(t), **kwargs, output_quantizer=stub, strict_quantization=True) is not None


def test_signatures_follow_the_reference():
    want = {
        "avg_pool1d": ["input", "kernel_size", "stride", "padding", "ceil_mode", "count_include_pad", "output_quantizer", "strict_quantization"],
        "avg_pool2d": ["input", "kernel_size", "stride", "padding", "ceil_mode", "count_include_pad", "output_quantizer", "strict_quantization"],
        "max_pool2d": ["input", "kernel_size", "stride", "padding", "dilation", "ceil_mode", "output_quantizer", "strict_quantization"],
        "interpolate": ["input", "size", "scale_factor", "mode", "align_corners", "recompute_scale_factor", "antialias", "output_quantizer",
                        "strict_quantization"],
    }
    for name, names in want.items():
        params = inspect.signature(getattr(F, name)).parameters
        assert list(params) == names
        assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in names[-2:])
    empty = inspect.Parameter.empty
    for name in ("avg_pool1d", "avg_pool2d"):  # `stride` is required on the average pools
        assert inspect.signature(getattr(F, name)).parameters["stride"].default is empty
        with pytest.raises(TypeError):
            getattr(F, name)(torch.randn(1, 1, 4, 4), 2)
    assert inspect.signature(F.max_pool2d).parameters["stride"].default is None
    x = torch.randn(2, 3, 9, 9).bfloat16()
    with ff.strict_quantization(False):
        assert torch.equal(F.max_pool2d(x, 3), torch.nn.functional.max_pool2d(x, 3))  # stride=None: the kernel size
        assert torch.equal(F.max_pool2d(x, 3, None, 1, 2, True), torch.nn.functional.max_pool2d(x, 3, None, 1, 2, True))
        assert torch.equal(F.avg_pool2d(x, 3, 2, 1, True, False), torch.nn.functional.avg_pool2d(x, 3, 2, 1, True, False))
        assert torch.equal(F.avg_pool1d(x[0], 3, 2, 1), torch.nn.functional.avg_pool1d(x[0], 3, 2, 1))
        assert torch.equal(F.interpolate(x, None, 1.5, "nearest-exact"), torch.nn.functional.interpolate(x, None, 1.5, "nearest-exact"))
        assert torch.equal(F.interpolate(x.float(), (5, 4), mode="bilinear", align_corners=True),
                           torch.nn.functional.interpolate(x.float(), (5, 4), mode="bilinear", align_corners=True))


# ---- the predicates ---------------------------------------------------------------------------------------------------------------
P = fused_pool


def _kw(**k):
    return dict(output_quantizer=None, strict_quantization=False, **k)


def test_the_predicates_decline_host_tensors_and_calls_without_the_strict_keyword():
    x = torch.randn(2, 3, 8, 8, dtype=torch.bfloat16)
    assert not P.avg_pool2d_predicate(input=x, kernel_size=2, stride=2, **_kw())
    assert not P.avg_pool1d_predicate(input=x[0], kernel_size=2, stride=2, **_kw())
    assert not P.max_pool2d_predicate(input=x, kernel_size=2, **_kw())
    assert not P.interpolate_predicate(input=x, scale_factor=2, **_kw())
    for pred in (P.avg_pool1d_predicate, P.avg_pool2d_predicate, P.max_pool2d_predicate, P.interpolate_predicate):
        assert not pred(x, x, 1, 2, 3, 4, 5, 6, 7, out=x)  # any call signature, without raising
        assert not pred()
        assert not pred(x)


@pytest.fixture()
def on_device(monkeypatch):
    """The predicates' device check answered yes for host tensors: what else they decline is what they test."""
    for module in (fused_pool, fused_math):
        monkeypatch.setattr(module, "_on_device", lambda *t: True)


def test_what_the_predicates_accept_and_decline(on_device):
    x = torch.randn(2, 3, 9, 14, dtype=torch.bfloat16)
    row = torch.randn(2, 3, 14, dtype=torch.float16)
    avg2, avg1, mx, ip = P.avg_pool2d_predicate, P.avg_pool1d_predicate, P.max_pool2d_predicate, P.interpolate_predicate
    qt = quantizer((8, False, "tensor", -3.0, 3.0))(x)
    qc = quantizer((8, False, ("channel", 1), torch.full((3,), -3.0), torch.full((3,), 3.0)))(x)
    # accepted (the device check aside): odd planes, ints and tuples, per-tensor and per-channel codes
    for t in (x, qt, qc):
        with torch.no_grad():  # (a quantizer's parameters need a gradient)
            assert avg2(input=t, kernel_size=3, stride=(2, 1), padding=1, ceil_mode=True, count_include_pad=False, **_kw())
            assert mx(input=t, kernel_size=(3, 2), stride=None, padding=(1, 0), dilation=2, ceil_mode=False, **_kw())
            assert ip(input=t, scale_factor=1.5, **_kw()) and ip(input=t, size=(13, 9), mode="nearest-exact", **_kw())
            assert ip(input=t, scale_factor=(2, 0.5), recompute_scale_factor=False, **_kw())
    assert not mx(input=qt, kernel_size=2, **_kw())  # grad mode: the quantizer's parameters need a gradient
    assert avg1(input=row, kernel_size=4, stride=4, **_kw()) and avg1(input=row, kernel_size=(3,), stride=(1,), padding=(1,), **_kw())
    assert ip(input=row, scale_factor=2.5, **_kw()) and ip(input=row, size=17, **_kw())
    assert avg2(input=torch.randn(2, 8, 7, 7, dtype=torch.bfloat16), kernel_size=7, stride=7, **_kw())  # the 7x7 head
    # calls without the strict_quantization keyword (the torch-function route)
    assert not mx(input=x, kernel_size=2, output_quantizer=None) and not ip(input=x, scale_factor=2, output_quantizer=None)
    # unbatched inputs
    assert not avg2(input=x[0], kernel_size=2, stride=2, **_kw()) and not mx(input=x[0], kernel_size=2, **_kw())
    assert not avg1(input=row[0], kernel_size=2, stride=2, **_kw()) and not ip(input=row[0], scale_factor=2, **_kw())
    assert not avg1(input=x, kernel_size=2, stride=2, **_kw()) and not avg2(input=row, kernel_size=2, stride=2, **_kw())
    # channels-last strides (ATen answers in channels-last); a permuted 3-D input that unsqueezes to them
    cl = x.contiguous(memory_format=torch.channels_last)
    assert not avg2(input=cl, kernel_size=2, stride=2, **_kw()) and not mx(input=cl, kernel_size=2, **_kw()) and not ip(input=cl, scale_factor=2, **_kw())
    assert not avg1(input=torch.randn(2, 14, 3, dtype=torch.float16).transpose(1, 2), kernel_size=2, stride=2, **_kw())
    assert avg2(input=x.transpose(-1, -2), kernel_size=2, stride=2, **_kw()) and mx(input=x[..., ::2], kernel_size=2, **_kw())  # other views
    # interpolate: other modes, align_corners, antialias, a recomputed scale factor, both or neither of size / scale_factor, the input's size
    assert not ip(input=x, scale_factor=2, mode="bilinear", **_kw()) and not ip(input=x, scale_factor=2, mode="bicubic", **_kw())
    assert not ip(input=row, scale_factor=2, mode="linear", **_kw()) and not ip(input=x, scale_factor=2, mode="area", **_kw())
    assert not ip(input=x, scale_factor=2, align_corners=False, **_kw()) and not ip(input=x, scale_factor=2, antialias=True, **_kw())
    assert not ip(input=x, scale_factor=1.5, recompute_scale_factor=True, **_kw())
    assert not ip(input=x, **_kw()) and not ip(input=x, size=(4, 4), scale_factor=2, **_kw())
    assert not ip(input=x, size=(9, 14), **_kw()) and not ip(input=x, scale_factor=1.0, **_kw())
    assert not ip(input=x, size=(4,), **_kw()) and not ip(input=x, scale_factor=(2, 2, 2), **_kw()) and not ip(input=x, size=(0, 4), **_kw())
    assert not ip(input=x, scale_factor=-1.0, **_kw()) and not ip(input=x, scale_factor=float("nan"), **_kw()) and not ip(input=x, scale_factor=0.01, **_kw())
    # geometry ATen refuses, or that is no int
    assert not avg2(input=x, kernel_size=3, stride=2, padding=2, **_kw()) and not mx(input=x, kernel_size=2, padding=2, **_kw())
    assert not avg2(input=x, kernel_size=0, stride=1, **_kw()) and not avg2(input=x, kernel_size=2, stride=0, **_kw())
    assert not mx(input=x, kernel_size=2, padding=-1, **_kw()) and not mx(input=x, kernel_size=2, dilation=0, **_kw())
    assert not mx(input=x, kernel_size=7, dilation=3, **_kw()) and not avg2(input=x, kernel_size=10, stride=1, **_kw())  # no output
    assert not avg2(input=x, kernel_size=2.0, stride=2, **_kw()) and not avg2(input=x, kernel_size=2, stride=None, **_kw())
    assert not avg2(input=x, kernel_size=(2, 2, 2), stride=2, **_kw()) and not avg2(input=x, kernel_size=True, stride=2, **_kw())
    assert not avg2(input=x, kernel_size=2, stride=2, ceil_mode=1, **_kw()) and not avg2(input=x, kernel_size=2, stride=2, count_include_pad=0, **_kw())
    # fp32 values, an empty tensor, parameters per row of the last dim
    assert not avg2(input=x.float(), kernel_size=2, stride=2, **_kw()) and not ip(input=x.float(), scale_factor=2, **_kw())
    assert not mx(input=x[:0], kernel_size=2, **_kw())
    qr = quantizer((8, False, ("channel", (0, 1, 2)), torch.full((54,), -3.0), torch.full((54,), 3.0)))(x)
    assert not mx(input=qr, kernel_size=2, **_kw())
    # grad mode with an operand that needs a gradient (not under no_grad)
    xg = x.clone().requires_grad_()
    assert not avg2(input=xg, kernel_size=2, stride=2, **_kw()) and not ip(input=xg, scale_factor=2, **_kw())
    with torch.no_grad():
        assert avg2(input=xg, kernel_size=2, stride=2, **_kw())
    # strict mode: only calls the fallback accepts
    assert not mx(input=x, kernel_size=2, output_quantizer=None, strict_quantization=True)
    assert not mx(input=x, kernel_size=2, output_quantizer=quantizer((8, False, "tensor", -3.0, 3.0)), strict_quantization=True)
    with torch.no_grad():
        assert mx(input=qt, kernel_size=2, output_quantizer=quantizer((8, False, "tensor", -3.0, 3.0)), strict_quantization=True)


def test_output_sizes_are_atens():
    rng = random.Random(24)
    for _ in range(2000):
        k, s, d, ceil_mode = rng.randint(1, 7), rng.randint(1, 4), rng.randint(1, 3), rng.random() < 0.5
        p = rng.randint(0, k // 2)
        n = rng.randint(max(1, d * (k - 1) + 1 - 2 * p), 57)
        x = torch.zeros(1, 1, n, 1)
        assert pooled_size(n, k, p, s, d, ceil_mode) == torch.nn.functional.max_pool2d(x, (k, 1), (s, 1), (p, 0), (d, 1), ceil_mode).shape[2]
        assert pooled_size(n, k, p, s, 1, ceil_mode) == torch.nn.functional.avg_pool2d(x, (k, 1), (s, 1), (p, 0), ceil_mode).shape[2] if n >= k - 2 * p else True
    x = torch.zeros(1, 1, 57, 23)
    for factor in (0.3, 0.6, 1.5, 1.7, 2, 2.5, 3.14159):
        out, _ = P.KERNELS._target(x, None, factor)
        assert out == tuple(torch.nn.functional.interpolate(x, scale_factor=factor).shape[2:])


# ---- the ctypes wrappers and the C ABI ----------------------------------------------------------------------------------------------
def test_the_wrappers_reject_bad_arguments_before_a_launch():
    x = torch.randn(2, 3, 8, 8, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="mode is one of"):
        ff.ops.pool2d_quantize("min", x, (2, 2), (2, 2))
    with pytest.raises(RuntimeError, match=r"\[B, C, H, W\]"):
        ff.ops.pool2d_quantize("max", x[0], (2, 2), (2, 2))
    with pytest.raises(RuntimeError, match="pair of ints"):
        ff.ops.pool2d_quantize("max", x, (2.0, 2), (2, 2))
    with pytest.raises(RuntimeError, match="must be positive"):
        ff.ops.pool2d_quantize("max", x, (2, 2), (0, 2))
    with pytest.raises(RuntimeError, match="value dtype"):
        ff.ops.pool2d_quantize("avg", x.float(), (2, 2), (2, 2), dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="parameters are one pair"):
        ff.ops.pool2d_quantize("avg", x.to(torch.int8), (2, 2), (2, 2), dtype=torch.bfloat16, dequant=(torch.ones(5), None))
    with pytest.raises(RuntimeError, match="mode is one of"):
        ff.ops.upsample_nearest_quantize(x, (4, 4), None, "bilinear")
    with pytest.raises(RuntimeError, match="greater than 0"):
        ff.ops.upsample_nearest_quantize(x, (0, 4))
    with pytest.raises(BackendError):  # a host tensor: there is no CPU implementation
        ff.ops.pool2d_quantize("max", x, (2, 2), (2, 2))
    with pytest.raises(BackendError):
        ff.ops.upsample_nearest_quantize(x, (16, 16), (2.0, 2.0))


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


def _pool(lib, mode=2, x=FAKE, x_dt=DType.I8, scale=FAKE, channels=0, dt=DType.BF16, planes=6, H=9, W=14, k=(3, 3), s=(2, 2), p=(1, 1), d=(1, 1),
          ceil_mode=0, out=(5, 7), fan=None):
    f = _fan() if fan is None else fan
    return lib.ffq_pool2d_quantize(mode, x, x_dt, scale, None, channels, dt, planes, H, W, *k, *s, *p, *d, ceil_mode, *out, None, ctypes.byref(f), None)


def _up(lib, x=FAKE, x_dt=DType.I8, scale=FAKE, channels=0, dt=DType.BF16, planes=6, H=9, W=14, out=(13, 21), factors=(1.5, 1.5), exact=0, fan=None):
    f = _fan() if fan is None else fan
    return lib.ffq_upsample_nearest_quantize(x, x_dt, scale, None, channels, dt, planes, H, W, *out, *factors, exact, None, ctypes.byref(f), None)


@pytest.mark.parametrize(
    "call,status",
    [
        (lambda lib: _pool(lib, mode=3), Status.ERR_ARG),
        (lambda lib: _pool(lib, dt=DType.F32), Status.ERR_DTYPE),
        (lambda lib: _pool(lib, dt=DType.F32, x=None), Status.ERR_DTYPE),       # the dtype first, before any buffer is looked at
        (lambda lib: _pool(lib, scale=None), Status.ERR_DTYPE),                # int8 codes without a scale
        (lambda lib: _pool(lib, x_dt=DType.F16), Status.ERR_DTYPE),            # codes of another value dtype
        (lambda lib: _pool(lib, x_dt=DType.BF16, scale=None, channels=3), Status.ERR_DTYPE),  # a plain input has no parameters
        (lambda lib: _pool(lib, k=(0, 3)), Status.ERR_ARG),
        (lambda lib: _pool(lib, s=(2, 0)), Status.ERR_ARG),
        (lambda lib: _pool(lib, p=(2, 1)), Status.ERR_ARG),                    # pad beyond half the kernel
        (lambda lib: _pool(lib, p=(-1, 1)), Status.ERR_ARG),
        (lambda lib: _pool(lib, mode=0, d=(2, 2)), Status.ERR_ARG),            # the averages have no dilation
        (lambda lib: _pool(lib, out=(5, 8)), Status.ERR_ARG),                  # not ATen's output size
        (lambda lib: _pool(lib, ceil_mode=1, out=(5, 7)), Status.ERR_ARG),     # ceil_mode: [5, 8]
        (lambda lib: _pool(lib, k=(7, 7), d=(3, 3), p=(0, 0), out=(0, 0)), Status.ERR_ARG),  # no output
        (lambda lib: _pool(lib, channels=4), Status.ERR_ARG),                  # 6 planes are not images of 4 channels
        (lambda lib: _pool(lib, planes=-1), Status.ERR_ARG),
        (lambda lib: _pool(lib, H=0, out=(0, 7)), Status.ERR_ARG),
        (lambda lib: _pool(lib, planes=1 << 20, H=64, W=64, out=(32, 32)), Status.ERR_DTYPE),  # 2^32 elements
        (lambda lib: _pool(lib, x=FAKE + 8), Status.ERR_ARG),                  # misaligned
        (lambda lib: _pool(lib, x=None), Status.ERR_ARG),
        (lambda lib: _pool(lib, fan=_fan(bits=9.0)), Status.ERR_PRECISION),
        (lambda lib: _pool(lib, fan=_fan(codes=None)), Status.ERR_ARG),
        (lambda lib: _pool(lib, planes=0), Status.OK),
        (lambda lib: _pool(lib, ceil_mode=1, out=(5, 8), planes=0), Status.OK),
        (lambda lib: _up(lib, dt=DType.F32), Status.ERR_DTYPE),
        (lambda lib: _up(lib, scale=None), Status.ERR_DTYPE),
        (lambda lib: _up(lib, factors=(-1.0, 1.5)), Status.ERR_ARG),
        (lambda lib: _up(lib, factors=(float("nan"), 1.5)), Status.ERR_ARG),
        (lambda lib: _up(lib, factors=(float("inf"), 1.5)), Status.ERR_ARG),
        (lambda lib: _up(lib, out=(0, 21)), Status.ERR_ARG),
        (lambda lib: _up(lib, W=0), Status.ERR_ARG),
        (lambda lib: _up(lib, channels=4), Status.ERR_ARG),
        (lambda lib: _up(lib, planes=1 << 16, out=(256, 256)), Status.ERR_DTYPE),  # 2^32 outputs
        (lambda lib: _up(lib, x=FAKE + 2), Status.ERR_ARG),
        (lambda lib: _up(lib, x=None), Status.ERR_ARG),
        (lambda lib: _up(lib, fan=_fan(count=3, codes=FAKE + 4)), Status.ERR_ARG),  # misaligned codes
        (lambda lib: _up(lib, planes=0), Status.OK),
    ],
)
def test_argument_checks_need_no_device(call, status):
    lib = FFQLibrary(HIP_SO)
    assert call(lib) == status
    if status != Status.OK:
        assert lib.ffq_last_error()


KERNELS = {  # kernel: instances (2 value dtypes x 3 input forms x 8 or 1 outputs per lane x ...)
    "pool2d_quantize_kernel": 36,            # x 3 modes
    "upsample_nearest_quantize_kernel": 12,
}


def test_the_new_kernels_spill_nothing_and_use_no_scratch():
    """No scratch and no spills; at most 64 VGPRs and 8 KiB of LDS per block of 256 lanes, i.e. 8 waves per SIMD by registers and
    every block slot of a CU by LDS: the loads of these memory-bound kernels have the whole machine's waves to hide behind."""
    if kernel_resources.readelf() is None or not kernel_resources.DEFAULT_LIBRARY.exists():
        pytest.skip("llvm-readelf or the built library is missing")
    rows = [k for k in kernel_resources.kernel_resources() if any(n in str(k["name"]) for n in KERNELS)]
    for needle, count in KERNELS.items():
        assert sum(needle in str(k["name"]) for k in rows) == count, needle
    bad = {str(k["name"]): k for k in rows if k["vgpr_spill_count"] or k["sgpr_spill_count"] or k["private_segment_fixed_size"]}
    assert not bad, bad
    assert all(k["group_segment_fixed_size"] <= 8192 for k in rows)
    assert all(k["vgpr_count"] <= 64 for k in rows), max(k["vgpr_count"] for k in rows)
