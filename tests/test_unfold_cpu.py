"""The quantized unfold without a GPU: the functional surface, the host path against the reference's outputs (fixture G30, sign bits
included), the strict-mode messages in the reference's order, the predicate on what it accepts and declines, the fifth header
``include/ffq_unfold.h`` against ``_cabi.SIGNATURES_UNFOLD`` (exported by the HIP library, absent from the oracle, the other tables
untouched), every argument error of the entry point in the documented order before any device call, the index formula of the header
against ``torch.nn.functional.unfold`` by brute force, and what hipcc emitted for the new kernels."""

import ctypes
import re
import sys

import pytest
import torch

import fastforward_amd as ff

from conftest import HIP_SO, ROOT, golden, load_oracle
from fastforward_amd import _cabi, dispatcher, fused_concat, fused_conv, fused_index, fused_unfold
from fastforward_amd._cabi import DType, FFQLibrary, Status
from fastforward_amd.exceptions import BackendError, QuantizationError

sys.path.insert(0, str(ROOT / "tools"))

import kernel_resources  # noqa: E402

F = ff.nn.functional
ENTRY = "ffq_unfold_quantize"
G30 = golden("g30_unfold.pt")
CASES = G30["cases"]

# ((B, C, H, W) or (C, H, W), kernel_size, dilation, padding, stride): the smallest shapes at which each branch of the kernel can go
# wrong (shared with the GPU tests)
GEOMETRIES = [
    ((1, 1, 1, 1), 1, 1, 0, 1),                              # one element, L = 1
    ((2, 3, 5, 7), (3, 2), (1, 2), (2, 1), (2, 1)),          # L = 28: element form, every parameter asymmetric
    ((1, 2, 6, 6), 3, 1, 0, 1),                              # OW = 4, L = 16: a group spans two output rows
    ((1, 2, 10, 5), 3, 1, 0, 1),                             # OW = 3, L = 24: a group spans three rows
    ((2, 1, 3, 10), 3, 1, 0, 1),                             # OW = 8, L = 8: group form
    ((1, 1, 3, 11), 3, 1, 0, 1),                             # OW = 9, L = 9: element form
    ((1, 1, 4, 3), (1, 3), 1, 0, 1),                         # OW = 1
    ((1, 3, 4, 4), 1, 1, 2, 1),                              # windows wholly in the padding
    ((1, 1, 3, 3), 2, 1, 3, 1),
    ((1, 2, 7, 9), 3, 1, 1, 2),                              # stride 2 on odd sizes
    ((1, 2, 8, 8), 2, 1, 0, 3),                              # pixels no window reads
    ((1, 2, 9, 9), 3, 3, 0, 1),                              # dilation
    ((1, 2, 5, 5), 3, 2, 2, 1),
    ((3, 4, 4, 6), 1, 1, 0, 1),                              # taps = 1: a reshape
    ((1, 17, 3, 9), (1, 5), 1, 0, 1),                        # 85 rows, PerChannel(1) with 17 pairs
    ((1, 2, 4, 6), (4, 6), 1, 0, 1),                         # window = image: L = 1, 48 rows
    ((1, 1, 1, 1500), (1, 3), 1, (0, 1), 1),                 # a long row (1-D sliding window)
    ((3, 5, 6), (2, 3), 1, 0, 1),                            # unbatched
]


def geometry_id(g):
    return re.sub(r"\s", "", f"{g[0]}k{g[1]}d{g[2]}p{g[3]}s{g[4]}")


# ---- the functional surface ---------------------------------------------------------------------------------------------------------
def test_the_function_exists():
    assert "unfold" in F.__all__ and callable(F.unfold) and "conv_transpose3d" not in F.__all__ and not hasattr(F, "conv_transpose3d")
    doc = " ".join(F.__doc__.split())
    scope = doc.split("out of scope")[0].rsplit(".", 1)[-1]  # the sentence that names what is out of scope
    assert "conv_transpose3d" in scope and "unfold" not in scope and "``unfold``" in doc
    assert "unfold_quantize" in ff.ops.__all__ and callable(ff.ops.unfold_quantize)
    assert [item.fn for item in dispatcher._DISPATCHER["unfold"]] == [fused_unfold.KERNELS.unfold]


# ---- the host path against the reference (G30) ------------------------------------------------------------------------------------
def g30_quantizer(spec, got, device="cpu"):
    bits, symmetric, gran, lo, hi = spec
    granularity = ff.PerTensor() if gran == "tensor" else ff.PerChannel(gran[1])
    q = ff.nn.LinearQuantizer(bits, symmetric=symmetric, granularity=granularity, quantized_dtype=torch.int8)
    q.quantization_range = (torch.as_tensor(lo, dtype=torch.float32), torch.as_tensor(hi, dtype=torch.float32))
    with torch.no_grad():
        q.scale.copy_(got["scale"])
        if got["offset"] is not None:
            q.offset.copy_(got["offset"])
    return q.to(device)


def run_g30(case, device="cpu"):
    """(result without an output quantizer, result with the fixture's) of the case's call (shared with the GPU tests)."""
    with torch.no_grad(), ff.strict_quantization(False):
        x = case["input"].to(device)
        arg = x if case["slot"] is None else g30_quantizer(case["slot"], case["params"], device)(x)
        oq = g30_quantizer(G30["out_slot"], G30["out_params"], device)
        return F.unfold(arg, **case["kwargs"]), F.unfold(arg, **case["kwargs"], output_quantizer=oq)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same_as_recorded(got, want):
    if want["type"] == "Tensor":
        assert type(got) is torch.Tensor and got.dtype == want["value"].dtype and got.shape == want["value"].shape
        assert torch.equal(_bits(got.cpu()), _bits(want["value"]))  # (integer patterns: the sign of a zero counts)
    else:
        assert isinstance(got, ff.QuantizedTensor) and torch.equal(got.raw_data.cpu(), want["codes"])
        assert torch.equal(_bits(got.dequantize().cpu()), _bits(want["dequantized"]))


@pytest.mark.parametrize("index", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_host_path_equals_the_reference_bit_for_bit(index):
    case = CASES[index]
    plain, quantized = run_g30(case)
    same_as_recorded(plain, case["plain"])
    same_as_recorded(quantized, case["quantized"])


def test_the_fixture_covers_what_it_names():
    assert len(CASES) == 88 and {c["dtype"] for c in CASES} == {"torch.float32", "torch.bfloat16"}
    assert {None if c["slot"] is None else c["slot"][2] if c["slot"][2] == "tensor" else "channel" for c in CASES} == {None, "tensor", "channel"}
    assert {c["slot"][1] for c in CASES if c["slot"] is not None} == {True, False} and G30["out_slot"][1] is False
    assert len({str(c["kwargs"]) + str(tuple(c["input"].shape)) for c in CASES}) == 11 and {c["input"].dim() for c in CASES} == {3, 4}
    padded = [c for c in CASES if "p2_s1_plain" in c["name"]]  # the +0.0 of the padding has the codes of 0.0, not code 0
    assert padded and all(int(c["quantized"]["codes"].flatten()[0]) not in (0, -128, 127) for c in padded)
    golden_dir = ROOT / "tests" / "golden"
    assert (golden_dir / "g30_unfold.pt").stat().st_size < (golden_dir / "g28_depthwise.pt").stat().st_size


# ---- strict mode: the reference's messages in its order ---------------------------------------------------------------------------
def test_strict_mode_messages_in_the_reference_order():
    q = ff.nn.LinearQuantizer(8, quantized_dtype=torch.int8)
    q.quantization_range = (torch.tensor(-1.0), torch.tensor(1.0))
    x = torch.randn(2, 3, 5, 5)
    with torch.no_grad():
        qx = q(x)
    no_oq = "'output_quantizer' must be provided if strict_quantization=True"
    expected = "Expected 'input' to be an instance of 'QuantizedTensor' because strict_quantization=True."
    with pytest.raises(QuantizationError, match=re.escape(no_oq)):
        F.unfold(x, 3, strict_quantization=True)                               # ... before the operand is looked at
    with pytest.raises(QuantizationError, match=re.escape(expected)):
        F.unfold(x, 3, output_quantizer=q, strict_quantization=True)
    with pytest.raises(QuantizationError, match=re.escape(no_oq)):
        F.unfold(qx, 3, strict_quantization=True)
    with torch.no_grad(), ff.strict_quantization(True):                        # the global flag is the default
        assert isinstance(F.unfold(qx, 3, padding=1, output_quantizer=q), ff.QuantizedTensor)
        with pytest.raises(QuantizationError, match=re.escape(no_oq)):
            F.unfold(qx, 3)
    with torch.no_grad():                                                      # every argument reaches F.unfold, by position and by keyword
        want = torch.nn.functional.unfold(x, (3, 2), (1, 2), (2, 1), (2, 1))
        assert torch.equal(F.unfold(x, (3, 2), (1, 2), (2, 1), (2, 1), strict_quantization=False), want)
        assert torch.equal(F.unfold(x, kernel_size=(3, 2), dilation=(1, 2), padding=(2, 1), stride=(2, 1), strict_quantization=False), want)
        with pytest.raises(RuntimeError):                                      # a window that does not fit: ATen's error
            F.unfold(x, 7, strict_quantization=False)


# ---- the predicate -----------------------------------------------------------------------------------------------------------------
def _codes(shape, granularity=None, channels=None, dtype=torch.bfloat16, container=torch.int8, bits=8):
    q = ff.nn.LinearQuantizer(bits, symmetric=False, granularity=granularity or ff.PerTensor(), quantized_dtype=container)
    q.quantization_range = (torch.tensor(-3.0), torch.tensor(3.0)) if channels is None else (torch.full((channels,), -3.0), torch.full((channels,), 3.0))
    with torch.no_grad():
        return q(torch.randn(shape).to(dtype))


def _out_quantizer():
    q = ff.nn.LinearQuantizer(8, quantized_dtype=torch.int8)
    q.quantization_range = (torch.tensor(-1.0), torch.tensor(1.0))
    return q


def test_the_unfold_predicate_accepts_and_declines(monkeypatch):
    x, oq = _codes((2, 3, 5, 7)), _out_quantizer()
    common = dict(output_quantizer=None, strict_quantization=False)
    assert not fused_unfold.unfold_predicate(input=x, kernel_size=3, **common)                                      # host tensors
    monkeypatch.setattr("fastforward_amd.fused_unfold._on_device", lambda *t: True)

    def ok(**k):
        with torch.no_grad():
            return fused_unfold.KERNELS.supported_unfold(**{**dict(input=x, kernel_size=3), **common, **k})

    assert ok() and ok(output_quantizer=oq) and ok(output_quantizer=oq, strict_quantization=True)
    assert ok(kernel_size=(3, 2), dilation=(1, 2), padding=(2, 1), stride=(2, 1)) and ok(kernel_size=[3, 2]) and ok(kernel_size=torch.Size((5, 7)))
    assert ok(kernel_size=1, padding=2) and ok(kernel_size=7, padding=1) and ok(kernel_size=2, dilation=4) and ok(stride=100)
    assert ok(input=torch.randn(2, 3, 5, 7).bfloat16(), output_quantizer=oq) and ok(input=torch.randn(2, 3, 5, 7).half(), output_quantizer=oq)
    assert ok(input=_codes((2, 3, 5, 7), dtype=torch.float16, container=torch.float16)) and ok(input=_codes((2, 3, 5, 7), bits=4))
    assert ok(input=_codes((2, 3, 5, 7), ff.PerChannel(1), 3)) and ok(input=_codes((2, 3, 5, 7), ff.PerChannel(1), 3), output_quantizer=oq)
    assert ok(input=_codes((3, 5, 7))) and ok(input=_codes((3, 5, 7), ff.PerChannel(0), 3))                         # unbatched
    # the call
    assert not fused_unfold.KERNELS.supported_unfold(x, 3) and not fused_unfold.KERNELS.supported_unfold(x, 3, output_quantizer=oq)   # not ff.nn.functional's
    assert not ok(out=torch.empty(1)) and not fused_unfold.KERNELS.supported_unfold(x, 3, 1, 0, 1, 5, **common)
    assert not ok(strict_quantization=True)                                                                          # the fallback's error
    assert not ok(input=torch.randn(2, 3, 5, 7).bfloat16(), output_quantizer=oq, strict_quantization=True)
    # the input
    assert not ok(input=torch.randn(2, 3, 5, 7).bfloat16())                                                          # plain without a quantizer: im2col alone
    assert not ok(input=torch.randn(2, 3, 5, 7), output_quantizer=oq) and not ok(input=_codes((2, 3, 5, 7), dtype=torch.float32))   # fp32
    assert not ok(input=_codes((2, 3, 5, 7), bits=16, container=torch.int16))
    assert not ok(input=_codes((2, 3, 5, 7), ff.PerChannel(0), 2)) and not ok(input=_codes((3, 5, 7), ff.PerChannel(1), 5))         # other tilings
    assert not ok(input=_codes((2, 3, 5, 7), ff.PerChannel((0, 1)), 6)) and not ok(input=_codes((2, 4, 5, 7), ff.PerBlock(1, 2), 2))
    assert not ok(input=_codes((2, 3, 5, 7), ff.PerChannel(3), 7))
    assert not ok(input=_codes((5, 7))) and not ok(input=_codes((1, 2, 3, 5, 7)))                                    # 2-D, 5-D
    assert not ok(input=_codes((2, 0, 5, 7))) and not ok(input=_codes((0, 3, 5, 7)))                                 # empty
    assert not ok(input=None) and not ok(input=3.0)
    # the geometry
    assert not ok(kernel_size=None) and not ok(kernel_size=3.0) and not ok(kernel_size="3") and not ok(kernel_size=True) and not ok(kernel_size=(3,))
    assert not ok(kernel_size=(3, 3, 3)) and not ok(kernel_size=(3, 2.0)) and not ok(kernel_size=torch.tensor(3))
    assert not ok(padding="same") and not ok(padding=1.0) and not ok(dilation=2.0) and not ok(stride=(1, True)) and not ok(stride=None)
    assert not ok(kernel_size=0) and not ok(kernel_size=(3, 0)) and not ok(kernel_size=-1) and not ok(stride=0) and not ok(dilation=0) and not ok(padding=-1)
    assert not ok(kernel_size=6) and not ok(kernel_size=(3, 8)) and not ok(kernel_size=3, dilation=3) and ok(kernel_size=3, dilation=3, padding=1)   # the window fits
    assert not ok(padding=2**24 + 1) and not ok(stride=2**24 + 1) and not ok(dilation=2**24 + 1)                      # the entry point's limits
    assert not ok(kernel_size=1, padding=2**14)                                                                      # 2^31 or more elements in the result
    with torch.enable_grad():
        assert not fused_unfold.KERNELS.supported_unfold(input=x, kernel_size=3, **common)                           # a gradient is needed
        leaf = torch.randn(2, 3, 5, 7).bfloat16().requires_grad_()
        assert not fused_unfold.KERNELS.supported_unfold(input=leaf, kernel_size=3, output_quantizer=oq, strict_quantization=False)
    # a library without the symbol
    monkeypatch.setattr(fused_unfold._native.library(), ENTRY, None, raising=False)
    assert not ok()


def test_the_other_predicates_are_untouched():
    from fastforward_amd import fused_conv3d

    assert type(fused_conv3d.KERNELS).supported is fused_conv.ConvKernels.supported
    assert not {"supported_cat", "supported_pad", "supported_permute", "supported_index_add", "supported"} & set(vars(fused_unfold.UnfoldKernels))
    assert [it.fn for it in dispatcher._DISPATCHER["pad"]] == [fused_concat.KERNELS.pad]
    assert fused_concat.KERNELS.cat in [it.fn for it in dispatcher._DISPATCHER["cat"]] and len(dispatcher._DISPATCHER["cat"]) == 2
    for op in ("index_add", "permute"):
        assert [it.fn for it in dispatcher._DISPATCHER[op]] == [getattr(fused_index.KERNELS, op)]
    for op in ("conv1d", "conv2d", "conv3d", "conv_transpose1d", "conv_transpose2d"):
        assert dispatcher._DISPATCHER[op] and all(getattr(it.fn, "__self__", None) is not fused_unfold.KERNELS for it in dispatcher._DISPATCHER[op])


def test_the_wrapper_says_not_covered_on_a_library_without_the_symbol(oracle_backend):
    with pytest.raises(BackendError, match="does not export ffq_unfold_quantize"):
        ff.ops.unfold_quantize(torch.zeros(1, 2, 4, 8, dtype=torch.bfloat16), 3)


def test_the_wrapper_checks_its_operands_and_refuses_host_tensors():
    x = torch.zeros(1, 2, 4, 8, dtype=torch.bfloat16)
    with pytest.raises(BackendError, match="HIP device only"):
        ff.ops.unfold_quantize(x, 3)
    for call in (lambda: ff.ops.unfold_quantize(x[0, 0], 3), lambda: ff.ops.unfold_quantize(x[None], 3), lambda: ff.ops.unfold_quantize(x, 3.0),
                 lambda: ff.ops.unfold_quantize(x, (3,)), lambda: ff.ops.unfold_quantize(x, 5), lambda: ff.ops.unfold_quantize(x, 3, stride=0),
                 lambda: ff.ops.unfold_quantize(x, 3, padding=-1), lambda: ff.ops.unfold_quantize(x.float(), 3, dtype=torch.bfloat16),
                 lambda: ff.ops.unfold_quantize(x.to(torch.int8), 3, dtype=torch.bfloat16, dequant=(torch.ones(3), None), per_channel=True)):
        with pytest.raises(RuntimeError):
            call()


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def _header(name):
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / name).read_text(), flags=re.S)


def _declared(name):
    return set(re.findall(r"\b(ffq_[a-z0-9_]+)\s*\(", _header(name)))


def test_the_fifth_header_and_its_table_agree():
    assert _declared("ffq_unfold.h") == set(_cabi.SIGNATURES_UNFOLD) == {ENTRY}
    assert '#include "ffq.h"' in (ROOT / "include" / "ffq_unfold.h").read_text()
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    pointers = {"ffq_fanout": ctypes.POINTER(_cabi.FanOut)}
    params = re.search(ENTRY + r"\s*\((.*?)\)\s*;", _header("ffq_unfold.h"), flags=re.S).group(1).split(",")
    names, want = [], []
    for p in params:
        words = p.replace("*", " * ").split()
        names.append(words[-1])
        want.append(pointers.get(words[words.index("*") - 1], ctypes.c_void_p) if "*" in words else kinds[words[-2]])
    restype, argtypes = _cabi.SIGNATURES_UNFOLD[ENTRY]
    assert restype is ctypes.c_int and argtypes == want
    assert names == ["x", "x_dt", "x_scale", "x_offset", "per_channel", "dt", "B", "C", "H", "W", "KH", "KW", "dil_h", "dil_w", "pad_h", "pad_w",
                     "stride_h", "stride_w", "out", "fan", "stream"]


def test_the_other_tables_are_untouched_and_disjoint():
    assert _declared("ffq.h") == set(_cabi.SIGNATURES) and _declared("ffq_3d.h") == set(_cabi.SIGNATURES_3D)
    assert _declared("ffq_depthwise.h") == set(_cabi.SIGNATURES_DEPTHWISE) and _declared("ffq_index.h") == set(_cabi.SIGNATURES_INDEX)
    mine = set(_cabi.SIGNATURES_UNFOLD)
    for other in (_cabi.SIGNATURES, _cabi.SIGNATURES_3D, _cabi.SIGNATURES_DEPTHWISE, _cabi.SIGNATURES_INDEX, _cabi.DEVICE_ONLY):
        assert not mine & set(other)
    assert _cabi.FFQ_ABI_VERSION == 9 and "#define FFQ_ABI_VERSION 9" in (ROOT / "include" / "ffq.h").read_text()


def test_the_hip_library_exports_it_and_the_oracle_loads_without_it():
    dll, lib, oracle = ctypes.CDLL(str(HIP_SO)), FFQLibrary(HIP_SO), load_oracle()
    assert hasattr(dll, ENTRY) and getattr(lib, ENTRY) is not None
    assert not oracle.is_device and getattr(oracle, ENTRY) is None


FAKE = 1 << 20  # never dereferenced: every call below returns from the argument checks
BF16, F16, I8, F32 = (int(t) for t in (DType.BF16, DType.F16, DType.I8, DType.F32))
BIG = (1 << 24) + 1


def _fan(count=1, bits=8.0, scale=FAKE, codes=FAKE):
    held = min(count, _cabi.FFQ_MAX_FANOUT)
    fan = _cabi.FanOut.make(bits, [scale] * held, [None] * held, [codes] * held)
    fan.count = count  # (a count beyond the struct's arrays is the entry point's to refuse)
    return ctypes.byref(fan)


def _unfold(lib, x=FAKE, x_dt=BF16, xs=None, xo=None, per_channel=0, dt=BF16, B=2, C=3, H=5, W=7, KH=3, KW=2, dh=1, dw=1, ph=0, pw=0, sh=1, sw=1,
            out=FAKE, fan=None):
    return lib.ffq_unfold_quantize(x, x_dt, xs, xo, per_channel, dt, B, C, H, W, KH, KW, dh, dw, ph, pw, sh, sw, out, fan, None)


# in the documented order: each call fails the named check and passes every check ahead of it; most fail a LATER check too and must
# report the earlier one
ERRORS = [
    (lambda lib: _unfold(lib, dt=F32, x_dt=I8), Status.ERR_DTYPE),                             # 1. the value dtype, before the form
    (lambda lib: _unfold(lib, dt=I8, x_dt=I8), Status.ERR_DTYPE),
    (lambda lib: _unfold(lib, x_dt=I8, B=-1), Status.ERR_DTYPE),                               # 2. codes without a scale; before the extents
    (lambda lib: _unfold(lib, x_dt=F16, xs=FAKE, B=-1), Status.ERR_DTYPE),                     #    codes of another float dtype
    (lambda lib: _unfold(lib, xo=FAKE, KH=0), Status.ERR_DTYPE),                               #    an offset without a scale
    (lambda lib: _unfold(lib, per_channel=1, KH=0), Status.ERR_DTYPE),                         #    per-channel without a scale
    (lambda lib: _unfold(lib, B=-1, KH=0), Status.ERR_ARG),                                    # 3. a negative extent; before the empty window
    (lambda lib: _unfold(lib, C=-1), Status.ERR_ARG),
    (lambda lib: _unfold(lib, H=-1), Status.ERR_ARG),
    (lambda lib: _unfold(lib, W=-1), Status.ERR_ARG),
    (lambda lib: _unfold(lib, KH=-1, KW=0), Status.ERR_ARG),
    (lambda lib: _unfold(lib, KW=-1), Status.ERR_ARG),
    (lambda lib: _unfold(lib, KH=0, sh=0), Status.ERR_EMPTY),                                  # 4. an empty window; before stride / dilation / padding
    (lambda lib: _unfold(lib, KW=0, ph=-1), Status.ERR_EMPTY),
    (lambda lib: _unfold(lib, sh=0, H=BIG), Status.ERR_ARG),                                   # 5. stride, dilation, padding; before the limits
    (lambda lib: _unfold(lib, sw=-2), Status.ERR_ARG),
    (lambda lib: _unfold(lib, dh=0), Status.ERR_ARG),
    (lambda lib: _unfold(lib, dw=0), Status.ERR_ARG),
    (lambda lib: _unfold(lib, ph=-1), Status.ERR_ARG),
    (lambda lib: _unfold(lib, pw=-1), Status.ERR_ARG),
    (lambda lib: _unfold(lib, H=BIG, B=1 << 20), Status.ERR_ARG),                              # 6. above 2^24 per axis; before the sizes (ERR_DTYPE)
    (lambda lib: _unfold(lib, W=BIG, B=1 << 20), Status.ERR_ARG),
    (lambda lib: _unfold(lib, KH=BIG, H=BIG - 1, B=1 << 20), Status.ERR_ARG),
    (lambda lib: _unfold(lib, KW=BIG, B=1 << 20), Status.ERR_ARG),
    (lambda lib: _unfold(lib, dh=BIG, KH=1, B=1 << 30), Status.ERR_ARG),                       #    (the window fits: only the limit refuses it)
    (lambda lib: _unfold(lib, dw=BIG, KW=1, B=1 << 30), Status.ERR_ARG),
    (lambda lib: _unfold(lib, ph=BIG, B=1 << 30), Status.ERR_ARG),
    (lambda lib: _unfold(lib, pw=BIG, B=1 << 30), Status.ERR_ARG),
    (lambda lib: _unfold(lib, sh=BIG, B=1 << 30), Status.ERR_ARG),
    (lambda lib: _unfold(lib, sw=BIG, B=1 << 30), Status.ERR_ARG),
    (lambda lib: _unfold(lib, KH=6, B=1 << 30), Status.ERR_ARG),                               # 7. the window does not fit; before the sizes
    (lambda lib: _unfold(lib, KW=8, B=1 << 30), Status.ERR_ARG),
    (lambda lib: _unfold(lib, dh=3, B=1 << 30), Status.ERR_ARG),
    (lambda lib: _unfold(lib, KH=7, ph=1, KW=10, pw=1, B=1 << 30), Status.ERR_ARG),
    (lambda lib: _unfold(lib, B=1 << 30, fan=_fan(4)), Status.ERR_DTYPE),                      # 8. 2^31 elements in x; before the fan-out
    (lambda lib: _unfold(lib, B=1 << 13, C=1 << 13, fan=_fan(4)), Status.ERR_DTYPE),           #    2^26 * 35 in x
    (lambda lib: _unfold(lib, B=1 << 12, C=1 << 12, H=8, W=8, KH=8, KW=8, ph=4, pw=4, fan=_fan(4)), Status.ERR_DTYPE),   # x has 2^30 elements, the result 81 * 2^30
    (lambda lib: _unfold(lib, B=1, C=1, H=4, W=4, KH=1, KW=1, ph=1 << 15, pw=1 << 15, fan=_fan(4)), Status.ERR_DTYPE),   # ... by the padding alone
    (lambda lib: _unfold(lib, B=1 << 62, C=1 << 62, fan=_fan(4)), Status.ERR_DTYPE),           #    no int64 overflow on the way
    (lambda lib: _unfold(lib, fan=_fan(4), x=None), Status.ERR_ARG),                           # 9. the fan-out; before the buffers
    (lambda lib: _unfold(lib, fan=_fan(1, bits=11.0), x=None), Status.ERR_PRECISION),
    (lambda lib: _unfold(lib, fan=_fan(1, scale=None), B=0), Status.ERR_ARG),                  #    ... and before an empty x returns OK
    (lambda lib: _unfold(lib, fan=_fan(1, bits=0.5), C=0), Status.ERR_PRECISION),
    (lambda lib: _unfold(lib, fan=_fan(1, codes=FAKE + 8)), Status.ERR_ARG),                   # 10. misaligned codes
    (lambda lib: _unfold(lib, x=None), Status.ERR_ARG),
    (lambda lib: _unfold(lib, x=FAKE + 2), Status.ERR_ARG),
    (lambda lib: _unfold(lib, x=FAKE + 8, x_dt=I8, xs=FAKE), Status.ERR_ARG),
    (lambda lib: _unfold(lib, out=FAKE + 8), Status.ERR_ARG),
    (lambda lib: _unfold(lib, B=0, x=None, out=None), Status.OK),                              # empty: nothing launched
    (lambda lib: _unfold(lib, C=0, x=None, out=None, fan=_fan(1, codes=FAKE + 8)), Status.OK),
]


@pytest.mark.parametrize("index", range(len(ERRORS)))
def test_argument_checks_need_no_device(index):
    call, status = ERRORS[index]
    lib = FFQLibrary(HIP_SO)
    assert call(lib) == status
    if status != Status.OK:
        assert lib.ffq_last_error()


# ---- the index formula --------------------------------------------------------------------------------------------------------------
def brute_force(x, kernel, dilation, padding, stride):
    """The header's formula, element by element: row c * KH * KW + kh * KW + kw, column oh * OW + ow of the result holds
    x[b, c, oh * sh - ph + kh * dh, ow * sw - pw + kw * dw], or 0 outside the image."""
    (KH, KW), (dh, dw), (ph, pw), (sh, sw) = (ff.ops.unfold.pair(v) for v in (kernel, dilation, padding, stride))
    B, C, H, W = x.shape
    OH, OW = ff.ops.unfold.output_extents(H, W, (KH, KW), (dh, dw), (ph, pw), (sh, sw))
    out = torch.zeros(B, C * KH * KW, OH * OW, dtype=x.dtype)
    for row in range(C * KH * KW):
        c, kh, kw = row // (KH * KW), row // KW % KH, row % KW
        for oh in range(OH):
            ih = oh * sh - ph + kh * dh
            for ow in range(OW):
                iw = ow * sw - pw + kw * dw
                if 0 <= ih < H and 0 <= iw < W:
                    out[:, row, oh * OW + ow] = x[:, c, ih, iw]
    return out


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=[geometry_id(g) for g in GEOMETRIES])
def test_the_index_formula_is_atens(geometry):
    shape, kernel, dilation, padding, stride = geometry
    x = torch.arange(1, 1 + torch.Size(shape).numel(), dtype=torch.float64).reshape(shape)  # (no zero in the image: padding stands out)
    want = torch.nn.functional.unfold(x, kernel, dilation, padding, stride)
    got = brute_force(x if x.dim() == 4 else x[None], kernel, dilation, padding, stride)
    assert torch.equal(got if x.dim() == 4 else got[0], want)


# ---- what hipcc emitted -------------------------------------------------------------------------------------------------------------
def test_the_new_kernels_spill_nothing_and_use_no_scratch():
    if kernel_resources.readelf() is None:
        pytest.skip("llvm-readelf is missing")
    assert kernel_resources.DEFAULT_LIBRARY.exists(), "build() leaves the HIP library in the tree"
    rows = [k for k in kernel_resources.kernel_resources() if "unfold_quantize_kernel" in str(k["name"])]
    assert len(rows) == 12, len(rows)  # {bf16, fp16} x {groups of 8, elements} x {plain, int8 codes, value-dtype codes}
    bad = {str(k["name"]): k for k in rows if k["vgpr_spill_count"] or k["sgpr_spill_count"] or k["private_segment_fixed_size"]}
    assert not bad, bad
    assert all(k["vgpr_count"] + k["agpr_count"] <= 64 for k in rows), rows  # (8 waves per SIMD)
    assert all(k["group_segment_fixed_size"] == 0 for k in rows)              # the patch is not staged in LDS
