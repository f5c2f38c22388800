"""MX formats without a GPU: the twelfth header ``include_mx/ffq_mx.h`` against ``_cabi.SIGNATURES_MX`` (exported by the HIP library, absent
from the oracle, the other tables untouched), every argument error of the four entry points in the documented order before any device
call, the host path (``_host.mx_*``) against the scalar statement of the rule on every bf16 pattern and on the named cases, round trips,
``MXQuantizer`` / ``functional.linear`` / ``QuantizedLinear`` on host tensors, the dispatcher predicates, and what hipcc emitted for the
twenty-one new kernels."""

import ctypes
import math
import re
import sys

import pytest
import torch

import fastforward_amd as ff
import mx_cases

from conftest import HIP_SO, ROOT, load_oracle
from fastforward_amd import _cabi, _host, fused_linear, fused_mx, ops
from fastforward_amd._cabi import DType, FFQLibrary, Status
from fastforward_amd.exceptions import BackendError, QuantizationError
from fastforward_amd.nn import functional as F
from fastforward_amd.quantization import mx

sys.path.insert(0, str(ROOT / "tools"))

import kernel_resources  # noqa: E402

ENTRIES = {"ffq_mx_quantize", "ffq_mx_dequantize", "ffq_linear_mx_supported", "ffq_linear_mx"}
HEADER = ROOT / "include_mx" / "ffq_mx.h"
FORMATS = ("e4m3", "e2m1")


def bits_of(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same(a, b):
    """Bit-equal, or NaN in the same places."""
    return a.shape == b.shape and a.dtype == b.dtype and bool(((bits_of(a) == bits_of(b)) | (a.isnan() & b.isnan())).all())


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
def test_the_functions_the_classes_and_the_header_exist():
    assert {"mx_quantize", "mx_dequantize", "linear_mx", "linear_mx_supported"} <= set(ops.__all__)
    assert all(callable(getattr(ops, n)) for n in ("mx_quantize", "mx_dequantize", "linear_mx", "linear_mx_supported"))
    assert all(callable(getattr(_host, n)) for n in ("mx_quantize", "mx_dequantize", "mx_pack", "mx_unpack"))
    assert ff.quantization.mx is mx and issubclass(mx.MXQuantizationFunction, ff.quantization.QuantizationFunction)
    assert [f.name for f in __import__("dataclasses").fields(mx.MXParameters)][:3] == ["scale", "element_format", "packed"]
    assert issubclass(ff.nn.MXQuantizer, ff.nn.Quantizer) and HEADER.exists()


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
def _strip(path):
    return re.sub(r"/\*.*?\*/", "", path.read_text(), flags=re.S)


def _declared(path):
    return set(re.findall(r"\b(ffq_[a-z0-9_]+)\s*\(", _strip(path)))


def test_the_twelfth_header_and_its_table_agree():
    assert _declared(HEADER) == set(_cabi.SIGNATURES_MX) == ENTRIES
    assert '#include "../include/ffq.h"' in HEADER.read_text()
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
    want_names = {
        "ffq_mx_quantize": ["x", "x_dt", "x_stride", "rows", "K", "format", "codes", "packed", "scales", "stream"],
        "ffq_mx_dequantize": ["codes", "is_packed", "scales", "rows", "K", "format", "out", "out_dt", "stream"],
        "ffq_linear_mx_supported": ["M", "N", "K", "a_format", "w_format"],
        "ffq_linear_mx": ["a_codes", "a_stride", "a_scales", "a_scale_stride", "a_format", "w_codes", "w_stride", "w_scales", "w_scale_stride", "w_format",
                          "bias", "bias_dt", "out", "out_dt", "M", "N", "K", "stream"],
    }
    for entry in ENTRIES:
        m = re.search(r"(\w+)\s+" + entry + r"\s*\((.*?)\)\s*;", _strip(HEADER), flags=re.S)
        names, want = [], []
        for p in m.group(2).split(","):
            words = p.replace("*", " * ").split()
            names.append(words[-1])
            want.append(ctypes.c_void_p if "*" in words else kinds[words[-2]])
        restype, argtypes = _cabi.SIGNATURES_MX[entry]
        assert m.group(1) == "int" and restype is ctypes.c_int and argtypes == want and names == want_names[entry], entry
    text = HEADER.read_text()
    assert "#define FFQ_MX_E4M3 0" in text and "#define FFQ_MX_E2M1 1" in text and (_cabi.MX_E4M3, _cabi.MX_E2M1) == (0, 1)


def test_the_other_tables_are_untouched_and_disjoint():
    others = {"ffq.h": _cabi.SIGNATURES, "ffq_3d.h": _cabi.SIGNATURES_3D, "ffq_depthwise.h": _cabi.SIGNATURES_DEPTHWISE, "ffq_index.h": _cabi.SIGNATURES_INDEX,
              "ffq_unfold.h": _cabi.SIGNATURES_UNFOLD, "ffq_sdpa_decode.h": _cabi.SIGNATURES_DECODE, "ffq_kv_cache.h": _cabi.SIGNATURES_KV,
              "ffq_kv_paged.h": _cabi.SIGNATURES_PAGED, "ffq_kv_token.h": _cabi.SIGNATURES_KV_TOKEN, "ffq_kv_paged_token.h": _cabi.SIGNATURES_PAGED_TOKEN,
              "lpbq/ffq_lpbq.h": _cabi.SIGNATURES_LPBQ}
    for header, table in others.items():
        assert _declared(ROOT / "include" / header) == set(table), header
        assert not ENTRIES & set(table), header
    assert not ENTRIES & set(_cabi.DEVICE_ONLY)
    assert _cabi.FFQ_ABI_VERSION == 9 and "#define FFQ_ABI_VERSION 9" in (ROOT / "include" / "ffq.h").read_text()
    assert sorted(p.name for p in (ROOT / "include_mx").rglob("*.h")) == ["ffq_mx.h"]


def test_the_hip_library_exports_them_and_the_oracle_loads_without_them():
    dll, lib, oracle = ctypes.CDLL(str(HIP_SO)), FFQLibrary(HIP_SO), load_oracle()
    for entry in ENTRIES:
        assert hasattr(dll, entry) and getattr(lib, entry) is not None
        assert not oracle.is_device and getattr(oracle, entry) is None


FAKE = 1 << 20  # never dereferenced: every call below returns from the argument checks
BF16, F16, F32, F64, I8 = (int(t) for t in (DType.BF16, DType.F16, DType.F32, DType.F64, DType.I8))
E4M3, E2M1 = 0, 1


def _quantize(lib, x=FAKE, x_dt=BF16, x_stride=None, rows=4, K=256, fmt=E2M1, codes=FAKE, packed=None, scales=FAKE):
    return lib.ffq_mx_quantize(x, x_dt, K if x_stride is None else x_stride, rows, K, fmt, codes, packed, scales, None)


def _dequantize(lib, codes=FAKE, is_packed=0, scales=FAKE, rows=4, K=256, fmt=E2M1, out=FAKE, out_dt=BF16):
    return lib.ffq_mx_dequantize(codes, is_packed, scales, rows, K, fmt, out, out_dt, None)


def _linear(lib, a=FAKE, a_stride=None, sa=FAKE, sa_stride=None, fa=E4M3, w=FAKE, w_stride=None, sw=FAKE, sw_stride=None, fw=E2M1, bias=None, bias_dt=F32,
            out=FAKE, out_dt=BF16, M=8, N=8, K=256):
    row = lambda f: K // 2 if f == E2M1 else K  # noqa: E731
    return lib.ffq_linear_mx(a, row(fa) if a_stride is None else a_stride, sa, K // 32 if sa_stride is None else sa_stride, fa, w,
                             row(fw) if w_stride is None else w_stride, sw, K // 32 if sw_stride is None else sw_stride, fw, bias, bias_dt, out, out_dt,
                             M, N, K, None)


# in the documented order: each call fails the named check and passes every check ahead of it; most fail a LATER check too and must
# report the earlier one. (call, status, words of the message)
QUANTIZE_ERRORS = [
    (lambda lib: _quantize(lib, x_dt=F64, fmt=7), Status.ERR_DTYPE, "bf16, fp16 or fp32"),                      # 1. the dtype; before the format
    (lambda lib: _quantize(lib, x_dt=I8), Status.ERR_DTYPE, "bf16, fp16 or fp32"),
    (lambda lib: _quantize(lib, fmt=2, rows=-1), Status.ERR_ARG, "element format"),                              # 2. the format; before the extents
    (lambda lib: _quantize(lib, fmt=-1), Status.ERR_ARG, "element format"),
    (lambda lib: _quantize(lib, rows=-1, K=33), Status.ERR_ARG, "bad extent"),                                   # 3. the extents; before K % 32
    (lambda lib: _quantize(lib, K=-32), Status.ERR_ARG, "bad extent"),
    (lambda lib: _quantize(lib, rows=1 << 30, K=64), Status.ERR_ARG, "bad extent"),
    (lambda lib: _quantize(lib, K=48, x_stride=0), Status.ERR_ARG, "K % 32"),                                    # 4. K % 32; before the stride
    (lambda lib: _quantize(lib, x_stride=255, fmt=E4M3, packed=FAKE), Status.ERR_ARG, "row stride 255 is below the row length 256"),   # 5. the stride
    (lambda lib: _quantize(lib, fmt=E4M3, packed=FAKE, x=None), Status.ERR_ARG, "only e2m1"),                    # 6. packed e4m3; before the NULLs
    (lambda lib: _quantize(lib, rows=0, x=None, codes=None, scales=None), Status.OK, ""),                        # 7. empty: nothing launched
    (lambda lib: _quantize(lib, K=0, x_stride=0, x=None, codes=None, scales=None), Status.OK, ""),
    (lambda lib: _quantize(lib, x=None), Status.ERR_ARG, "NULL buffer"),                                         # 8. NULLs; before the alignment
    (lambda lib: _quantize(lib, scales=None, x=FAKE + 1), Status.ERR_ARG, "NULL buffer"),
    (lambda lib: _quantize(lib, codes=None, packed=None, x=FAKE + 1), Status.ERR_ARG, "NULL buffer"),
    (lambda lib: _quantize(lib, x=FAKE + 1), Status.ERR_ARG, "aligned to its element"),                          # 9. the element alignment
    (lambda lib: _quantize(lib, x=FAKE + 2, x_dt=F32), Status.ERR_ARG, "aligned to its element"),
]
DEQUANTIZE_ERRORS = [
    (lambda lib: _dequantize(lib, out_dt=I8, fmt=9), Status.ERR_DTYPE, "bf16, fp16 or fp32"),                    # 1. the dtype
    (lambda lib: _dequantize(lib, fmt=2, is_packed=3), Status.ERR_ARG, "element format"),                        # 2. the format
    (lambda lib: _dequantize(lib, is_packed=2, rows=-1), Status.ERR_ARG, "is_packed is 0 or 1"),                 # 3. is_packed
    (lambda lib: _dequantize(lib, is_packed=1, fmt=E4M3, rows=-1), Status.ERR_ARG, "is_packed is 0 or 1"),
    (lambda lib: _dequantize(lib, rows=-1, K=33), Status.ERR_ARG, "bad extent"),                                 # 4. the extents
    (lambda lib: _dequantize(lib, rows=1 << 30, K=64), Status.ERR_ARG, "bad extent"),
    (lambda lib: _dequantize(lib, K=100, codes=None), Status.ERR_ARG, "K % 32"),                                 # 5. K % 32
    (lambda lib: _dequantize(lib, rows=0, codes=None, scales=None, out=None), Status.OK, ""),                    # 6. empty
    (lambda lib: _dequantize(lib, codes=None, out=FAKE + 1), Status.ERR_ARG, "NULL buffer"),                     # 7. NULLs
    (lambda lib: _dequantize(lib, scales=None), Status.ERR_ARG, "NULL buffer"),
    (lambda lib: _dequantize(lib, out=None), Status.ERR_ARG, "NULL buffer"),
    (lambda lib: _dequantize(lib, out=FAKE + 1), Status.ERR_ARG, "aligned to its element"),                      # 8. the alignment
]
LINEAR_ERRORS = [
    (lambda lib: _linear(lib, fa=2, out_dt=I8), Status.ERR_ARG, "element format"),                               # 1. the formats
    (lambda lib: _linear(lib, fw=-1), Status.ERR_ARG, "element format"),
    (lambda lib: _linear(lib, fa=E2M1, fw=E4M3, out_dt=I8), Status.ERR_ARG, "(A e2m1, W e4m3) is not covered"),   # 2. the refused pair
    (lambda lib: _linear(lib, out_dt=F64, M=-1), Status.ERR_DTYPE, "fp32, bf16 or fp16"),                        # 3. the dtypes
    (lambda lib: _linear(lib, bias=FAKE, bias_dt=F16, out_dt=BF16, M=-1), Status.ERR_DTYPE, "the bias is fp32 or of the output's dtype"),
    (lambda lib: _linear(lib, M=-1, K=100), Status.ERR_ARG, "bad extent"),                                       # 4. the extents
    (lambda lib: _linear(lib, N=1 << 31, K=100), Status.ERR_ARG, "bad extent"),
    (lambda lib: _linear(lib, M=0, K=100, a=None), Status.OK, ""),                                               # 5. empty: nothing launched
    (lambda lib: _linear(lib, N=0, a=None, w=None, out=None), Status.OK, ""),
    (lambda lib: _linear(lib, K=0, a=None), Status.ERR_ARG, "positive multiple of 128"),                         # 6. K % 128
    (lambda lib: _linear(lib, K=96, a=None), Status.ERR_ARG, "positive multiple of 128"),
    (lambda lib: _linear(lib, K=320, a=None), Status.ERR_ARG, "positive multiple of 128"),
    (lambda lib: _linear(lib, a_stride=255, a=None), Status.ERR_ARG, "row stride is below"),                     # 7. the strides
    (lambda lib: _linear(lib, w_stride=127, a=None), Status.ERR_ARG, "row stride is below"),
    (lambda lib: _linear(lib, sa_stride=7, a=None), Status.ERR_ARG, "row stride is below"),
    (lambda lib: _linear(lib, sw_stride=4, a=None), Status.ERR_ARG, "row stride is below"),
    (lambda lib: _linear(lib, a=None, w=FAKE + 1), Status.ERR_ARG, "NULL buffer"),                               # 8. NULLs
    (lambda lib: _linear(lib, sa=None), Status.ERR_ARG, "NULL buffer"),
    (lambda lib: _linear(lib, w=None), Status.ERR_ARG, "NULL buffer"),
    (lambda lib: _linear(lib, sw=None), Status.ERR_ARG, "NULL buffer"),
    (lambda lib: _linear(lib, out=None), Status.ERR_ARG, "NULL buffer"),
    (lambda lib: _linear(lib, a=FAKE + 8, sa=FAKE + 1), Status.ERR_ARG, "code pointers and code row strides must be 16-byte aligned"),   # 9. codes
    (lambda lib: _linear(lib, w=FAKE + 4), Status.ERR_ARG, "code pointers and code row strides must be 16-byte aligned"),
    (lambda lib: _linear(lib, a_stride=264), Status.ERR_ARG, "code pointers and code row strides must be 16-byte aligned"),
    (lambda lib: _linear(lib, w_stride=136), Status.ERR_ARG, "code pointers and code row strides must be 16-byte aligned"),
    (lambda lib: _linear(lib, sa=FAKE + 2, out=FAKE + 1), Status.ERR_ARG, "scale pointers and scale row strides must be 4-byte aligned"),   # 10. scales
    (lambda lib: _linear(lib, sw=FAKE + 1), Status.ERR_ARG, "scale pointers and scale row strides must be 4-byte aligned"),
    (lambda lib: _linear(lib, sa_stride=10), Status.ERR_ARG, "scale pointers and scale row strides must be 4-byte aligned"),
    (lambda lib: _linear(lib, sw_stride=9), Status.ERR_ARG, "scale pointers and scale row strides must be 4-byte aligned"),
    (lambda lib: _linear(lib, out=FAKE + 1), Status.ERR_ARG, "aligned to their elements"),                       # 11. out and bias
    (lambda lib: _linear(lib, bias=FAKE + 2, bias_dt=F32), Status.ERR_ARG, "aligned to their elements"),
]


@pytest.mark.parametrize("errors", [QUANTIZE_ERRORS, DEQUANTIZE_ERRORS, LINEAR_ERRORS], ids=["quantize", "dequantize", "linear"])
def test_argument_errors_in_the_documented_order(errors):
    lib = FFQLibrary(HIP_SO)
    for i, (call, status, words) in enumerate(errors):
        got = call(lib)
        assert got == status, (i, got, lib.ffq_last_error())
        if status != Status.OK:
            assert words in lib.ffq_last_error().decode(), (i, lib.ffq_last_error())


def test_the_shape_predicate():
    lib = FFQLibrary(HIP_SO)
    ok = lib.ffq_linear_mx_supported
    for fa, fw in ((E4M3, E4M3), (E4M3, E2M1), (E2M1, E2M1)):
        assert ok(1, 1, 128, fa, fw) == 1 and ok(300, 129, 640, fa, fw) == 1 and ok(16384, 14336, 4096, fa, fw) == 1
        assert ok(4, 4, 96, fa, fw) == 0 and ok(4, 4, 0, fa, fw) == 0 and ok(4, 4, 192, fa, fw) == 0 and ok(0, 4, 128, fa, fw) == 0 and ok(4, 0, 128, fa, fw) == 0
        assert ok(1 << 31, 4, 128, fa, fw) == 0
    assert ok(4, 4, 128, E2M1, E4M3) == 0 and ok(4, 4, 128, 2, 0) == 0 and ok(4, 4, 128, 0, -1) == 0


def test_the_wrappers_refuse_host_tensors_and_bad_operands():
    x = torch.randn(2, 64)
    with pytest.raises(BackendError):
        ops.mx_quantize(x, "e2m1")
    c, s = _host.mx_quantize(x, "e2m1")
    with pytest.raises(BackendError):
        ops.mx_dequantize(c, s, "e2m1")
    with pytest.raises(BackendError):
        ops.linear_mx(_host.mx_pack(c), s, "e2m1", _host.mx_pack(c), s, "e2m1")
    with pytest.raises(ValueError, match="element format"):
        ops.mx_quantize(x, "e5m2")
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.mx_quantize(torch.randn(2, 48), "e4m3")
    with pytest.raises(ValueError, match="packed form"):
        ops.mx_quantize(x, "e4m3", packed=True)
    with pytest.raises(RuntimeError, match="do not match"):
        ops.linear_mx(c, s, "e2m1", c, s, "e2m1")  # e2m1 operands are packed: [rows, K / 2]
    assert ops.linear_mx_supported(4, 4, 128, "e2m1", "e4m3") is False and ops.linear_mx_supported(4, 4, 128, "e5m2", "e4m3") is False
    assert ops.linear_mx_supported(4, 4, 128, "e4m3", "e2m1") is True and ops.linear_mx_supported(4, 4, 96, "e4m3", "e2m1") is False


# ---- the host path against the scalar rule ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_bf16_pattern_at_five_depths_equals_the_scalar_rule(fmt):
    table = mx_cases.exhaustive_bf16()
    assert table.shape[1] == 32 and table.dtype == torch.bfloat16
    seen = bits_of(table[:, 1:]).to(torch.int32) & 0xFFFF
    assert torch.unique(seen).numel() == 65536  # every pattern, beside a setter
    codes, scales = _host.mx_quantize(table, fmt)
    want_codes, want_scales = mx_cases.scalar_quantize(table, fmt)
    assert codes.dtype == torch.uint8 and codes.shape == table.shape and scales.dtype == torch.uint8 and scales.shape == (table.shape[0], 1)
    assert torch.equal(scales, want_scales)
    assert torch.equal(codes, want_codes), (codes != want_codes).nonzero()[:5]
    # all five depths occur: the setter's block scale exceeds what the patterns alone would give
    assert len(set(scales.flatten().tolist())) > 200


def _block(values, dtype=torch.float32):
    x = torch.zeros(32, dtype=dtype)
    x[: len(values)] = torch.tensor(values, dtype=dtype)
    return x[None]


def test_the_named_roundings():
    # e4m3: the block's amax 448 = 1.75 * 2^8 gives scale 127 (x 1); 17 -> 16, 19 -> 20 (ties to even), 2^-10 -> 0 (half the smallest
    # subnormal 2^-9, tie to the even code 0), 465 saturates at 448 instead of becoming NaN
    codes, scales = _host.mx_quantize(_block([448.0, 17.0, 19.0, 2.0**-10, 3 * 2.0**-10, -17.0]), "e4m3")
    assert int(scales) == 127
    got = _host.mx_dequantize(codes, scales, "e4m3")[0, :6].tolist()
    assert got == [448.0, 16.0, 20.0, 0.0, 2.0**-8, -16.0]
    codes, scales = _host.mx_quantize(_block([465.0, 300.0]), "e4m3")
    assert int(scales) == 127 and _host.mx_dequantize(codes, scales, "e4m3")[0, :2].tolist() == [448.0, 288.0] and int(codes[0, 0]) == 0x7E
    # e2m1 on the scaled value (amax 6 = 1.5 * 2^2: scale 127)
    ties = [6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 7.0, -0.25, -0.75, -5.0, -0.0, 0.2, 0.3]
    want = [6.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 6.0, -0.0, -1.0, -4.0, -0.0, 0.0, 0.5]
    codes, scales = _host.mx_quantize(_block(ties), "e2m1")
    got = _host.mx_dequantize(codes, scales, "e2m1")[0, : len(ties)]
    assert int(scales) == 127 and same(got, torch.tensor(want))
    assert codes[0, 9] == 0x8 and codes[0, 12] == 0x8 and codes[0, 1] == 0  # -0.25 -> -0.0 and -0.0 keep the sign bit
    # the same through a scale: amax 7 * 2^20 has exponent 22 + 127, code 22 + 127 - 2
    codes, scales = _host.mx_quantize(_block([v * 2.0**20 for v in ties[1:]]), "e2m1")
    assert int(scales) == 147 and same(_host.mx_dequantize(codes, scales, "e2m1")[0, : len(ties) - 1], torch.tensor(want[1:]) * 2.0**20)
    for fmt in FORMATS:
        assert torch.equal(torch.stack(mx_cases.scalar_quantize(_block(ties), fmt)[:1]), torch.stack(_host.mx_quantize(_block(ties), fmt)[:1]))


@pytest.mark.parametrize("fmt", FORMATS)
def test_zero_subnormal_huge_and_poisoned_blocks(fmt):
    tiny = torch.tensor([1, 2, 3, 0x7FFFFF, 1 - 2**31], dtype=torch.int32).view(torch.float32).tolist()  # fp32 subnormals
    x = torch.randn(8, 96, generator=torch.Generator().manual_seed(5))
    x[0, :32] = 0.0
    x[0, 5] = -0.0
    x[1, 32:64] = 0.0
    x[1, 32:37] = torch.tensor(tiny)
    x[2, 64:96] = 0.0
    x[2, 64] = 3e38
    x[2, 65] = -1e38
    x[2, 66] = 1.0
    x[3, 40] = math.nan
    x[4, 0] = math.inf
    x[5, 95] = -math.inf
    codes, scales = _host.mx_quantize(x, fmt)
    want_codes, want_scales = mx_cases.scalar_quantize(x, fmt)
    assert torch.equal(codes, want_codes) and torch.equal(scales, want_scales)
    # an all-zero block: code 0 and signed-zero elements; subnormals: e = 0, code 0 (elements times 2^127)
    assert int(scales[0, 0]) == 0 and int(codes[0, :32].sum()) == int(codes[0, 5]) == (0x80 if fmt == "e4m3" else 0x8)
    assert int(scales[1, 1]) == 0
    assert int(scales[2, 2]) == 127 + 127 - mx_cases.EMAX[fmt]
    # a poisoned block: scale 255, zero codes, NaN in all 32 places; its neighbours are untouched
    clean_codes, clean_scales = _host.mx_quantize(torch.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0), fmt)
    deq = _host.mx_dequantize(codes, scales, fmt)
    for row, block in ((3, 1), (4, 0), (5, 2)):
        cols = slice(32 * block, 32 * block + 32)
        assert int(scales[row, block]) == 255 and int(codes[row, cols].sum()) == 0 and bool(deq[row, cols].isnan().all())
        keep = torch.ones(96, dtype=torch.bool)
        keep[cols] = False
        assert torch.equal(codes[row, keep], clean_codes[row, keep]) and not deq[row, keep].isnan().any()
        assert torch.equal(scales[row, [b for b in range(3) if b != block]], clean_scales[row, [b for b in range(3) if b != block]])
    assert int((scales == 255).sum()) == 3


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
def test_dequantization_is_the_scalar_product_and_requantization_is_idempotent(fmt, dtype):
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(6, 128, generator=g) * torch.logspace(-12, 12, 6, base=2.0)[:, None]).to(dtype)
    codes, scales = _host.mx_quantize(x, fmt)
    assert torch.equal(codes, mx_cases.scalar_quantize(x, fmt)[0])
    deq = _host.mx_dequantize(codes, scales, fmt, dtype)
    want = torch.tensor([[mx_cases.scalar_dequantize(int(c), int(scales[r, k // 32]), fmt) for k, c in enumerate(row)] for r, row in enumerate(codes)],
                        dtype=torch.float64)
    assert deq.dtype == dtype and torch.equal(deq, want.to(torch.float32).to(dtype))  # (every product is an fp32 number: one rounding)
    if dtype != torch.float16:  # (fp16 rounds the 2^+-12 rows to subnormals or Inf: not a fixed point)
        again_codes, again_scales = _host.mx_quantize(deq, fmt)
        assert torch.equal(again_codes, codes) and torch.equal(again_scales, scales)
    every = torch.arange(256, dtype=torch.uint8).repeat(1, 1)[:, : 256 if fmt == "e4m3" else 16].repeat(1, 1 if fmt == "e4m3" else 16)
    for code in (0, 1, 127, 254, 255):
        s = torch.full((1, 8), code, dtype=torch.uint8)
        got = _host.mx_dequantize(every, s, fmt)
        want = torch.tensor([mx_cases.scalar_dequantize(int(c), code, fmt) for c in every[0]], dtype=torch.float64).to(torch.float32)
        assert same(got[0], want), code


def test_pack_and_unpack_round_trip():
    codes = torch.randint(0, 16, (3, 5, 64), dtype=torch.uint8, generator=torch.Generator().manual_seed(2))
    packed = _host.mx_pack(codes)
    assert packed.shape == (3, 5, 32) and packed.dtype == torch.uint8
    assert torch.equal(packed[..., 0], codes[..., 0] | (codes[..., 1] << 4))  # element 2i in the low nibble: torch.float4_e2m1fn_x2's order
    assert torch.equal(_host.mx_unpack(packed), codes)
    every = torch.arange(256, dtype=torch.uint8)
    assert torch.equal(_host.mx_pack(_host.mx_unpack(every)), every)


# ---- the quantizer and the modules on host tensors --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_the_quantizer_on_host_tensors(fmt):
    q = ff.nn.MXQuantizer(fmt)
    assert not q.has_uninitialized_params and list(q.parameters()) == [] and f"element_format={fmt}" in repr(q) and "block_size=32" in q.extra_repr()
    x = torch.randn(2, 3, 64, dtype=torch.bfloat16, generator=torch.Generator().manual_seed(3))
    out = q(x)
    codes, scales = _host.mx_quantize(x, fmt)
    assert isinstance(out, ff.QuantizedTensor) and out.raw_data.dtype == torch.uint8 and out.shape == x.shape and torch.equal(out.raw_data, codes)
    params = out.quantization_context.quantization_params
    assert isinstance(params, mx.MXParameters) and torch.equal(params.scale, scales) and params.element_format == fmt and params.packed is None
    assert out.quantization_context.quantization_fn is mx.MXQuantizationFunction
    deq = out.dequantize()
    assert deq.dtype == torch.bfloat16 and torch.equal(deq, _host.mx_dequantize(codes, scales, fmt, torch.bfloat16))
    with ff.strict_quantization(False):
        assert torch.equal((out + 1.0), deq + 1.0) and torch.equal(out.reshape(6, 64), deq.reshape(6, 64))  # float fallbacks and views dequantize
    with pytest.raises(QuantizationError, match="no backward"):
        q(x.float().requires_grad_())
    with torch.no_grad():
        assert torch.equal(q(x.float().requires_grad_()).raw_data, _host.mx_quantize(x.float(), fmt)[0])
    with pytest.raises(ValueError, match="multiple of 32"):
        q(torch.randn(4, 48))
    with pytest.raises(ValueError, match="element format"):
        ff.nn.MXQuantizer("e5m2")
    assert ff.nn.MXQuantizer().element_format == "e2m1"


def _mx_layer(fmt_in, fmt_w, K=64, N=10, bias=True, out=None):
    torch.manual_seed(4)
    layer = ff.nn.QuantizedLinear(K, N, bias=bias)
    layer.input_quantizer = ff.nn.MXQuantizer(fmt_in)
    layer.weight_quantizer = ff.nn.MXQuantizer(fmt_w)
    if out is not None:
        layer.output_quantizer = out
    return layer


def test_linear_on_host_tensors_is_the_float_chain():
    x = torch.randn(5, 64, generator=torch.Generator().manual_seed(6))
    for fmt_in, fmt_w in (("e4m3", "e2m1"), ("e2m1", "e2m1"), ("e2m1", "e4m3")):
        layer = _mx_layer(fmt_in, fmt_w)
        with torch.no_grad(), ff.strict_quantization(False):
            qx, qw = layer.input_quantizer(x), layer.weight_quantizer(layer.weight)
            want = torch.nn.functional.linear(qx.dequantize(), qw.dequantize(), layer.bias)
            assert not fused_mx.fused_linear_mx_predicate(input=qx, weight=qw, bias=layer.bias)  # host tensors: declined
            assert torch.equal(F.linear(qx, qw, layer.bias, strict_quantization=False), want)
            assert torch.equal(layer(x), want)
            assert torch.equal(torch.nn.functional.linear(qx, qw, layer.bias), want)
        with pytest.raises(QuantizationError, match="no backward"):
            layer(x)  # the weight wants a gradient


def test_estimate_ranges_leaves_the_quantizer_alone():
    layer = _mx_layer("e4m3", "e2m1", out=ff.nn.LinearQuantizer(8))
    x = torch.randn(5, 64, generator=torch.Generator().manual_seed(7))
    before = {k: v.detach().clone() for k, v in layer.named_parameters() if "output_quantizer" not in k}
    with torch.no_grad(), ff.strict_quantization(False), ff.estimate_ranges(layer, ff.range_setting.running_minmax, skip_unsupported_quantizers=True):
        layer(x)
    assert not layer.output_quantizer.has_uninitialized_params  # the affine quantizer got its range ...
    for q in (layer.input_quantizer, layer.weight_quantizer):  # ... and the MX quantizers were passed by
        assert isinstance(q, ff.nn.MXQuantizer) and list(q.overrides) == [] and list(q.parameters()) == [] and not q.has_uninitialized_params
    assert sorted(before) == ["bias", "weight"] and all(torch.equal(dict(layer.named_parameters())[k], v) for k, v in before.items())
    with torch.no_grad(), ff.strict_quantization(False):
        out = layer(x)
        qx, qw = layer.input_quantizer(x), layer.weight_quantizer(layer.weight)
        assert torch.equal(out.dequantize(), layer.output_quantizer(torch.nn.functional.linear(qx.dequantize(), qw.dequantize(), layer.bias)).dequantize())


def test_the_predicates_decline_each_others_tensors():
    x, w = torch.randn(4, 128), torch.randn(8, 128)
    affine = ff.nn.LinearQuantizer(8)
    affine.quantization_range = (-3.0, 3.0)
    ax, aw = affine(x), affine(w)
    mq = ff.nn.MXQuantizer("e4m3")
    mxx, mxw = mq(x), mq(w)
    for kwargs in (dict(input=ax, weight=aw), dict(input=ax, weight=mxw), dict(input=mxx, weight=aw), dict(input=x, weight=mxw), dict(input=mxx, weight=w),
                   dict(input=x, weight=w), dict(input=mxx, weight=mxw)):
        assert fused_mx.supported_linear_mx(**kwargs) is False  # (the last: host tensors)
    for kwargs in (dict(input=mxx, weight=mxw), dict(input=ax, weight=mxw), dict(input=mxx, weight=aw), dict(input=x, weight=mxw)):
        assert not fused_linear.fused_linear_predicate(**kwargs) and not fused_linear.fused_linear_weight_only_predicate(**kwargs)
    want = torch.nn.functional.linear(ax.dequantize(), mxw.dequantize())
    assert torch.equal(F.linear(ax, mxw, strict_quantization=False), want)  # a mixed pair takes the float chain


# ---- what hipcc emitted -----------------------------------------------------------------------------------------------------------------
def test_the_mx_kernels_spill_nothing_and_use_no_scratch():
    if kernel_resources.readelf() is None:
        pytest.skip("llvm-readelf is missing")
    assert kernel_resources.DEFAULT_LIBRARY.exists(), "build() leaves the HIP library in the tree"
    rows = [k for k in kernel_resources.kernel_resources() if "mx_" in str(k["name"]) and "kernel" in str(k["name"])]
    rows = [k for k in rows if any(tag in str(k["name"]) for tag in ("mx_quantize_kernel", "mx_dequantize_kernel", "mx_gemm_kernel"))]
    count = lambda tag: len([k for k in rows if tag in str(k["name"])])  # noqa: E731
    # the quantizer and its inverse for bf16 / fp16 / fp32 x {16-byte, element} form; the GEMM for three format pairs x three output dtypes
    assert len(rows) == 21 and count("mx_quantize_kernel") == 6 and count("mx_dequantize_kernel") == 6 and count("mx_gemm_kernel") == 9, [k["name"] for k in rows]
    bad = {str(k["name"]): k for k in rows if k["vgpr_spill_count"] or k["sgpr_spill_count"] or k["private_segment_fixed_size"]}
    assert not bad, bad
    for k in rows:
        name = str(k["name"])
        # the GEMM's LDS: two stages of a 128-row tile per operand, 128 B rows for e4m3 and 64 B rows for e2m1; the others use none
        want = 0
        if "mx_gemm_kernel" in name:
            want = {"Li0ELi0E": 65536, "Li0ELi4E": 49152, "Li4ELi4E": 32768}[re.search(r"Li\dELi\dE", name).group(0)]
        assert k["group_segment_fixed_size"] == want, k
