"""LPBQ weights without a GPU: the eleventh header ``include/lpbq/ffq_lpbq.h`` against ``_cabi.SIGNATURES_LPBQ`` (exported by the HIP
library, absent from the oracle, the ten other tables untouched), every argument error of the three entry points in the documented
order before any device call, the wrappers' operand checks, the host path against the reference's recorded outputs (G32,
tests/golden/g32_lpbq.pt) bit for bit, ``decompress`` / ``LPBQLinearQuantizer`` / ``convert_model`` on host tensors, and what hipcc
emitted for the seventeen new kernels."""

import ctypes
import re
import sys

import pytest
import torch

import fastforward_amd as ff

from conftest import HIP_SO, ROOT, golden, load_oracle
from fastforward_amd import _cabi, ops
from fastforward_amd._cabi import DType, FFQLibrary, Status
from fastforward_amd.exceptions import BackendError, QuantizationError
from fastforward_amd.nn import lpbq_quantizer
from fastforward_amd.quantization import lpbq
from fastforward_amd.quantization.affine.function import StaticAffineQuantParams

sys.path.insert(0, str(ROOT / "tools"))

import kernel_resources  # noqa: E402

ENTRIES = {"ffq_lpbq_compress_scales", "ffq_lpbq_quantize", "ffq_lpbq_expand"}
HEADER = ROOT / "include" / "lpbq" / "ffq_lpbq.h"


def bits_of(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
def test_the_functions_the_class_and_the_header_exist():
    assert {"lpbq_compress_scales", "lpbq_quantize", "lpbq_expand"} <= set(ops.__all__)
    assert callable(ops.lpbq_compress_scales) and callable(ops.lpbq_quantize) and callable(ops.lpbq_expand)
    assert ff.quantization.lpbq is lpbq
    for name in ("LPBQEncoding", "encode", "decompress", "convert_model"):
        assert hasattr(lpbq, name), name
    assert ff.nn.LPBQLinearQuantizer is lpbq_quantizer.LPBQLinearQuantizer and issubclass(ff.nn.LPBQLinearQuantizer, ff.nn.LinearQuantizer)
    assert [f.name for f in __import__("dataclasses").fields(lpbq.LPBQEncoding)] == ["int_scale", "channel_scale", "block_size", "compressed_bw", "decompressed_bw"]
    assert HEADER.exists()


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
def _strip(path):
    return re.sub(r"/\*.*?\*/", "", path.read_text(), flags=re.S)


def _declared(path):
    return set(re.findall(r"\b(ffq_[a-z0-9_]+)\s*\(", _strip(path)))


def test_the_eleventh_header_and_its_table_agree():
    assert _declared(HEADER) == set(_cabi.SIGNATURES_LPBQ) == ENTRIES
    assert '#include "../ffq.h"' in HEADER.read_text()
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
    want_names = {
        "ffq_lpbq_compress_scales": ["scales", "scale_stride", "N", "J", "bits", "int_scale", "channel_scale", "stream"],
        "ffq_lpbq_quantize": ["w", "w_dt", "w_stride", "scales", "scale_stride", "N", "K", "G", "bits", "requantize", "codes8", "channel_scale", "int_scale", "stream"],
        "ffq_lpbq_expand": ["codes4", "packed", "block", "int_scale", "N", "K", "G", "codes8", "stream"],
    }
    for entry in ENTRIES:
        m = re.search(r"(\w+)\s+" + entry + r"\s*\((.*?)\)\s*;", _strip(HEADER), flags=re.S)
        names, want = [], []
        for p in m.group(2).split(","):
            words = p.replace("*", " * ").split()
            names.append(words[-1])
            want.append(ctypes.c_void_p if "*" in words else kinds[words[-2]])
        restype, argtypes = _cabi.SIGNATURES_LPBQ[entry]
        assert m.group(1) == "int" and restype is ctypes.c_int and argtypes == want and names == want_names[entry], entry


def test_the_other_tables_are_untouched_and_disjoint():
    others = {"ffq.h": _cabi.SIGNATURES, "ffq_3d.h": _cabi.SIGNATURES_3D, "ffq_depthwise.h": _cabi.SIGNATURES_DEPTHWISE, "ffq_index.h": _cabi.SIGNATURES_INDEX,
              "ffq_unfold.h": _cabi.SIGNATURES_UNFOLD, "ffq_sdpa_decode.h": _cabi.SIGNATURES_DECODE, "ffq_kv_cache.h": _cabi.SIGNATURES_KV,
              "ffq_kv_paged.h": _cabi.SIGNATURES_PAGED, "ffq_kv_token.h": _cabi.SIGNATURES_KV_TOKEN, "ffq_kv_paged_token.h": _cabi.SIGNATURES_PAGED_TOKEN}
    assert len(others) == 10
    for header, table in others.items():
        assert _declared(ROOT / "include" / header) == set(table), header
        assert not ENTRIES & set(table), header
    assert not ENTRIES & set(_cabi.DEVICE_ONLY)
    assert _cabi.FFQ_ABI_VERSION == 9 and "#define FFQ_ABI_VERSION 9" in (ROOT / "include" / "ffq.h").read_text()
    assert sorted(p.name for p in (ROOT / "include").rglob("*.h")) == sorted([*others, "ffq_lpbq.h"])


def test_the_hip_library_exports_them_and_the_oracle_loads_without_them():
    dll, lib, oracle = ctypes.CDLL(str(HIP_SO)), FFQLibrary(HIP_SO), load_oracle()
    for entry in ENTRIES:
        assert hasattr(dll, entry) and getattr(lib, entry) is not None
        assert not oracle.is_device and getattr(oracle, entry) is None


FAKE = 1 << 20  # never dereferenced: every call below returns from the argument checks
BF16, F16, F32, F64, I8 = (int(t) for t in (DType.BF16, DType.F16, DType.F32, DType.F64, DType.I8))


def _compress(lib, scales=FAKE, stride=None, N=4, J=8, bits=4, int_scale=FAKE, channel=FAKE):
    return lib.ffq_lpbq_compress_scales(scales, J if stride is None else stride, N, J, bits, int_scale, channel, None)


def _quantize(lib, w=FAKE, w_dt=BF16, w_stride=None, scales=FAKE, scale_stride=None, N=4, K=256, G=32, bits=4, requantize=0, codes8=FAKE, channel=FAKE,
              int_scale=FAKE):
    J = K // G if G > 0 else 0
    return lib.ffq_lpbq_quantize(w, w_dt, K if w_stride is None else w_stride, scales, J if scale_stride is None else scale_stride, N, K, G, bits, requantize,
                                 codes8, channel, int_scale, None)


def _expand(lib, codes4=FAKE, packed=0, block=32, int_scale=FAKE, N=4, K=256, G=32, codes8=FAKE):
    return lib.ffq_lpbq_expand(codes4, packed, block, int_scale, N, K, G, codes8, None)


# in the documented order: each call fails the named check and passes every check ahead of it; most fail a LATER check too and must
# report the earlier one. (call, status, words of the message)
COMPRESS_ERRORS = [
    (lambda lib: _compress(lib, bits=5, N=-1), Status.ERR_ARG, "bits must be 2, 3 or 4"),                    # 1. bits; before the extents
    (lambda lib: _compress(lib, bits=1, J=2000), Status.ERR_ARG, "bits must be 2, 3 or 4"),
    (lambda lib: _compress(lib, bits=8), Status.ERR_ARG, "bits must be 2, 3 or 4"),
    (lambda lib: _compress(lib, N=-1, J=2000), Status.ERR_ARG, "bad extent"),                                # 2. the extents; before J's limit
    (lambda lib: _compress(lib, J=-1), Status.ERR_ARG, "bad extent"),
    (lambda lib: _compress(lib, N=1 << 31, J=2000), Status.ERR_ARG, "bad extent"),
    (lambda lib: _compress(lib, J=1025, stride=0), Status.ERR_ARG, "at most 1024"),                          # 3. J <= 1024; before the stride
    (lambda lib: _compress(lib, stride=7, scales=None), Status.ERR_ARG, "row stride 7 is below the row length 8"),   # 4. the stride; before the NULLs
    (lambda lib: _compress(lib, N=0, scales=None, int_scale=None, channel=None), Status.OK, ""),             # 5. empty: nothing launched
    (lambda lib: _compress(lib, J=0, stride=0, scales=None, int_scale=None, channel=None), Status.OK, ""),
    (lambda lib: _compress(lib, scales=None, channel=FAKE + 2), Status.ERR_ARG, "NULL buffer"),              # 6. NULL buffers; before the alignment
    (lambda lib: _compress(lib, int_scale=None, scales=FAKE + 2), Status.ERR_ARG, "NULL buffer"),
    (lambda lib: _compress(lib, channel=None), Status.ERR_ARG, "NULL buffer"),
    (lambda lib: _compress(lib, scales=FAKE + 2), Status.ERR_ARG, "4-byte aligned"),                         # 7. alignment
    (lambda lib: _compress(lib, channel=FAKE + 1), Status.ERR_ARG, "4-byte aligned"),
]

QUANTIZE_ERRORS = [
    (lambda lib: _quantize(lib, w_dt=I8, bits=9), Status.ERR_DTYPE, "bf16, fp16 or fp32"),                   # 1. the weight's dtype; before bits
    (lambda lib: _quantize(lib, w_dt=F64), Status.ERR_DTYPE, "bf16, fp16 or fp32"),
    (lambda lib: _quantize(lib, w_dt=99), Status.ERR_DTYPE, "bf16, fp16 or fp32"),
    (lambda lib: _quantize(lib, bits=5, requantize=2), Status.ERR_ARG, "bits must be 2, 3 or 4"),            # 2. bits; before requantize
    (lambda lib: _quantize(lib, bits=1), Status.ERR_ARG, "bits must be 2, 3 or 4"),
    (lambda lib: _quantize(lib, requantize=2, N=-1), Status.ERR_ARG, "requantize is 0 or 1"),                # 3. requantize; before the extents
    (lambda lib: _quantize(lib, requantize=-1), Status.ERR_ARG, "requantize is 0 or 1"),
    (lambda lib: _quantize(lib, N=-1, K=100), Status.ERR_ARG, "bad extent"),                                 # 4. the extents; before K % G
    (lambda lib: _quantize(lib, K=-32), Status.ERR_ARG, "bad extent"),
    (lambda lib: _quantize(lib, K=1 << 31, G=1 << 20), Status.ERR_ARG, "bad extent"),
    (lambda lib: _quantize(lib, N=1 << 31), Status.ERR_ARG, "bad extent"),
    (lambda lib: _quantize(lib, G=0), Status.ERR_ARG, "bad extent"),
    (lambda lib: _quantize(lib, K=100, G=16, w_stride=1), Status.ERR_ARG, "K % G != 0"),                     # 5. K % G; before the stride
    (lambda lib: _quantize(lib, K=16 * 1025, G=16, w_stride=1), Status.ERR_ARG, "at most 1024"),             # 6. K / G <= 1024; before the stride
    (lambda lib: _quantize(lib, w_stride=255, w=None), Status.ERR_ARG, "row stride is below the row length"),   # 7. the strides; before the NULLs
    (lambda lib: _quantize(lib, scale_stride=7, w=None), Status.ERR_ARG, "row stride is below the row length"),
    (lambda lib: _quantize(lib, N=0, w=None, scales=None, codes8=None, channel=None, int_scale=None), Status.OK, ""),   # 8. empty: nothing launched
    (lambda lib: _quantize(lib, K=0, w=None, scales=None, codes8=None, channel=None, int_scale=None), Status.OK, ""),
    (lambda lib: _quantize(lib, w=None, scales=FAKE + 2), Status.ERR_ARG, "NULL buffer"),                    # 9. NULL buffers; before the alignment
    (lambda lib: _quantize(lib, scales=None, w=FAKE + 1), Status.ERR_ARG, "NULL buffer"),
    (lambda lib: _quantize(lib, codes8=None), Status.ERR_ARG, "NULL buffer"),
    (lambda lib: _quantize(lib, channel=None), Status.ERR_ARG, "NULL buffer"),
    (lambda lib: _quantize(lib, w=FAKE + 1), Status.ERR_ARG, "aligned to its element"),                      # 10. alignment
    (lambda lib: _quantize(lib, w=FAKE + 2, w_dt=F32), Status.ERR_ARG, "aligned to its element"),
    (lambda lib: _quantize(lib, scales=FAKE + 2), Status.ERR_ARG, "aligned to its element"),
    (lambda lib: _quantize(lib, channel=FAKE + 3), Status.ERR_ARG, "aligned to its element"),
]

EXPAND_ERRORS = [
    (lambda lib: _expand(lib, packed=2, N=-1), Status.ERR_ARG, "packed is 0 or 1"),                          # 1. packed; before the extents
    (lambda lib: _expand(lib, packed=-1), Status.ERR_ARG, "packed is 0 or 1"),
    (lambda lib: _expand(lib, N=-1, K=100), Status.ERR_ARG, "bad extent"),                                   # 2. the extents; before K % G
    (lambda lib: _expand(lib, K=1 << 31), Status.ERR_ARG, "bad extent"),
    (lambda lib: _expand(lib, G=0), Status.ERR_ARG, "bad extent"),
    (lambda lib: _expand(lib, K=100, G=16, packed=1, block=0), Status.ERR_ARG, "K % G != 0"),                # 3. K % G; before the block
    (lambda lib: _expand(lib, K=16 * 1025, G=16, packed=1, block=0), Status.ERR_ARG, "at most 1024"),        # 4. K / G <= 1024; before the block
    (lambda lib: _expand(lib, packed=1, block=0, codes4=None), Status.ERR_ARG, "bad block"),                 # 5. a bad block; before the NULLs
    (lambda lib: _expand(lib, packed=1, block=7, codes4=None), Status.ERR_ARG, "bad block"),
    (lambda lib: _expand(lib, packed=1, block=-2, codes4=None), Status.ERR_ARG, "bad block"),
    (lambda lib: _expand(lib, packed=1, block=48, codes4=None), Status.ERR_ARG, "bad block"),                #    48 does not divide 4 * 256
    (lambda lib: _expand(lib, N=0, codes4=None, int_scale=None, codes8=None), Status.OK, ""),                # 6. empty: nothing launched
    (lambda lib: _expand(lib, K=0, packed=1, codes4=None, int_scale=None, codes8=None), Status.OK, ""),
    (lambda lib: _expand(lib, codes4=None, block=7), Status.ERR_ARG, "NULL buffer"),                         # 7. NULL buffers (plain codes ignore the block)
    (lambda lib: _expand(lib, int_scale=None), Status.ERR_ARG, "NULL buffer"),
    (lambda lib: _expand(lib, codes8=None, packed=1), Status.ERR_ARG, "NULL buffer"),
]


@pytest.mark.parametrize("entry,table", [("lpbq_compress_scales", COMPRESS_ERRORS), ("lpbq_quantize", QUANTIZE_ERRORS), ("lpbq_expand", EXPAND_ERRORS)])
def test_argument_checks_need_no_device(entry, table):
    lib = FFQLibrary(HIP_SO)
    for index, (call, status, words) in enumerate(table):
        assert call(lib) == status, (entry, index)
        if status != Status.OK:
            message = lib.ffq_last_error().decode()
            assert message.startswith(f"{entry}: ") and words in message, (index, message)


# ---- the wrappers -----------------------------------------------------------------------------------------------------------------------
def test_the_wrappers_say_not_covered_on_a_library_without_the_symbols(oracle_backend):
    w, s = torch.zeros(4, 64, dtype=torch.bfloat16), torch.ones(4, 4)
    with pytest.raises(BackendError, match="not covered.*ffq_lpbq_compress_scales"):
        ops.lpbq_compress_scales(s)
    with pytest.raises(BackendError, match="not covered.*ffq_lpbq_quantize"):
        ops.lpbq_quantize(w, s, 16)
    with pytest.raises(BackendError, match="not covered.*ffq_lpbq_expand"):
        ops.lpbq_expand(torch.zeros(4, 64, dtype=torch.int8), torch.ones(4, 4, dtype=torch.uint8), 16)


def test_the_wrappers_check_their_operands_and_refuse_host_tensors():
    w, s = torch.zeros(4, 64, dtype=torch.bfloat16), torch.ones(4, 4)
    c, q = torch.zeros(4, 64, dtype=torch.int8), torch.ones(4, 4, dtype=torch.uint8)
    wide_w, wide_s = torch.zeros(4, 96, dtype=torch.bfloat16), torch.ones(4, 9)
    accepted = [lambda: ops.lpbq_compress_scales(s), lambda: ops.lpbq_compress_scales(wide_s[:, 2:6], 2), lambda: ops.lpbq_quantize(w, s, 16),
                lambda: ops.lpbq_quantize(wide_w[:, 8:72], wide_s[:, 1:5], 16, 3, True, False), lambda: ops.lpbq_quantize(w.float(), torch.ones(4, 1), 64),
                lambda: ops.lpbq_expand(c, q, 16), lambda: ops.lpbq_expand(torch.zeros(128, dtype=torch.uint8), q, 16, shape=(4, 64), block=32)]
    for call in accepted:  # views included: they pass the checks and reach the device check
        with pytest.raises(BackendError, match="HIP device only"):
            call()
    refused = [lambda: ops.lpbq_compress_scales(s, 5), lambda: ops.lpbq_compress_scales(s, True), lambda: ops.lpbq_compress_scales(s.double()),
               lambda: ops.lpbq_compress_scales(s[0]), lambda: ops.lpbq_compress_scales(torch.ones(2, 1025)), lambda: ops.lpbq_compress_scales(wide_s[:, ::2]),
               lambda: ops.lpbq_compress_scales(torch.ones(1, 4).expand(4, 4)),
               lambda: ops.lpbq_quantize(w, s, 16, bits=8), lambda: ops.lpbq_quantize(w.to(torch.int8), s, 16), lambda: ops.lpbq_quantize(w[0], s, 16),
               lambda: ops.lpbq_quantize(w, s, 24), lambda: ops.lpbq_quantize(w, s, 0), lambda: ops.lpbq_quantize(w, s, 32), lambda: ops.lpbq_quantize(w, s[:3], 16),
               lambda: ops.lpbq_quantize(w, s.half(), 16), lambda: ops.lpbq_quantize(w.t().contiguous().t(), s, 16), lambda: ops.lpbq_quantize(w, wide_s[:, ::2][:, :4], 16),
               lambda: ops.lpbq_quantize(torch.zeros(2, 2050, dtype=torch.bfloat16), torch.ones(2, 1025), 2),
               lambda: ops.lpbq_expand(c.to(torch.int16), q, 16), lambda: ops.lpbq_expand(c[0], q, 16), lambda: ops.lpbq_expand(c, q.to(torch.int8), 16),
               lambda: ops.lpbq_expand(c, q[:, :3], 16), lambda: ops.lpbq_expand(c, q, 24), lambda: ops.lpbq_expand(c, q, 16, shape=(4, 64)),
               lambda: ops.lpbq_expand(torch.zeros(128, dtype=torch.uint8), q, 16, shape=(4, 64), block=48),
               lambda: ops.lpbq_expand(torch.zeros(128, dtype=torch.uint8), q, 16, shape=(4, 64), block=7),
               lambda: ops.lpbq_expand(torch.zeros(100, dtype=torch.uint8), q, 16, shape=(4, 64)),
               lambda: ops.lpbq_expand(torch.zeros(128, dtype=torch.uint8), q, 16, shape=(4, 8, 8))]
    for i, call in enumerate(refused):
        with pytest.raises(RuntimeError) as caught:
            call()
        assert not isinstance(caught.value, BackendError), f"call {i} reached the library"


# ---- the host path against the reference's recorded outputs (G32) ----------------------------------------------------------------------
G32 = golden("g32_lpbq.pt")


def test_g32_covers_what_it_claims():
    records = G32["compress"]
    assert {(r["J"], r["bits"], r["orientation"], r["dtype"]) for r in records} == {
        (J, b, o, d) for J in (1, 2, 5, 64, 65, 112) for b in (2, 3, 4) for o in ("rows", "columns") for d in ("float32", "bfloat16")}
    seen = set()
    for r in records:
        axis = 1 if r["orientation"] == "rows" else 0
        assert bool((r["q"].amax(dim=axis) == 2 ** r["bits"]).all()) and int(r["q"].min()) >= 1
        if r["bits"] == 4:
            seen |= set(r["q"].flatten().tolist())
    assert seen == set(range(1, 17))
    assert len(G32["encodings"]) == 4 and {e["kind"] for e in G32["errors"]} == {"bitwidths", "unsuitable"}


@pytest.mark.parametrize("index", range(len(G32["compress"])))
def test_the_host_compression_equals_the_reference_bit_for_bit(index):
    r = G32["compress"][index]
    q, d = lpbq.compress_scales(r["scales"], 1 if r["orientation"] == "rows" else 0, r["bits"])
    assert q.dtype == torch.uint8 and q.shape == r["scales"].shape and torch.equal(q, r["q"])
    assert d.dtype == r["scales"].dtype == r["d"].dtype and d.dim() == 1 and torch.equal(bits_of(d), bits_of(r["d"]))


def _recorded_weight(rec):
    granularity = ff.PerBlock(tuple(rec["block_dims"]), tuple(rec["block_sizes"]), tuple(rec["per_channel_dims"]))
    return ff.quantization.affine.quantize_per_granularity(rec["weight"], rec["scale"], None, granularity, 4, torch.int8), granularity


@pytest.mark.parametrize("index", range(len(G32["encodings"])))
def test_the_encoding_dict_equals_the_reference(index):
    rec = G32["encodings"][index]
    qweight, granularity = _recorded_weight(rec)
    assert torch.equal(qweight.raw_data, rec["codes"])  # (the codes the reference's own quantizer produced)
    encoding = lpbq.encode(qweight, name=rec["name"])
    assert encoding.block_size == rec["block_sizes"][0] and encoding.compressed_bw == 4 and encoding.decompressed_bw == 8
    got = encoding.as_dict(rec["name"])
    assert list(got) == list(rec["encoding"]) and got == rec["encoding"]
    assert all(isinstance(v, int) for v in got["per_block_int_scale"]) and got["enc_type"] == "LPBQ" and set(got["offset"]) == {-128.0}
    # the parameters alone, with the shape, give the same
    params = qweight.quantization_context.quantization_params
    assert lpbq.encode(params, data_shape=rec["shape"]).as_dict(rec["name"]) == rec["encoding"]
    # an explicit tile instead of the PerBlock granularity is as suitable as for the reference (granularity_from_sizes)
    tiled = StaticAffineQuantParams(rec["scale"], None, 4, ff.PerTile(granularity.tile_size(torch.Size(rec["shape"]))))
    assert lpbq.encode(tiled, data_shape=rec["shape"]).as_dict(rec["name"]) == rec["encoding"]


def test_the_references_error_texts():
    qweight, _ = _recorded_weight(G32["encodings"][0])
    shape = (8, 32)
    block = ff.PerBlock(1, 16, 0)
    unsuitable = {
        "per_channel": StaticAffineQuantParams(torch.full((8,), 0.1), None, 4, ff.PerChannel(0)),
        "per_tensor": StaticAffineQuantParams(torch.full((1,), 0.1), None, 4, ff.PerTensor()),
        "two_block_dims": StaticAffineQuantParams(torch.full((8,), 0.1), None, 4, ff.PerTile((4, 8))),
        "asymmetric": StaticAffineQuantParams(torch.full((16,), 0.1), torch.full((16,), 3.0), 4, block),
        "bitwidth": StaticAffineQuantParams(torch.full((16,), 0.1), torch.zeros(16), 8, block),
    }
    seen = set()
    for rec in G32["errors"]:
        with pytest.raises(ValueError) as caught:
            if rec["kind"] == "bitwidths":
                lpbq.encode(qweight, rec["compressed_bw"], rec["decompressed_bw"])
            else:
                lpbq.encode(unsuitable[rec["what"]], name=rec["name"], data_shape=shape)
        assert str(caught.value) == rec["text"], rec
        seen.add(rec.get("what", (rec.get("compressed_bw"), rec.get("decompressed_bw"))))
    assert set(unsuitable) <= seen and len(seen) == len(G32["errors"]) == 11
    lpbq.encode(StaticAffineQuantParams(torch.full((16,), 0.1), torch.zeros(16), 4, block), data_shape=shape)  # an all-zero offset is symmetric
    with pytest.raises(TypeError):
        lpbq.encode(unsuitable["bitwidth"])                                                                    # parameters without a shape


# ---- decompress and the quantizer on host tensors -----------------------------------------------------------------------------------------
def block_range(w, G):
    blocks = w.float().reshape(w.shape[0], w.shape[1] // G, G)
    return blocks.amin(-1).reshape(-1), blocks.amax(-1).reshape(-1)


def make_quantizer(w, G, bits=4, **kw):
    q = ff.nn.LPBQLinearQuantizer(bits, G, **kw)
    q.quantization_range = block_range(w, G)
    return q


@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
def test_decompress_and_the_quantizer_on_host_tensors(dtype, bits):
    torch.manual_seed(bits)
    N, K, G = 7, 96, 16
    w = (torch.randn(N, K) * torch.rand(N, 1).add(0.1) * torch.rand(1, K // G).add(0.05).repeat_interleave(G, 1)).to(dtype)
    q = make_quantizer(w, G, bits)
    assert not q.is_plain() and q.symmetric and q.offset is None and q.granularity == ff.PerBlock(1, G, 0) and q.scale.shape == (N * K // G,)
    with torch.no_grad():
        out, compressed = q(w), q.compressed(w)
    p4 = compressed.quantization_context.quantization_params
    assert p4.num_bits == bits and p4.granularity == ff.PerBlock(1, G, 0) and compressed.raw_data.dtype == dtype
    int_scale, channel_scale = lpbq.compress_scales(q.scale.detach().reshape(N, K // G), 1, bits)
    want = compressed.raw_data.to(torch.int32) * int_scale.to(torch.int32).repeat_interleave(G, 1)
    lo, hi = -(2 ** (2 * bits - 1)), 2 ** (2 * bits - 1) - 2**bits
    assert lo <= int(want.min()) and int(want.max()) <= hi and int(int_scale.max()) == 2**bits
    for got in (out, lpbq.decompress(compressed)):
        p = got.quantization_context.quantization_params
        assert isinstance(got, ff.QuantizedTensor) and got.raw_data.dtype == torch.int8 and torch.equal(got.raw_data.to(torch.int32), want)
        assert p.granularity == ff.PerChannel(0) and p.num_bits == 8 and p.offset is None and p.quantized_dtype == torch.int8 and p.dequantize_dtype == dtype
        assert torch.equal(bits_of(p.scale), bits_of(channel_scale)) and p.scale.shape == (N,)
        exact = (want.double() * channel_scale.double()[:, None]).to(dtype)  # one rounding: the fp32 product is exact (8 x 24 bits)
        assert got.dequantize().dtype == dtype and torch.equal(bits_of(got.dequantize()), bits_of(exact))
    encoding = q.encoding(w.shape)
    assert torch.equal(encoding.int_scale, int_scale) and torch.equal(encoding.channel_scale, channel_scale) and encoding.block_size == G
    assert encoding.compressed_bw == bits and encoding.decompressed_bw == 8


def test_requantize_rounds_against_the_scale_that_is_applied():
    torch.manual_seed(5)
    N, K, G = 5, 64, 16
    w = torch.randn(N, K).to(torch.bfloat16)
    plain, again = make_quantizer(w, G), make_quantizer(w, G, requantize=True)
    with torch.no_grad():
        a, b = plain(w), again(w)
    int_scale, channel_scale = lpbq.compress_scales(again.scale.detach().reshape(N, K // G), 1, 4)
    applied = channel_scale[:, None] * int_scale.float()
    codes4 = ops.quantize_by_tile(w, applied, (1, G), 4, torch.int8)
    assert torch.equal(b.raw_data, (codes4.int() * int_scale.int().repeat_interleave(G, 1)).to(torch.int8))
    assert torch.equal(bits_of(b.quantization_context.quantization_params.scale), bits_of(a.quantization_context.quantization_params.scale))
    assert torch.equal(again.encoding(w.shape).int_scale, plain.encoding(w.shape).int_scale)
    assert not torch.equal(a.raw_data, b.raw_data)  # (the two roundings do differ somewhere on this weight)


def test_the_constructor_gradients_and_the_uninitialised_quantizer():
    for bad in (dict(num_bits=5), dict(num_bits=0), dict(num_bits=4, decompressed_bits=16), dict(num_bits=4, decompressed_bits=7), dict(num_bits=3.0),
                dict(num_bits=4, block_size=0), dict(num_bits=4, block_size=None), dict(num_bits=True)):
        with pytest.raises(ValueError, match="^LPBQLinearQuantizer: "):
            ff.nn.LPBQLinearQuantizer(**{"block_size": 16, **bad})
    q = ff.nn.LPBQLinearQuantizer(4, 16)
    assert not q.is_plain() and q.num_bits == 4 and q.requantize is False and q.decompressed_bits == 8
    w = torch.randn(4, 32)
    with pytest.raises(ValueError, match="uninitialized quantizer"):
        q(w)
    q.quantization_range = block_range(w, 16)
    leaf = w.clone().requires_grad_()
    with pytest.raises(QuantizationError, match="LPBQLinearQuantizer has no backward"):
        q(leaf)
    with torch.no_grad():
        assert q(leaf).raw_data.dtype == torch.int8
    assert q(leaf.detach()).raw_data.dtype == torch.int8
    with ff.estimate_ranges(q, ff.range_setting.running_minmax), torch.no_grad():   # range estimation moves the block scales
        q(w * 3)
    assert q.scale.shape == (8,) and bool((q.scale > 0).all())


# ---- convert_model ------------------------------------------------------------------------------------------------------------------------
def _layers():
    torch.manual_seed(11)
    model = torch.nn.Sequential(*[torch.nn.Linear(32, 8) for _ in range(8)])
    ff.quantize_model(model)
    LQ, G = ff.nn.LinearQuantizer, 16
    block = lambda: ff.PerBlock(1, G, 0)  # noqa: E731
    quantizers = {
        0: LQ(4, symmetric=True, allow_one_sided=False, granularity=block(), quantized_dtype=torch.int8),   # converted
        1: LQ(4, symmetric=True, granularity=block()),                                                      # converted: its offset buffer is all zero
        2: LQ(4, symmetric=True, allow_one_sided=False, granularity=ff.PerChannel(0)),                      # per channel
        3: LQ(4, symmetric=False, granularity=block()),                                                     # asymmetric
        4: LQ(8, symmetric=True, allow_one_sided=False, granularity=block()),                               # 8 bits
        5: LQ(4, symmetric=True, granularity=block()),                                                      # one-sided: a non-zero offset
        6: LQ(4, symmetric=True, allow_one_sided=False, granularity=block()),                               # uninitialised
        7: LQ(3, symmetric=True, allow_one_sided=False, granularity=block()),                               # converted: 3 bits
    }
    with torch.no_grad():
        model[5].weight.abs_()
    for i, q in quantizers.items():
        layer = model[i]
        layer.weight_quantizer = q
        if i == 6:
            continue
        w = layer.weight.detach()
        q.quantization_range = (w.amin(1), w.amax(1)) if i == 2 else block_range(w, G)
        layer.input_quantizer = LQ(8, symmetric=False, quantized_dtype=torch.int8)
        layer.input_quantizer.quantization_range = (-4.0, 4.0)
    return model, quantizers


def test_convert_model_replaces_exactly_the_matching_quantizers():
    model, before = _layers()
    assert bool((before[1].offset == 0).all()) and bool((before[5].offset != 0).all())
    x = torch.randn(3, 32)
    replaced = lpbq.convert_model(model)
    assert replaced == ["0.weight_quantizer", "1.weight_quantizer", "7.weight_quantizer"]
    for i, old in before.items():
        new = model[i].weight_quantizer
        if i in (0, 1, 7):
            assert type(new) is ff.nn.LPBQLinearQuantizer and new.scale is old.scale and new.num_bits == old.num_bits and new.block_size == 16
            assert new.quantized_dtype == old.quantized_dtype and new.offset is None and new.quant_metadata is old.quant_metadata and not new.is_plain()
            assert dict(model[i].named_parameters())["weight_quantizer.scale"] is old.scale
        else:
            assert new is old
        assert type(model[i].input_quantizer) is not ff.nn.LPBQLinearQuantizer
    assert lpbq.convert_model(model) == []  # nothing left to convert
    # a converted layer on host tensors: the float fallback's value of the int8 tensor
    with torch.no_grad(), ff.strict_quantization(False):
        for i in (0, 1, 7):
            layer = model[i]
            got = layer(x)
            qx, qw = layer.input_quantizer(x), layer.weight_quantizer(layer.weight)
            assert qw.raw_data.dtype == torch.int8 and qw.quantization_context.quantization_params.granularity == ff.PerChannel(0)
            assert torch.equal(got, torch.nn.functional.linear(qx.dequantize(), qw.dequantize(), layer.bias))
    # range setting through the shared parameter reaches the converted quantizer
    with torch.no_grad():
        before[0].scale.mul_(2.0)
    assert model[0].weight_quantizer.scale is before[0].scale


# ---- what hipcc emitted -----------------------------------------------------------------------------------------------------------------
def test_the_lpbq_kernels_spill_nothing_and_use_no_scratch():
    if kernel_resources.readelf() is None:
        pytest.skip("llvm-readelf is missing")
    assert kernel_resources.DEFAULT_LIBRARY.exists(), "build() leaves the HIP library in the tree"
    rows = [k for k in kernel_resources.kernel_resources() if "lpbq" in str(k["name"])]
    count = lambda tag: len([k for k in rows if tag in str(k["name"])])  # noqa: E731
    # one compression kernel; the quantizer for bf16 / fp16 / fp32 x {wave, workgroup} per row x {group, element}; expand x {codes, nibbles} x {group, element}
    assert len(rows) == 17 and count("lpbq_compress_kernel") == 1 and count("lpbq_quantize_kernel") == 12, [k["name"] for k in rows]
    assert count("lpbq_expand_group_kernel") == 2 and count("lpbq_expand_element_kernel") == 2
    bad = {str(k["name"]): k for k in rows if k["vgpr_spill_count"] or k["sgpr_spill_count"] or k["private_segment_fixed_size"]}
    assert not bad, bad
    for k in rows:
        name = str(k["name"])
        # the quantizer's LDS: a row's q (1024 bytes) per row of the workgroup, and four wave maxima where the workgroup owns one row
        want = 4 * 1024 if "Li64E" in name else 1024 + 16 if "Li256E" in name else 0
        assert k["group_segment_fixed_size"] == want, k
