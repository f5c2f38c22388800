"""The paged KV cache with per-token dynamic scales without a GPU: the tenth header ``include/ffq_kv_paged_token.h`` against
``_cabi.SIGNATURES_PAGED_TOKEN`` (exported by the HIP library, absent from the oracle, the nine other tables untouched), every argument
error of ``ffq_kv_paged_token_append`` and ``ffq_kv_paged_token_decode`` in the documented order before any device call, the wrappers'
operand checks, what ``nn.PagedDynamicQuantizedKVCache`` takes and refuses (and that the two classes it combines still take and refuse
what they did), its free list and reference counts over a seeded run of operations, the composed route on host tensors against
``nn.DynamicQuantizedKVCache`` bit for bit, and what hipcc emitted for the eight new kernels."""

import ctypes
import random
import re
import sys

import pytest
import torch

import fastforward_amd as ff

import kv_cache_cases as dense_cases
import kv_paged_token_cases as cases

from conftest import HIP_SO, ROOT, load_oracle
from fastforward_amd import _cabi, ops
from fastforward_amd._cabi import DType, FFQLibrary, Status
from fastforward_amd.exceptions import BackendError
from fastforward_amd.nn import kv_cache
from fastforward_amd.ops import decode

sys.path.insert(0, str(ROOT / "tools"))

import kernel_resources  # noqa: E402

ENTRIES = {"ffq_kv_paged_token_append", "ffq_kv_paged_token_decode"}
HEADER = "ffq_kv_paged_token.h"


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
def test_the_functions_and_the_class_exist():
    assert {"kv_paged_token_append", "kv_paged_token_decode"} <= set(ops.__all__)
    assert callable(ops.kv_paged_token_append) and callable(ops.kv_paged_token_decode)
    assert ff.nn.PagedDynamicQuantizedKVCache is kv_cache.PagedDynamicQuantizedKVCache
    assert issubclass(kv_cache.PagedDynamicQuantizedKVCache, kv_cache._CacheBase)
    assert callable(kv_cache.composed_paged_token_append) and callable(kv_cache.composed_paged_token_attend)
    # the bookkeeping is stated once: both paged classes run the same functions
    for method in ("reserve", "release", "share_prefix", "pages"):
        assert getattr(kv_cache.PagedDynamicQuantizedKVCache, method) is getattr(kv_cache.PagedQuantizedKVCache, method), method
    assert kv_cache.PagedDynamicQuantizedKVCache.free_pages is kv_cache.PagedQuantizedKVCache.free_pages


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
def _header(name):
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / name).read_text(), flags=re.S)


def _declared(name):
    return set(re.findall(r"\b(ffq_[a-z0-9_]+)\s*\(", _header(name)))


def test_the_tenth_header_and_its_table_agree():
    assert _declared(HEADER) == set(_cabi.SIGNATURES_PAGED_TOKEN) == ENTRIES
    text = (ROOT / "include" / HEADER).read_text()
    assert '#include "ffq_kv_paged.h"' in text and '#include "ffq_kv_token.h"' in text
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
    want_names = {
        "ffq_kv_paged_token_append": ["k_new", "v_new", "dt", "k_pool", "v_pool", "param_pool", "lens", "block_table", "batch", "kv_heads", "L", "num_pages",
                                      "P", "max_pages", "table_stride", "E", "strides", "k_num_bits", "k_symmetric", "v_num_bits", "v_symmetric",
                                      "cos_table", "sin_table", "table_rows", "stream"],
        "ffq_kv_paged_token_decode": ["q", "q_dt", "k_pool", "v_pool", "dt", "q_scale", "q_offset", "param_pool", "lens", "block_table", "batch", "q_heads",
                                      "kv_heads", "L", "num_pages", "P", "max_pages", "table_stride", "E", "strides", "causal", "sqrt_scale", "out_scale",
                                      "out_offset", "out_num_bits", "splits", "plan_len", "out", "workspace", "workspace_bytes", "stream"],
    }
    for entry in ENTRIES:
        m = re.search(r"(\w+)\s+" + entry + r"\s*\((.*?)\)\s*;", _header(HEADER), flags=re.S)
        names, want = [], []
        for p in m.group(2).split(","):
            words = p.replace("*", " * ").split()
            names.append(words[-1])
            if "*" in words:
                want.append(ctypes.POINTER(ctypes.c_int64) if words[words.index("*") - 1] == "int64_t" else ctypes.c_void_p)
            else:
                want.append(kinds[words[-2]])
        restype, argtypes = _cabi.SIGNATURES_PAGED_TOKEN[entry]
        assert m.group(1) == "int" and restype is ctypes.c_int and argtypes == want and names == want_names[entry], entry


def test_the_other_tables_are_untouched_and_disjoint():
    others = {"ffq.h": _cabi.SIGNATURES, "ffq_3d.h": _cabi.SIGNATURES_3D, "ffq_depthwise.h": _cabi.SIGNATURES_DEPTHWISE, "ffq_index.h": _cabi.SIGNATURES_INDEX,
              "ffq_unfold.h": _cabi.SIGNATURES_UNFOLD, "ffq_sdpa_decode.h": _cabi.SIGNATURES_DECODE, "ffq_kv_cache.h": _cabi.SIGNATURES_KV,
              "ffq_kv_paged.h": _cabi.SIGNATURES_PAGED, "ffq_kv_token.h": _cabi.SIGNATURES_KV_TOKEN}
    assert len(others) == 9
    for header, table in others.items():
        assert _declared(header) == set(table), header
        assert not ENTRIES & set(table), header
    assert not ENTRIES & set(_cabi.DEVICE_ONLY)
    assert set(_cabi.SIGNATURES_KV) == {"ffq_kv_append", "ffq_kv_decode"}
    assert set(_cabi.SIGNATURES_PAGED) == {"ffq_kv_paged_append", "ffq_kv_paged_decode"}
    assert set(_cabi.SIGNATURES_KV_TOKEN) == {"ffq_kv_token_append", "ffq_kv_token_decode"}
    assert set(_cabi.SIGNATURES_DECODE) == {"ffq_sdpa_decode", "ffq_sdpa_decode_splits", "ffq_sdpa_decode_workspace_bytes"}
    assert _cabi.FFQ_ABI_VERSION == 9 and "#define FFQ_ABI_VERSION 9" in (ROOT / "include" / "ffq.h").read_text()
    assert len(list((ROOT / "include").glob("*.h"))) == 10


def test_the_hip_library_exports_them_and_the_oracle_loads_without_them():
    dll, lib, oracle = ctypes.CDLL(str(HIP_SO)), FFQLibrary(HIP_SO), load_oracle()
    for entry in ENTRIES:
        assert hasattr(dll, entry) and getattr(lib, entry) is not None
        assert not oracle.is_device and getattr(oracle, entry) is None


FAKE = 1 << 20  # never dereferenced: every call below returns from the argument checks
BF16, F16, I8, F32 = (int(t) for t in (DType.BF16, DType.F16, DType.I8, DType.F32))


def _append_strides(HKV=2, L=1, P=16, E=128, **change):
    s = [HKV * L * E, L * E, E] * 2 + [HKV * P * E, P * E, E] * 2 + [HKV * P * 4, P * 4, 4]
    for i, value in change.items():
        s[int(i[1:])] = value
    return tuple(s)


def _append(lib, k_new=FAKE, v_new=FAKE, dt=BF16, k_pool=FAKE, v_pool=FAKE, params=FAKE, lens=FAKE, table=FAKE, B=2, HKV=2, L=1, num_pages=40, P=16,
            max_pages=8, table_stride=None, E=128, strides="dense", kbits=8.0, ksym=0, vbits=4.0, vsym=1, cos=None, sin=None, table_rows=0):
    if strides == "dense":
        strides = _append_strides()
    return lib.ffq_kv_paged_token_append(k_new, v_new, dt, k_pool, v_pool, params, lens, table, B, HKV, L, num_pages, P, max_pages,
                                         max_pages if table_stride is None else table_stride, E,
                                         None if strides is None else (ctypes.c_int64 * 15)(*strides), kbits, ksym, vbits, vsym, cos, sin, table_rows, None)


# in the documented order: each call fails the named check and passes every check ahead of it; most fail a LATER check too and must
# report the earlier one. (call, status, words of the message)
APPEND_ERRORS = [
    (lambda lib: _append(lib, dt=F32, strides=None), Status.ERR_DTYPE, "bf16 or fp16 values"),                    # 1. the value dtype; before the table
    (lambda lib: _append(lib, dt=I8, E=96), Status.ERR_DTYPE, "bf16 or fp16 values"),
    (lambda lib: _append(lib, strides=None, E=96), Status.ERR_ARG, "NULL strides table"),                         # 2. the strides table; before E
    (lambda lib: _append(lib, E=96, B=-1), Status.ERR_ARG, "E must be 64 or 128"),                                # 3. E; before the extents
    (lambda lib: _append(lib, E=32), Status.ERR_ARG, "E must be 64 or 128"),
    (lambda lib: _append(lib, B=-1, P=24), Status.ERR_ARG, "bad extent"),                                         # 4. the extents; before the geometry
    (lambda lib: _append(lib, L=-1, P=24), Status.ERR_ARG, "bad extent"),
    (lambda lib: _append(lib, HKV=0, P=24), Status.ERR_ARG, "bad extent"),
    (lambda lib: _append(lib, P=24, kbits=9.0), Status.ERR_ARG, "power of two in 16..256"),                       # 5. the geometry, in paging_error's order
    (lambda lib: _append(lib, P=8, kbits=9.0), Status.ERR_ARG, "power of two in 16..256"),
    (lambda lib: _append(lib, P=512, kbits=9.0), Status.ERR_ARG, "power of two in 16..256"),
    (lambda lib: _append(lib, P=0, num_pages=0), Status.ERR_ARG, "power of two in 16..256"),
    (lambda lib: _append(lib, num_pages=0, max_pages=0), Status.ERR_ARG, "num_pages must be"),
    (lambda lib: _append(lib, num_pages=1 << 31, kbits=9.0), Status.ERR_ARG, "num_pages must be"),
    (lambda lib: _append(lib, max_pages=0, table_stride=0, kbits=9.0), Status.ERR_ARG, "max_pages must be >= 1"),
    (lambda lib: _append(lib, max_pages=1 << 26, kbits=9.0), Status.ERR_ARG, "below 2^30"),                       #    16 * 2^26 = 2^30 positions
    (lambda lib: _append(lib, max_pages=1 << 62, kbits=9.0), Status.ERR_ARG, "below 2^30"),
    (lambda lib: _append(lib, table_stride=7, kbits=9.0), Status.ERR_ARG, "row stride is below max_pages"),
    (lambda lib: _append(lib, kbits=9.0, ksym=2), Status.ERR_ARG, "bit-width in 2..8"),                           # 6. the bit-widths; before the flags
    (lambda lib: _append(lib, kbits=1.0), Status.ERR_ARG, "bit-width in 2..8"),
    (lambda lib: _append(lib, vbits=3.5), Status.ERR_ARG, "bit-width in 2..8"),
    (lambda lib: _append(lib, vbits=0.0, L=0), Status.ERR_ARG, "bit-width in 2..8"),
    (lambda lib: _append(lib, ksym=2, cos=FAKE), Status.ERR_ARG, "symmetric is 0"),                               # 7. the symmetric flags; before the tables
    (lambda lib: _append(lib, vsym=-1, cos=FAKE), Status.ERR_ARG, "symmetric is 0"),
    (lambda lib: _append(lib, cos=FAKE, sin=None, table_rows=1), Status.ERR_ARG, "come as a pair"),               # 8. one rotary table without the other
    (lambda lib: _append(lib, cos=None, sin=FAKE, B=0), Status.ERR_ARG, "come as a pair"),
    (lambda lib: _append(lib, cos=FAKE, sin=FAKE, table_rows=127, L=0), Status.ERR_ARG, "position of a sequence (127 < 128)"),  # 9. table_rows < C = 128
    (lambda lib: _append(lib, B=0, k_new=None, lens=None, table=None, params=None, k_pool=FAKE + 1), Status.OK, ""),             # 10. empty: nothing launched
    (lambda lib: _append(lib, L=0, k_new=None, lens=None, table=None, params=None, k_pool=FAKE + 1), Status.OK, ""),
    (lambda lib: _append(lib, L=1 << 40, k_new=None), Status.ERR_ARG, "too large"),                               # 11. the sizes
    (lambda lib: _append(lib, B=1 << 20, L=1 << 20, k_new=None), Status.ERR_ARG, "too large"),
    (lambda lib: _append(lib, k_new=FAKE + 8, v_pool=None), Status.ERR_ARG, "16-byte aligned (lens, block_table: 4-byte)"),      # 12. alignment; before the NULLs
    (lambda lib: _append(lib, v_new=FAKE + 2, v_pool=None), Status.ERR_ARG, "16-byte aligned"),
    (lambda lib: _append(lib, k_pool=FAKE + 4, v_pool=None), Status.ERR_ARG, "16-byte aligned"),
    (lambda lib: _append(lib, v_pool=FAKE + 1, k_new=None), Status.ERR_ARG, "16-byte aligned"),
    (lambda lib: _append(lib, params=FAKE + 4, k_new=None), Status.ERR_ARG, "16-byte aligned"),
    (lambda lib: _append(lib, lens=FAKE + 2, k_new=None), Status.ERR_ARG, "16-byte aligned"),
    (lambda lib: _append(lib, table=FAKE + 2, k_new=None), Status.ERR_ARG, "16-byte aligned"),
    (lambda lib: _append(lib, cos=FAKE + 8, sin=FAKE, table_rows=128, k_new=None), Status.ERR_ARG, "16-byte aligned"),
    (lambda lib: _append(lib, strides=_append_strides(s2=-128), k_new=None), Status.ERR_ARG, ": strides must be"),               # 13. the first twelve strides
    (lambda lib: _append(lib, strides=_append_strides(s2=132), k_new=None), Status.ERR_ARG, ": strides must be"),                #     bf16 rows 264 bytes apart
    (lambda lib: _append(lib, strides=_append_strides(s5=4), k_new=None), Status.ERR_ARG, ": strides must be"),
    (lambda lib: _append(lib, strides=_append_strides(s6=-4096), k_new=None), Status.ERR_ARG, ": strides must be"),              #     a negative page stride
    (lambda lib: _append(lib, strides=_append_strides(s8=136), k_new=None), Status.ERR_ARG, ": strides must be"),                #     int8 rows 136 bytes apart
    (lambda lib: _append(lib, strides=_append_strides(s11=8), k_new=None), Status.ERR_ARG, ": strides must be"),
    (lambda lib: _append(lib, k_new=None, strides=_append_strides(s14=2)), Status.ERR_ARG, "NULL buffer"),                       # 14. NULL buffers; before 15
    (lambda lib: _append(lib, v_new=None), Status.ERR_ARG, "NULL buffer"),
    (lambda lib: _append(lib, k_pool=None), Status.ERR_ARG, "NULL buffer"),
    (lambda lib: _append(lib, v_pool=None), Status.ERR_ARG, "NULL buffer"),
    (lambda lib: _append(lib, params=None), Status.ERR_ARG, "NULL buffer"),
    (lambda lib: _append(lib, lens=None), Status.ERR_ARG, "NULL buffer"),
    (lambda lib: _append(lib, table=None), Status.ERR_ARG, "NULL buffer"),
    (lambda lib: _append(lib, strides=_append_strides(s14=2)), Status.ERR_ARG, "the strides of param_pool"),                     # 15. the three param strides
    (lambda lib: _append(lib, strides=_append_strides(s12=-128)), Status.ERR_ARG, "the strides of param_pool"),
    (lambda lib: _append(lib, strides=_append_strides(s13=66)), Status.ERR_ARG, "the strides of param_pool"),
]


def _decode_strides(H=8, HKV=2, L=1, P=16, E=128, **change):
    s = [H * L * E, L * E, E, HKV * P * E, P * E, E, HKV * P * E, P * E, E, 0, 0, 0, HKV * P * 4, P * 4, 4]
    for i, value in change.items():
        s[int(i[1:])] = value
    return tuple(s)


def _decode(lib, q=FAKE, q_dt=BF16, k=FAKE, v=FAKE, dt=BF16, q_s=None, q_o=None, params=FAKE, lens=FAKE, table=FAKE, B=2, H=8, HKV=2, L=1, num_pages=40, P=16,
            max_pages=19, table_stride=None, E=128, strides="dense", causal=0, sqrt_scale=0.3, out_s=None, out_o=None, bits=8.0, splits=0, plan_len=0,
            out=FAKE, ws=FAKE, ws_bytes=None):
    if strides == "dense":
        strides = _decode_strides(H, HKV, L, P, E)
    if ws_bytes is None:
        rows = L * (H // HKV if HKV > 0 else 1)
        count = splits or lib.ffq_sdpa_decode_splits(B, HKV, plan_len or max_pages * P, rows, E)
        ws_bytes = lib.ffq_sdpa_decode_workspace_bytes(B, HKV, rows, E, count)
    return lib.ffq_kv_paged_token_decode(q, q_dt, k, v, dt, q_s, q_o, params, lens, table, B, H, HKV, L, num_pages, P, max_pages,
                                         max_pages if table_stride is None else table_stride, E,
                                         None if strides is None else (ctypes.c_int64 * 15)(*strides), causal, sqrt_scale, out_s, out_o, bits, splits,
                                         plan_len, out, ws, ws_bytes, None)


DECODE_ERRORS = [
    (lambda lib: _decode(lib, dt=F32, q_dt=I8), Status.ERR_DTYPE, "bf16 or fp16 values"),                         # 1. the value dtype
    (lambda lib: _decode(lib, q_dt=F16, strides=None), Status.ERR_DTYPE, "q is held in the value dtype or in int8"),   # 2. q's container; before the table
    (lambda lib: _decode(lib, strides=None, E=96), Status.ERR_ARG, "NULL argument table"),                        # 3. the strides table; before E
    (lambda lib: _decode(lib, q_dt=I8, params=None), Status.ERR_DTYPE, "int8 q codes need their scale"),          # 4. int8 q without q_scale; before the pool
    (lambda lib: _decode(lib, params=None, E=96), Status.ERR_ARG, "need their scales"),                           # 5. no parameter pool; before E
    (lambda lib: _decode(lib, E=96, B=-1), Status.ERR_ARG, "E must be 64 or 128"),                                # 6. E
    (lambda lib: _decode(lib, B=-1, P=24), Status.ERR_ARG, "bad extent"),                                         # 7. the extents; before the geometry
    (lambda lib: _decode(lib, L=-1, P=24), Status.ERR_ARG, "bad extent"),
    (lambda lib: _decode(lib, H=7, HKV=2, P=24), Status.ERR_ARG, "bad extent"),
    (lambda lib: _decode(lib, HKV=0, P=24), Status.ERR_ARG, "bad extent"),
    (lambda lib: _decode(lib, P=24, L=40, ws_bytes=0), Status.ERR_ARG, "power of two in 16..256"),                # 8. the geometry; before the rows
    (lambda lib: _decode(lib, P=512, L=40, ws_bytes=0), Status.ERR_ARG, "power of two in 16..256"),
    (lambda lib: _decode(lib, num_pages=0, L=40, ws_bytes=0), Status.ERR_ARG, "num_pages must be"),
    (lambda lib: _decode(lib, num_pages=1 << 31, L=40, ws_bytes=0), Status.ERR_ARG, "num_pages must be"),
    (lambda lib: _decode(lib, max_pages=0, table_stride=0, L=40, ws_bytes=0), Status.ERR_ARG, "max_pages must be >= 1"),
    (lambda lib: _decode(lib, max_pages=1 << 26, L=40, ws_bytes=0), Status.ERR_ARG, "below 2^30"),
    (lambda lib: _decode(lib, table_stride=18, L=40, ws_bytes=0), Status.ERR_ARG, "row stride is below max_pages"),
    (lambda lib: _decode(lib, L=33, H=2, causal=2, ws_bytes=0), Status.ERR_ARG, "must be <= 32"),                 # 9. the rows; before causal
    (lambda lib: _decode(lib, L=9, causal=2, ws_bytes=0), Status.ERR_ARG, "must be <= 32"),
    (lambda lib: _decode(lib, causal=2, out_o=FAKE), Status.ERR_ARG, "causal is 0"),                              # 10. causal; before the quantizer
    (lambda lib: _decode(lib, causal=-1), Status.ERR_ARG, "causal is 0"),
    (lambda lib: _decode(lib, out_o=FAKE, splits=65), Status.ERR_ARG, "an output offset needs its scale"),        # 11. the output quantizer; before the splits
    (lambda lib: _decode(lib, out_s=FAKE, bits=9.0, splits=65), Status.ERR_ARG, "bit-width in 1..8"),
    (lambda lib: _decode(lib, out_s=FAKE, bits=3.5), Status.ERR_ARG, "bit-width in 1..8"),
    (lambda lib: _decode(lib, splits=65, plan_len=305, ws_bytes=0), Status.ERR_ARG, "splits must be"),            # 12. the splits; before plan_len
    (lambda lib: _decode(lib, splits=-1, ws_bytes=0), Status.ERR_ARG, "splits must be"),
    (lambda lib: _decode(lib, plan_len=305, ws_bytes=0, q=None), Status.ERR_ARG, "plan_len must be"),             # 13. plan_len (C = 19 * 16 = 304)
    (lambda lib: _decode(lib, plan_len=-1, ws_bytes=0), Status.ERR_ARG, "plan_len must be"),
    (lambda lib: _decode(lib, B=0, q=None, out=None, lens=None, table=None, ws=None), Status.OK, ""),             # 14. empty: nothing launched
    (lambda lib: _decode(lib, L=0, q=None, out=None, lens=None, table=None, ws=None, ws_bytes=0), Status.OK, ""),
    (lambda lib: _decode(lib, B=1 << 23, q=None, ws_bytes=0), Status.ERR_ARG, "too large"),                       # 15. batch * kv_heads >= 2^24
    (lambda lib: _decode(lib, q=None, ws=None, strides=_decode_strides(s14=2)), Status.ERR_ARG, "NULL buffer"),   # 16. NULL buffers; before the param strides
    (lambda lib: _decode(lib, k=None, ws=None), Status.ERR_ARG, "NULL buffer"),
    (lambda lib: _decode(lib, v=None, ws=None), Status.ERR_ARG, "NULL buffer"),
    (lambda lib: _decode(lib, out=None, ws=None), Status.ERR_ARG, "NULL buffer"),
    (lambda lib: _decode(lib, lens=None, ws=None), Status.ERR_ARG, "NULL buffer"),
    (lambda lib: _decode(lib, table=None, ws=None), Status.ERR_ARG, "NULL buffer"),
    (lambda lib: _decode(lib, strides=_decode_strides(s14=2), q=FAKE + 8), Status.ERR_ARG, "the strides of param_pool"),         # 17. the param strides
    (lambda lib: _decode(lib, strides=_decode_strides(s12=-128), ws=None), Status.ERR_ARG, "the strides of param_pool"),
    (lambda lib: _decode(lib, strides=_decode_strides(s13=66), ws=None), Status.ERR_ARG, "the strides of param_pool"),
    (lambda lib: _decode(lib, q=FAKE + 8, ws=None), Status.ERR_ARG, "16-byte aligned (lens, block_table: 4-byte)"),              # 18. alignment
    (lambda lib: _decode(lib, k=FAKE + 4, ws=None), Status.ERR_ARG, "16-byte aligned"),
    (lambda lib: _decode(lib, out=FAKE + 2, ws=None), Status.ERR_ARG, "16-byte aligned"),
    (lambda lib: _decode(lib, params=FAKE + 8, ws=None), Status.ERR_ARG, "16-byte aligned"),
    (lambda lib: _decode(lib, lens=FAKE + 2, ws=None), Status.ERR_ARG, "16-byte aligned"),
    (lambda lib: _decode(lib, table=FAKE + 2, ws=None), Status.ERR_ARG, "16-byte aligned"),
    (lambda lib: _decode(lib, strides=_decode_strides(s2=-128), ws=None), Status.ERR_ARG, ": strides must be"),   # 19. the q, k and v strides
    (lambda lib: _decode(lib, strides=_decode_strides(s2=132), ws=None), Status.ERR_ARG, ": strides must be"),
    (lambda lib: _decode(lib, strides=_decode_strides(s3=-4096), ws=None), Status.ERR_ARG, ": strides must be"),
    (lambda lib: _decode(lib, strides=_decode_strides(s5=136), ws=None), Status.ERR_ARG, ": strides must be"),
    (lambda lib: _decode(lib, strides=_decode_strides(s6=4100), ws=None), Status.ERR_ARG, ": strides must be"),
    (lambda lib: _decode(lib, ws=None), Status.ERR_WORKSPACE, "the workspace needs"),                             # 20. the workspace
    (lambda lib: _decode(lib, ws=FAKE + 8), Status.ERR_WORKSPACE, "the workspace needs"),
    (lambda lib: _decode(lib, ws_bytes=0), Status.ERR_WORKSPACE, "the workspace needs"),
    (lambda lib: _decode(lib, splits=3, ws_bytes=decode.sdpa_decode_workspace_bytes(2, 2, 4, 128, 3) - 1), Status.ERR_WORKSPACE, "the workspace needs"),
    # the plan is the dense entry's at C = 64 * 16 = 1024 keys: 2 splits for 128 groups
    (lambda lib: _decode(lib, B=16, H=8, HKV=8, max_pages=64, ws_bytes=decode.sdpa_decode_workspace_bytes(16, 8, 1, 128, 1)), Status.ERR_WORKSPACE,
     "the workspace needs"),
]


@pytest.mark.parametrize("index", range(len(APPEND_ERRORS)))
def test_append_argument_checks_need_no_device(index):
    call, status, words = APPEND_ERRORS[index]
    lib = FFQLibrary(HIP_SO)
    assert call(lib) == status
    if status != Status.OK:
        message = lib.ffq_last_error().decode()
        assert message.startswith("kv_paged_token_append: ") and words in message, message


@pytest.mark.parametrize("index", range(len(DECODE_ERRORS)))
def test_decode_argument_checks_need_no_device(index):
    call, status, words = DECODE_ERRORS[index]
    lib = FFQLibrary(HIP_SO)
    assert call(lib) == status
    if status != Status.OK:
        message = lib.ffq_last_error().decode()
        assert message.startswith("kv_paged_token_decode: ") and words in message, message


def test_the_plan_hint_sizes_the_workspace():
    """``splits = 0``: the count is ``ffq_sdpa_decode_splits`` at `plan_len` keys (the capacity when 0), as in ``ffq_kv_paged_decode``."""
    lib = FFQLibrary(HIP_SO)
    one, two = (decode.sdpa_decode_workspace_bytes(16, 8, 1, 128, n) for n in (1, 2))
    kw = dict(B=16, H=8, HKV=8, max_pages=8, P=128, num_pages=200)
    for plan_len, need in ((0, two), (1024, two), (385, two), (384, one), (200, one), (1, one)):
        assert _decode(lib, plan_len=plan_len, ws_bytes=need - 1, **kw) == Status.ERR_WORKSPACE
        assert f"needs {need} bytes".encode() in lib.ffq_last_error(), plan_len
    assert _decode(lib, splits=5, plan_len=1, ws_bytes=0, **kw) == Status.ERR_WORKSPACE     # a forced count overrides the hint
    assert f"needs {decode.sdpa_decode_workspace_bytes(16, 8, 1, 128, 5)} bytes".encode() in lib.ffq_last_error()


# ---- the wrappers -----------------------------------------------------------------------------------------------------------------------
def _operands(dtype=torch.bfloat16, Bc=2, H=2, L=3, P=16, pages=6, max_pages=2, E=64, G=2):
    k_new, v_new = torch.zeros(Bc, H, L, E, dtype=dtype), torch.zeros(Bc, H, L, E, dtype=dtype)
    kp, vp = torch.zeros(pages, H, P, E, dtype=torch.int8), torch.zeros(pages, H, P, E, dtype=torch.int8)
    table = torch.zeros(Bc, max_pages, dtype=torch.int32)
    return k_new, v_new, kp, vp, torch.zeros(pages, H, P, 4), torch.zeros(Bc, dtype=torch.int32), table, torch.zeros(Bc, H * G, L, E, dtype=dtype)


def test_the_wrappers_say_not_covered_on_a_library_without_the_symbols(oracle_backend):
    k_new, v_new, kp, vp, pp, lens, table, q = _operands()
    with pytest.raises(BackendError, match="does not export ffq_kv_paged_token_append"):
        ops.kv_paged_token_append(k_new, v_new, kp, vp, pp, lens, table, (8, False), (4, True))
    with pytest.raises(BackendError, match="does not export ffq_kv_paged_token_decode"):
        ops.kv_paged_token_decode(q, kp, vp, pp, lens, table)


def test_the_wrappers_check_their_operands_and_refuse_host_tensors():
    bf = torch.bfloat16
    k_new, v_new, kp, vp, pp, lens, table, q = _operands()
    with pytest.raises(BackendError, match="HIP device only"):
        ops.kv_paged_token_append(k_new, v_new, kp, vp, pp, lens, table, (8, False), (4, True))
    with pytest.raises(BackendError, match="HIP device only"):
        ops.kv_paged_token_decode(q, kp, vp, pp, lens, table)
    with pytest.raises(BackendError, match="HIP device only"):  # both layouts of the three pools and a table that is a window of a wider one pass the checks
        ops.kv_paged_token_decode(q, kp.transpose(1, 2).contiguous().transpose(1, 2), vp, pp.transpose(1, 2).contiguous().transpose(1, 2), lens,
                                  torch.zeros(2, 5, dtype=torch.int32)[:, 1:3], q_dequant=None, plan_len=32, splits=3)
    rope = torch.zeros(32, 64, dtype=bf)

    def append(**change):
        a = dict(k_new=k_new, v_new=v_new, k_pool=kp, v_pool=vp, param_pool=pp, lens=lens, block_table=table, k_spec=(8, False), v_spec=(4, True))
        return lambda: ops.kv_paged_token_append(**{**a, **change})

    def attend(**change):
        a = dict(query=q, k_pool=kp, v_pool=vp, param_pool=pp, lens=lens, block_table=table)
        return lambda: ops.kv_paged_token_decode(**{**a, **change})

    small = torch.zeros(6, 2, 8, 64, dtype=torch.int8)
    odd = torch.zeros(6, 2, 24, 64, dtype=torch.int8)
    refused = [append(k_new=k_new[0]), append(k_new=k_new.float(), v_new=v_new.float()), append(v_new=v_new.half()), append(k_pool=kp.to(bf)),
               append(v_new=v_new[:, :1]), append(v_pool=vp[:, :, :8]), append(k_pool=kp[:, :1]), append(k_pool=kp[0]),
               append(k_new=k_new[..., :32], v_new=v_new[..., :32], k_pool=kp[..., :32], v_pool=vp[..., :32]),
               append(k_pool=odd, v_pool=odd, param_pool=torch.zeros(6, 2, 24, 4)), append(k_pool=small, v_pool=small, param_pool=torch.zeros(6, 2, 8, 4)),
               append(param_pool=pp.double()), append(param_pool=pp[:5]), append(param_pool=pp[:, :, :8]), append(param_pool=pp[..., :3]), append(param_pool=pp[0]),
               append(param_pool=torch.zeros(6, 2, 16, 8)[..., ::2]), append(param_pool=torch.zeros(6, 2, 16, 6)[..., 1:5]),
               append(lens=lens.long()), append(lens=lens[:1]), append(lens=torch.zeros(4, dtype=torch.int32)[::2]),
               append(block_table=table.long()), append(block_table=table[:1]), append(block_table=table[0]),
               append(block_table=torch.zeros(2, 4, dtype=torch.int32)[:, ::2]), append(block_table=torch.zeros(2, 0, dtype=torch.int32)),
               append(block_table=torch.zeros(1, 2, dtype=torch.int32).expand(2, 2)),
               append(k_new=k_new.transpose(2, 3).contiguous().transpose(2, 3)),
               append(k_spec=(9, False)), append(v_spec=(1, True)), append(k_spec=(3.5, False)),
               append(rope=(rope[:31], rope[:31])), append(rope=(rope, rope.half())), append(rope=(rope, torch.zeros(33, 64, dtype=bf))),
               attend(k_pool=kp.to(bf)), attend(query=q[0]), attend(query=q.float()), attend(query=q.to(torch.int8), dtype=bf),
               attend(query=torch.zeros(2, 2, 33, 64, dtype=bf)), attend(query=torch.zeros(2, 3, 1, 64, dtype=bf)), attend(v_pool=vp[:, :, :8]), attend(v_pool=vp[:5]),
               attend(param_pool=pp.double()), attend(param_pool=pp[:5]), attend(param_pool=torch.zeros(6, 2, 16, 8)[..., ::2]),
               attend(splits=65), attend(splits=-1), attend(plan_len=0), attend(plan_len=33), attend(lens=lens.long()), attend(lens=lens[:1]),
               attend(block_table=table.long()), attend(block_table=table[:1]), attend(block_table=torch.zeros(2, 4, dtype=torch.int32)[:, ::2])]
    for i, call in enumerate(refused):
        with pytest.raises(RuntimeError) as caught:
            call()
        assert not isinstance(caught.value, BackendError), f"call {i} reached the library"


# ---- the class ------------------------------------------------------------------------------------------------------------------------------
NAME = "PagedDynamicQuantizedKVCache"


def make(dtype=torch.bfloat16, layout="phse", **change):
    kw = dict(num_pages=10, page_size=16, kv_heads=2, head_dim=64, key_quantizer=cases.quantizer(8), value_quantizer=cases.quantizer(4, symmetric=True, tile=True),
              batch=3, max_pages_per_seq=4, dtype=dtype, device="cpu", layout=layout)
    return ff.nn.PagedDynamicQuantizedKVCache(**{**kw, **change})


def test_the_constructor_append_and_attend_take_and_refuse():
    D = ff.nn.DynamicLinearQuantizer
    cache = make()
    assert cache.k_pool.shape == cache.v_pool.shape == (10, 2, 16, 64) and cache.k_pool.dtype == torch.int8 and cache.k_pool.is_contiguous()
    assert cache.param_pool.shape == (10, 2, 16, 4) and cache.param_pool.dtype == torch.float32 and cache.param_pool.is_contiguous()
    assert cache.block_table.dtype == torch.int32 and cache.block_table.tolist() == [[-1] * 4] * 3
    assert cache.lengths.dtype == torch.int32 and cache.lengths.tolist() == [0, 0, 0] and cache.capacity == 64 and cache.free_pages == 10
    other = make(torch.float16, "pshe")
    assert other.k_pool.shape == (10, 2, 16, 64) and other.k_pool.transpose(1, 2).is_contiguous() and other.k_pool.stride(2) == 2 * 64
    assert other.param_pool.shape == (10, 2, 16, 4) and other.param_pool.transpose(1, 2).is_contiguous() and other.param_pool.stride(2) == 2 * 4
    # every accept of _dynamic_spec: 2..8 bits, both granularities, asymmetric (whatever allow_one_sided says), symmetric without the one-sided rule
    for bits in range(2, 9):
        make(key_quantizer=cases.quantizer(bits), value_quantizer=cases.quantizer(bits, symmetric=True, tile=True))
    make(key_quantizer=D(8, granularity=ff.PerChannel((0, 1, 2)), quantized_dtype=torch.int8, symmetric=False, allow_one_sided=True))
    make(head_dim=128, key_quantizer=cases.quantizer(8, E=128, tile=True), value_quantizer=cases.quantizer(4, E=128))
    for page_size in cases.PAGE_SIZES + (64,):
        make(page_size=page_size)
    int8 = dict(quantized_dtype=torch.int8)
    rows = ff.PerChannel((0, 1, 2))
    bad = [D(8, granularity=rows), D(8, granularity=rows, quantized_dtype=torch.bfloat16), D(16, granularity=rows, **int8), D(1, granularity=rows, **int8),
           D(3.5, granularity=rows, **int8), D(8, granularity=rows, parameter_inference_fn=lambda p, x: (torch.ones(1), None), **int8),
           D(8, **int8), D(8, granularity=ff.PerChannel(1), **int8), D(8, granularity=ff.PerChannel((0, 1)), **int8),
           D(8, granularity=ff.PerTile((1, 1, 1, 32)), **int8), D(8, granularity=ff.PerTile((1, 1, 2, 64)), **int8),
           D(8, granularity=rows, symmetric=True, **int8), D(8, granularity=rows, symmetric=True, allow_one_sided=True, **int8),
           dense_cases.quantizer((8, 0.5, 0.0)), ff.nn.QuantizerStub(), None]
    for q in bad:
        for slot, what in (("key_quantizer", "key"), ("value_quantizer", "value")):
            with pytest.raises(ValueError, match=f"^{NAME}: the {what} quantizer must be a DynamicLinearQuantizer"):
                make(**{slot: q})
    for change in (dict(layout="bhse"), dict(layout="bshe"), dict(dtype=torch.float32), dict(head_dim=96), dict(batch=0), dict(num_pages=0), dict(kv_heads=0),
                   dict(max_pages_per_seq=0), dict(page_size=8), dict(page_size=24), dict(page_size=512), dict(page_size=256, max_pages_per_seq=1 << 22),
                   dict(head_dim=128)):  # (the last: a PerTile of 64 columns is not one tile per row of 128)
        with pytest.raises(ValueError, match=f"^{NAME}: "):
            make(**change)
    k = torch.zeros(3, 2, 3, 64, dtype=torch.bfloat16)
    for key, value in ((k.half(), k.half()), (k[:1], k[:1]), (k, k[:, :, :2]), (k[..., :32], k[..., :32]), (k[0], k[0])):
        with pytest.raises(ValueError, match=f"^{NAME}.append: "):
            cache.append(key, value)
    q = torch.zeros(3, 4, 1, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match=f"^{NAME}.attend: "):
        cache.attend(q.half())
    with pytest.raises(ValueError, match=f"^{NAME}.attend: the output quantizer"):
        cache.attend(q, output_quantizer=dense_cases.quantizer((16, 0.5, 0.0), container=None))
    assert cache.lengths.tolist() == [0, 0, 0]  # (a refused call moved nothing)
    for seq in range(3):
        cache.reserve(seq, 3)
    cache.append(k, k)                         # ... and a sound one runs (the composed route, on host tensors)
    assert cache.lengths.tolist() == [3, 3, 3] and cache.attend(q).shape == q.shape


def test_the_classes_it_combines_still_take_and_refuse_what_they_did():
    static, dynamic = dense_cases.quantizer((8, 0.5, 0.0)), cases.quantizer(8)
    paged = lambda kq, vq: ff.nn.PagedQuantizedKVCache(10, 16, 2, 64, kq, vq, 3, 4, device="cpu")  # noqa: E731
    paged(static, static)
    with pytest.raises(ValueError, match="^QuantizedKVCache: the key quantizer must be a LinearQuantizer, got DynamicLinearQuantizer$"):
        paged(dynamic, static)
    with pytest.raises(ValueError, match="^QuantizedKVCache: the value quantizer must be a LinearQuantizer, got DynamicLinearQuantizer$"):
        paged(static, dynamic)
    with pytest.raises(ValueError, match=r"^PagedQuantizedKVCache: page_size is a power of two in 16\.\.256, got 24$"):
        ff.nn.PagedQuantizedKVCache(10, 24, 2, 64, static, static, 3, 4, device="cpu")
    with pytest.raises(ValueError, match=r"^PagedQuantizedKVCache: layout is one of \('phse', 'pshe'\), got 'bhse'$"):
        ff.nn.PagedQuantizedKVCache(10, 16, 2, 64, static, static, 3, 4, device="cpu", layout="bhse")
    cache = paged(static, static)
    assert not hasattr(cache, "param_pool") and len(cache.dense()) == 2
    with pytest.raises(ValueError, match=r"^PagedQuantizedKVCache\.reserve: a sequence holds 0\.\.64 positions, got 65$"):
        cache.reserve(0, 65)
    cache.reserve(0, 64)
    cache.reserve(1, 64)
    with pytest.raises(RuntimeError, match=r"^PagedQuantizedKVCache\.reserve: the pool is exhausted \(4 pages wanted, 2 free\)$"):
        cache.reserve(2, 64)
    with pytest.raises(ValueError, match=r"^PagedQuantizedKVCache\.share_prefix: the receiving sequence is another one and holds no page yet \(release it first\)$"):
        cache.share_prefix(0, 1, 16)
    with pytest.raises(ValueError, match=r"^PagedQuantizedKVCache\.share_prefix: sequence 0 holds 4 pages, 5 wanted$"):
        cache.share_prefix(0, 2, 80)
    ff.nn.DynamicQuantizedKVCache(2, 2, 16, 64, dynamic, cases.quantizer(4, symmetric=True, tile=True), device="cpu")
    with pytest.raises(ValueError, match="^DynamicQuantizedKVCache: the key quantizer must be a DynamicLinearQuantizer, got LinearQuantizer$"):
        ff.nn.DynamicQuantizedKVCache(2, 2, 16, 64, static, dynamic, device="cpu")
    with pytest.raises(ValueError, match="^DynamicQuantizedKVCache: the value quantizer must be a DynamicLinearQuantizer with quantized_dtype=torch.int8"):
        ff.nn.DynamicQuantizedKVCache(2, 2, 16, 64, dynamic, ff.nn.DynamicLinearQuantizer(8, granularity=ff.PerChannel(1), quantized_dtype=torch.int8), device="cpu")


def test_reserve_release_and_share_prefix():
    cache = make()
    cache.reserve(0, 17)                      # two pages
    cache.reserve(0, 30)                      # still two
    assert cache.pages(0) == (0, 1) and cache.block_table[0].tolist() == [0, 1, -1, -1] and cache.free_pages == 8
    cache.reserve(1, 64)
    assert cache.pages(1) == (2, 3, 4, 5) and cache.free_pages == 4
    for bad in (65, -1):
        with pytest.raises(ValueError, match=rf"^{NAME}\.reserve: a sequence holds 0\.\.64 positions, got {bad}$"):
            cache.reserve(2, bad)
    cache.reserve(2, 48)
    with pytest.raises(RuntimeError, match=rf"^{NAME}\.reserve: the pool is exhausted \(2 pages wanted, 1 free\)$"):   # nothing is taken
        cache.reserve(0, 64)
    assert cache.pages(0) == (0, 1) and cache.free_pages == 1 and cache.block_table[0].tolist() == [0, 1, -1, -1] and cache._refs == [1] * 9 + [0]
    cache.lengths.copy_(torch.tensor([30, 64, 48], dtype=torch.int32))
    cache.release(2)
    assert cache.pages(2) == () and cache.block_table[2].tolist() == [-1] * 4 and cache.lengths.tolist() == [30, 64, 0] and cache.free_pages == 4
    cache.share_prefix(1, 2, 40)              # 40 // 16 = 2 whole pages
    assert cache.pages(2) == (2, 3) and cache.block_table[2].tolist() == [2, 3, -1, -1] and cache.lengths.tolist() == [30, 64, 32] and cache.free_pages == 4
    assert cache._refs[2] == cache._refs[3] == 2
    for call in (lambda: cache.share_prefix(1, 2, 16), lambda: cache.share_prefix(1, 1, 16), lambda: cache.share_prefix(0, 2, 16)):
        with pytest.raises(ValueError, match=rf"^{NAME}\.share_prefix: the receiving sequence"):       # the receiver holds pages already / is the giver
            call()
    cache.release(1)                          # pages 2 and 3 stay with sequence 2; 4 and 5 are free again
    assert cache.free_pages == 6 and cache.pages(2) == (2, 3)
    cache.release(2)
    assert cache.free_pages == 8
    cache.release(2)                          # (releasing an empty sequence is nothing)
    with pytest.raises(ValueError, match=rf"^{NAME}\.share_prefix: sequence 0 holds 2 pages, 3 wanted$"):
        cache.share_prefix(0, 2, 48)
    cache.reserve(2, 64)                      # every freed page is reusable
    assert sorted(cache.pages(2)) == [2, 3, 4, 5] and cache.free_pages == 4


def test_the_free_list_and_the_reference_counts_over_200_operations():
    """The invariants tests/test_kv_paged_cpu.py states, after every one of 200 seeded operations: a page is held by several sequences
    only through ``share_prefix``; the counts sum to the number of table entries; free and held pages partition the pool; the device
    table is the host's copy; every freed page comes back."""
    rng = random.Random(5)
    batch, num_pages, P, per = 5, 23, 16, 6
    cache = make(num_pages=num_pages, batch=batch, max_pages_per_seq=per)
    shared: set[tuple[int, int]] = set()      # (sequence, page) pairs that came from share_prefix
    seen_free: set[int] = set()
    for step in range(200):
        op, seq = rng.choice(("reserve", "reserve", "release", "share")), rng.randrange(batch)
        if op == "reserve":
            want = rng.randrange(0, per * P + 1)
            need = -(-want // P) - len(cache.pages(seq))
            if need > cache.free_pages:
                before = (cache.pages(seq), cache.free_pages, list(cache._refs))
                with pytest.raises(RuntimeError, match="exhausted"):
                    cache.reserve(seq, want)
                assert (cache.pages(seq), cache.free_pages, cache._refs) == before   # exhaustion takes nothing
            else:
                cache.reserve(seq, want)
                assert len(cache.pages(seq)) * P >= want
        elif op == "release":
            cache.release(seq)
            shared = {(s, p) for s, p in shared if s != seq}
            assert cache.pages(seq) == () and cache.lengths[seq].item() == 0
        else:
            src = rng.randrange(batch)
            n = rng.randrange(0, per * P + 1)
            if src == seq or cache.pages(seq) or n // P > len(cache.pages(src)):
                with pytest.raises(ValueError):
                    cache.share_prefix(src, seq, n)
            else:
                cache.share_prefix(src, seq, n)
                assert cache.pages(seq) == cache.pages(src)[:n // P] and cache.lengths[seq].item() == (n // P) * P
                shared |= {(seq, p) for p in cache.pages(seq)}
        held = [p for b in range(batch) for p in cache.pages(b)]
        owners = {p: [b for b in range(batch) if p in cache.pages(b)] for p in set(held)}
        for p, who in owners.items():         # one owner that reserved it at most; everyone else got it by sharing
            assert sum((b, p) not in shared for b in who) <= 1, (step, p, who)
            assert cache._refs[p] == len(who)
        assert all(len(set(cache.pages(b))) == len(cache.pages(b)) for b in range(batch))
        assert sum(cache._refs) == len(held) == int((cache.block_table >= 0).sum())
        assert sorted(set(held) | set(cache._free)) == list(range(num_pages)) and not set(held) & set(cache._free) and len(set(cache._free)) == cache.free_pages
        assert cache.block_table.tolist() == [list(cache.pages(b)) + [-1] * (per - len(cache.pages(b))) for b in range(batch)]
        seen_free |= set(cache._free)
    for b in range(batch):
        cache.release(b)
    assert cache.free_pages == num_pages and cache._refs == [0] * num_pages and seen_free == set(range(num_pages))
    for b in range(3):                        # ... and the whole pool can be taken again
        cache.reserve(b, per * P)
    assert cache.free_pages == num_pages - 3 * per


def bits_of(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("layout", cases.LAYOUTS)
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_the_composed_route_gives_the_dense_dynamic_caches_bits(layout, dtype):
    """On host tensors the class runs the composed route. After every append ``dense()`` equals a ``DynamicQuantizedKVCache`` fed the
    same rows (a prompt that crosses pages, single steps, rows past the capacity, with and without rotation; a constant and an all-zero
    row): codes byte for byte, parameters as bit patterns. ``attend`` equals that class's composed ``attend`` bit for bit; a sequence
    that shares another's prefix page gives the bits of one that appended the rows itself, and the giver's codes and parameters stay."""
    Bc, H, HKV, P, per, E = 4, 4, 2, 16, 3, 64
    Cc = per * P
    gen = torch.Generator().manual_seed(13 + cases.DTYPES.index(dtype))
    kq, vq = cases.quantizer(8), cases.quantizer(4, symmetric=True, tile=True)
    paged = ff.nn.PagedDynamicQuantizedKVCache(Bc * per + 3, P, HKV, E, kq, vq, Bc, per, dtype, "cpu", layout=layout)
    dense = ff.nn.DynamicQuantizedKVCache(Bc, HKV, Cc, E, kq, vq, dtype, "cpu")
    for b in (2, 0, 3, 1):                    # (interleaved, so that no sequence's pages are in order with its neighbour's)
        paged.reserve(b, 20)
    for b in (1, 3, 0, 2):
        paged.reserve(b, Cc)
    assert paged.pages(0) == (2, 3, 10) and paged.free_pages == 3
    cos, sin = (torch.randn(Cc + 3, E, generator=gen).to(dtype) for _ in range(2))
    start = [0, 3, 30, 45]
    paged.lengths.copy_(torch.tensor(start, dtype=torch.int32))
    dense.reset(start)

    def same(seq=None):
        got = paged.dense(seq)
        want = (dense.k_cache, dense.v_cache, dense.params) if seq is None else (dense.k_cache[seq], dense.v_cache[seq], dense.params[seq])
        return torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(bits_of(got[2]), bits_of(want[2]))

    for L, rope in ((5, True), (1, True), (17, False), (1, False)):   # the last sequence runs past its capacity: rows dropped
        k_new = (torch.randn(Bc, HKV, L, E, generator=gen) * 3 + 9.4).to(dtype)
        v_new = (torch.randn(Bc, HKV, L, E, generator=gen) * 2 - 50).to(dtype)
        v_new[1, 0, 0] = 0.0                  # an all-zero row and a constant one: the eps clamp
        k_new[1, 1, 0] = 2.5
        paged.append(k_new, v_new, rope=(cos, sin) if rope else None)
        dense.append(k_new, v_new, rope=(cos, sin) if rope else None)
        assert paged.lengths.tolist() == dense.lengths.tolist()
        assert paged.dense()[0].shape == (Bc, HKV, Cc, E) and paged.dense()[2].shape == (Bc, HKV, Cc, 4) and same() and same(1)
    assert paged.lengths.tolist() == [24, 27, 54, 69] and bool(dense.k_cache[3, :, Cc - 1].any()) and bool(dense.params[3, :, Cc - 1, 0].all())
    for unowned in set(range(Bc * per + 3)) - {p for b in range(Bc) for p in paged.pages(b)}:
        assert not bool(paged.k_pool[unowned].any()) and not bool(paged.v_pool[unowned].any()) and not bool(paged.param_pool[unowned].any())
    for L, causal in ((1, True), (3, True), (3, False)):
        q = torch.randn(Bc, H, L, E, generator=gen).to(dtype)
        got, want = paged.attend(q, is_causal=causal), dense.attend(q, is_causal=causal)
        assert got.dtype == dtype and torch.equal(got.view(torch.int16), want.view(torch.int16)) and bool(got.any())
    # ---- sharing: sequence 3 gives way to a copy of sequence 1's first 16 positions and appends the rest itself
    paged.release(3)
    paged.share_prefix(1, 3, 27)              # one whole page of 16; the 11 rows after it are not shared
    assert paged.pages(3) == paged.pages(1)[:1] and paged.lengths.tolist() == [24, 27, 54, 16]
    paged.reserve(3, Cc)
    assert paged.pages(3)[0] == paged.pages(1)[0] and not set(paged.pages(3)[1:]) & set(paged.pages(1))
    tail_k, tail_v = (torch.randn(Bc, HKV, 11, E, generator=gen).to(dtype) for _ in range(2))
    before = paged.dense(1)
    mask = torch.tensor([0, 0, 0, 1], dtype=torch.int32)
    # rows for sequence 3 only: the others' lengths are parked so that their rows fall before position 0 and are dropped
    parked = paged.lengths.clone()
    paged.lengths.copy_(torch.where(mask.bool(), parked, torch.full_like(parked, -11)))
    paged.append(tail_k, tail_v)
    paged.lengths.copy_(torch.where(mask.bool(), paged.lengths, parked))
    own = ff.nn.DynamicQuantizedKVCache(1, HKV, Cc, E, kq, vq, dtype, "cpu")   # a sequence that appended all 27 rows itself
    own.k_cache[0, :, :16], own.v_cache[0, :, :16], own.params[0, :, :16] = before[0][:, :16], before[1][:, :16], before[2][:, :16]
    own.reset([16])
    own.append(tail_k[3:], tail_v[3:])
    got = paged.dense(3)
    assert paged.lengths.tolist() == [24, 27, 54, 27]
    assert torch.equal(got[0][:, :27], own.k_cache[0, :, :27]) and torch.equal(got[1][:, :27], own.v_cache[0, :, :27])
    assert torch.equal(bits_of(got[2][:, :27]), bits_of(own.params[0, :, :27]))
    after = paged.dense(1)                    # the giver's codes and parameters did not move
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1]) and torch.equal(bits_of(after[2]), bits_of(before[2]))
    q = torch.randn(Bc, H, 2, E, generator=gen).to(dtype)
    assert torch.equal(paged.attend(q)[3:].view(torch.int16), own.attend(q[3:]).view(torch.int16))
    # the composed route refuses what the kernel masks: a length that reaches a page never reserved
    paged.release(0)
    paged.lengths[0] = 5
    with pytest.raises(ValueError, match="never reserved"):
        paged.attend(q)


def test_the_scatter_and_the_gather_of_a_parameter_store_are_inverse():
    """tests/kv_paged_token_cases.py: a store scattered through the permuted table and gathered again is itself, bit for bit (NaN
    included); unowned pages keep their fill; an entry outside the pool is skipped and gathers as the fill."""
    for P in cases.PAGE_SIZES:
        rows, num_pages = cases.page_table(P)
        store = torch.randn(cases.B, cases.HKV, cases.C, 4, generator=torch.Generator().manual_seed(P))
        store[1, 0, 3, 2] = float("nan")
        for layout in cases.LAYOUTS:
            pool = cases.scatter_params(store, rows, cases.param_pool_of(num_pages, P, layout, "cpu", cases.PARAM_SENTINEL))
            assert pool.shape == (num_pages, cases.HKV, P, 4) and torch.equal(bits_of(cases.gather_dense(pool, rows)), bits_of(store))
            owned = {page for row in rows for page in row}
            assert len(owned) == num_pages - cases.UNOWNED
            assert all(bool((pool[page] == cases.PARAM_SENTINEL).all()) for page in set(range(num_pages)) - owned)
            holes = tuple((-1,) + row[1:-1] + (num_pages,) for row in rows)
            again = cases.gather_dense(pool, holes, fill=cases.PARAM_SENTINEL)
            assert bool((again[:, :, :P] == cases.PARAM_SENTINEL).all()) and bool((again[:, :, -P:] == cases.PARAM_SENTINEL).all())
            assert torch.equal(bits_of(again[:, :, P:-P]), bits_of(store[:, :, P:-P]))
    uniform = cases.uniform_store((0.031, 3.4), (0.027, -9.0))
    assert uniform.shape == (cases.B, cases.HKV, cases.C, 4) and uniform[2, 1, 300].tolist() == torch.tensor([0.031, 3.0, 0.027, -9.0]).tolist()


# ---- what hipcc emitted -----------------------------------------------------------------------------------------------------------------
def test_the_paged_token_kernels_spill_nothing_and_keep_the_dense_kernels_lds():
    if kernel_resources.readelf() is None:
        pytest.skip("llvm-readelf is missing")
    assert kernel_resources.DEFAULT_LIBRARY.exists(), "build() leaves the HIP library in the tree"
    rows = kernel_resources.kernel_resources()
    partial = [k for k in rows if "kv_paged_token_partial_kernel" in str(k["name"])]
    store = [k for k in rows if "kv_paged_token_store_kernel" in str(k["name"])]
    assert len(partial) == 4 and len(store) == 4, (len(partial), len(store))  # E 64 / 128 x bf16 / fp16; bf16 / fp16 x plain / rotary
    bad = {str(k["name"]): k for k in partial + store if k["vgpr_spill_count"] or k["sgpr_spill_count"] or k["private_segment_fixed_size"]}
    assert not bad, bad
    want = {"Li64E": 25600, "Li128E": 50176}  # the dense partial kernels' LDS (docs/kernels.md)
    for k in partial:
        assert k["group_segment_fixed_size"] == want[next(tag for tag in want if tag in str(k["name"]))], k
    assert all(k["group_segment_fixed_size"] == 0 for k in store)
    # every count the existing tests pin: the names the other kernels are counted by still count those kernels alone
    for name, count in (("sdpa_decode_partial_kernel", 4), ("sdpa_decode_combine_kernel", 2), ("kv_append", 4), ("kv_paged_partial_kernel", 4),
                        ("kv_paged_store_kernel", 4), ("kv_token_partial_kernel", 4), ("kv_token_store_kernel", 4)):
        assert len([k for k in rows if name in str(k["name"])]) == count, name
