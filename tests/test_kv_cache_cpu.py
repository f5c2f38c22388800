"""The preallocated int8 KV cache without a GPU: the seventh header ``include/ffq_kv_cache.h`` against ``_cabi.SIGNATURES_KV``
(exported by the HIP library, absent from the oracle, the other tables untouched), every argument error of ``ffq_kv_append`` and
``ffq_kv_decode`` in the documented order before any device call, the wrappers' operand checks, what the cache's constructor
refuses, the composed route (``nn.kv_cache.composed_append`` / ``composed_attend``) against a float64 restatement, and what hipcc
emitted for the append kernels."""

import ctypes
import re
import sys

import pytest
import torch

import fastforward_amd as ff

import kv_cache_cases as cases

from conftest import HIP_SO, ROOT, load_oracle
from fastforward_amd import _cabi, ops
from fastforward_amd._cabi import DType, FFQLibrary, Status
from fastforward_amd.exceptions import BackendError
from fastforward_amd.nn import kv_cache
from fastforward_amd.ops import decode

sys.path.insert(0, str(ROOT / "tools"))

import kernel_resources  # noqa: E402

ENTRIES = {"ffq_kv_append", "ffq_kv_decode"}


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
def test_the_functions_and_the_class_exist():
    assert {"kv_append", "kv_decode"} <= set(ops.__all__) and callable(ops.kv_append) and callable(ops.kv_decode)
    assert ff.nn.QuantizedKVCache is kv_cache.QuantizedKVCache and callable(kv_cache.composed_append) and callable(kv_cache.composed_attend)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
def _header(name):
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / name).read_text(), flags=re.S)


def _declared(name):
    return set(re.findall(r"\b(ffq_[a-z0-9_]+)\s*\(", _header(name)))


def test_the_seventh_header_and_its_table_agree():
    assert _declared("ffq_kv_cache.h") == set(_cabi.SIGNATURES_KV) == ENTRIES
    assert '#include "ffq_sdpa_decode.h"' in (ROOT / "include" / "ffq_kv_cache.h").read_text()
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
    want_names = {
        "ffq_kv_append": ["k_new", "v_new", "dt", "k_cache", "v_cache", "lens", "batch", "kv_heads", "L", "S_max", "E", "strides", "k_scale", "k_offset",
                          "k_num_bits", "v_scale", "v_offset", "v_num_bits", "cos_table", "sin_table", "table_rows", "stream"],
        "ffq_kv_decode": ["q", "q_dt", "k", "v", "dt", "deq_scale", "deq_offset", "lens", "batch", "q_heads", "kv_heads", "L", "S_max", "E", "strides", "causal",
                          "sqrt_scale", "out_scale", "out_offset", "out_num_bits", "splits", "plan_len", "out", "workspace", "workspace_bytes", "stream"],
    }
    for entry in ENTRIES:
        m = re.search(r"(\w+)\s+" + entry + r"\s*\((.*?)\)\s*;", _header("ffq_kv_cache.h"), flags=re.S)
        names, want = [], []
        for p in m.group(2).split(","):
            words = p.replace("*", " * ").split()
            names.append(words[-1])
            if words.count("*") == 2:    # const float* const*: an array of pointers
                want.append(ctypes.POINTER(ctypes.c_void_p))
            elif "*" in words:
                want.append(ctypes.POINTER(ctypes.c_int64) if words[words.index("*") - 1] == "int64_t" else ctypes.c_void_p)
            else:
                want.append(kinds[words[-2]])
        restype, argtypes = _cabi.SIGNATURES_KV[entry]
        assert m.group(1) == "int" and restype is ctypes.c_int and argtypes == want and names == want_names[entry], entry


def test_the_other_tables_are_untouched_and_disjoint():
    assert _declared("ffq.h") == set(_cabi.SIGNATURES) and _declared("ffq_sdpa_decode.h") == set(_cabi.SIGNATURES_DECODE)
    assert set(_cabi.SIGNATURES_DECODE) == {"ffq_sdpa_decode", "ffq_sdpa_decode_splits", "ffq_sdpa_decode_workspace_bytes"}
    for other in (_cabi.SIGNATURES, _cabi.SIGNATURES_3D, _cabi.SIGNATURES_DEPTHWISE, _cabi.SIGNATURES_INDEX, _cabi.SIGNATURES_UNFOLD, _cabi.SIGNATURES_DECODE,
                  _cabi.DEVICE_ONLY):
        assert not ENTRIES & set(other)
    assert _cabi.FFQ_ABI_VERSION == 9 and "#define FFQ_ABI_VERSION 9" in (ROOT / "include" / "ffq.h").read_text()


def test_the_hip_library_exports_them_and_the_oracle_loads_without_them():
    dll, lib, oracle = ctypes.CDLL(str(HIP_SO)), FFQLibrary(HIP_SO), load_oracle()
    for entry in ENTRIES:
        assert hasattr(dll, entry) and getattr(lib, entry) is not None
        assert not oracle.is_device and getattr(oracle, entry) is None


FAKE = 1 << 20  # never dereferenced: every call below returns from the argument checks
BF16, F16, I8, F32 = (int(t) for t in (DType.BF16, DType.F16, DType.I8, DType.F32))


def _append(lib, k_new=FAKE, v_new=FAKE, dt=BF16, k_cache=FAKE, v_cache=FAKE, lens=FAKE, B=2, HKV=2, L=1, S_max=300, E=128, strides="dense", ks=FAKE, ko=None,
            kbits=8.0, vs=FAKE, vo=None, vbits=8.0, cos=None, sin=None, table_rows=0):
    if strides == "dense":
        strides = _append_strides()
    return lib.ffq_kv_append(k_new, v_new, dt, k_cache, v_cache, lens, B, HKV, L, S_max, E, None if strides is None else (ctypes.c_int64 * 12)(*strides), ks, ko,
                             kbits, vs, vo, vbits, cos, sin, table_rows, None)


def _append_strides(HKV=2, L=1, S_max=300, E=128, **change):
    s = [HKV * L * E, L * E, E] * 2 + [HKV * S_max * E, S_max * E, E] * 2
    for i, value in change.items():
        s[int(i[1:])] = value
    return tuple(s)


# in the documented order: each call fails the named check and passes every check ahead of it; most fail a LATER check too and must
# report the earlier one
APPEND_ERRORS = [
    (lambda lib: _append(lib, dt=F32, strides=None), Status.ERR_DTYPE),                          # 1. the value dtype; before the table
    (lambda lib: _append(lib, dt=I8, E=96), Status.ERR_DTYPE),
    (lambda lib: _append(lib, strides=None, E=96), Status.ERR_ARG),                              # 2. the strides table; before E
    (lambda lib: _append(lib, E=96, B=-1), Status.ERR_ARG),                                      # 3. E; before the extents
    (lambda lib: _append(lib, E=32), Status.ERR_ARG),
    (lambda lib: _append(lib, B=-1, kbits=9.0), Status.ERR_ARG),                                 # 4. the extents; before the bit-widths
    (lambda lib: _append(lib, L=-1, kbits=9.0), Status.ERR_ARG),
    (lambda lib: _append(lib, S_max=-1, kbits=9.0), Status.ERR_ARG),
    (lambda lib: _append(lib, HKV=0, kbits=9.0), Status.ERR_ARG),
    (lambda lib: _append(lib, kbits=9.0, ks=None), Status.ERR_ARG),                              # 5. the bit-widths; before the scales
    (lambda lib: _append(lib, kbits=1.0), Status.ERR_ARG),
    (lambda lib: _append(lib, vbits=3.5), Status.ERR_ARG),
    (lambda lib: _append(lib, vbits=0.0, L=0), Status.ERR_ARG),
    (lambda lib: _append(lib, ks=None, ko=FAKE, cos=FAKE), Status.ERR_ARG),                      # 6. an offset without its scale; before the tables
    (lambda lib: _append(lib, vs=None, cos=FAKE), Status.ERR_ARG),
    (lambda lib: _append(lib, cos=FAKE, sin=None, table_rows=1), Status.ERR_ARG),                # 7. one rotary table without the other; before the rows
    (lambda lib: _append(lib, cos=None, sin=FAKE, B=0), Status.ERR_ARG),
    (lambda lib: _append(lib, cos=FAKE, sin=FAKE, table_rows=299, L=0), Status.ERR_ARG),         # 8. table_rows < S_max; before the empty return
    (lambda lib: _append(lib, B=0, k_new=None, lens=None, k_cache=FAKE + 1), Status.OK),         # 9. empty: nothing launched (before alignment, NULL buffers)
    (lambda lib: _append(lib, L=0, k_new=None, lens=None, k_cache=FAKE + 1), Status.OK),
    (lambda lib: _append(lib, S_max=1 << 30, k_new=None), Status.ERR_ARG),                       # 10. the sizes
    (lambda lib: _append(lib, L=1 << 40, k_new=None), Status.ERR_ARG),
    (lambda lib: _append(lib, B=1 << 20, L=1 << 20, k_new=None), Status.ERR_ARG),
    (lambda lib: _append(lib, k_new=FAKE + 8, v_cache=None), Status.ERR_ARG),                    # 11. alignment; before the NULL buffers
    (lambda lib: _append(lib, v_new=FAKE + 2, v_cache=None), Status.ERR_ARG),
    (lambda lib: _append(lib, k_cache=FAKE + 4, v_cache=None), Status.ERR_ARG),
    (lambda lib: _append(lib, v_cache=FAKE + 1, k_new=None), Status.ERR_ARG),
    (lambda lib: _append(lib, lens=FAKE + 2, k_new=None), Status.ERR_ARG),
    (lambda lib: _append(lib, cos=FAKE + 8, sin=FAKE, table_rows=300, k_new=None), Status.ERR_ARG),
    (lambda lib: _append(lib, strides=_append_strides(s2=-128), k_new=None), Status.ERR_ARG),    # 12. the strides; before the NULL buffers
    (lambda lib: _append(lib, strides=_append_strides(s2=132), k_new=None), Status.ERR_ARG),     #     bf16 rows 264 bytes apart
    (lambda lib: _append(lib, strides=_append_strides(s5=4), k_new=None), Status.ERR_ARG),
    (lambda lib: _append(lib, strides=_append_strides(s8=136), k_new=None), Status.ERR_ARG),     #     int8 rows 136 bytes apart
    (lambda lib: _append(lib, strides=_append_strides(s11=8), k_new=None), Status.ERR_ARG),
    (lambda lib: _append(lib, k_new=None), Status.ERR_ARG),                                      # 13. NULL buffers
    (lambda lib: _append(lib, v_new=None), Status.ERR_ARG),
    (lambda lib: _append(lib, k_cache=None), Status.ERR_ARG),
    (lambda lib: _append(lib, v_cache=None), Status.ERR_ARG),
    (lambda lib: _append(lib, lens=None), Status.ERR_ARG),
    (lambda lib: _append(lib, S_max=0), Status.OK),                                              # 14. a cache without a position: nothing to write
]


def _table(*values):
    return (ctypes.c_void_p * 3)(*values)


def _decode(lib, q=FAKE, q_dt=BF16, k=FAKE, v=FAKE, dt=BF16, deq_s=(None, FAKE, FAKE), deq_o=(None, None, None), lens=FAKE, B=2, H=8, HKV=2, L=1, S_max=300,
            E=128, strides="dense", causal=0, sqrt_scale=0.3, out_s=None, out_o=None, bits=8.0, splits=0, plan_len=0, out=FAKE, ws=FAKE, ws_bytes=None):
    if strides == "dense":
        strides = _decode_strides(H, HKV, L, S_max, E)
    if ws_bytes is None:
        rows = L * (H // HKV if HKV > 0 else 1)
        count = splits or lib.ffq_sdpa_decode_splits(B, HKV, plan_len or S_max, rows, E)
        ws_bytes = lib.ffq_sdpa_decode_workspace_bytes(B, HKV, rows, E, count)
    return lib.ffq_kv_decode(q, q_dt, k, v, dt, None if deq_s is None else _table(*deq_s), None if deq_o is None else _table(*deq_o), lens, B, H, HKV, L, S_max, E,
                             None if strides is None else (ctypes.c_int64 * 9)(*strides), causal, sqrt_scale, out_s, out_o, bits, splits, plan_len, out, ws,
                             ws_bytes, None)


def _decode_strides(H=8, HKV=2, L=1, S_max=300, E=128, **change):
    s = [H * L * E, L * E, E, HKV * S_max * E, S_max * E, E, HKV * S_max * E, S_max * E, E]
    for i, value in change.items():
        s[int(i[1:])] = value
    return tuple(s)


DECODE_ERRORS = [
    (lambda lib: _decode(lib, dt=F32, q_dt=I8, deq_s=None), Status.ERR_DTYPE),                   # 1. the value dtype
    (lambda lib: _decode(lib, q_dt=F16, strides=None), Status.ERR_DTYPE),                        # 2. q's container; before the tables
    (lambda lib: _decode(lib, strides=None, E=96), Status.ERR_ARG),                              # 3. the tables; before E
    (lambda lib: _decode(lib, deq_s=None, q_dt=I8), Status.ERR_ARG),
    (lambda lib: _decode(lib, deq_o=None, L=-1), Status.ERR_ARG),
    (lambda lib: _decode(lib, q_dt=I8, deq_s=(None, None, FAKE)), Status.ERR_DTYPE),             # 4. int8 q codes without a scale; before k / v
    (lambda lib: _decode(lib, deq_s=(None, None, FAKE), E=96), Status.ERR_ARG),                  # 5. k or v without a scale; before E
    (lambda lib: _decode(lib, E=96, B=-1), Status.ERR_ARG),                                      # 6. E
    (lambda lib: _decode(lib, B=-1, L=40), Status.ERR_ARG),                                      # 7. the extents; before the rows
    (lambda lib: _decode(lib, S_max=-1, causal=2), Status.ERR_ARG),
    (lambda lib: _decode(lib, H=7, HKV=2, causal=2), Status.ERR_ARG),
    (lambda lib: _decode(lib, HKV=0, causal=2), Status.ERR_ARG),
    (lambda lib: _decode(lib, L=33, H=2, causal=2, ws_bytes=0), Status.ERR_ARG),                 # 8. the rows; before causal
    (lambda lib: _decode(lib, L=9, causal=2, ws_bytes=0), Status.ERR_ARG),
    (lambda lib: _decode(lib, causal=2, out_o=FAKE), Status.ERR_ARG),                            # 9. causal; before the quantizer
    (lambda lib: _decode(lib, causal=-1), Status.ERR_ARG),
    (lambda lib: _decode(lib, out_o=FAKE, splits=65), Status.ERR_ARG),                           # 10. the output quantizer; before the splits
    (lambda lib: _decode(lib, out_s=FAKE, bits=9.0, splits=65), Status.ERR_ARG),
    (lambda lib: _decode(lib, out_s=FAKE, bits=3.5), Status.ERR_ARG),
    (lambda lib: _decode(lib, splits=65, plan_len=301, ws_bytes=0), Status.ERR_ARG),             # 11. the splits; before plan_len
    (lambda lib: _decode(lib, splits=-1, ws_bytes=0), Status.ERR_ARG),
    (lambda lib: _decode(lib, plan_len=301, ws_bytes=0, q=None), Status.ERR_ARG),                # 12. plan_len
    (lambda lib: _decode(lib, plan_len=-1, ws_bytes=0), Status.ERR_ARG),
    (lambda lib: _decode(lib, B=0, S_max=0, q=None, out=None, lens=None, ws=None), Status.OK),   # 13. empty: nothing launched
    (lambda lib: _decode(lib, L=0, S_max=0, q=None, out=None, lens=None, ws=None, ws_bytes=0), Status.OK),
    (lambda lib: _decode(lib, S_max=0, q=None, ws_bytes=0), Status.ERR_ARG),                     # 14. S_max == 0; before the buffers
    (lambda lib: _decode(lib, S_max=1 << 30, q=None, ws_bytes=0), Status.ERR_ARG),               # 15. the sizes
    (lambda lib: _decode(lib, B=1 << 23, q=None, ws_bytes=0), Status.ERR_ARG),
    (lambda lib: _decode(lib, q=None, ws=None), Status.ERR_ARG),                                 # 16. NULL buffers; before the workspace
    (lambda lib: _decode(lib, k=None, ws=None), Status.ERR_ARG),
    (lambda lib: _decode(lib, v=None, ws=None), Status.ERR_ARG),
    (lambda lib: _decode(lib, out=None, ws=None), Status.ERR_ARG),
    (lambda lib: _decode(lib, lens=None, ws=None), Status.ERR_ARG),
    (lambda lib: _decode(lib, q=FAKE + 8, ws=None), Status.ERR_ARG),                             # 17. alignment; before the workspace
    (lambda lib: _decode(lib, k=FAKE + 4, ws=None), Status.ERR_ARG),
    (lambda lib: _decode(lib, out=FAKE + 2, ws=None), Status.ERR_ARG),
    (lambda lib: _decode(lib, lens=FAKE + 2, ws=None), Status.ERR_ARG),
    (lambda lib: _decode(lib, strides=_decode_strides(s2=-128), ws=None), Status.ERR_ARG),       # 18. the strides; before the workspace
    (lambda lib: _decode(lib, strides=_decode_strides(s2=132), ws=None), Status.ERR_ARG),
    (lambda lib: _decode(lib, strides=_decode_strides(s5=136), ws=None), Status.ERR_ARG),
    (lambda lib: _decode(lib, ws=None), Status.ERR_WORKSPACE),                                   # 19. the workspace
    (lambda lib: _decode(lib, ws=FAKE + 8), Status.ERR_WORKSPACE),
    (lambda lib: _decode(lib, ws_bytes=0), Status.ERR_WORKSPACE),
    (lambda lib: _decode(lib, splits=3, ws_bytes=decode.sdpa_decode_workspace_bytes(2, 2, 4, 128, 3) - 1), Status.ERR_WORKSPACE),
    # the plan is the dense entry's at plan_len keys: 1024 keys plan 2 splits for 128 groups (below: a hint of 200 keys plans 1)
    (lambda lib: _decode(lib, B=16, H=8, HKV=8, S_max=1024, ws_bytes=decode.sdpa_decode_workspace_bytes(16, 8, 1, 128, 1)), Status.ERR_WORKSPACE),
]


@pytest.mark.parametrize("index", range(len(APPEND_ERRORS)))
def test_append_argument_checks_need_no_device(index):
    call, status = APPEND_ERRORS[index]
    lib = FFQLibrary(HIP_SO)
    assert call(lib) == status
    if status != Status.OK:
        assert lib.ffq_last_error().startswith(b"kv_append")


@pytest.mark.parametrize("index", range(len(DECODE_ERRORS)))
def test_decode_argument_checks_need_no_device(index):
    call, status = DECODE_ERRORS[index]
    lib = FFQLibrary(HIP_SO)
    assert call(lib) == status
    if status != Status.OK:
        assert lib.ffq_last_error().startswith(b"kv_decode")


def test_the_plan_hint_sizes_the_workspace():
    """``splits = 0``: the count is ``ffq_sdpa_decode_splits`` at `plan_len` keys (S_max when 0), and the workspace check asks for it."""
    lib = FFQLibrary(HIP_SO)
    assert ops.sdpa_decode_plan(16, 8, 1024) == 2 and ops.sdpa_decode_plan(16, 8, 200) == 1
    one, two = (decode.sdpa_decode_workspace_bytes(16, 8, 1, 128, n) for n in (1, 2))
    kw = dict(B=16, H=8, HKV=8, S_max=1024)
    for plan_len, need in ((0, two), (1024, two), (385, two), (384, one), (200, one), (1, one)):
        assert _decode(lib, plan_len=plan_len, ws_bytes=need - 1, **kw) == Status.ERR_WORKSPACE
        assert f"needs {need} bytes".encode() in lib.ffq_last_error(), plan_len
    assert _decode(lib, splits=5, plan_len=1, ws_bytes=0, **kw) == Status.ERR_WORKSPACE     # a forced count overrides the hint
    assert f"needs {decode.sdpa_decode_workspace_bytes(16, 8, 1, 128, 5)} bytes".encode() in lib.ffq_last_error()


# ---- the wrappers -----------------------------------------------------------------------------------------------------------------------
def _operands(dtype=torch.bfloat16, B=2, HKV=2, L=3, S_max=20, E=64, G=2):
    k_new, v_new = torch.zeros(B, HKV, L, E, dtype=dtype), torch.zeros(B, HKV, L, E, dtype=dtype)
    kc, vc = torch.zeros(B, HKV, S_max, E, dtype=torch.int8), torch.zeros(B, HKV, S_max, E, dtype=torch.int8)
    return k_new, v_new, kc, vc, torch.zeros(B, dtype=torch.int32), torch.zeros(B, HKV * G, L, E, dtype=dtype)


def test_the_wrappers_say_not_covered_on_a_library_without_the_symbols(oracle_backend):
    k_new, v_new, kc, vc, lens, q = _operands()
    kq, vq = cases.params((8, 0.5, 0.0), "cpu"), cases.params((8, 0.5, 0.0), "cpu")
    with pytest.raises(BackendError, match="does not export ffq_kv_append"):
        ops.kv_append(k_new, v_new, kc, vc, lens, kq, vq)
    with pytest.raises(BackendError, match="does not export ffq_kv_decode"):
        ops.kv_decode(q, kc, vc, lens, dequant=(None, kq[:2], vq[:2]))


def wrapper_refusals():
    """The calls ``ops.kv_append`` / ``ops.kv_decode`` refuse on host tensors, ahead of any library call
    (tests/golden/gen_decode_refusals.py records their texts from the same list)."""
    bf = torch.bfloat16
    k_new, v_new, kc, vc, lens, q = _operands()
    kq, vq = cases.params((8, 0.5, 0.0), "cpu"), cases.params((4, 0.5, 1.0), "cpu")
    one = (torch.ones(1), None)
    table = torch.zeros(20, 64, dtype=bf)
    return [lambda: ops.kv_append(k_new[0], v_new, kc, vc, lens, kq, vq), lambda: ops.kv_append(k_new.float(), v_new.float(), kc, vc, lens, kq, vq),
            lambda: ops.kv_append(k_new, v_new.half(), kc, vc, lens, kq, vq), lambda: ops.kv_append(k_new, v_new, kc.to(bf), vc, lens, kq, vq),
            lambda: ops.kv_append(k_new, v_new[:, :1], kc, vc, lens, kq, vq), lambda: ops.kv_append(k_new, v_new, kc, vc[:, :, :19], lens, kq, vq),
            lambda: ops.kv_append(k_new[..., :32], v_new[..., :32], kc[..., :32], vc[..., :32], lens, kq, vq),
            lambda: ops.kv_append(k_new, v_new, kc, vc, lens.long(), kq, vq), lambda: ops.kv_append(k_new, v_new, kc, vc, lens[:1], kq, vq),
            lambda: ops.kv_append(k_new, v_new, kc, vc, torch.zeros(4, dtype=torch.int32)[::2], kq, vq),
            lambda: ops.kv_append(k_new.transpose(2, 3).contiguous().transpose(2, 3), v_new, kc, vc, lens, kq, vq),
            lambda: ops.kv_append(k_new, v_new, kc, vc, lens, (kq[0], kq[1], 9.0), vq), lambda: ops.kv_append(k_new, v_new, kc, vc, lens, kq, (vq[0], vq[1], 1.0)),
            lambda: ops.kv_append(k_new, v_new, kc, vc, lens, (None, kq[1], 8.0), vq), lambda: ops.kv_append(k_new, v_new, kc, vc, lens, (torch.ones(2), None, 8.0), vq),
            lambda: ops.kv_append(k_new, v_new, kc, vc, lens, kq, vq, rope=(table[:19], table[:19])),
            lambda: ops.kv_append(k_new, v_new, kc, vc, lens, kq, vq, rope=(table, table.half())),
            lambda: ops.kv_append(k_new, v_new, kc, vc, lens, kq, vq, rope=(table, torch.zeros(21, 64, dtype=bf))),
            lambda: ops.kv_decode(q, kc, vc, lens), lambda: ops.kv_decode(q, kc.to(bf), vc, lens, dequant=(None, one, one)),
            lambda: ops.kv_decode(q[0], kc, vc, lens, dequant=(None, one, one)), lambda: ops.kv_decode(q.float(), kc, vc, lens, dequant=(None, one, one)),
            lambda: ops.kv_decode(q.to(torch.int8), kc, vc, lens, dequant=(None, one, one), dtype=bf),
            lambda: ops.kv_decode(torch.zeros(2, 2, 33, 64, dtype=bf), kc, vc, lens, dequant=(None, one, one)),
            lambda: ops.kv_decode(torch.zeros(2, 3, 1, 64, dtype=bf), kc, vc, lens, dequant=(None, one, one)),
            lambda: ops.kv_decode(q, kc, vc[:, :, :4], lens, dequant=(None, one, one)), lambda: ops.kv_decode(q, kc, vc, lens, dequant=(None, one, one), splits=65),
            lambda: ops.kv_decode(q, kc, vc, lens, dequant=(None, one, one), splits=-1), lambda: ops.kv_decode(q, kc, vc, lens, dequant=(None, one, one), plan_len=0),
            lambda: ops.kv_decode(q, kc, vc, lens, dequant=(None, one, one), plan_len=21), lambda: ops.kv_decode(q, kc, vc, lens.long(), dequant=(None, one, one)),
            lambda: ops.kv_decode(q, kc, vc, lens[:1], dequant=(None, one, one))]


def test_the_wrappers_check_their_operands_and_refuse_host_tensors():
    k_new, v_new, kc, vc, lens, q = _operands()
    kq, vq = cases.params((8, 0.5, 0.0), "cpu"), cases.params((4, 0.5, 1.0), "cpu")
    one = (torch.ones(1), None)
    with pytest.raises(BackendError, match="HIP device only"):
        ops.kv_append(k_new, v_new, kc, vc, lens, kq, vq)
    with pytest.raises(BackendError, match="HIP device only"):
        ops.kv_decode(q, kc, vc, lens, dequant=(None, one, one))
    for call in wrapper_refusals():
        with pytest.raises(RuntimeError):
            call()


# ---- the class ------------------------------------------------------------------------------------------------------------------------------
def _estimating(build, quantizer):
    """`build` while a range estimator is installed on `quantizer`."""
    def call():
        with ff.estimate_ranges(quantizer, ff.range_setting.running_minmax):
            build()
    return call


def class_refusals():
    """(a sound cache, its keyword arguments, [(call, the words its ValueError must hold or None)]): what the constructor, ``append``
    and ``attend`` of ``QuantizedKVCache`` refuse (tests/golden/gen_decode_refusals.py records the texts from the same list)."""
    good = cases.quantizer((8, 0.5, 3.0))
    ok = dict(batch=2, kv_heads=2, max_len=16, head_dim=64, key_quantizer=good, value_quantizer=cases.quantizer((4, 0.25, -1.0)), dtype=torch.bfloat16, device="cpu")
    cache = ff.nn.QuantizedKVCache(**ok)
    per_channel = ff.nn.LinearQuantizer(8, granularity=ff.PerChannel(1), quantized_dtype=torch.int8)
    per_channel.quantization_range = (torch.full((2,), -1.0), torch.full((2,), 1.0))
    estimating = cases.quantizer((8, 0.5, 3.0))
    bad_quantizers = [ff.nn.LinearQuantizer(8, quantized_dtype=torch.int8), per_channel, cases.quantizer((16, 0.5, 0.0)), cases.quantizer((8, 0.5, 0.0), container=None),
                      cases.quantizer((8, 0.5, 0.0), container=torch.bfloat16), cases.quantizer((1, 0.5, 0.0)), ff.nn.QuantizerStub(), None,
                      ff.nn.DynamicLinearQuantizer(8)]
    build = lambda **change: lambda: ff.nn.QuantizedKVCache(**{**ok, **change})  # noqa: E731
    # not initialised; per channel; 16 bits; codes held in the data dtype; 1 bit; not a LinearQuantizer
    refused = [(build(**{slot: q}), "quantizer") for q in bad_quantizers for slot in ("key_quantizer", "value_quantizer")]
    refused.append((_estimating(build(key_quantizer=estimating), estimating), "quantizer"))  # not static while a range estimator is installed
    refused += [(build(**change), None)
                for change in (dict(layout="sbhe"), dict(dtype=torch.float32), dict(head_dim=96), dict(batch=0), dict(max_len=0), dict(kv_heads=0))]
    k = torch.zeros(2, 2, 3, 64, dtype=torch.bfloat16)
    refused += [(lambda key=key, value=value: cache.append(key, value), None)
                for key, value in ((k.half(), k.half()), (k[:1], k[:1]), (k, k[:, :, :2]), (k[..., :32], k[..., :32]), (k[0], k[0]))]
    q = torch.zeros(2, 4, 1, 64, dtype=torch.bfloat16)
    refused.append((lambda: cache.attend(q.half()), None))
    refused.append((lambda: cache.attend(q, output_quantizer=cases.quantizer((16, 0.5, 0.0), container=None)), "output quantizer"))
    return cache, ok, refused


def test_the_constructor_refuses_what_the_kernels_do_not_reproduce():
    cache, ok, refused = class_refusals()
    assert cache.k_cache.shape == cache.v_cache.shape == (2, 2, 16, 64) and cache.k_cache.dtype == torch.int8 and cache.k_cache.is_contiguous()
    assert cache.lengths.dtype == torch.int32 and cache.lengths.tolist() == [0, 0]
    other = ff.nn.QuantizedKVCache(**{**ok, "layout": "bshe", "dtype": torch.float16})
    assert other.k_cache.shape == (2, 2, 16, 64) and other.k_cache.transpose(1, 2).is_contiguous() and other.k_cache.stride(2) == 2 * 64
    for call, words in refused:
        with pytest.raises(ValueError, match=words):
            call()
    assert cache.lengths.tolist() == [0, 0]  # (a refused call moved nothing)


# exact parameters for the float64 restatement (kv_cache_cases.codes64): power-of-two scales, integral offsets beyond int8
EXACT_K, EXACT_V = (8, 2.0**-5, 300.0), (4, 2.0**-2, -200.0)


@pytest.mark.parametrize("layout", kv_cache.LAYOUTS)
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_the_composed_route_equals_a_float64_restatement(layout, dtype):
    """On host tensors the class runs the composed route. Codes: equal to A1 restated in float64 at the restated positions (rotary
    included), nothing else written. Attention: within one rounding of the data dtype at the largest |V| (the math path contracts in
    fp32 and rounds once, by at most 2^-9 / 2^-12 of the value: twice that, for the fp32 sums) of float64 attention over the dequantized codes,
    with exact zeros where nothing is visible."""
    Bc, H, HKV, S_max, E = 4, 4, 2, 24, 64
    gen = torch.Generator().manual_seed(7 + cases.DTYPES.index(dtype))
    kq, vq = cases.quantizer(EXACT_K), cases.quantizer(EXACT_V)
    cache = ff.nn.QuantizedKVCache(Bc, HKV, S_max, E, kq, vq, dtype, "cpu", layout=layout)
    for buffer in (cache.k_cache, cache.v_cache):
        buffer.fill_(cases.SENTINEL)
    cos, sin = (torch.randn(S_max + 3, E, generator=gen).to(dtype) for _ in range(2))
    want_k, want_v = (torch.full((Bc, HKV, S_max, E), cases.SENTINEL, dtype=torch.int8) for _ in range(2))
    lens = [0, 0, 0, 0]
    for start, L, rope in (([0, 3, 17, 22], 5, True), (None, 1, True), (None, 3, False)):
        if start is not None:
            cache.reset(start)
            lens = list(start)
        k_new = (torch.randn(Bc, HKV, L, E, generator=gen) * 3 + 9.4).to(dtype)   # around the K grid's centre, past both clamps
        v_new = (torch.randn(Bc, HKV, L, E, generator=gen) * 2 - 50).to(dtype)
        # both clamps, and two exact ties (x / scale - offset = 7.5 and 8.5; they are numbers of fp16, bf16 rounds them off the tie)
        k_new[0, 0, 0, :4] = torch.tensor([(7 + 300 + 0.5) * 2.0**-5, (8 + 300 + 0.5) * 2.0**-5, 1e4, -1e4]).to(dtype)
        cache.append(k_new, v_new, rope=(cos, sin) if rope else None)
        lens = [n + L for n in lens]
        assert cache.lengths.tolist() == lens
        for b, n in enumerate(lens):
            for l, pos in cases.positions(n, L, S_max):
                row = cases.rotate_rounded(k_new[b, :, l], cos[pos], sin[pos]) if rope else k_new[b, :, l]
                want_k[b, :, pos], want_v[b, :, pos] = cases.codes64(row, EXACT_K), cases.codes64(v_new[b, :, l], EXACT_V)
        assert torch.equal(cache.k_cache, want_k) and torch.equal(cache.v_cache, want_v)
    assert lens == [9, 12, 26, 31] and bool((want_k[2, :, 23] != cases.SENTINEL).any())
    for L, causal in ((1, True), (3, True), (3, False), (11, True)):
        q = torch.randn(Bc, H, L, E, generator=gen).to(dtype)
        got = cache.attend(q, is_causal=causal)
        assert got.shape == (Bc, H, L, E) and got.dtype == dtype
        ref = cases.attend64(q, want_k, want_v, lens, EXACT_K, EXACT_V, causal)
        bound = 2.0 ** (-8 if dtype == torch.bfloat16 else -11) * (8 + 200) * EXACT_V[1]  # (|V| <= (8 + 200) * scale)
        assert float((got.double() - ref).abs().max()) <= bound
        if L == 11 and causal:  # 9 keys under 11 rows: rows 0 and 1 of the first sequence see nothing
            assert torch.equal(got[0, :, :2], torch.zeros_like(got[0, :, :2])) and bool(got[0, :, 2].any())
    cache.reset()
    q = torch.randn(Bc, H, 2, E, generator=gen).to(dtype)
    assert cache.lengths.tolist() == [0] * Bc and torch.equal(cache.attend(q), torch.zeros_like(q))
    # keys(length) / values(length): what the quantizers themselves would have returned for those codes
    keys, values = cache.keys(9), cache.values(9)
    assert isinstance(keys, ff.QuantizedTensor) and keys.shape == (Bc, HKV, 9, E) and keys.raw_data.dtype == torch.int8
    assert torch.equal(keys.dequantize(), ((want_k[:, :, :9].float() + 300.0) * 2.0**-5).to(dtype)) and keys.dequantize().dtype == dtype
    assert torch.equal(values.dequantize(), ((want_v[:, :, :9].float() - 200.0) * 2.0**-2).to(dtype))


# ---- what hipcc emitted -----------------------------------------------------------------------------------------------------------------
def test_the_append_kernels_spill_nothing_and_use_neither_scratch_nor_lds():
    if kernel_resources.readelf() is None:
        pytest.skip("llvm-readelf is missing")
    assert kernel_resources.DEFAULT_LIBRARY.exists(), "build() leaves the HIP library in the tree"
    kernels = [k for k in kernel_resources.kernel_resources() if "kv_append" in str(k["name"])]
    assert len(kernels) == 4, [k["name"] for k in kernels]  # bf16 / fp16 x plain / rotary
    bad = {str(k["name"]): k for k in kernels
           if k["vgpr_spill_count"] or k["sgpr_spill_count"] or k["private_segment_fixed_size"] or k["group_segment_fixed_size"]}
    assert not bad, bad
