"""The KV cache with per-token dynamic scales without a GPU: the ninth header ``include/ffq_kv_token.h`` against
``_cabi.SIGNATURES_KV_TOKEN`` (exported by the HIP library, absent from the oracle, the other tables untouched), every argument error
of ``ffq_kv_token_append`` and ``ffq_kv_token_decode`` in the documented order before any device call, the wrappers' operand checks,
what ``nn.DynamicQuantizedKVCache`` takes and refuses, the composed route on host tensors against ``_host.quantize_dynamic_by_tile``
and float64 attention, the point of the feature as a property (a row's error is bounded by its OWN range), the re-expression helper
the GPU tests lean on, and what hipcc emitted for the eight new kernels."""

import ctypes
import re
import sys

import pytest
import torch

import fastforward_amd as ff

import kv_cache_cases as dense_cases
import kv_token_cases as cases

from conftest import HIP_SO, ROOT, load_oracle
from fastforward_amd import _cabi, ops
from fastforward_amd._cabi import DType, FFQLibrary, Status
from fastforward_amd.exceptions import BackendError
from fastforward_amd.nn import kv_cache
from fastforward_amd.ops import decode

sys.path.insert(0, str(ROOT / "tools"))

import kernel_resources  # noqa: E402

ENTRIES = {"ffq_kv_token_append", "ffq_kv_token_decode"}


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
def test_the_functions_and_the_class_exist():
    assert {"kv_token_append", "kv_token_decode"} <= set(ops.__all__) and callable(ops.kv_token_append) and callable(ops.kv_token_decode)
    assert ff.nn.DynamicQuantizedKVCache is kv_cache.DynamicQuantizedKVCache and issubclass(kv_cache.DynamicQuantizedKVCache, kv_cache._CacheBase)
    assert callable(kv_cache.composed_token_append) and callable(kv_cache.composed_token_attend)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
def _header(name):
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / name).read_text(), flags=re.S)


def _declared(name):
    return set(re.findall(r"\b(ffq_[a-z0-9_]+)\s*\(", _header(name)))


def test_the_ninth_header_and_its_table_agree():
    assert _declared("ffq_kv_token.h") == set(_cabi.SIGNATURES_KV_TOKEN) == ENTRIES
    assert '#include "ffq_kv_cache.h"' in (ROOT / "include" / "ffq_kv_token.h").read_text()
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
    want_names = {
        "ffq_kv_token_append": ["k_new", "v_new", "dt", "k_cache", "v_cache", "params", "lens", "batch", "kv_heads", "L", "S_max", "E", "strides",
                                "k_num_bits", "k_symmetric", "v_num_bits", "v_symmetric", "cos_table", "sin_table", "table_rows", "stream"],
        "ffq_kv_token_decode": ["q", "q_dt", "k", "v", "dt", "q_scale", "q_offset", "params", "lens", "batch", "q_heads", "kv_heads", "L", "S_max", "E",
                                "strides", "causal", "sqrt_scale", "out_scale", "out_offset", "out_num_bits", "splits", "plan_len", "out", "workspace",
                                "workspace_bytes", "stream"],
    }
    for entry in ENTRIES:
        m = re.search(r"(\w+)\s+" + entry + r"\s*\((.*?)\)\s*;", _header("ffq_kv_token.h"), flags=re.S)
        names, want = [], []
        for p in m.group(2).split(","):
            words = p.replace("*", " * ").split()
            names.append(words[-1])
            if "*" in words:
                want.append(ctypes.POINTER(ctypes.c_int64) if words[words.index("*") - 1] == "int64_t" else ctypes.c_void_p)
            else:
                want.append(kinds[words[-2]])
        restype, argtypes = _cabi.SIGNATURES_KV_TOKEN[entry]
        assert m.group(1) == "int" and restype is ctypes.c_int and argtypes == want and names == want_names[entry], entry


def test_the_other_tables_are_untouched_and_disjoint():
    others = {"ffq.h": _cabi.SIGNATURES, "ffq_3d.h": _cabi.SIGNATURES_3D, "ffq_depthwise.h": _cabi.SIGNATURES_DEPTHWISE, "ffq_index.h": _cabi.SIGNATURES_INDEX,
              "ffq_unfold.h": _cabi.SIGNATURES_UNFOLD, "ffq_sdpa_decode.h": _cabi.SIGNATURES_DECODE, "ffq_kv_cache.h": _cabi.SIGNATURES_KV,
              "ffq_kv_paged.h": _cabi.SIGNATURES_PAGED}
    assert len(others) == 8
    for header, table in others.items():
        assert _declared(header) == set(table), header
        assert not ENTRIES & set(table), header
    assert not ENTRIES & set(_cabi.DEVICE_ONLY)
    assert set(_cabi.SIGNATURES_KV) == {"ffq_kv_append", "ffq_kv_decode"}
    assert set(_cabi.SIGNATURES_PAGED) == {"ffq_kv_paged_append", "ffq_kv_paged_decode"}
    assert set(_cabi.SIGNATURES_DECODE) == {"ffq_sdpa_decode", "ffq_sdpa_decode_splits", "ffq_sdpa_decode_workspace_bytes"}
    assert _cabi.FFQ_ABI_VERSION == 9 and "#define FFQ_ABI_VERSION 9" in (ROOT / "include" / "ffq.h").read_text()


def test_the_hip_library_exports_them_and_the_oracle_loads_without_them():
    dll, lib, oracle = ctypes.CDLL(str(HIP_SO)), FFQLibrary(HIP_SO), load_oracle()
    for entry in ENTRIES:
        assert hasattr(dll, entry) and getattr(lib, entry) is not None
        assert not oracle.is_device and getattr(oracle, entry) is None


FAKE = 1 << 20  # never dereferenced: every call below returns from the argument checks
BF16, F16, I8, F32 = (int(t) for t in (DType.BF16, DType.F16, DType.I8, DType.F32))


def _append_strides(HKV=2, L=1, S=128, E=128, **change):
    s = [HKV * L * E, L * E, E] * 2 + [HKV * S * E, S * E, E] * 2 + [HKV * S * 4, S * 4, 4]
    for i, value in change.items():
        s[int(i[1:])] = value
    return tuple(s)


def _append(lib, k_new=FAKE, v_new=FAKE, dt=BF16, k_cache=FAKE, v_cache=FAKE, params=FAKE, lens=FAKE, B=2, HKV=2, L=1, S=128, E=128, strides="dense",
            kbits=8.0, ksym=0, vbits=4.0, vsym=1, cos=None, sin=None, table_rows=0):
    if strides == "dense":
        strides = _append_strides()
    return lib.ffq_kv_token_append(k_new, v_new, dt, k_cache, v_cache, params, lens, B, HKV, L, S, E, None if strides is None else (ctypes.c_int64 * 15)(*strides),
                                   kbits, ksym, vbits, vsym, cos, sin, table_rows, None)


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
    (lambda lib: _append(lib, S=-1, kbits=9.0), Status.ERR_ARG),
    (lambda lib: _append(lib, HKV=0, kbits=9.0), Status.ERR_ARG),
    (lambda lib: _append(lib, kbits=9.0, ksym=2), Status.ERR_ARG),                               # 5. the bit-widths; before the symmetric flags
    (lambda lib: _append(lib, kbits=1.0), Status.ERR_ARG),
    (lambda lib: _append(lib, vbits=3.5), Status.ERR_ARG),
    (lambda lib: _append(lib, vbits=0.0, L=0), Status.ERR_ARG),
    (lambda lib: _append(lib, ksym=2, cos=FAKE), Status.ERR_ARG),                                # 6. the symmetric flags; before the tables
    (lambda lib: _append(lib, vsym=-1, cos=FAKE), Status.ERR_ARG),
    (lambda lib: _append(lib, cos=FAKE, sin=None, table_rows=1), Status.ERR_ARG),                # 7. one rotary table without the other; before the rows
    (lambda lib: _append(lib, cos=None, sin=FAKE, B=0), Status.ERR_ARG),
    (lambda lib: _append(lib, cos=FAKE, sin=FAKE, table_rows=127, L=0), Status.ERR_ARG),         # 8. table_rows < S_max = 128; before the empty return
    (lambda lib: _append(lib, B=0, k_new=None, lens=None, params=None, k_cache=FAKE + 1), Status.OK),  # 9. empty: nothing launched
    (lambda lib: _append(lib, L=0, k_new=None, lens=None, params=None, k_cache=FAKE + 1), Status.OK),
    (lambda lib: _append(lib, S=1 << 30, k_new=None), Status.ERR_ARG),                           # 10. the sizes
    (lambda lib: _append(lib, L=1 << 40, k_new=None), Status.ERR_ARG),
    (lambda lib: _append(lib, B=1 << 20, L=1 << 20, k_new=None), Status.ERR_ARG),
    (lambda lib: _append(lib, k_new=FAKE + 8, v_cache=None), Status.ERR_ARG),                    # 11. alignment; before the NULL buffers
    (lambda lib: _append(lib, v_new=FAKE + 2, v_cache=None), Status.ERR_ARG),
    (lambda lib: _append(lib, k_cache=FAKE + 4, v_cache=None), Status.ERR_ARG),
    (lambda lib: _append(lib, v_cache=FAKE + 1, k_new=None), Status.ERR_ARG),
    (lambda lib: _append(lib, params=FAKE + 4, k_new=None), Status.ERR_ARG),
    (lambda lib: _append(lib, lens=FAKE + 2, k_new=None), Status.ERR_ARG),
    (lambda lib: _append(lib, cos=FAKE + 8, sin=FAKE, table_rows=128, k_new=None), Status.ERR_ARG),
    (lambda lib: _append(lib, strides=_append_strides(s2=-128), k_new=None), Status.ERR_ARG),    # 12. the twelve strides; before the NULL buffers
    (lambda lib: _append(lib, strides=_append_strides(s2=132), k_new=None), Status.ERR_ARG),     #     bf16 rows 264 bytes apart
    (lambda lib: _append(lib, strides=_append_strides(s5=4), k_new=None), Status.ERR_ARG),
    (lambda lib: _append(lib, strides=_append_strides(s8=136), k_new=None), Status.ERR_ARG),     #     int8 rows 136 bytes apart
    (lambda lib: _append(lib, strides=_append_strides(s9=-16), k_new=None), Status.ERR_ARG),
    (lambda lib: _append(lib, k_new=None, strides=_append_strides(s14=2)), Status.ERR_ARG),      # 13. NULL buffers; before the strides of params
    (lambda lib: _append(lib, v_new=None), Status.ERR_ARG),
    (lambda lib: _append(lib, k_cache=None), Status.ERR_ARG),
    (lambda lib: _append(lib, v_cache=None), Status.ERR_ARG),
    (lambda lib: _append(lib, params=None), Status.ERR_ARG),
    (lambda lib: _append(lib, lens=None), Status.ERR_ARG),
    (lambda lib: _append(lib, strides=_append_strides(s14=2)), Status.ERR_ARG),                  # 14. the strides of params: 8 bytes apart
    (lambda lib: _append(lib, strides=_append_strides(s12=-1024)), Status.ERR_ARG),
    (lambda lib: _append(lib, strides=_append_strides(s13=514)), Status.ERR_ARG),
    (lambda lib: _append(lib, S=0, k_cache=FAKE, strides=_append_strides(S=0)), Status.OK),      # 15. no position to write to: nothing launched
]


def _decode_strides(H=8, HKV=2, L=1, S=304, E=128, **change):
    s = [H * L * E, L * E, E, HKV * S * E, S * E, E, HKV * S * E, S * E, E, 0, 0, 0, HKV * S * 4, S * 4, 4]
    for i, value in change.items():
        s[int(i[1:])] = value
    return tuple(s)


def _decode(lib, q=FAKE, q_dt=BF16, k=FAKE, v=FAKE, dt=BF16, q_s=None, q_o=None, params=FAKE, lens=FAKE, B=2, H=8, HKV=2, L=1, S=304, E=128, strides="dense",
            causal=0, sqrt_scale=0.3, out_s=None, out_o=None, bits=8.0, splits=0, plan_len=0, out=FAKE, ws=FAKE, ws_bytes=None):
    if strides == "dense":
        strides = _decode_strides(H, HKV, L, S, E)
    if ws_bytes is None:
        rows = L * (H // HKV if HKV > 0 else 1)
        count = splits or lib.ffq_sdpa_decode_splits(B, HKV, plan_len or S, rows, E)
        ws_bytes = lib.ffq_sdpa_decode_workspace_bytes(B, HKV, rows, E, count)
    return lib.ffq_kv_token_decode(q, q_dt, k, v, dt, q_s, q_o, params, lens, B, H, HKV, L, S, E, None if strides is None else (ctypes.c_int64 * 15)(*strides),
                                   causal, sqrt_scale, out_s, out_o, bits, splits, plan_len, out, ws, ws_bytes, None)


DECODE_ERRORS = [
    (lambda lib: _decode(lib, dt=F32, q_dt=I8), Status.ERR_DTYPE),                               # 1. the value dtype
    (lambda lib: _decode(lib, q_dt=F16, strides=None), Status.ERR_DTYPE),                        # 2. q's container; before the table
    (lambda lib: _decode(lib, strides=None, E=96), Status.ERR_ARG),                              # 3. the strides table; before E
    (lambda lib: _decode(lib, q_dt=I8, params=None), Status.ERR_DTYPE),                          # 4. int8 q codes without a scale; before params
    (lambda lib: _decode(lib, params=None, E=96), Status.ERR_ARG),                               # 5. no parameter store; before E
    (lambda lib: _decode(lib, E=96, B=-1), Status.ERR_ARG),                                      # 6. E
    (lambda lib: _decode(lib, B=-1, L=40), Status.ERR_ARG),                                      # 7. the extents; before the rows
    (lambda lib: _decode(lib, S=-1, L=40), Status.ERR_ARG),
    (lambda lib: _decode(lib, H=7, HKV=2, L=40), Status.ERR_ARG),
    (lambda lib: _decode(lib, HKV=0, L=40), Status.ERR_ARG),
    (lambda lib: _decode(lib, L=33, H=2, causal=2, ws_bytes=0), Status.ERR_ARG),                 # 8. the rows; before causal
    (lambda lib: _decode(lib, L=9, causal=2, ws_bytes=0), Status.ERR_ARG),
    (lambda lib: _decode(lib, causal=2, out_o=FAKE), Status.ERR_ARG),                            # 9. causal; before the quantizer
    (lambda lib: _decode(lib, causal=-1), Status.ERR_ARG),
    (lambda lib: _decode(lib, out_o=FAKE, splits=65), Status.ERR_ARG),                           # 10. the output quantizer; before the splits
    (lambda lib: _decode(lib, out_s=FAKE, bits=9.0, splits=65), Status.ERR_ARG),
    (lambda lib: _decode(lib, out_s=FAKE, bits=3.5), Status.ERR_ARG),
    (lambda lib: _decode(lib, splits=65, plan_len=305, ws_bytes=0), Status.ERR_ARG),             # 11. the splits; before plan_len
    (lambda lib: _decode(lib, splits=-1, ws_bytes=0), Status.ERR_ARG),
    (lambda lib: _decode(lib, plan_len=305, ws_bytes=0, q=None), Status.ERR_ARG),                # 12. plan_len (S_max = 304)
    (lambda lib: _decode(lib, plan_len=-1, ws_bytes=0), Status.ERR_ARG),
    (lambda lib: _decode(lib, B=0, q=None, out=None, lens=None, ws=None), Status.OK),            # 13. empty: nothing launched
    (lambda lib: _decode(lib, L=0, q=None, out=None, lens=None, ws=None, ws_bytes=0), Status.OK),
    (lambda lib: _decode(lib, S=0, q=None, ws_bytes=0), Status.ERR_ARG),                         # 14. S_max == 0
    (lambda lib: _decode(lib, S=1 << 30, q=None, ws_bytes=0), Status.ERR_ARG),                   # 15. the sizes
    (lambda lib: _decode(lib, B=1 << 23, q=None, ws_bytes=0), Status.ERR_ARG),
    (lambda lib: _decode(lib, q=None, ws=None, strides=_decode_strides(s14=2)), Status.ERR_ARG), # 16. NULL buffers; before the strides of params
    (lambda lib: _decode(lib, k=None, ws=None), Status.ERR_ARG),
    (lambda lib: _decode(lib, v=None, ws=None), Status.ERR_ARG),
    (lambda lib: _decode(lib, out=None, ws=None), Status.ERR_ARG),
    (lambda lib: _decode(lib, lens=None, ws=None), Status.ERR_ARG),
    (lambda lib: _decode(lib, strides=_decode_strides(s14=2), q=FAKE + 8), Status.ERR_ARG),      # 17. the strides of params; before alignment
    (lambda lib: _decode(lib, strides=_decode_strides(s12=-1216), ws=None), Status.ERR_ARG),
    (lambda lib: _decode(lib, strides=_decode_strides(s13=1218), ws=None), Status.ERR_ARG),
    (lambda lib: _decode(lib, q=FAKE + 8, ws=None), Status.ERR_ARG),                             # 18. alignment; before the workspace
    (lambda lib: _decode(lib, k=FAKE + 4, ws=None), Status.ERR_ARG),
    (lambda lib: _decode(lib, out=FAKE + 2, ws=None), Status.ERR_ARG),
    (lambda lib: _decode(lib, params=FAKE + 8, ws=None), Status.ERR_ARG),
    (lambda lib: _decode(lib, lens=FAKE + 2, ws=None), Status.ERR_ARG),
    (lambda lib: _decode(lib, strides=_decode_strides(s2=-128), ws=None), Status.ERR_ARG),       # 19. the nine strides; before the workspace
    (lambda lib: _decode(lib, strides=_decode_strides(s2=132), ws=None), Status.ERR_ARG),
    (lambda lib: _decode(lib, strides=_decode_strides(s5=136), ws=None), Status.ERR_ARG),
    (lambda lib: _decode(lib, strides=_decode_strides(s6=4100), ws=None), Status.ERR_ARG),
    (lambda lib: _decode(lib, ws=None), Status.ERR_WORKSPACE),                                   # 20. the workspace
    (lambda lib: _decode(lib, ws=FAKE + 8), Status.ERR_WORKSPACE),
    (lambda lib: _decode(lib, ws_bytes=0), Status.ERR_WORKSPACE),
    (lambda lib: _decode(lib, splits=3, ws_bytes=decode.sdpa_decode_workspace_bytes(2, 2, 4, 128, 3) - 1), Status.ERR_WORKSPACE),
    # the plan is the dense entry's at S_max = 1024 keys: 2 splits for 128 groups
    (lambda lib: _decode(lib, B=16, H=8, HKV=8, S=1024, ws_bytes=decode.sdpa_decode_workspace_bytes(16, 8, 1, 128, 1)), Status.ERR_WORKSPACE),
]


@pytest.mark.parametrize("index", range(len(APPEND_ERRORS)))
def test_append_argument_checks_need_no_device(index):
    call, status = APPEND_ERRORS[index]
    lib = FFQLibrary(HIP_SO)
    assert call(lib) == status
    if status != Status.OK:
        assert lib.ffq_last_error().startswith(b"kv_token_append")


@pytest.mark.parametrize("index", range(len(DECODE_ERRORS)))
def test_decode_argument_checks_need_no_device(index):
    call, status = DECODE_ERRORS[index]
    lib = FFQLibrary(HIP_SO)
    assert call(lib) == status
    if status != Status.OK:
        assert lib.ffq_last_error().startswith(b"kv_token_decode")


def test_the_plan_hint_sizes_the_workspace():
    """``splits = 0``: the count is ``ffq_sdpa_decode_splits`` at `plan_len` keys (S_max when 0), as in ``ffq_kv_decode``."""
    lib = FFQLibrary(HIP_SO)
    one, two = (decode.sdpa_decode_workspace_bytes(16, 8, 1, 128, n) for n in (1, 2))
    kw = dict(B=16, H=8, HKV=8, S=1024)
    for plan_len, need in ((0, two), (1024, two), (385, two), (384, one), (200, one), (1, one)):
        assert _decode(lib, plan_len=plan_len, ws_bytes=need - 1, **kw) == Status.ERR_WORKSPACE
        assert f"needs {need} bytes".encode() in lib.ffq_last_error(), plan_len
    assert _decode(lib, splits=5, plan_len=1, ws_bytes=0, **kw) == Status.ERR_WORKSPACE     # a forced count overrides the hint
    assert f"needs {decode.sdpa_decode_workspace_bytes(16, 8, 1, 128, 5)} bytes".encode() in lib.ffq_last_error()


# ---- the wrappers -----------------------------------------------------------------------------------------------------------------------
def _operands(dtype=torch.bfloat16, Bc=2, H=2, L=3, S=20, E=64, G=2):
    k_new, v_new = torch.zeros(Bc, H, L, E, dtype=dtype), torch.zeros(Bc, H, L, E, dtype=dtype)
    kc, vc = torch.zeros(Bc, H, S, E, dtype=torch.int8), torch.zeros(Bc, H, S, E, dtype=torch.int8)
    return k_new, v_new, kc, vc, torch.zeros(Bc, H, S, 4), torch.zeros(Bc, dtype=torch.int32), torch.zeros(Bc, H * G, L, E, dtype=dtype)


def test_the_wrappers_say_not_covered_on_a_library_without_the_symbols(oracle_backend):
    k_new, v_new, kc, vc, params, lens, q = _operands()
    with pytest.raises(BackendError, match="does not export ffq_kv_token_append"):
        ops.kv_token_append(k_new, v_new, kc, vc, params, lens, (8, False), (4, True))
    with pytest.raises(BackendError, match="does not export ffq_kv_token_decode"):
        ops.kv_token_decode(q, kc, vc, params, lens)


def test_the_wrappers_check_their_operands_and_refuse_host_tensors():
    bf = torch.bfloat16
    k_new, v_new, kc, vc, params, lens, q = _operands()
    with pytest.raises(BackendError, match="HIP device only"):
        ops.kv_token_append(k_new, v_new, kc, vc, params, lens, (8, False), (4, True))
    with pytest.raises(BackendError, match="HIP device only"):
        ops.kv_token_decode(q, kc, vc, params, lens)
    with pytest.raises(BackendError, match="HIP device only"):  # both layouts of the store pass the checks
        ops.kv_token_decode(q, kc, vc, params.transpose(1, 2).contiguous().transpose(1, 2), lens, q_dequant=None, plan_len=20, splits=3)
    table = torch.zeros(20, 64, dtype=bf)

    def append(**change):
        a = dict(k_new=k_new, v_new=v_new, k_cache=kc, v_cache=vc, params=params, lens=lens, k_spec=(8, False), v_spec=(4, True))
        return lambda: ops.kv_token_append(**{**a, **change})

    def attend(**change):
        a = dict(query=q, k_cache=kc, v_cache=vc, params=params, lens=lens)
        return lambda: ops.kv_token_decode(**{**a, **change})

    refused = [append(k_new=k_new[0]), append(k_new=k_new.float(), v_new=v_new.float()), append(v_new=v_new.half()), append(k_cache=kc.to(bf)),
               append(v_new=v_new[:, :1]), append(v_cache=vc[:, :, :19]),
               append(k_new=k_new[..., :32], v_new=v_new[..., :32], k_cache=kc[..., :32], v_cache=vc[..., :32]),
               append(params=params.double()), append(params=params[:, :, :19]), append(params=params[..., :3]), append(params=params[0]),
               append(params=torch.zeros(2, 2, 20, 8)[..., ::2]), append(params=torch.zeros(2, 2, 20, 6)[..., 1:5]),
               append(lens=lens.long()), append(lens=lens[:1]), append(lens=torch.zeros(4, dtype=torch.int32)[::2]),
               append(k_new=k_new.transpose(2, 3).contiguous().transpose(2, 3)),
               append(k_spec=(9, False)), append(v_spec=(1, True)), append(k_spec=(3.5, False)),
               append(rope=(table[:19], table[:19])), append(rope=(table, table.half())), append(rope=(table, torch.zeros(21, 64, dtype=bf))),
               attend(k_cache=kc.to(bf)), attend(query=q[0]), attend(query=q.float()), attend(query=q.to(torch.int8), dtype=bf),
               attend(query=torch.zeros(2, 2, 33, 64, dtype=bf)), attend(query=torch.zeros(2, 3, 1, 64, dtype=bf)), attend(v_cache=vc[:, :, :4]),
               attend(params=params.double()), attend(params=params[:, :, :19]), attend(params=torch.zeros(2, 2, 20, 8)[..., ::2]),
               attend(splits=65), attend(splits=-1), attend(plan_len=0), attend(plan_len=21), attend(lens=lens.long()), attend(lens=lens[:1])]
    for i, call in enumerate(refused):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"call {i} was not refused")


# ---- the class ------------------------------------------------------------------------------------------------------------------------------
def make(dtype=torch.bfloat16, layout="bhse", **change):
    kw = dict(batch=2, kv_heads=2, max_len=16, head_dim=64, key_quantizer=cases.quantizer(8), value_quantizer=cases.quantizer(4, symmetric=True, tile=True),
              dtype=dtype, device="cpu", layout=layout)
    return ff.nn.DynamicQuantizedKVCache(**{**kw, **change})


def test_the_constructor_takes_and_refuses():
    D = ff.nn.DynamicLinearQuantizer
    cache = make()
    assert cache.k_cache.shape == cache.v_cache.shape == (2, 2, 16, 64) and cache.k_cache.dtype == torch.int8 and cache.k_cache.is_contiguous()
    assert cache.params.shape == (2, 2, 16, 4) and cache.params.dtype == torch.float32 and cache.params.is_contiguous()
    assert cache.lengths.dtype == torch.int32 and cache.lengths.tolist() == [0, 0]
    other = make(torch.float16, "bshe")
    assert other.k_cache.shape == (2, 2, 16, 64) and other.k_cache.transpose(1, 2).is_contiguous() and other.k_cache.stride(2) == 2 * 64
    assert other.params.shape == (2, 2, 16, 4) and other.params.transpose(1, 2).is_contiguous() and other.params.stride(2) == 2 * 4
    # every accept: 2..8 bits, both granularities, asymmetric (whatever allow_one_sided says) and symmetric without the one-sided rule
    for bits in range(2, 9):
        make(key_quantizer=cases.quantizer(bits), value_quantizer=cases.quantizer(bits, symmetric=True, tile=True))
    make(key_quantizer=D(8, granularity=ff.PerChannel((0, 1, 2)), quantized_dtype=torch.int8, symmetric=False, allow_one_sided=True))
    make(head_dim=128, key_quantizer=cases.quantizer(8, E=128, tile=True), value_quantizer=cases.quantizer(4, E=128))
    int8 = dict(quantized_dtype=torch.int8)
    rows = ff.PerChannel((0, 1, 2))
    bad = [D(8, granularity=rows), D(8, granularity=rows, quantized_dtype=torch.bfloat16), D(16, granularity=rows, **int8), D(1, granularity=rows, **int8),
           D(3.5, granularity=rows, **int8), D(8, granularity=rows, parameter_inference_fn=lambda p, x: (torch.ones(1), None), **int8),
           D(8, **int8), D(8, granularity=ff.PerChannel(1), **int8), D(8, granularity=ff.PerChannel((0, 1)), **int8),
           D(8, granularity=ff.PerTile((1, 1, 1, 32)), **int8), D(8, granularity=ff.PerTile((1, 1, 2, 64)), **int8),
           D(8, granularity=rows, symmetric=True, **int8), D(8, granularity=rows, symmetric=True, allow_one_sided=True, **int8),
           dense_cases.quantizer((8, 0.5, 0.0)), ff.nn.QuantizerStub(), None]
    for q in bad:
        for slot in ("key_quantizer", "value_quantizer"):
            with pytest.raises(ValueError, match="quantizer"):
                make(**{slot: q})
    for change in (dict(layout="sbhe"), dict(dtype=torch.float32), dict(head_dim=96), dict(batch=0), dict(max_len=0), dict(kv_heads=0),
                   dict(head_dim=128)):  # (the last: a PerTile of 64 columns is not one tile per row of 128)
        with pytest.raises(ValueError):
            make(**change)
    k = torch.zeros(2, 2, 3, 64, dtype=torch.bfloat16)
    for key, value in ((k.half(), k.half()), (k[:1], k[:1]), (k, k[:, :, :2]), (k[..., :32], k[..., :32]), (k[0], k[0])):
        with pytest.raises(ValueError):
            cache.append(key, value)
    q = torch.zeros(2, 4, 1, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        cache.attend(q.half())
    with pytest.raises(ValueError, match="output quantizer"):
        cache.attend(q, output_quantizer=dense_cases.quantizer((16, 0.5, 0.0), container=None))
    assert cache.lengths.tolist() == [0, 0]  # (a refused call moved nothing)
    # the static caches accept, refuse and say what they did
    with pytest.raises(ValueError, match="QuantizedKVCache: the key quantizer must be a LinearQuantizer, got DynamicLinearQuantizer"):
        ff.nn.QuantizedKVCache(2, 2, 16, 64, cases.quantizer(8), dense_cases.quantizer((8, 0.5, 0.0)), device="cpu")
    ff.nn.QuantizedKVCache(2, 2, 16, 64, dense_cases.quantizer((8, 0.5, 0.0)), dense_cases.quantizer((8, 0.5, 0.0)), device="cpu")


@pytest.mark.parametrize("layout", kv_cache.LAYOUTS)
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_the_composed_route_equals_the_dynamic_quantizer_row_by_row(layout, dtype):
    """On host tensors the class runs the composed route. Codes and parameters: ``_host.quantize_dynamic_by_tile`` of the restated rows
    (rotary included) at the restated positions, ragged lengths with rows dropped before position 0 and past the end; everything else at
    the sentinel. Attention: within one rounding of the data dtype at the largest |V| (the bound tests/test_kv_cache_cpu.py uses for its
    composed route) of float64 attention over the per-row dequantized codes."""
    Bc, H, HKV, S_max, E = 4, 4, 2, 24, 64
    gen = torch.Generator().manual_seed(7 + cases.DTYPES.index(dtype))
    K_BITS, V_BITS = (8, False), (4, True)
    cache = ff.nn.DynamicQuantizedKVCache(Bc, HKV, S_max, E, cases.quantizer(*K_BITS), cases.quantizer(*V_BITS, tile=True), dtype, "cpu", layout=layout)
    cache.k_cache.fill_(cases.SENTINEL)
    cache.v_cache.fill_(cases.SENTINEL)
    cache.params.fill_(cases.PARAM_SENTINEL)
    cos, sin = (torch.randn(S_max + 3, E, generator=gen).to(dtype) for _ in range(2))
    want_k, want_v = (torch.full((Bc, HKV, S_max, E), cases.SENTINEL, dtype=torch.int8) for _ in range(2))
    want_p = torch.full((Bc, HKV, S_max, 4), cases.PARAM_SENTINEL)
    lens = [0, 0, 0, 0]
    for start, L, rope in (([-2, 3, 17, 22], 5, True), (None, 1, True), (None, 3, False)):
        if start is not None:
            cache.reset(start)
            lens = list(start)
        k_new = (torch.randn(Bc, HKV, L, E, generator=gen) * 3 + 9.4).to(dtype)
        v_new = (torch.randn(Bc, HKV, L, E, generator=gen) * 2 - 50).to(dtype)
        v_new[1, 0, 0] = 0.0          # an all-zero row and a constant one: the eps clamp
        k_new[1, 1, 0] = 2.5
        cache.append(k_new, v_new, rope=(cos, sin) if rope else None)
        lens = [n + L for n in lens]
        assert cache.lengths.tolist() == lens
        for b, n in enumerate(lens):
            for l, pos in dense_cases.positions(n, L, S_max):
                row = dense_cases.rotate_rounded(k_new[b, :, l], cos[pos], sin[pos]) if rope else k_new[b, :, l]
                want_k[b, :, pos], want_p[b, :, pos, 0], want_p[b, :, pos, 1] = cases.dynamic_rows(row, *K_BITS)
                want_v[b, :, pos], want_p[b, :, pos, 2], want_p[b, :, pos, 3] = cases.dynamic_rows(v_new[b, :, l], *V_BITS)
        assert torch.equal(cache.k_cache, want_k) and torch.equal(cache.v_cache, want_v)
        assert torch.equal(cache.params.contiguous().view(torch.int32), want_p.view(torch.int32))
    assert lens == [7, 12, 26, 31] and bool((want_k[2, :, 23] != cases.SENTINEL).any()) and bool((want_p[0, :, 0, 0] != cases.PARAM_SENTINEL).all())
    assert float(want_p[1, 0, 9, 2]) == 0.0 and float(want_p[1, 1, 9, 0]) == 2.0**-23  # (no rotation) the zero V row (symmetric: scale 0), the constant K row (eps)
    for L, causal in ((1, True), (3, True), (3, False), (11, True)):
        q = torch.randn(Bc, H, L, E, generator=gen).to(dtype)
        got = cache.attend(q, is_causal=causal)
        assert got.shape == (Bc, H, L, E) and got.dtype == dtype
        ref = cases.attend64(q, want_k, want_v, want_p, lens, causal)
        v_max = max(float(cases.dequant64(want_v[b, :, :min(n, S_max)], want_p[b, :, :min(n, S_max)], 1, dtype).abs().max()) for b, n in enumerate(lens))
        bound = 2.0 ** (-8 if dtype == torch.bfloat16 else -11) * v_max
        assert float((got.double() - ref).abs().max()) <= bound
        if L == 11 and causal:  # 7 keys under 11 rows: rows 0 .. 3 of the first sequence see nothing
            assert torch.equal(got[0, :, :4], torch.zeros_like(got[0, :, :4])) and bool(got[0, :, 4].any())
    # keys(length) / values(length): per-row parameters, dequantized as the restatement says
    keys, values = cache.keys(7), cache.values(7)
    assert isinstance(keys, ff.QuantizedTensor) and keys.shape == (Bc, HKV, 7, E) and keys.raw_data.dtype == torch.int8
    assert keys.dequantize().dtype == dtype and torch.equal(keys.dequantize().double(), cases.dequant64(want_k[:, :, :7], want_p[:, :, :7], 0, dtype))
    assert torch.equal(values.dequantize().double(), cases.dequant64(want_v[:, :, :7], want_p[:, :, :7], 1, dtype))
    cache.reset()
    q = torch.randn(Bc, H, 2, E, generator=gen).to(dtype)
    assert cache.lengths.tolist() == [0] * Bc and torch.equal(cache.attend(q), torch.zeros_like(q))


# ---- the point of the feature ---------------------------------------------------------------------------------------------------------------
def _ulp(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """One unit in the last place of `dtype` at |x| (float64)."""
    mant = 8 if dtype == torch.bfloat16 else 11
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0**-126))) - (mant - 1))


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_every_row_keeps_its_own_resolution_and_a_per_tensor_cache_does_not(dtype, bits):
    """Rows x_r = 2^(e_r) u_r, e_r cycling over -6 .. 6, u_r uniform in [-1, 1]. In the token cache every element's reconstruction error
    is at most one step of ITS row, (max_r - min_r) / (2^bits - 1): half a step from rounding the code plus up to half a step from the
    rounded offset; one ulp of the data dtype at |x| on top (the dequantized value is rounded to the dtype). A static per-tensor cache
    calibrated on the whole tensor's min / max breaks that bound on the smallest rows."""
    Bc, HKV, S, E = 2, 2, 26, 64
    gen = torch.Generator().manual_seed(bits)
    expo = (torch.arange(Bc * HKV * S) % 13 - 6).reshape(Bc, HKV, S, 1).double()
    x = (torch.exp2(expo) * (torch.rand(Bc, HKV, S, E, generator=gen, dtype=torch.float64) * 2 - 1)).to(dtype)
    step = (x.double().amax(-1, keepdim=True) - x.double().amin(-1, keepdim=True)) / (2**bits - 1)
    bound = step + _ulp(x.double(), dtype)
    cache = ff.nn.DynamicQuantizedKVCache(Bc, HKV, S, E, cases.quantizer(bits), cases.quantizer(bits, tile=True), dtype, "cpu")
    cache.append(x, x)
    for got in (cache.keys(S).dequantize(), cache.values(S).dequantize()):
        assert bool(((got.double() - x.double()).abs() <= bound).all())
    static = ff.nn.LinearQuantizer(bits, symmetric=False, granularity=ff.PerTensor(), quantized_dtype=torch.int8)
    static.quantization_range = (x.float().min(), x.float().max())
    per_tensor = ff.nn.QuantizedKVCache(Bc, HKV, S, E, static, static, dtype, "cpu")
    per_tensor.append(x, x)
    err = (per_tensor.keys(S).dequantize().detach().double() - x.double()).abs()
    smallest = (expo == -6).expand_as(err)
    assert bool((err > bound)[smallest].any()) and float(err[smallest].max()) > 4 * float(bound[smallest].max())


# ---- the re-expression helper ----------------------------------------------------------------------------------------------------------------
def test_every_variant_dequantizes_to_the_identical_fp32_value():
    gen = torch.Generator().manual_seed(3)
    for s, o in ((2.0**-5, 0.0), (2.0**-3, 200.0), (1.0, -200.0), (2.0**-7, 37.0)):
        codes = torch.randint(-31, 32, (cases.B, cases.HKV, cases.S_MAX, 64), generator=gen).to(torch.int8)
        new, scale, offset, took = cases.reexpress(codes, s, o, gen)
        want = (codes.float() + o) * s
        got = (new.float() + offset.unsqueeze(-1)) * scale.unsqueeze(-1)      # the kernel's two fp32 steps
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        biased = ((new.float() + 128.0) + (offset.unsqueeze(-1) - 128.0)) * scale.unsqueeze(-1)  # ... as dequant4 takes them
        assert torch.equal(biased.view(torch.int32), want.view(torch.int32))
        assert torch.equal(offset, offset.round()) and set(took.unique().tolist()) == set(range(7))  # codes in [-31, 31]: every variant fits
        assert float((took != 0).float().mean()) >= 0.5
        for dtype in cases.DTYPES:
            assert torch.equal(cases.dequant64(new, cases.pack(scale, offset, scale, offset), 0, dtype), want.to(dtype).double())


@pytest.mark.parametrize("lens", cases.LENS_SETS)
def test_every_k_row_of_the_exact_cases_takes_a_shift(lens):
    """kv_cache_cases.exact_case: all 770 / 2148 K rows inside the two length sets allow d = +-5; V rows whose codes span too much of
    int8 keep the identity."""
    inside = torch.zeros(cases.B, cases.HKV, cases.S_MAX, dtype=torch.bool)
    for b, n in enumerate(lens):
        inside[b, :, :dense_cases.clamp_len(n)] = True
    assert int(inside.sum()) == {cases.LENS_SETS[0]: 770, cases.LENS_SETS[1]: 2148}[lens]
    for kind, causal in (("select", False), ("staircase", True), ("uniform", False)):
        for E in cases.ES:
            q, kc, vc, k_param, v_param, expected = dense_cases.exact_case(kind, causal, 4, 4, E, torch.bfloat16, lens)
            new, scale, offset, shifted = cases.shift_rows(kc, *k_param)
            assert bool(shifted[inside].all()) and bool((new[inside] != kc[inside]).all())
            assert torch.equal((new.float() + offset.unsqueeze(-1)) * scale.unsqueeze(-1), (kc.float() + k_param[1]) * k_param[0])
            _, _, _, v_shifted = cases.shift_rows(vc, *v_param)
            assert kind == "uniform" or not bool(v_shifted[inside].all())


# ---- what hipcc emitted -----------------------------------------------------------------------------------------------------------------
def test_the_token_kernels_spill_nothing_and_keep_the_dense_kernels_lds():
    if kernel_resources.readelf() is None:
        pytest.skip("llvm-readelf is missing")
    assert kernel_resources.DEFAULT_LIBRARY.exists(), "build() leaves the HIP library in the tree"
    rows = kernel_resources.kernel_resources()
    partial = [k for k in rows if "kv_token_partial_kernel" in str(k["name"])]
    store = [k for k in rows if "kv_token_store_kernel" in str(k["name"])]
    assert len(partial) == 4 and len(store) == 4, (len(partial), len(store))  # E 64 / 128 x bf16 / fp16; bf16 / fp16 x plain / rotary
    bad = {str(k["name"]): k for k in partial + store if k["vgpr_spill_count"] or k["sgpr_spill_count"] or k["private_segment_fixed_size"]}
    assert not bad, bad
    want = {"Li64E": 25600, "Li128E": 50176}  # the dense partial kernels' LDS (docs/kernels.md)
    for k in partial:
        assert k["group_segment_fixed_size"] == want[next(tag for tag in want if tag in str(k["name"]))], k
    assert all(k["group_segment_fixed_size"] == 0 for k in store)
    # the names the other kernels are counted by still count those kernels alone
    for name, count in (("sdpa_decode_partial_kernel", 4), ("sdpa_decode_combine_kernel", 2), ("kv_append", 4), ("kv_paged_partial_kernel", 4),
                        ("kv_paged_store_kernel", 4)):
        assert len([k for k in rows if name in str(k["name"])]) == count, name
