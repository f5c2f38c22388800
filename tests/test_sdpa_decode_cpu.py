"""Attention for a short query over int8 K / V codes without a GPU: every accept and decline of the predicate, the sixth header
``include/ffq_sdpa_decode.h`` against ``_cabi.SIGNATURES_DECODE`` (exported by the HIP library, absent from the oracle, the other
tables untouched), every argument error of the entry point in the documented order before any device call, the split plan (the
Python restatement against the C query; every key in exactly one split), the workspace formula, the host math path against the
reference's outputs (fixture G31) and what hipcc emitted for the new kernels."""

import ctypes
import itertools
import re
import sys

import pytest
import torch

import fastforward_amd as ff

from conftest import HIP_SO, ROOT, golden, load_oracle
from fastforward_amd import _cabi, dispatcher, fused_sdpa, fused_sdpa_decode, ops
from fastforward_amd._cabi import DType, FFQLibrary, Status
from fastforward_amd.exceptions import BackendError
from fastforward_amd.nn.quantizer import QuantizerStub
from fastforward_amd.nn.sdpa import scaled_dot_product_attention_math
from fastforward_amd.ops import decode
from fastforward_amd.quantization.affine import static

sys.path.insert(0, str(ROOT / "tools"))

import kernel_resources  # noqa: E402

F = ff.nn.functional
ENTRIES = {"ffq_sdpa_decode", "ffq_sdpa_decode_splits", "ffq_sdpa_decode_workspace_bytes"}
G31 = golden("g31_sdpa_decode.pt")


# ---- operands (shared with the GPU tests) -----------------------------------------------------------------------------------------------
def as_codes(codes, scale, offset, dtype, device="cpu", bits=8):
    """`codes` (an integer tensor, or value-dtype codes) as a per-tensor QuantizedTensor that dequantizes to `dtype`."""
    scale = torch.tensor([scale], dtype=torch.float32, device=device)
    offset = None if offset is None else torch.tensor([offset], dtype=torch.float32, device=device)
    context = static.quantization_context(scale, offset, num_bits=bits, output_dtype=codes.dtype, dequantize_dtype=dtype)
    return ff.QuantizedTensor(codes.to(device), context)


def random_codes(shape, scale=2.0**-5, offset=3.0, dtype=torch.bfloat16, device="cpu", seed=0, container=torch.int8):
    c = torch.randint(-128, 128, shape, generator=torch.Generator().manual_seed(seed)).to(container)
    return as_codes(c, scale, offset, dtype, device)


def linear_quantizer(spec, device="cpu", container=None):
    bits, scale, offset = spec
    q = ff.nn.LinearQuantizer(bits, symmetric=False, granularity=ff.PerTensor(), quantized_dtype=container, device=device)
    q.quantization_range = (torch.tensor(-1.0, device=device), torch.tensor(1.0, device=device))
    with torch.no_grad():
        q.scale.fill_(scale)
        q.offset.fill_(offset)
    return q


def run_g31(case, device="cpu", fn=None):
    """The case's call through `fn` (default: ``ff.nn.functional.scaled_dot_product_attention``) on `device`."""
    fn = fn or F.scaled_dot_product_attention
    with torch.no_grad():
        q, k, v = (case[n].to(device) for n in "qkv")
        if case["q_spec"] is not None:
            q = linear_quantizer(case["q_spec"], device, case["q_container"])(q)
        kq = linear_quantizer(case["k_spec"], device, torch.int8)(k)
        vq = linear_quantizer(case["v_spec"], device, torch.int8)(v)
        extra = {} if case["out_spec"] is None else dict(output_quantizer=linear_quantizer(case["out_spec"], device))
        mask = None if case["mask"] is None else case["mask"].to(device)
        H, HKV = case["q"].shape[1], case["k"].shape[1]
        out = fn(q, kq, vq, attn_mask=mask, enable_gqa=H != HKV, strict_quantization=False, **case["kwargs"], **extra)
        return out.dequantize() if isinstance(out, ff.QuantizedTensor) else out


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
def test_the_functions_exist_and_the_registration_stands_in_front():
    assert {"sdpa_decode", "sdpa_decode_plan"} <= set(ops.__all__) and callable(ops.sdpa_decode) and callable(ops.sdpa_decode_plan)
    fns = [it.fn for it in dispatcher._DISPATCHER["scaled_dot_product_attention"]]
    assert fused_sdpa_decode.KERNELS.sdpa in fns and fused_sdpa.KERNELS.sdpa in fns and scaled_dot_product_attention_math in fns
    assert fns.index(fused_sdpa_decode.KERNELS.sdpa) < fns.index(scaled_dot_product_attention_math)
    assert fns.index(fused_sdpa.KERNELS.sdpa) < fns.index(scaled_dot_product_attention_math)
    doc = " ".join(F.__doc__.split())
    assert "ffq_sdpa_decode" in doc or "sdpa_decode" in doc


# ---- the predicate ----------------------------------------------------------------------------------------------------------------------
def test_the_predicate_accepts_and_declines(monkeypatch):
    B, H, HKV, L, S, E = 2, 8, 2, 1, 70, 64
    bf, hf = torch.bfloat16, torch.float16
    q = torch.randn(B, H, L, E).to(bf)
    k, v = random_codes((B, HKV, S, E), seed=1), random_codes((B, HKV, S, E), scale=0.03, offset=-200.0, seed=2)
    common = dict(enable_gqa=True, strict_quantization=False)
    assert not fused_sdpa_decode.sdpa_decode_predicate(query=q, key=k, value=v, **common)                           # host tensors
    monkeypatch.setattr("fastforward_amd.fused_sdpa_decode._on_device", lambda *t: True)
    oq = linear_quantizer((8, 2.0**-5, 0.0))

    def ok(**kw):
        with torch.no_grad():
            return fused_sdpa_decode.KERNELS.supported(**{**dict(query=q, key=k, value=v), **common, **kw})

    # accepted
    assert ok() and ok(output_quantizer=oq) and ok(output_quantizer=QuantizerStub()) and ok(attn_weights_quantizer=QuantizerStub())
    assert ok(output_quantizer=linear_quantizer((4, 0.1, 1.0))) and ok(scale=0.3) and ok(neg_inf=float("-inf")) and ok(dropout_p=0)
    assert ok(query=random_codes((B, H, L, E), seed=3)) and ok(query=random_codes((B, H, L, E), container=bf, seed=3))   # q codes, either container
    assert ok(query=q.half(), key=random_codes((B, HKV, S, E), dtype=hf), value=random_codes((B, HKV, S, E), dtype=hf))
    assert ok(query=torch.randn(B, HKV, 32, E).to(bf), enable_gqa=False) and ok(query=torch.randn(B, 4, 16, E).to(bf))  # 32 rows
    assert ok(query=torch.randn(B, 2, 1, 128).to(bf), key=random_codes((B, 2, 5, 128)), value=random_codes((B, 2, 5, 128)))
    assert ok(key=random_codes((B, HKV, 1, E)), value=random_codes((B, HKV, 1, E)))                                  # S = 1
    assert ok(key=as_codes(torch.randint(-8, 8, (B, HKV, S, E)).to(torch.int8), 0.1, None, bf, bits=4), value=v)    # 4 bits, no offset
    for mask in (torch.rand(L, S) > 0.5, torch.randn(L, S), torch.randn(1, 1, L, S).to(bf), torch.randn(B, 1, L, S), torch.randn(B, H, L, S),
                 torch.randn(1, H, L, S)):
        assert ok(attn_mask=mask), mask.shape
    assert ok(query=torch.randn(B, H, 4, E).to(bf), is_causal=True)
    kt = random_codes((B, S, HKV, E), seed=4)                                                                        # the projection's layout, seen transposed
    assert ok(key=as_codes(kt.raw_data.transpose(1, 2), 2.0**-5, 3.0, bf), value=v)
    longer = torch.randint(-128, 128, (B, HKV, S + 30, E)).to(torch.int8)
    assert ok(key=as_codes(longer[:, :, :S], 2.0**-5, 3.0, bf), value=v)                                             # a slice of a longer buffer
    # the call
    assert not ok(strict_quantization=True) and not ok(strict_quantization=None) and not ok(dropout_p=0.1) and not ok(dropout_p="0")
    assert not ok(some_other_quantizer=oq) and not fused_sdpa_decode.KERNELS.supported(q, k, v, None, 0.0, False, None, True, 1, strict_quantization=False)
    assert not ok(neg_inf=-1e4) and not ok(neg_inf=float("inf")) and not ok(neg_inf=None) and not ok(scale="1") and not ok(is_causal=1) and not ok(enable_gqa=1)
    with ff.sdpa_upcast(False):
        assert not ok()
    with ff.sdpa_upcast(torch.float64):
        assert not ok()
    # K and V
    assert not ok(key=k.dequantize()) and not ok(value=v.dequantize()) and not ok(key=k.dequantize(), value=v.dequantize())
    assert not ok(value=random_codes((B, HKV, S, E), container=bf))                                                  # V codes in a bf16 container
    assert not ok(key=random_codes((B, HKV, S, E), container=bf), value=random_codes((B, HKV, S, E), container=bf))  # fused_sdpa's call
    assert not ok(key=random_codes((B, HKV, S, E), dtype=hf))                                                        # K fp16, V bf16
    assert not ok(key=random_codes((B, HKV, S, E), dtype=torch.float32), value=random_codes((B, HKV, S, E), dtype=torch.float32))
    pc = ff.nn.LinearQuantizer(8, granularity=ff.PerChannel(1), quantized_dtype=torch.int8)
    pc.quantization_range = (torch.full((HKV,), -3.0), torch.full((HKV,), 3.0))
    with torch.no_grad():
        assert not ok(key=pc(torch.randn(B, HKV, S, E).to(bf)))                                                      # per-channel K codes
    wide = as_codes(torch.randint(-128, 128, (B, HKV, S, E)).to(torch.int16), 0.01, None, bf, bits=16)
    assert not ok(key=wide)
    half_scale = static.quantization_context(torch.tensor([0.1], dtype=bf), None, num_bits=8, output_dtype=torch.int8, dequantize_dtype=bf)
    assert not ok(key=ff.QuantizedTensor(k.raw_data, half_scale))                                                    # parameters that are not fp32
    # Q
    assert not ok(query=q.half()) and not ok(query=q.float()) and not ok(query=random_codes((B, H, L, E), dtype=hf)) and not ok(query=None)
    # shapes
    assert not ok(query=q[0]) and not ok(key=as_codes(k.raw_data[0], 2.0**-5, 3.0, bf)) and not ok(enable_gqa=False) and not ok(query=torch.randn(B, 3, L, E).to(bf))
    assert not ok(query=torch.randn(B, H, 9, E).to(bf)) and not ok(query=torch.randn(B, HKV, 33, E).to(bf), enable_gqa=False)   # 36 and 33 rows
    assert not ok(query=torch.randn(B, H, L, 96).to(bf), key=random_codes((B, HKV, S, 96)), value=random_codes((B, HKV, S, 96)))
    assert not ok(query=torch.randn(B, H, L, 32).to(bf), key=random_codes((B, HKV, S, 32)), value=random_codes((B, HKV, S, 32)))
    assert not ok(value=random_codes((B, HKV, S + 1, E))) and not ok(value=random_codes((B, HKV, S, 128))) and not ok(query=torch.randn(1, H, L, E).to(bf))
    assert not ok(key=random_codes((B, HKV, 0, E)), value=random_codes((B, HKV, 0, E)))
    # layouts
    flat = torch.randint(-128, 128, (B * HKV * S * E + 16,)).to(torch.int8)
    assert not ok(key=as_codes(flat[8:8 + B * HKV * S * E].view(B, HKV, S, E), 2.0**-5, 3.0, bf))                    # a misaligned pointer
    assert ok(key=as_codes(flat[16:].view(B, HKV, S, E), 2.0**-5, 3.0, bf))                                          # offset by 16 bytes
    assert not ok(key=as_codes(torch.randint(-128, 128, (B, HKV, E, S)).to(torch.int8).transpose(2, 3), 2.0**-5, 3.0, bf))   # last dim strided
    assert not ok(key=as_codes(torch.randint(-128, 128, (B, HKV, S, E + 8)).to(torch.int8)[..., :E], 2.0**-5, 3.0, bf))     # rows 72 bytes apart
    # masks
    assert not ok(attn_mask=torch.randn(L, S), is_causal=True) and not ok(attn_mask=torch.randn(L, S + 1)) and not ok(attn_mask=torch.randn(3, H, L, S))
    assert not ok(attn_mask=torch.randn(L, S).double()) and not ok(attn_mask=torch.randn(L, S).half()) and not ok(attn_mask=torch.ones(L, S, dtype=torch.int32))
    assert not ok(attn_mask=torch.randn(S)) and not ok(attn_mask=torch.randn(1, B, H, L, S)) and not ok(attn_mask=as_codes(torch.zeros(L, S, dtype=torch.int8), 1.0, None, bf))
    # quantizers
    for name in ("attn_scores_quantizer", "attn_mask_quantizer", "masked_scores_quantizer", "attn_weights_quantizer", "scaled_query_quantizer",
                 "scaled_key_quantizer", "dropout_quantizer"):
        assert not ok(**{name: oq}), name
    assert not ok(output_quantizer=linear_quantizer((16, 0.1, 0.0)))
    per_channel = ff.nn.LinearQuantizer(8, granularity=ff.PerChannel(1))
    per_channel.quantization_range = (torch.full((H,), -1.0), torch.full((H,), 1.0))
    assert not ok(output_quantizer=per_channel) and not ok(output_quantizer=ff.nn.LinearQuantizer(8))               # not one _requant fuses; not initialised
    with ff.estimate_ranges(oq, ff.range_setting.running_minmax):
        assert not ok(output_quantizer=oq)
    # gradients
    with torch.enable_grad():
        assert fused_sdpa_decode.KERNELS.supported(query=q, key=k, value=v, **common)
        assert not fused_sdpa_decode.KERNELS.supported(query=q.clone().requires_grad_(), key=k, value=v, **common)
    # a library without the symbol
    monkeypatch.setattr(fused_sdpa_decode._native.library(), "ffq_sdpa_decode", None, raising=False)
    assert not ok()


def test_the_existing_route_is_untouched(monkeypatch):
    """What ``fused_sdpa`` serves is declined here, and what is served here is declined there: no call changes its route."""
    monkeypatch.setattr("fastforward_amd.fused_sdpa_decode._on_device", lambda *t: True)
    monkeypatch.setattr("fastforward_amd.fused_sdpa._on_device", lambda *t: True)
    bf = torch.bfloat16
    q = torch.randn(1, 2, 1, 64).to(bf)
    plain = (q, torch.randn(1, 2, 9, 64).to(bf), torch.randn(1, 2, 9, 64).to(bf))
    held = (q, random_codes((1, 2, 9, 64), container=bf), random_codes((1, 2, 9, 64), container=bf))
    cached = (q, random_codes((1, 2, 9, 64)), random_codes((1, 2, 9, 64)))
    with torch.no_grad():
        for operands, old, new in ((plain, True, False), (held, True, False), (cached, False, True)):
            kw = dict(zip(("query", "key", "value"), operands), strict_quantization=False)
            assert fused_sdpa.KERNELS.supported(**kw) is old and fused_sdpa_decode.KERNELS.supported(**kw) is new
    assert type(fused_sdpa.KERNELS) is fused_sdpa.SdpaKernels and "supported" in vars(fused_sdpa_decode.SdpaDecodeKernels)


def test_the_wrapper_says_not_covered_on_a_library_without_the_symbol(oracle_backend):
    q, k = torch.zeros(1, 2, 1, 64, dtype=torch.bfloat16), torch.zeros(1, 2, 5, 64, dtype=torch.int8)
    one = (torch.ones(1), None)
    with pytest.raises(BackendError, match="does not export ffq_sdpa_decode"):
        ops.sdpa_decode(q, k, k, dequant=(None, one, one))


def wrapper_refusals():
    """The calls ``ops.sdpa_decode`` refuses on host tensors, ahead of any library call (tests/golden/gen_decode_refusals.py records
    their texts from the same list)."""
    bf = torch.bfloat16
    q, k = torch.zeros(1, 2, 1, 64, dtype=bf), torch.zeros(1, 2, 5, 64, dtype=torch.int8)
    one = (torch.ones(1), None)
    return [lambda: ops.sdpa_decode(q, k, k), lambda: ops.sdpa_decode(q, k.to(bf), k, dequant=(None, one, one)), lambda: ops.sdpa_decode(q[0], k, k, dequant=(None, one, one)),
            lambda: ops.sdpa_decode(q.float(), k, k, dequant=(None, one, one)), lambda: ops.sdpa_decode(q.to(torch.int8), k, k, dequant=(None, one, one), dtype=bf),
            lambda: ops.sdpa_decode(torch.zeros(1, 2, 17, 64, dtype=bf), k, k, dequant=(None, one, one), splits=65),
            lambda: ops.sdpa_decode(torch.zeros(1, 2, 33, 64, dtype=bf), k, k, dequant=(None, one, one)),
            lambda: ops.sdpa_decode(torch.zeros(1, 3, 1, 64, dtype=bf), k, k, dequant=(None, one, one)),
            lambda: ops.sdpa_decode(q, k, k[:, :, :4], dequant=(None, one, one)), lambda: ops.sdpa_decode(q, k, k, dequant=(None, one, one), splits=-1),
            lambda: ops.sdpa_decode(q, k, k, dequant=(None, one, one), attn_mask=torch.zeros(1, 4)),
            lambda: ops.sdpa_decode(q, k, k, dequant=(None, one, one), attn_mask=torch.zeros(1, 5, dtype=torch.int32))]


def causal_with_a_mask():
    q, k = torch.zeros(1, 2, 1, 64, dtype=torch.bfloat16), torch.zeros(1, 2, 5, 64, dtype=torch.int8)
    one = (torch.ones(1), None)
    return ops.sdpa_decode(q, k, k, dequant=(None, one, one), attn_mask=torch.zeros(1, 5), is_causal=True)


def test_the_wrapper_checks_its_operands_and_refuses_host_tensors():
    q, k = torch.zeros(1, 2, 1, 64, dtype=torch.bfloat16), torch.zeros(1, 2, 5, 64, dtype=torch.int8)
    one = (torch.ones(1), None)
    with pytest.raises(BackendError, match="HIP device only"):
        ops.sdpa_decode(q, k, k, dequant=(None, one, one))
    for call in wrapper_refusals():
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(ValueError, match="is_causal"):
        causal_with_a_mask()


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
def _header(name):
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / name).read_text(), flags=re.S)


def _declared(name):
    return set(re.findall(r"\b(ffq_[a-z0-9_]+)\s*\(", _header(name)))


def test_the_sixth_header_and_its_table_agree():
    assert _declared("ffq_sdpa_decode.h") == set(_cabi.SIGNATURES_DECODE) == ENTRIES
    text = (ROOT / "include" / "ffq_sdpa_decode.h").read_text()
    assert '#include "ffq.h"' in text
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
    results = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t}
    want_names = {
        "ffq_sdpa_decode_splits": ["batch", "kv_heads", "S", "rows", "E"],
        "ffq_sdpa_decode_workspace_bytes": ["batch", "kv_heads", "rows", "E", "splits"],
        "ffq_sdpa_decode": ["q", "q_dt", "k", "v", "dt", "deq_scale", "deq_offset", "batch", "q_heads", "kv_heads", "L", "S", "E", "strides", "mask",
                            "mask_kind", "mask_dt", "mask_strides", "sqrt_scale", "out_scale", "out_offset", "out_num_bits", "splits", "out", "workspace",
                            "workspace_bytes", "stream"],
    }
    for entry in ENTRIES:
        m = re.search(r"(\w+)\s+" + entry + r"\s*\((.*?)\)\s*;", _header("ffq_sdpa_decode.h"), flags=re.S)
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
        restype, argtypes = _cabi.SIGNATURES_DECODE[entry]
        assert restype is results[m.group(1)] and argtypes == want and names == want_names[entry], entry
    for name, value in (("MAX_ROWS", _cabi.SDPA_DECODE_MAX_ROWS), ("KEY_TILE", _cabi.SDPA_DECODE_KEY_TILE), ("MAX_SPLITS", _cabi.SDPA_DECODE_MAX_SPLITS)):
        assert re.search(rf"#define FFQ_SDPA_DECODE_{name} {value}\b", text), name
    assert (decode.MAX_ROWS, decode.KEY_TILE, decode.MAX_SPLITS) == (32, 128, 64)


def test_the_other_tables_are_untouched_and_disjoint():
    assert _declared("ffq.h") == set(_cabi.SIGNATURES) and _declared("ffq_3d.h") == set(_cabi.SIGNATURES_3D)
    assert _declared("ffq_depthwise.h") == set(_cabi.SIGNATURES_DEPTHWISE) and _declared("ffq_index.h") == set(_cabi.SIGNATURES_INDEX)
    assert _declared("ffq_unfold.h") == set(_cabi.SIGNATURES_UNFOLD)
    mine = set(_cabi.SIGNATURES_DECODE)
    for other in (_cabi.SIGNATURES, _cabi.SIGNATURES_3D, _cabi.SIGNATURES_DEPTHWISE, _cabi.SIGNATURES_INDEX, _cabi.SIGNATURES_UNFOLD, _cabi.DEVICE_ONLY):
        assert not mine & set(other)
    assert _cabi.FFQ_ABI_VERSION == 9 and "#define FFQ_ABI_VERSION 9" in (ROOT / "include" / "ffq.h").read_text()


def test_the_hip_library_exports_them_and_the_oracle_loads_without_them():
    dll, lib, oracle = ctypes.CDLL(str(HIP_SO)), FFQLibrary(HIP_SO), load_oracle()
    for entry in ENTRIES:
        assert hasattr(dll, entry) and getattr(lib, entry) is not None
        assert not oracle.is_device and getattr(oracle, entry) is None


FAKE = 1 << 20  # never dereferenced: every call below returns from the argument checks
BF16, F16, I8, F32, F64 = (int(t) for t in (DType.BF16, DType.F16, DType.I8, DType.F32, DType.F64))


def _table(*values):
    return (ctypes.c_void_p * 3)(*values)


def _call(lib, q=FAKE, q_dt=BF16, k=FAKE, v=FAKE, dt=BF16, deq_s=(None, FAKE, FAKE), deq_o=(None, None, None), B=2, H=8, HKV=2, L=1, S=300, E=128,
          strides="dense", mask=None, mask_kind=0, mask_dt=F32, mask_strides=None, sqrt_scale=0.3, out_s=None, out_o=None, bits=8.0, splits=0, out=FAKE,
          ws=FAKE, ws_bytes=None):
    if strides == "dense":
        strides = (H * L * E, L * E, E, HKV * S * E, S * E, E, HKV * S * E, S * E, E)
    if ws_bytes is None:
        count = splits or lib.ffq_sdpa_decode_splits(B, HKV, S, L * (H // HKV if HKV > 0 else 1), E)
        ws_bytes = lib.ffq_sdpa_decode_workspace_bytes(B, HKV, L * (H // HKV if HKV > 0 else 1), E, count)
    return lib.ffq_sdpa_decode(q, q_dt, k, v, dt, None if deq_s is None else _table(*deq_s), None if deq_o is None else _table(*deq_o), B, H, HKV, L, S, E,
                               None if strides is None else (ctypes.c_int64 * 9)(*strides), mask, mask_kind, mask_dt,
                               None if mask_strides is None else (ctypes.c_int64 * 4)(*mask_strides), sqrt_scale, out_s, out_o, bits, splits, out, ws,
                               ws_bytes, None)


def _dense(H=8, HKV=2, L=1, S=300, E=128, **change):
    s = [H * L * E, L * E, E, HKV * S * E, S * E, E, HKV * S * E, S * E, E]
    for i, value in change.items():
        s[int(i[1:])] = value
    return tuple(s)


# in the documented order: each call fails the named check and passes every check ahead of it; most fail a LATER check too and must
# report the earlier one
ERRORS = [
    (lambda lib: _call(lib, dt=F32, q_dt=I8, deq_s=None), Status.ERR_DTYPE),                    # 1. the value dtype
    (lambda lib: _call(lib, dt=I8, q_dt=I8, E=96), Status.ERR_DTYPE),
    (lambda lib: _call(lib, q_dt=F16, strides=None), Status.ERR_DTYPE),                         # 2. q's container; before the tables
    (lambda lib: _call(lib, q_dt=F32, E=96), Status.ERR_DTYPE),
    (lambda lib: _call(lib, strides=None, E=96), Status.ERR_ARG),                               # 3. the tables; before E
    (lambda lib: _call(lib, deq_s=None, q_dt=I8), Status.ERR_ARG),
    (lambda lib: _call(lib, deq_o=None, L=-1), Status.ERR_ARG),
    (lambda lib: _call(lib, q_dt=I8, deq_s=(None, None, FAKE)), Status.ERR_DTYPE),              # 4. int8 q codes without a scale; before k / v
    (lambda lib: _call(lib, deq_s=(None, None, FAKE), E=96), Status.ERR_ARG),                   # 5. k or v without a scale; before E
    (lambda lib: _call(lib, deq_s=(FAKE, FAKE, None), B=-1), Status.ERR_ARG),
    (lambda lib: _call(lib, E=96, B=-1), Status.ERR_ARG),                                       # 6. E
    (lambda lib: _call(lib, E=32), Status.ERR_ARG),
    (lambda lib: _call(lib, E=256, L=40), Status.ERR_ARG),
    (lambda lib: _call(lib, B=-1, L=40), Status.ERR_ARG),                                       # 7. the extents; before the rows
    (lambda lib: _call(lib, L=-1, mask_kind=7), Status.ERR_ARG),
    (lambda lib: _call(lib, S=-1, mask_kind=7), Status.ERR_ARG),
    (lambda lib: _call(lib, H=0, mask_kind=7), Status.ERR_ARG),
    (lambda lib: _call(lib, HKV=0, mask_kind=7), Status.ERR_ARG),
    (lambda lib: _call(lib, H=7, HKV=2, mask_kind=7), Status.ERR_ARG),
    (lambda lib: _call(lib, L=33, H=2, mask_kind=3, mask_dt=F64, ws_bytes=0), Status.ERR_ARG),  # 8. the rows; before the mask (ERR_DTYPE)
    (lambda lib: _call(lib, L=9, mask_kind=3, mask_dt=F64, ws_bytes=0), Status.ERR_ARG),        #    9 * 4 = 36
    (lambda lib: _call(lib, L=1 << 40, H=2, mask_kind=3, mask_dt=F64, ws_bytes=0), Status.ERR_ARG),   # no int64 overflow on the way
    (lambda lib: _call(lib, mask_kind=4, mask_dt=F64), Status.ERR_ARG),                         # 9. the mask kind; before its dtype
    (lambda lib: _call(lib, mask_kind=-1), Status.ERR_ARG),
    (lambda lib: _call(lib, mask_kind=3, mask_dt=F64, out_o=FAKE), Status.ERR_DTYPE),           # 10. the float mask's dtype; before the quantizer
    (lambda lib: _call(lib, mask_kind=3, mask_dt=I8, splits=65), Status.ERR_DTYPE),
    (lambda lib: _call(lib, out_o=FAKE, splits=65), Status.ERR_ARG),                            # 11. the output quantizer; before the splits
    (lambda lib: _call(lib, out_s=FAKE, bits=9.0, splits=65), Status.ERR_ARG),
    (lambda lib: _call(lib, out_s=FAKE, bits=0.0), Status.ERR_ARG),
    (lambda lib: _call(lib, out_s=FAKE, bits=3.5), Status.ERR_ARG),
    (lambda lib: _call(lib, splits=65, S=0, ws_bytes=0), Status.ERR_ARG),                       # 12. the splits
    (lambda lib: _call(lib, splits=-1, ws_bytes=0), Status.ERR_ARG),
    (lambda lib: _call(lib, B=0, S=0, q=None, out=None, ws=None), Status.OK),                   # 13. empty: nothing launched (before S == 0, NULL buffers)
    (lambda lib: _call(lib, L=0, S=0, q=None, out=None, ws=None, ws_bytes=0), Status.OK),
    (lambda lib: _call(lib, S=0, q=None, ws_bytes=0), Status.ERR_ARG),                          # 14. S == 0; before the buffers
    (lambda lib: _call(lib, S=1 << 30, q=None, ws_bytes=0), Status.ERR_ARG),                    # 15. the sizes
    (lambda lib: _call(lib, B=1 << 23, q=None, ws_bytes=0), Status.ERR_ARG),
    (lambda lib: _call(lib, q=None, ws=None), Status.ERR_ARG),                                  # 16. NULL buffers; before the workspace
    (lambda lib: _call(lib, k=None, ws=None), Status.ERR_ARG),
    (lambda lib: _call(lib, v=None, ws=None), Status.ERR_ARG),
    (lambda lib: _call(lib, out=None, ws=None), Status.ERR_ARG),
    (lambda lib: _call(lib, mask_kind=2, mask=None, q=FAKE + 8), Status.ERR_ARG),               # 17. the mask's data and strides; before alignment
    (lambda lib: _call(lib, mask_kind=3, mask=FAKE, mask_strides=None, ws=None), Status.ERR_ARG),
    (lambda lib: _call(lib, q=FAKE + 8, ws=None), Status.ERR_ARG),                              # 18. alignment; before the workspace
    (lambda lib: _call(lib, k=FAKE + 4, ws=None), Status.ERR_ARG),
    (lambda lib: _call(lib, v=FAKE + 1, ws=None), Status.ERR_ARG),
    (lambda lib: _call(lib, out=FAKE + 2, ws=None), Status.ERR_ARG),
    (lambda lib: _call(lib, strides=_dense(s2=-128), ws=None), Status.ERR_ARG),                 # 19. the strides; before the workspace
    (lambda lib: _call(lib, strides=_dense(s2=132), ws=None), Status.ERR_ARG),                  #     bf16 rows 264 bytes apart
    (lambda lib: _call(lib, strides=_dense(s5=136), ws=None), Status.ERR_ARG),                  #     int8 rows 136 bytes apart (a multiple of 8, not of 16)
    (lambda lib: _call(lib, strides=_dense(s8=8), ws=None), Status.ERR_ARG),
    (lambda lib: _call(lib, q_dt=I8, deq_s=(FAKE, FAKE, FAKE), strides=_dense(s2=136), ws=None), Status.ERR_ARG),   # int8 q rows
    (lambda lib: _call(lib, ws=None), Status.ERR_WORKSPACE),                                    # 20. the workspace
    (lambda lib: _call(lib, ws=FAKE + 8), Status.ERR_WORKSPACE),
    (lambda lib: _call(lib, ws_bytes=0), Status.ERR_WORKSPACE),
    (lambda lib: _call(lib, splits=3, ws_bytes=decode.sdpa_decode_workspace_bytes(2, 2, 4, 128, 3) - 1), Status.ERR_WORKSPACE),
    (lambda lib: _call(lib, splits=64, ws_bytes=decode.sdpa_decode_workspace_bytes(2, 2, 4, 128, 63)), Status.ERR_WORKSPACE),
]


@pytest.mark.parametrize("index", range(len(ERRORS)))
def test_argument_checks_need_no_device(index):
    call, status = ERRORS[index]
    lib = FFQLibrary(HIP_SO)
    assert call(lib) == status
    if status != Status.OK:
        assert lib.ffq_last_error()


# ---- the split plan and the workspace ---------------------------------------------------------------------------------------------------
PLAN_GRID = list(itertools.product((1, 2, 3, 8, 64, 300), (1, 2, 8, 32), (1, 2, 63, 127, 128, 129, 255, 256, 257, 1000, 4096, 8192, 32768, 100001, 2**20 + 5)))


def test_the_plan_is_the_c_query_and_covers_every_key_once():
    lib = FFQLibrary(HIP_SO)
    for (B, HKV, S), rows, E in zip(PLAN_GRID, itertools.cycle((1, 4, 8, 32)), itertools.cycle((64, 128))):
        splits = ops.sdpa_decode_plan(B, HKV, S, rows, E)
        assert splits == lib.ffq_sdpa_decode_splits(B, HKV, S, rows, E), (B, HKV, S)
        assert 1 <= splits <= decode.MAX_SPLITS
        ranges = decode.sdpa_decode_split_ranges(S, splits)
        assert ranges[0][0] == 0 and ranges[-1][1] == S and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))   # every key in exactly one split
        assert all((end - begin) % decode.KEY_TILE == 0 for begin, end in ranges[:-1])                             # whole tiles but for the last
        assert all(end > begin for begin, end in ranges)                                                            # none is empty
    # what the rule is for: enough workgroups for the chip where the keys allow it, one split where they do not
    assert ops.sdpa_decode_plan(1, 8, 32768) == 32 and ops.sdpa_decode_plan(8, 8, 8192) == 4 and ops.sdpa_decode_plan(64, 8, 8192) == 1 and ops.sdpa_decode_plan(1, 1, 2**20) == 64
    assert ops.sdpa_decode_plan(1, 1, 1) == ops.sdpa_decode_plan(1, 1, 255) == 1 and ops.sdpa_decode_plan(1, 1, 256) == 1 and ops.sdpa_decode_plan(1, 1, 512) == 2
    # a forced count may leave splits without a key, never a key without a split
    for S, forced in ((1, 3), (129, 64), (300, 2), (1000, 3), (1000, 64)):
        ranges = decode.sdpa_decode_split_ranges(S, forced)
        assert len(ranges) == forced and ranges[0][0] == 0 and ranges[-1][1] == S and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))


def test_the_workspace_formula():
    lib = FFQLibrary(HIP_SO)
    for B, HKV, rows, E, splits in itertools.product((1, 3), (1, 8), (1, 5, 32), (64, 128), (1, 7, 64)):
        want = B * HKV * splits * rows * (E + 2) * 4
        assert lib.ffq_sdpa_decode_workspace_bytes(B, HKV, rows, E, splits) == want == ops.sdpa_decode_workspace_bytes(B, HKV, rows, E, splits)
        assert want % 16 == 0 or rows * splits * B * HKV % 2  # (O comes first: its rows stay 16-byte aligned whatever the counts)
    for zero in ((0, 1, 1, 64, 1), (1, 0, 1, 64, 1), (1, 1, 0, 64, 1), (1, 1, 1, 64, 0), (-1, 1, 1, 64, 1)):
        assert lib.ffq_sdpa_decode_workspace_bytes(*zero) == 0 == ops.sdpa_decode_workspace_bytes(*zero)


# ---- the host math path against the reference (G31) -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(G31))
def test_host_path_equals_the_reference_bit_for_bit(name):
    case = G31[name]
    got = run_g31(case)
    assert type(got) is torch.Tensor and got.dtype == case["out"].dtype and got.shape == case["out"].shape
    assert torch.equal(got.view(torch.int16), case["out"].view(torch.int16))


def test_the_fixture_covers_what_it_names():
    cases = list(G31.values())
    assert len(cases) == 9 and {c["q"].shape[2] for c in cases} == {1, 4} and {c["k"].shape[2] for c in cases} == {1, 65, 300}
    assert {c["q"].shape[1] == c["k"].shape[1] for c in cases} == {True, False}                                     # MHA and GQA
    assert {None if c["mask"] is None else c["mask"].dtype == torch.bool for c in cases} == {None, True, False}
    assert {c["out_spec"] is None for c in cases} == {True, False} and {c["q"].dtype for c in cases} == {torch.bfloat16, torch.float16}
    assert any(c["q_container"] is torch.int8 for c in cases)
    assert all(c["q"].shape[2] * (c["q"].shape[1] // c["k"].shape[1]) <= decode.MAX_ROWS for c in cases)
    row = G31["bf16_L4_S300_gqa_bool_masked_row"]
    assert not bool(row["mask"][..., 2, :].any()) and not bool(row["out"][:, :, 2].any())                           # the safe softmax's zeros
    assert (ROOT / "tests" / "golden" / "g31_sdpa_decode.pt").stat().st_size < 1 << 20


# ---- what hipcc emitted -----------------------------------------------------------------------------------------------------------------
def test_the_new_kernels_spill_nothing_and_use_no_scratch():
    if kernel_resources.readelf() is None:
        pytest.skip("llvm-readelf is missing")
    assert kernel_resources.DEFAULT_LIBRARY.exists(), "build() leaves the HIP library in the tree"
    rows = kernel_resources.kernel_resources()
    partial = [k for k in rows if "sdpa_decode_partial_kernel" in str(k["name"])]
    combine = [k for k in rows if "sdpa_decode_combine_kernel" in str(k["name"])]
    assert len(partial) == 4 and len(combine) == 2, (len(partial), len(combine))  # E 64 / 128 x bf16 / fp16; bf16 / fp16
    bad = {str(k["name"]): k for k in partial + combine if k["vgpr_spill_count"] or k["sgpr_spill_count"] or k["private_segment_fixed_size"]}
    assert not bad, bad
    # the documented LDS bytes (docs/kernels.md): max(four V^T images, the three O tiles of the merge) + the waves' m and l
    want = {"Li64E": max(4 * 64 * 72, 3 * 2 * 16 * 64 * 4) + 1024, "Li128E": max(4 * 128 * 72, 3 * 4 * 16 * 64 * 4) + 1024}
    assert want == {"Li64E": 25600, "Li128E": 50176}
    for k in partial:
        key = next(tag for tag in want if tag in str(k["name"]))
        assert k["group_segment_fixed_size"] == want[key], k
    assert all(k["group_segment_fixed_size"] == 0 for k in combine)
