"""The quantized index_add and permute, and the code-level expand / unsqueeze / take_along_dim / topk, without a GPU: the functional
surface, the host path against the reference's outputs (fixture G29), the strict-mode messages in the reference's order, the
predicates on what they accept and decline, the fourth header ``include/ffq_index.h`` against ``_cabi.SIGNATURES_INDEX`` (exported by
the HIP library, absent from the oracle, the other tables untouched), every argument error of the two entry points in the
documented order before any device call, and what hipcc emitted for the new kernels."""

import ctypes
import re
import sys

import pytest
import torch

import fastforward_amd as ff

from conftest import HIP_SO, ROOT, golden, load_oracle
from fastforward_amd import _cabi, dispatcher, fused_concat, fused_conv, fused_index
from fastforward_amd._cabi import DType, FFQLibrary, Status
from fastforward_amd.exceptions import BackendError, QuantizationError

sys.path.insert(0, str(ROOT / "tools"))

import kernel_resources  # noqa: E402

F = ff.nn.functional
ENTRIES = {"ffq_index_add_quantize", "ffq_permute_quantize"}
G29 = golden("g29_index.pt")
CASES, CODE_LEVEL = G29["cases"], G29["code_level"]


# ---- the functional surface ---------------------------------------------------------------------------------------------------------
def test_the_functions_exist():
    assert "index_add" in F.__all__ and "permute" in F.__all__ and callable(F.index_add) and callable(F.permute)
    assert "index_add" in F.__doc__ and "permute" in F.__doc__
    assert {"index_add_quantize", "permute_quantize"} <= set(ff.ops.__all__)
    for op in ("index_add", "permute"):
        fns = [item.fn for item in dispatcher._DISPATCHER[op]]
        assert fns == [getattr(fused_index.KERNELS, op)]


# ---- the host path against the reference (G29) ------------------------------------------------------------------------------------
def g29_quantizer(spec, got, device="cpu"):
    bits, symmetric, gran, lo, hi = spec
    granularity = ff.PerTensor() if gran == "tensor" else ff.PerChannel(gran[1])
    q = ff.nn.LinearQuantizer(bits, symmetric=symmetric, granularity=granularity, quantized_dtype=torch.int8)
    q.quantization_range = (torch.as_tensor(lo, dtype=torch.float32), torch.as_tensor(hi, dtype=torch.float32))
    with torch.no_grad():
        q.scale.copy_(got["scale"])
        if got["offset"] is not None:
            q.offset.copy_(got["offset"])
    return q.to(device)


def run_g29(case, device="cpu", dtype=None):
    """(result without an output quantizer, result with the case's) of the case's call (shared with the GPU tests)."""
    with torch.no_grad(), ff.strict_quantization(False):
        args = []
        for x, slot, got in zip(case["inputs"], case["slots"], case["params"]):
            x = x.to(device, dtype or x.dtype)
            args.append(x if slot is None else g29_quantizer(slot, got, device)(x))
        oq = g29_quantizer(case["out_slot"], case["out_params"], device)
        if case["op"] == "index_add":
            call = lambda **k: F.index_add(args[0], case["kwargs"]["dim"], case["index"].to(device), args[1], alpha=case["kwargs"]["alpha"], **k)  # noqa: E731
        else:
            call = lambda **k: F.permute(args[0], case["kwargs"]["dims"], **k)  # noqa: E731
        return call(), call(output_quantizer=oq)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same_as_recorded(got, want):
    if want["type"] == "Tensor":
        assert type(got) is torch.Tensor and got.dtype == want["value"].dtype and got.shape == want["value"].shape
        assert torch.equal(_bits(got), _bits(want["value"]))
    else:
        assert isinstance(got, ff.QuantizedTensor) and torch.equal(got.raw_data, want["codes"])
        assert torch.equal(_bits(got.dequantize()), _bits(want["dequantized"]))


@pytest.mark.parametrize("index", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_host_path_equals_the_reference_bit_for_bit(index):
    case = CASES[index]
    plain, quantized = run_g29(case)
    same_as_recorded(plain, case["plain"])
    same_as_recorded(quantized, case["quantized"])


def run_code_level(case, device="cpu", dtype=None):
    """(input QuantizedTensor, result, the torch op on its raw data) of a code-level case (shared with the GPU tests)."""
    x = case["x"].to(device, dtype or case["x"].dtype)
    args = tuple(a.to(device) if isinstance(a, torch.Tensor) else a for a in case["args"])

    def call(t):
        return getattr(torch, case["method"])(t, *args, **case["kwargs"]) if case["through_torch"] else getattr(t, case["method"])(*args, **case["kwargs"])

    with torch.no_grad():
        q = g29_quantizer(case["slot"], case["params"], device)(x)
        return q, call(q), call(q.raw_data)


@pytest.mark.parametrize("index", range(len(CODE_LEVEL)), ids=[c["name"] for c in CODE_LEVEL])
def test_code_level_ops_move_codes_and_keep_the_context(index):
    case = CODE_LEVEL[index]
    with ff.strict_quantization(True):  # no dequantization on the way
        q, got, raw = run_code_level(case)
    values = got.values if isinstance(got, torch.return_types.topk) else got
    raw_values = raw.values if isinstance(raw, torch.return_types.topk) else raw
    assert isinstance(values, ff.QuantizedTensor) and values.quantization_context is q.quantization_context
    assert torch.equal(values.raw_data, raw_values) and torch.equal(values.raw_data, case["result"]["codes"])
    assert torch.equal(_bits(values.dequantize()), _bits(case["result"]["dequantized"]))
    if case["indices"] is not None:
        assert type(got) is torch.return_types.topk and type(got.indices) is torch.Tensor
        assert torch.equal(got.indices, case["indices"]) and torch.equal(got.indices, raw.indices)


def test_getitem_stays_forbidden_and_other_granularities_keep_their_route():
    q = ff.quantization.affine.quantize_per_tensor(torch.randn(4, 6), torch.tensor([0.05]), None, 8)
    with pytest.raises(NotImplementedError):
        q[0]
    pc = ff.quantization.affine.quantize_per_channel(torch.randn(4, 6), torch.ones(4), None, 0, 8)
    for call in (lambda t: t.unsqueeze(0), lambda t: t.expand(4, 6), lambda t: t.topk(2), lambda t: t.take_along_dim(torch.zeros(4, 1, dtype=torch.long), 1)):
        with pytest.raises(QuantizationError):  # no kernel: the dequantization fallback, which strict mode refuses
            call(pc)
        with ff.strict_quantization(False):
            out = call(pc)
            assert not isinstance(out.values if isinstance(out, torch.return_types.topk) else out, ff.QuantizedTensor)


def test_the_fixture_covers_what_it_names():
    assert len(CASES) == 120 and len(CODE_LEVEL) == 16 and {c["dtype"] for c in CASES} == {"torch.float32", "torch.bfloat16"}
    adds = [c for c in CASES if c["op"] == "index_add"]
    assert {c["kwargs"]["dim"] for c in adds} == {0, 1, -1} and {c["kwargs"]["alpha"] for c in adds} == {1, 0.5, -2}
    assert any(c["index"].unique().numel() < c["index"].numel() for c in adds) and any(c["index"].unique().numel() == c["index"].numel() for c in adds)
    assert {tuple(s is None for s in c["slots"]) for c in adds} == {(False, False), (True, False), (False, True), (True, True)}
    perms = [c for c in CASES if c["op"] == "permute"]
    assert {c["inputs"][0].dim() for c in perms} == {2, 3, 4, 5}
    assert {None if c["slots"][0] is None else c["slots"][0][2] if c["slots"][0][2] == "tensor" else "channel" for c in perms} == {None, "tensor", "channel"}
    assert (ROOT / "tests" / "golden" / "g29_index.pt").stat().st_size <= 1 << 20


# ---- strict mode: the reference's messages in its order ---------------------------------------------------------------------------
def test_strict_mode_messages_in_the_reference_order():
    q = ff.nn.LinearQuantizer(8, quantized_dtype=torch.int8)
    q.quantization_range = (torch.tensor(-1.0), torch.tensor(1.0))
    x, s, i = torch.randn(4, 8), torch.randn(2, 8), torch.tensor([0, 3])
    with torch.no_grad():
        qx, qs = q(x), q(s)
    no_oq = "'output_quantizer' must be provided if strict_quantization=True"
    expected = "Expected '{}' to be an instance of 'QuantizedTensor' because strict_quantization=True."
    with pytest.raises(QuantizationError, match=re.escape(no_oq)):
        F.index_add(x, 0, i, s, strict_quantization=True)              # ... before the operands are looked at
    with pytest.raises(QuantizationError, match=re.escape(expected.format("input"))):
        F.index_add(x, 0, i, s, output_quantizer=q, strict_quantization=True)   # input before source
    with pytest.raises(QuantizationError, match=re.escape(expected.format("source"))):
        F.index_add(qx, 0, i, s, output_quantizer=q, strict_quantization=True)
    with pytest.raises(QuantizationError, match=re.escape(no_oq)):
        F.permute(x, (1, 0), strict_quantization=True)
    with pytest.raises(QuantizationError, match=re.escape(expected.format("input"))):
        F.permute(x, (1, 0), output_quantizer=q, strict_quantization=True)
    with torch.no_grad(), ff.strict_quantization(True):                # the global flag is the default
        assert isinstance(F.index_add(qx, 0, i, qs, 0.5, output_quantizer=q), ff.QuantizedTensor)
        assert isinstance(F.permute(qx, (1, 0), output_quantizer=q), ff.QuantizedTensor)
        with pytest.raises(QuantizationError, match=re.escape(no_oq)):
            F.permute(qx, (1, 0))
    with torch.no_grad():
        want = torch.index_add(x, 0, i, s, alpha=-2)                     # alpha reaches torch.index_add
        assert torch.equal(F.index_add(x, 0, i, s, -2, strict_quantization=False), want)
        assert torch.equal(F.index_add(x, 0, i, s, alpha=-2, strict_quantization=False), want)


# ---- the predicates --------------------------------------------------------------------------------------------------------------
def _codes(shape, granularity=None, channels=None, dtype=torch.bfloat16, container=torch.int8, bits=8):
    q = ff.nn.LinearQuantizer(bits, symmetric=False, granularity=granularity or ff.PerTensor(), quantized_dtype=container)
    q.quantization_range = (torch.tensor(-3.0), torch.tensor(3.0)) if channels is None else (torch.full((channels,), -3.0), torch.full((channels,), 3.0))
    with torch.no_grad():
        return q(torch.randn(shape).to(dtype))


def _out_quantizer():
    q = ff.nn.LinearQuantizer(8, quantized_dtype=torch.int8)
    q.quantization_range = (torch.tensor(-1.0), torch.tensor(1.0))
    return q


def test_the_index_add_predicate_accepts_and_declines(monkeypatch):
    x, s, i = _codes((4, 6, 9)), _codes((4, 3, 9)), torch.tensor([0, 5, 0])
    common = dict(output_quantizer=None, strict_quantization=False)
    assert not fused_index.index_add_predicate(input=x, dim=1, index=i, source=s, **common)     # host tensors
    monkeypatch.setattr("fastforward_amd.fused_index._on_device", lambda *t: True)

    def ok(**k):
        with torch.no_grad():
            return fused_index.KERNELS.supported_index_add(**{**dict(input=x, dim=1, index=i, source=s), **common, **k})

    assert ok() and ok(dim=-2) and ok(alpha=0.5) and ok(alpha=-2) and ok(index=i.int()) and ok(output_quantizer=_out_quantizer())
    assert ok(input=torch.randn(4, 6, 9).bfloat16()) and ok(source=torch.randn(4, 3, 9).bfloat16())            # plain / codes mixes
    assert ok(input=_codes((4, 6, 9), dtype=torch.float16), source=_codes((4, 3, 9), dtype=torch.float16, container=torch.float16))
    assert ok(index=torch.zeros(0, dtype=torch.long), source=_codes((4, 0, 9)))                                # a requantization
    assert ok(input=_codes((6,)), dim=0, source=_codes((3,)))
    assert ok(output_quantizer=_out_quantizer(), strict_quantization=True)
    # the call
    assert not fused_index.KERNELS.supported_index_add(x, 1, i, s) and not ok(out=torch.empty(1))             # not ff.nn.functional's
    assert not ok(strict_quantization=True) and not ok(output_quantizer=_out_quantizer(), strict_quantization=True, source=torch.randn(4, 3, 9).bfloat16())
    # operands
    assert not ok(input=_codes((4, 6, 9), ff.PerChannel(1), 6)) and not ok(source=_codes((4, 3, 9), ff.PerChannel(0), 4))   # per channel
    assert not ok(input=_codes((4, 6, 9), dtype=torch.float32), source=_codes((4, 3, 9), dtype=torch.float32))   # fp32
    assert not ok(source=_codes((4, 3, 9), dtype=torch.float16)) and not ok(input=torch.randn(4, 6, 9))          # mixed dtypes
    assert not ok(input=_codes((4, 6, 9), bits=16, container=torch.int16))
    assert not ok(input=_codes(()), dim=0, source=_codes(()), index=torch.tensor([0]))                          # 0-dim
    assert not ok(input=_codes((4, 0, 9)))                                                                        # empty input
    # dim, index, source, alpha
    assert not ok(dim=3) and not ok(dim=-4) and not ok(dim=True) and not ok(dim=1.0) and not ok(dim=None)
    assert not ok(index=i.reshape(1, 3)) and not ok(index=i.float()) and not ok(index=[0, 5, 0]) and not ok(index=i.short())
    assert not ok(source=_codes((4, 2, 9))) and not ok(source=_codes((4, 3, 8))) and not ok(source=_codes((3, 9))) and not ok(dim=0)
    assert not ok(alpha=torch.tensor(2.0)) and not ok(alpha=True) and not ok(alpha=float("inf")) and not ok(alpha=float("nan")) and not ok(alpha=None)
    assert not ok(alpha=1e39) and ok(alpha=3e38)                                                                 # finite in bf16
    assert not ok(input=_codes((4, 6, 9), dtype=torch.float16), source=_codes((4, 3, 9), dtype=torch.float16), alpha=1e5)   # ... not in fp16
    with torch.enable_grad():
        assert not fused_index.KERNELS.supported_index_add(input=x, dim=1, index=i, source=s, **common)          # a gradient is needed
        plain = torch.randn(4, 6, 9).bfloat16().requires_grad_()
        assert not fused_index.KERNELS.supported_index_add(input=plain, dim=1, index=i, source=torch.randn(4, 3, 9).bfloat16(), **common)


def test_the_permute_predicate_accepts_and_declines(monkeypatch):
    x, oq = _codes((2, 3, 5, 7)), _out_quantizer()
    common = dict(output_quantizer=oq, strict_quantization=False)
    assert not fused_index.permute_predicate(input=x, dims=(0, 2, 3, 1), **common)                                # host tensors
    monkeypatch.setattr("fastforward_amd.fused_index._on_device", lambda *t: True)

    def ok(**k):
        with torch.no_grad():
            return fused_index.KERNELS.supported_permute(**{**dict(input=x, dims=(0, 2, 3, 1)), **common, **k})

    assert ok() and ok(dims=[0, -2, -1, 1]) and ok(dims=(0, 1, 2, 3)) and ok(dims=torch.Size((3, 2, 1, 0))) and ok(strict_quantization=True)
    assert ok(input=torch.randn(2, 3, 5, 7).half()) and ok(input=_codes((2, 3, 5, 7), dtype=torch.float16, container=torch.float16))
    for axis in range(4):
        assert ok(input=_codes((2, 3, 5, 7), ff.PerChannel(axis), (2, 3, 5, 7)[axis]))
    assert ok(input=_codes((2, 1, 2, 1, 2, 3)), dims=(5, 4, 3, 2, 1, 0)) and ok(input=_codes((5,)), dims=(0,))
    assert not ok(output_quantizer=None)                                                                         # a view is free
    assert not fused_index.KERNELS.supported_permute(x, (0, 2, 3, 1), output_quantizer=oq)                       # not ff.nn.functional's
    assert not ok(input=_codes((1, 2, 1, 2, 1, 2, 3)), dims=(6, 5, 4, 3, 2, 1, 0))                               # rank 7
    assert not ok(input=_codes(()), dims=())
    assert not ok(dims=(0, 2, 3)) and not ok(dims=(0, 2, 2, 1)) and not ok(dims=(0, 2, 3, 4)) and not ok(dims=(0, 2, 3, 1.0)) and not ok(dims=None)
    assert not ok(dims=(False, 2, 3, 1))
    assert not ok(input=_codes((2, 3, 5, 7), dtype=torch.float32)) and not ok(input=torch.randn(2, 3, 5, 7))     # fp32
    assert not ok(input=_codes((2, 3, 5, 7), ff.PerChannel((0, 1)), 6))                                          # two axes
    assert not ok(input=_codes((2, 4, 5, 7), ff.PerBlock(1, 2), 2))                                              # blocks along one axis
    assert not ok(input=_codes((2, 0, 5, 7)))
    assert not ok(input=torch.randn(2, 3, 5, 7).bfloat16(), strict_quantization=True)
    with torch.enable_grad():
        assert not fused_index.KERNELS.supported_permute(input=x, dims=(0, 2, 3, 1), **common)


def test_the_other_predicates_are_untouched():
    from fastforward_amd import fused_conv3d

    assert type(fused_conv3d.KERNELS).supported is fused_conv.ConvKernels.supported
    assert not {"supported_cat", "supported_pad", "supported"} & set(vars(fused_index.IndexKernels))
    assert [it.fn for it in dispatcher._DISPATCHER["pad"]] == [fused_concat.KERNELS.pad]
    assert fused_concat.KERNELS.cat in [it.fn for it in dispatcher._DISPATCHER["cat"]] and len(dispatcher._DISPATCHER["cat"]) == 2


def test_the_wrappers_say_not_covered_on_a_library_without_the_symbols(oracle_backend):
    x, s, i = torch.zeros(4, 8, dtype=torch.bfloat16), torch.zeros(2, 8, dtype=torch.bfloat16), torch.tensor([0, 1])
    with pytest.raises(BackendError, match="does not export ffq_index_add_quantize"):
        ff.ops.index_add_quantize(x, 0, i, s)
    with pytest.raises(BackendError, match="does not export ffq_permute_quantize"):
        ff.ops.permute_quantize(x, (1, 0))


def test_the_wrappers_check_their_operands_and_refuse_host_tensors():
    x, s, i = torch.zeros(4, 8, dtype=torch.bfloat16), torch.zeros(2, 8, dtype=torch.bfloat16), torch.tensor([0, 1])
    with pytest.raises(BackendError, match="HIP device only"):
        ff.ops.index_add_quantize(x, 0, i, s)
    with pytest.raises(BackendError, match="HIP device only"):
        ff.ops.permute_quantize(x, (1, 0))
    for call in (lambda: ff.ops.index_add_quantize(x, 2, i, s), lambda: ff.ops.index_add_quantize(x, 0, i.float(), s),
                 lambda: ff.ops.index_add_quantize(x, 0, i, s[:1]), lambda: ff.ops.index_add_quantize(x, 0, i, s, alpha=torch.tensor(1.0)),
                 lambda: ff.ops.index_add_quantize(x.float(), 0, i, s.float(), dtype=torch.bfloat16),
                 lambda: ff.ops.permute_quantize(x, (0, 0)), lambda: ff.ops.permute_quantize(x, (0,)), lambda: ff.ops.permute_quantize(x.reshape(()), ())):
        with pytest.raises(RuntimeError):
            call()


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def _header(name):
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / name).read_text(), flags=re.S)


def _declared(name):
    return set(re.findall(r"\b(ffq_[a-z0-9_]+)\s*\(", _header(name)))


def test_the_fourth_header_and_its_table_agree():
    assert _declared("ffq_index.h") == set(_cabi.SIGNATURES_INDEX) == ENTRIES
    assert '#include "ffq.h"' in (ROOT / "include" / "ffq_index.h").read_text()
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    pointers = {"ffq_fanout": ctypes.POINTER(_cabi.FanOut), "int64_t": ctypes.POINTER(ctypes.c_int64)}
    for entry in ENTRIES:
        params = re.search(entry + r"\s*\((.*?)\)\s*;", _header("ffq_index.h"), flags=re.S).group(1).split(",")
        want = []
        for p in params:
            words = p.replace("*", " * ").split()
            want.append(pointers.get(words[words.index("*") - 1], ctypes.c_void_p) if "*" in words else kinds[words[-2]])
        restype, argtypes = _cabi.SIGNATURES_INDEX[entry]
        assert restype is ctypes.c_int and argtypes == want, entry


def test_the_other_tables_are_untouched_and_disjoint():
    assert _declared("ffq.h") == set(_cabi.SIGNATURES) and _declared("ffq_3d.h") == set(_cabi.SIGNATURES_3D)
    assert _declared("ffq_depthwise.h") == set(_cabi.SIGNATURES_DEPTHWISE)
    mine = set(_cabi.SIGNATURES_INDEX)
    for other in (_cabi.SIGNATURES, _cabi.SIGNATURES_3D, _cabi.SIGNATURES_DEPTHWISE, _cabi.DEVICE_ONLY):
        assert not mine & set(other)
    assert _cabi.FFQ_ABI_VERSION == 9 and "#define FFQ_ABI_VERSION 9" in (ROOT / "include" / "ffq.h").read_text()


def test_the_hip_library_exports_them_and_the_oracle_loads_without_them():
    dll, lib, oracle = ctypes.CDLL(str(HIP_SO)), FFQLibrary(HIP_SO), load_oracle()
    for entry in ENTRIES:
        assert hasattr(dll, entry) and getattr(lib, entry) is not None
        assert not oracle.is_device and getattr(oracle, entry) is None


FAKE = 1 << 20  # never dereferenced: every call below returns from the argument checks
BF16, F16, I8, I32, I64, F32 = (int(t) for t in (DType.BF16, DType.F16, DType.I8, DType.I32, DType.I64, DType.F32))


def _fan(count=1, bits=8.0, scale=FAKE, codes=FAKE):
    held = min(count, _cabi.FFQ_MAX_FANOUT)
    fan = _cabi.FanOut.make(bits, [scale] * held, [None] * held, [codes] * held)
    fan.count = count  # (a count beyond the struct's arrays is the entry point's to refuse)
    return ctypes.byref(fan)


def _add(lib, x=FAKE, x_dt=BF16, xs=None, xo=None, index=FAKE, index_dt=I64, n=3, src=FAKE, src_dt=BF16, ss=None, so=None, alpha=1.0, dt=BF16,
         outer=2, R=5, inner=8, out=FAKE, fan=None):
    return lib.ffq_index_add_quantize(x, x_dt, xs, xo, index, index_dt, n, src, src_dt, ss, so, alpha, dt, outer, R, inner, out, fan, None)


def _perm(lib, x=FAKE, x_dt=BF16, xs=None, xo=None, axis=-1, dt=BF16, rank=3, shape=(2, 3, 4), dims=(2, 0, 1), out=FAKE, fan=None):
    arr = lambda v: None if v is None else (ctypes.c_int64 * len(v))(*v)  # noqa: E731
    return lib.ffq_permute_quantize(x, x_dt, xs, xo, axis, dt, rank, arr(shape), arr(dims), out, fan, None)


# in the documented order: each call fails the named check and passes every check ahead of it; most fail a LATER check too and must
# report the earlier one
ERRORS = [
    (lambda lib: _add(lib, dt=F32, x_dt=I8), Status.ERR_DTYPE),                                # the value dtype, before the forms
    (lambda lib: _add(lib, x_dt=I8, src_dt=I8), Status.ERR_DTYPE),                             # x: codes without a scale; before src
    (lambda lib: _add(lib, x_dt=F16, xs=FAKE, index_dt=I8), Status.ERR_DTYPE),                 # x: codes of another float dtype
    (lambda lib: _add(lib, xo=FAKE, n=-1), Status.ERR_DTYPE),                                  # x: an offset without a scale
    (lambda lib: _add(lib, x_dt=I8, xs=FAKE, src_dt=I8, n=-1), Status.ERR_DTYPE),              # src; before the extents
    (lambda lib: _add(lib, index_dt=I8, n=-1), Status.ERR_DTYPE),                              # the index dtype; before the extents
    (lambda lib: _add(lib, index_dt=F32), Status.ERR_DTYPE),
    (lambda lib: _add(lib, n=-1, alpha=float("inf")), Status.ERR_ARG),                         # negative extents; before alpha
    (lambda lib: _add(lib, outer=-1), Status.ERR_ARG),
    (lambda lib: _add(lib, R=-1), Status.ERR_ARG),
    (lambda lib: _add(lib, inner=-1), Status.ERR_ARG),
    (lambda lib: _add(lib, alpha=float("inf"), R=1 << 31), Status.ERR_ARG),                    # alpha; before the sizes
    (lambda lib: _add(lib, alpha=float("nan")), Status.ERR_ARG),
    (lambda lib: _add(lib, alpha=1e39), Status.ERR_ARG),                                       # beyond fp32, so beyond bf16
    (lambda lib: _add(lib, alpha=1e5, dt=F16, x_dt=F16, src_dt=F16), Status.ERR_ARG),          # ... beyond fp16
    (lambda lib: _add(lib, alpha=1e5, R=1 << 31), Status.ERR_DTYPE),                           # ... and fine in bf16: on to the sizes
    (lambda lib: _add(lib, R=1 << 31, fan=_fan(4)), Status.ERR_DTYPE),                         # sizes; before the fan-out
    (lambda lib: _add(lib, outer=1 << 20, R=1 << 10, inner=2, fan=_fan(4)), Status.ERR_DTYPE),
    (lambda lib: _add(lib, outer=1 << 20, n=1 << 10, inner=2), Status.ERR_DTYPE),              # the source's size
    (lambda lib: _add(lib, outer=1 << 40, R=1 << 40, inner=1 << 40), Status.ERR_DTYPE),        # no int64 overflow on the way
    (lambda lib: _add(lib, fan=_fan(4), x=None), Status.ERR_ARG),                              # the fan-out; before the buffers
    (lambda lib: _add(lib, fan=_fan(1, bits=11.0), x=None), Status.ERR_PRECISION),
    (lambda lib: _add(lib, fan=_fan(1, scale=None), R=0), Status.ERR_ARG),                     # ... and before an empty x returns OK
    (lambda lib: _add(lib, fan=_fan(1, codes=FAKE + 8)), Status.ERR_ARG),                      # misaligned codes
    (lambda lib: _add(lib, x=None), Status.ERR_ARG),
    (lambda lib: _add(lib, x=FAKE + 2), Status.ERR_ARG),
    (lambda lib: _add(lib, out=FAKE + 8), Status.ERR_ARG),
    (lambda lib: _add(lib, index=None), Status.ERR_ARG),
    (lambda lib: _add(lib, src=None), Status.ERR_ARG),
    (lambda lib: _add(lib, src=FAKE + 4), Status.ERR_ARG),
    (lambda lib: _add(lib, R=0, x=None, out=None, src=None, index=None), Status.OK),           # empty: nothing launched
    (lambda lib: _add(lib, outer=0, x=None), Status.OK),
    (lambda lib: _add(lib, inner=0, x=None), Status.OK),
    (lambda lib: _perm(lib, dt=I8, x_dt=F32), Status.ERR_DTYPE),                               # the value dtype, before the form
    (lambda lib: _perm(lib, x_dt=I8, rank=0), Status.ERR_DTYPE),                               # codes without a scale; before the rank
    (lambda lib: _perm(lib, axis=1, rank=7), Status.ERR_DTYPE),                                # per-channel without a scale
    (lambda lib: _perm(lib, rank=0), Status.ERR_ARG),
    (lambda lib: _perm(lib, rank=7, shape=(1,) * 7, dims=tuple(range(7))), Status.ERR_ARG),
    (lambda lib: _perm(lib, shape=None), Status.ERR_ARG),
    (lambda lib: _perm(lib, dims=None), Status.ERR_ARG),
    (lambda lib: _perm(lib, shape=(2, -3, 4), dims=(0, 0, 1)), Status.ERR_ARG),                # a negative extent; before dims
    (lambda lib: _perm(lib, dims=(0, 0, 1), xs=FAKE, axis=3), Status.ERR_ARG),                 # dims; before the parameter axis
    (lambda lib: _perm(lib, dims=(0, 3, 1)), Status.ERR_ARG),
    (lambda lib: _perm(lib, dims=(0, -1, 1)), Status.ERR_ARG),
    (lambda lib: _perm(lib, xs=FAKE, x_dt=I8, axis=3, shape=(1 << 20, 1 << 10, 4)), Status.ERR_ARG),   # the parameter axis; before the size
    (lambda lib: _perm(lib, shape=(1 << 20, 1 << 10, 2), fan=_fan(4)), Status.ERR_DTYPE),      # the size; before the fan-out
    (lambda lib: _perm(lib, shape=(1 << 40, 1 << 40, 1 << 40)), Status.ERR_DTYPE),
    (lambda lib: _perm(lib, fan=_fan(4), x=None), Status.ERR_ARG),                             # the fan-out; before the buffers
    (lambda lib: _perm(lib, fan=_fan(1, bits=0.5), shape=(2, 0, 4)), Status.ERR_PRECISION),    # ... and before an empty x returns OK
    (lambda lib: _perm(lib, x=None), Status.ERR_ARG),
    (lambda lib: _perm(lib, x=FAKE + 2), Status.ERR_ARG),
    (lambda lib: _perm(lib, out=FAKE + 4), Status.ERR_ARG),
    (lambda lib: _perm(lib, shape=(2, 0, 4), x=None, out=None), Status.OK),
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
    found = {}
    for family, count in (("index_add_quantize_kernel", 4), ("permute_rows_kernel", 12), ("permute_transpose_kernel", 6)):
        rows = [k for k in kernel_resources.kernel_resources() if family in str(k["name"])]
        assert len(rows) == count, (family, len(rows))  # {bf16, fp16} x {groups of 8, elements} [x {plain, int8 codes, value-dtype codes}]
        found[family] = rows
        bad = {str(k["name"]): k for k in rows if k["vgpr_spill_count"] or k["sgpr_spill_count"] or k["private_segment_fixed_size"]}
        assert not bad, bad
        assert all(k["vgpr_count"] + k["agpr_count"] <= 128 for k in rows), rows
    # the transposed tile is the only LDS: 64 rows of 65 dwords
    assert all(k["group_segment_fixed_size"] == 64 * 65 * 4 for k in found["permute_transpose_kernel"])
    assert all(k["group_segment_fixed_size"] == 0 for k in found["index_add_quantize_kernel"] + found["permute_rows_kernel"])
