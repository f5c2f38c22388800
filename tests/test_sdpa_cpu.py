"""The quantized scaled_dot_product_attention without a GPU: the public names, the math path against the reference's outputs (fixture
G22) including the ranges one calibration pass leaves, the reference's errors, the flag and upcast contexts, the dispatcher
registration and its CPU decline, the C-ABI entry point (declared in the header and the ctypes table, exported by the HIP library,
absent from the oracle) and what hipcc emitted for the kernel."""

import ctypes
import re
import sys

import pytest
import torch

import fastforward_amd as ff

from conftest import HIP_SO, ROOT, golden, load_oracle
from fastforward_amd import _cabi, dispatcher, fused_sdpa, ops
from fastforward_amd.exceptions import QuantizationError
from fastforward_amd.nn.sdpa import QUANTIZER_NAMES, scaled_dot_product_attention_math

sys.path.insert(0, str(ROOT / "tools"))

import kernel_resources  # noqa: E402

F = ff.nn.functional


def quantizer(bits, scale, offset, container=None):
    q = ff.nn.LinearQuantizer(bits, symmetric=False, granularity=ff.PerTensor(), quantized_dtype=container)
    q.quantization_range = (torch.tensor(-1.0), torch.tensor(1.0))
    with torch.no_grad():
        q.scale.fill_(scale)
        q.offset.fill_(offset)
    return q


G22 = golden("g22_sdpa.pt")
CASES = sorted(n for n in G22 if n != "calibration")


def test_public_names():
    assert callable(F.scaled_dot_product_attention) and callable(F.dropout)
    assert ff.sdpa_upcast.dtype == torch.float32
    assert ff.get_sdpa_torch_fallback_allowed() is False
    for name in ("set_sdpa_torch_fallback_allowed", "get_sdpa_torch_fallback_allowed", "sdpa_torch_fallback_allowed", "sdpa_upcast"):
        assert hasattr(ff, name), name


@pytest.mark.parametrize("name", CASES)
def test_math_path_equals_the_reference(name):
    """Every step is the reference's own ATen call on the same values (fp32 after the upcast): bit-exact, case by case."""
    c = G22[name]
    quantizers = {n: quantizer(*spec) for n, spec in c["quantizers"].items()}
    operands = (c["q"], c["k"], c["v"])
    if c["quantized_qkv"]:
        operands = tuple(quantizer(8, 2.0**-5, 0.0, container=torch.int8)(t) for t in operands)
    with torch.no_grad():
        out = F.scaled_dot_product_attention(*operands, attn_mask=c["mask"], **c["kwargs"], **quantizers)
    assert out.dtype == c["out"].dtype and torch.equal(out, c["out"]), name


def test_fully_masked_row_is_zero():
    c = G22["float32_bool_masked_row"]
    assert torch.equal(c["out"][:, :, 3], torch.zeros_like(c["out"][:, :, 3]))


def test_calibration_ranges_equal_the_reference():
    c = G22["calibration"]
    qs = {n: ff.nn.LinearQuantizer(8, symmetric=False, granularity=ff.PerTensor()) for n in QUANTIZER_NAMES}
    with torch.no_grad(), ff.estimate_ranges(torch.nn.ModuleList(qs.values()), ff.range_setting.running_minmax):
        out = F.scaled_dot_product_attention(c["q"], c["k"], c["v"], is_causal=True, neg_inf=-100.0, strict_quantization=False, **qs)
    assert torch.equal(out, c["out"])
    for n in QUANTIZER_NAMES:
        scale, offset = c["ranges"][n]
        assert torch.equal(qs[n].scale.detach(), scale) and torch.equal(qs[n].offset.detach(), offset), n


def test_errors_are_the_reference_errors():
    q = torch.randn(1, 2, 4, 16)
    with pytest.raises(ValueError, match="Explicit attn_mask should not be set when is_causal=True"):
        F.scaled_dot_product_attention(q, q, q, attn_mask=torch.ones(4, 4, dtype=torch.bool), is_causal=True, strict_quantization=False)
    with pytest.raises(QuantizationError, match="Strict quantization currently not supported when enable_gqa=True"):
        F.scaled_dot_product_attention(q, q[:, :1], q[:, :1], enable_gqa=True, strict_quantization=True)
    with pytest.raises(QuantizationError, match="'output_quantizer' must be provided if strict_quantization=True"):
        F.scaled_dot_product_attention(q, q, q, strict_quantization=True)
    qq = quantizer(8, 2.0**-5, 0.0, container=torch.int8)(q)
    with pytest.raises(QuantizationError, match="'output_quantizer' must be provided"):
        F.scaled_dot_product_attention(qq, qq, qq, strict_quantization=True, scaled_query_quantizer=quantizer(8, 0.01, 0.0))
    with pytest.raises(QuantizationError, match="'output_quantizer' must be provided"):
        F.dropout(q, 0.0, strict_quantization=True)


def test_flags_and_upcast_contexts_restore_their_values():
    with ff.sdpa_torch_fallback_allowed(True):
        assert ff.get_sdpa_torch_fallback_allowed() is True
    assert ff.get_sdpa_torch_fallback_allowed() is False
    with ff.set_sdpa_torch_fallback_allowed(True):
        pass
    assert ff.get_sdpa_torch_fallback_allowed() is False
    with ff.sdpa_upcast(torch.float64):
        assert ff.sdpa_upcast.dtype == torch.float64
        with ff.sdpa_upcast(False):
            assert ff.sdpa_upcast.dtype is None
        with ff.sdpa_upcast(True):
            assert ff.sdpa_upcast.dtype == torch.float32
        assert ff.sdpa_upcast.dtype == torch.float64
    assert ff.sdpa_upcast.dtype == torch.float32
    x = torch.randn(2, 3).bfloat16()
    assert ff.sdpa_upcast.upcast(x).dtype == torch.float32


def test_torch_fallback_flag_returns_the_math_value():
    """The reference discards the result of its torch fallback: the value is the math path's either way."""
    q, k, v = (torch.randn(1, 2, 5, 16).bfloat16() for _ in range(3))
    with torch.no_grad():
        a = F.scaled_dot_product_attention(q, k, v, strict_quantization=False, sdpa_torch_fallback=True)
        b = scaled_dot_product_attention_math(q, k, v, strict_quantization=False)
    assert torch.equal(a, b)


def test_dispatcher_registration_declines_cpu_tensors():
    items = dispatcher._DISPATCHER["scaled_dot_product_attention"]
    fns = [it.fn for it in items]
    assert scaled_dot_product_attention_math in fns and fused_sdpa.KERNELS.sdpa in fns
    assert fns.index(fused_sdpa.KERNELS.sdpa) < fns.index(scaled_dot_product_attention_math)
    q = torch.randn(1, 2, 4, 64).bfloat16()
    assert not fused_sdpa.sdpa_predicate(query=q, key=q, value=q, strict_quantization=False)


def test_header_and_ctypes_table_agree():
    header = (ROOT / "include" / "ffq.h").read_text()
    m = re.search(r"int ffq_sdpa_quantize\(([^;]*)\);", header)
    assert m is not None
    params = [p for p in m.group(1).replace("\n", " ").split(",") if p.strip()]
    restype, argtypes = _cabi.SIGNATURES["ffq_sdpa_quantize"]
    assert restype is ctypes.c_int and len(argtypes) == len(params) == 25
    assert "ffq_sdpa_quantize" in _cabi.DEVICE_ONLY
    assert [f[0] for f in _cabi.SdpaQuantizer._fields_] == ["scale", "offset", "num_bits"]
    assert ctypes.sizeof(_cabi.SdpaQuantizer) == 24 and _cabi.SDPA_QUANTIZERS == len(QUANTIZER_NAMES) == 8
    # one order of the eight slots: the header's enum, the ops table, the functional keywords
    enum = re.search(r"FFQ_SDPA_SCORES = 0,([^}]*)\}", header)
    assert enum is not None
    slots = ["SCORES"] + [w.strip().removeprefix("FFQ_SDPA_") for w in enum.group(1).split(",") if w.strip()]
    assert slots[-1] == "QUANTIZERS" and len(slots) == 9
    keyword = {"SCORES": "attn_scores_quantizer", "MASK": "attn_mask_quantizer", "MASKED": "masked_scores_quantizer",
               "WEIGHTS": "attn_weights_quantizer", "QUERY": "scaled_query_quantizer", "KEY": "scaled_key_quantizer",
               "DROPOUT": "dropout_quantizer", "OUTPUT": "output_quantizer"}
    assert tuple(keyword[w] for w in slots[:-1]) == ops.sdpa.QUANTIZER_SLOTS == QUANTIZER_NAMES
    if HIP_SO.exists():
        assert hasattr(ctypes.CDLL(str(HIP_SO)), "ffq_sdpa_quantize")
    oracle = load_oracle()
    if oracle is not None:
        assert oracle.ffq_sdpa_quantize is None


def test_kernel_resources_have_no_scratch():
    if kernel_resources.readelf() is None or not kernel_resources.DEFAULT_LIBRARY.exists():
        pytest.skip("llvm-readelf or the built library is missing")
    rows = [k for k in kernel_resources.kernel_resources() if "sdpa_quantize_kernel" in str(k["name"])]
    assert len(rows) == 8  # E 64 / 128 x one / two passes x bf16 / fp16
    # no scratch and no VGPR spill; the scalar state of the eight quantizers may spill SGPRs into VGPR lanes (no memory traffic)
    bad = {str(k["name"]): k for k in rows if k["vgpr_spill_count"] or k["private_segment_fixed_size"]}
    assert not bad, bad
    assert all(k["group_segment_fixed_size"] <= 64 * 1024 for k in rows)
