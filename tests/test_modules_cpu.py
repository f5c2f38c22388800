"""The generic quantized modules (LayerNorm / Embedding / ReLU / SiLU) without a GPU: conversion by ``quantize_model``, the
reference's quantizer tags and strict-mode errors, the host path against the reference's outputs (fixture G19), range estimation,
the module map next to the Llama harness, the three C-ABI entry points (exported by the HIP library, absent from the oracle,
argument checks before any device call) and what hipcc emitted for their kernels."""

import ctypes
import logging
import sys

import pytest
import torch

import fastforward_amd as ff

from conftest import HIP_SO, ROOT, golden, load_oracle
from fastforward_amd import _cabi, fused_modules, llama
from fastforward_amd._cabi import DType, FanOut, FFQLibrary, Status
from fastforward_amd.exceptions import QuantizationError

sys.path.insert(0, str(ROOT / "tools"))

import kernel_resources  # noqa: E402

ENTRY_POINTS = ("ffq_layer_norm_quantize", "ffq_embedding_quantize", "ffq_pointwise_quantize")
KERNELS = ("layer_norm_quantize_kernel", "embedding_quantize_kernel", "pointwise_quantize_kernel")


# ---- a tiny OPT-like model built from torch.nn parts (shared with tests/test_modules_gpu.py) -------------------------------------
class Block(torch.nn.Module):
    def __init__(self, hidden: int, ffn: int) -> None:
        super().__init__()
        self.norm = torch.nn.LayerNorm(hidden)
        self.fc1 = torch.nn.Linear(hidden, ffn)
        self.act = torch.nn.ReLU()
        self.fc2 = torch.nn.Linear(ffn, hidden)

    def forward(self, h: torch.Tensor) -> torch.Tensor:
        return self.fc2(self.act(self.fc1(self.norm(h))))


def _plain(t):
    return t.dequantize() if isinstance(t, ff.QuantizedTensor) else t


class TinyOPT(torch.nn.Module):
    """Embedding -> [LayerNorm -> Linear -> ReLU -> Linear] x 2 (residual) -> LayerNorm -> SiLU."""

    def __init__(self, vocab: int = 96, hidden: int = 64, ffn: int = 128) -> None:
        super().__init__()
        self.embed = torch.nn.Embedding(vocab, hidden)
        self.layers = torch.nn.ModuleList([Block(hidden, ffn) for _ in range(2)])
        self.final_norm = torch.nn.LayerNorm(hidden)
        self.act = torch.nn.SiLU()

    def forward(self, ids: torch.Tensor) -> torch.Tensor:
        h = _plain(self.embed(ids))
        for layer in self.layers:
            h = h + _plain(layer(h))
        return self.act(self.final_norm(h))


def tiny_opt(device="cpu", dtype=torch.float32, seed=0) -> TinyOPT:
    torch.manual_seed(seed)
    model = TinyOPT().to(device, dtype)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0.0, 0.1)
    return model


def quantize_tiny(model: TinyOPT) -> TinyOPT:
    """quantize_model with pass-through surrogates for the model's own container classes (reference recipe)."""
    return ff.quantize_model(model, extra_conversion=ff.nn.surrogate_quantized_modules(model))


def install_quantizers(model: torch.nn.Module, device="cpu") -> None:
    """W8A8: per-tensor asymmetric int8 activations, per-channel symmetric int8 weights. Every activation is quantized once: the
    generic modules quantize their outputs, and the linears take those codes as their inputs (their input slots stay stubs); the
    final LayerNorm leaves its output to the SiLU's input quantizer."""
    act = lambda: ff.nn.LinearQuantizer(8, symmetric=False, quantized_dtype=torch.int8, device=device)  # noqa: E731
    for name, m in model.named_modules():
        if isinstance(m, (ff.nn.QuantizedLayerNorm, ff.nn.QuantizedRelu, ff.nn.QuantizedSilu)):
            m.input_quantizer = act()
        if isinstance(m, (ff.nn.QuantizedLayerNorm, ff.nn.QuantizedRelu, ff.nn.QuantizedSilu, ff.nn.QuantizedEmbedding)) and name != "final_norm":
            m.output_quantizer = act()
        if isinstance(m, (ff.nn.QuantizedLinear, ff.nn.QuantizedEmbedding)):
            m.weight_quantizer = ff.nn.LinearQuantizer(8, granularity=ff.PerChannel(0), quantized_dtype=torch.int8, device=device)
        if isinstance(m, ff.nn.QuantizedLayerNorm):
            m.weight_quantizer = ff.nn.LinearQuantizer(8, quantized_dtype=torch.int8, device=device)


def test_quantize_model_converts_the_tiny_opt_model_with_the_reference_tags():
    model = quantize_tiny(tiny_opt())
    assert type(model.embed) is ff.nn.QuantizedEmbedding
    assert type(model.final_norm) is ff.nn.QuantizedLayerNorm and type(model.act) is ff.nn.QuantizedSilu
    for layer in model.layers:
        assert type(layer.norm) is ff.nn.QuantizedLayerNorm and type(layer.act) is ff.nn.QuantizedRelu
        assert not layer.act.inplace
    expected = {
        model.embed: {"weight_quantizer": "parameter/weight", "output_quantizer": "activation/output"},
        model.final_norm: {"input_quantizer": "activation/input", "weight_quantizer": "parameter/weight", "bias_quantizer": "parameter/bias",
                           "output_quantizer": "activation/output"},
        model.act: {"input_quantizer": "activation/input", "output_quantizer": "activation/output"},
        model.layers[0].act: {"input_quantizer": "activation/input", "output_quantizer": "activation/output"},
    }
    for module, slots in expected.items():
        for name, tag in slots.items():
            stub = getattr(module, name)
            assert isinstance(stub, ff.nn.QuantizerStub) and tag in stub.quant_metadata, (module, name)


def test_layer_norm_without_affine_has_no_parameter_quantizers():
    model = ff.quantize_model(torch.nn.Sequential(torch.nn.LayerNorm(16, elementwise_affine=False)))
    assert model[0].weight_quantizer is None and model[0].bias_quantizer is None
    assert isinstance(model[0].output_quantizer, ff.nn.QuantizerStub)


def test_quantized_activation_is_not_in_the_module_map():
    mapping = ff.nn.quantized_module_map()
    assert ff.nn.QuantizedActivation not in mapping.values()
    assert mapping[torch.nn.ReLU] is ff.nn.QuantizedRelu and mapping[torch.nn.SiLU] is ff.nn.QuantizedSilu
    assert mapping[torch.nn.LayerNorm] is ff.nn.QuantizedLayerNorm


def test_the_generic_embedding_owns_the_module_map_and_the_harness_keeps_its_own(caplog):
    with caplog.at_level(logging.WARNING):
        mapping = ff.nn.quantized_module_map()
    assert mapping[torch.nn.Embedding] is ff.nn.QuantizedEmbedding
    assert "Multiple quantized versions" not in caplog.text
    cfg = llama.LlamaConfig(hidden_size=64, intermediate_size=160, num_layers=1, num_heads=4, num_kv_heads=2, vocab_size=97)
    model = llama.build_model(cfg, "cpu", dtype=torch.float32)
    llama.quantize_llama(model, w_bits=8, a_bits=8, quantized_dtype=torch.int8)
    assert type(model.embed_tokens) is llama.QuantizedEmbedding


# ---- strict quantization: the reference's messages (_gen/fallback.py) ------------------------------------------------------------
OUTPUT_MSG = "'output_quantizer' must be provided if strict_quantization=True"


def _expected(name):
    return f"Expected '{name}' to be an instance of 'QuantizedTensor' because strict_quantization=True."


def test_strict_mode_errors_match_the_reference():
    x = torch.randn(4, 16)
    stub = ff.nn.QuantizerStub(output_quantizer=True)
    F = ff.nn.functional
    for fn in (F.relu, F.silu):
        with pytest.raises(QuantizationError, match=OUTPUT_MSG.replace("(", r"\(")):
            fn(x, strict_quantization=True)
        with pytest.raises(QuantizationError) as e:
            fn(x, output_quantizer=stub, strict_quantization=True)
        assert str(e.value) == _expected("input")
    with pytest.raises(QuantizationError) as e:
        F.layer_norm(x, (16,), output_quantizer=stub, strict_quantization=True)
    assert str(e.value) == _expected("input")
    q = ff.nn.LinearQuantizer(8, symmetric=False)
    q.quantization_range = (torch.tensor(-3.0), torch.tensor(3.0))
    with pytest.raises(QuantizationError) as e:
        F.layer_norm(q(x), (16,), weight=torch.ones(16), output_quantizer=stub, strict_quantization=True)
    assert str(e.value) == _expected("weight")
    with pytest.raises(QuantizationError) as e:
        F.embedding(torch.tensor([0, 1]), torch.randn(4, 8), output_quantizer=stub, strict_quantization=True)
    assert str(e.value) == _expected("weight")
    # the module default is strict, as in the reference: a stub input quantizer leaves a plain tensor
    model = ff.quantize_model(torch.nn.Sequential(torch.nn.ReLU()))
    with pytest.raises(QuantizationError) as e:
        model(x)
    assert str(e.value) == _expected("input")


# ---- the host path against the reference (G19) -----------------------------------------------------------------------------------
def _set(module, name, spec, got):
    bits, symmetric, gran, lo, hi = spec
    granularity = ff.PerTensor() if gran == "tensor" else ff.PerChannel(gran[1])
    q = ff.nn.LinearQuantizer(bits, symmetric=symmetric, granularity=granularity, quantized_dtype=torch.int8)
    q.quantization_range = (torch.as_tensor(lo, dtype=torch.float32), torch.as_tensor(hi, dtype=torch.float32))
    with torch.no_grad():
        q.scale.copy_(got["scale"])
        if got["offset"] is not None:
            q.offset.copy_(got["offset"])
    setattr(module, name, q)


def build_g19_module(case, device="cpu"):
    """The case's module, converted, with its quantizers; returns (module, input)."""
    dtype = case["x"].dtype if "x" in case else case["weight"].dtype
    if case["op"] == "layer_norm":
        module = torch.nn.LayerNorm(case["normalized_shape"], eps=case["eps"]).to(dtype)
        with torch.no_grad():
            module.weight.copy_(case["weight"])
            module.bias.copy_(case["bias"])
        x = case["x"]
    elif case["op"] == "embedding":
        module = torch.nn.Embedding(*case["weight"].shape).to(dtype)
        with torch.no_grad():
            module.weight.copy_(case["weight"])
        x = case["ids"]
    else:
        module = {"relu": torch.nn.ReLU, "silu": torch.nn.SiLU}[case["op"]]()
        x = case["x"]
    module = module.to(device)
    ff.quantize_model(module)
    for name, spec in case["slots"].items():
        _set(module, name, spec, case["params"][name])
    module.to(device)
    return module, x.to(device)


def run_g19_case(case, device="cpu"):
    """(value with a stub output quantizer, output QuantizedTensor) of the case's module."""
    module, x = build_g19_module(case, device)
    out_q = module.output_quantizer
    with torch.no_grad(), ff.strict_quantization(False):
        module.output_quantizer = ff.nn.QuantizerStub(output_quantizer=True)
        value = module(x)
        module.output_quantizer = out_q
        quantized = module(x)
    return value, quantized


@pytest.mark.parametrize("index", range(8))
def test_host_path_equals_the_reference_bit_for_bit(index):
    case = golden("g19_modules.pt")[index]
    value, quantized = run_g19_case(case)
    assert value.dtype == case["value"].dtype
    assert torch.equal(value.view(torch.int16 if value.dtype == torch.bfloat16 else torch.int32), case["value"].view(torch.int16 if value.dtype == torch.bfloat16 else torch.int32)), case["op"]
    assert isinstance(quantized, ff.QuantizedTensor)
    assert torch.equal(quantized.raw_data, case["codes"]), case["op"]
    assert torch.equal(quantized.dequantize(), case["dequantized"]), case["op"]


def test_estimate_ranges_calibrates_the_tiny_opt_model():
    model = quantize_tiny(tiny_opt())
    install_quantizers(model)
    ids = torch.randint(0, 96, (2, 12), generator=torch.Generator().manual_seed(3))
    with ff.strict_quantization(False):
        with ff.estimate_ranges(model, ff.range_setting.running_minmax):
            model(ids)
        out = model(ids)
    assert all(not q.has_uninitialized_params for q in ff.nn.named_quantizers(model) for q in [q[1]])
    assert isinstance(out, ff.QuantizedTensor) and out.shape == (2, 12, 64)
    assert torch.isfinite(out.dequantize()).all()


def test_the_predicates_decline_host_tensors():
    x = torch.randn(4, 16, dtype=torch.bfloat16)
    assert not fused_modules.pointwise_predicate(input=x, output_quantizer=None, strict_quantization=False)
    assert not fused_modules.layer_norm_predicate(input=x, normalized_shape=(16,), output_quantizer=None, strict_quantization=False)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_the_hip_library_exports_the_three_entry_points():
    dll = ctypes.CDLL(str(HIP_SO))
    lib = FFQLibrary(HIP_SO)
    for name in ENTRY_POINTS:
        assert hasattr(dll, name) and name in _cabi.SIGNATURES and name in _cabi.DEVICE_ONLY
        assert getattr(lib, name) is not None
    assert ff.ops.layer_norm_quantize and ff.ops.embedding_quantize and ff.ops.pointwise_quantize
    assert {"layer_norm_quantize", "embedding_quantize", "pointwise_quantize"} <= set(ff.ops.__all__)


def test_the_oracle_loads_without_them():
    lib = load_oracle()
    assert not lib.is_device
    for name in ENTRY_POINTS:
        assert getattr(lib, name) is None


FAKE = 1 << 20  # never dereferenced: every call below returns from the argument checks


def _fan(count=1, bits=8.0, codes=FAKE):
    return FanOut.make(bits, [FAKE] * count, [None] * count, [codes] * count)


def _fan_of_count(n):
    f = _fan()
    f.count = n
    return f


def _ln(lib, x=FAKE, x_dt=DType.BF16, scale=None, offset=None, per_row=0, dt=DType.BF16, rows=4, cols=64, fan=None):
    f = _fan() if fan is None else fan
    return lib.ffq_layer_norm_quantize(x, x_dt, scale, offset, per_row, None, None, dt, rows, cols, 1e-5, None, ctypes.byref(f), None)


def _emb(lib, ids=FAKE, ids_dt=DType.I64, n=4, table=FAKE, table_dt=DType.I8, V=16, D=64, scale=FAKE, per_row=1, group=64, dt=DType.BF16, bad=FAKE):
    f = _fan()
    return lib.ffq_embedding_quantize(ids, ids_dt, n, table, table_dt, V, D, scale, None, per_row, group, dt, None, ctypes.byref(f), bad, None)


def _pw(lib, op=0, x=FAKE, x_dt=DType.I8, scale=FAKE, run=0, dt=DType.BF16, numel=64, fan=None):
    f = _fan() if fan is None else fan
    return lib.ffq_pointwise_quantize(op, x, x_dt, scale, None, run, dt, numel, None, ctypes.byref(f), None)


@pytest.mark.parametrize(
    "call,status",
    [
        (lambda lib: _ln(lib, rows=-1), Status.ERR_ARG),
        (lambda lib: _ln(lib, dt=DType.F32, x_dt=DType.F32), Status.ERR_DTYPE),
        (lambda lib: _ln(lib, x_dt=DType.I8), Status.ERR_DTYPE),              # codes without a scale
        (lambda lib: _ln(lib, cols=0), Status.ERR_EMPTY),
        (lambda lib: _ln(lib, cols=36), Status.ERR_DTYPE),
        (lambda lib: _ln(lib, cols=16392), Status.ERR_DTYPE),
        (lambda lib: _ln(lib, fan=_fan_of_count(4)), Status.ERR_ARG),
        (lambda lib: _ln(lib, fan=_fan(bits=9.0)), Status.ERR_PRECISION),
        (lambda lib: _ln(lib, fan=_fan(codes=None)), Status.ERR_ARG),
        (lambda lib: _ln(lib, x=None), Status.ERR_ARG),
        (lambda lib: _ln(lib, x=FAKE + 8), Status.ERR_ARG),                   # misaligned
        (lambda lib: _ln(lib, rows=0), Status.OK),
        (lambda lib: _emb(lib, ids_dt=DType.I16), Status.ERR_DTYPE),
        (lambda lib: _emb(lib, table_dt=DType.F16), Status.ERR_DTYPE),
        (lambda lib: _emb(lib, D=60, group=60), Status.ERR_DTYPE),
        (lambda lib: _emb(lib, group=48), Status.ERR_TILE_DIVIDE),
        (lambda lib: _emb(lib, group=4), Status.ERR_DTYPE),
        (lambda lib: _emb(lib, group=1, per_row=1), Status.ERR_DTYPE),
        (lambda lib: _emb(lib, bad=None), Status.ERR_ARG),
        (lambda lib: _emb(lib, scale=None), Status.ERR_ARG),
        (lambda lib: _emb(lib, V=0), Status.ERR_EMPTY),
        (lambda lib: _emb(lib, n=0), Status.OK),
        (lambda lib: _pw(lib, op=2), Status.ERR_ARG),
        (lambda lib: _pw(lib, numel=60), Status.ERR_DTYPE),
        (lambda lib: _pw(lib, run=24), Status.ERR_DTYPE),
        (lambda lib: _pw(lib, x_dt=DType.I16), Status.ERR_DTYPE),
        (lambda lib: _pw(lib, scale=None), Status.ERR_DTYPE),                 # int8 codes without a scale
        (lambda lib: _pw(lib, x=None), Status.ERR_ARG),
        (lambda lib: _pw(lib, numel=0), Status.OK),
    ],
)
def test_argument_checks_need_no_device(call, status):
    lib = FFQLibrary(HIP_SO)
    assert call(lib) == status
    if status != Status.OK:
        assert lib.ffq_last_error()


def test_the_new_kernels_spill_nothing_and_use_no_scratch():
    if kernel_resources.readelf() is None or not kernel_resources.DEFAULT_LIBRARY.exists():
        pytest.skip("llvm-readelf or the built library is missing")
    rows = [k for k in kernel_resources.kernel_resources() if any(n in str(k["name"]) for n in KERNELS)]
    for needle, count in zip(KERNELS, (30, 16, 15)):
        assert sum(needle in str(k["name"]) for k in rows) == count, needle
    bad = {str(k["name"]): k for k in rows if k["vgpr_spill_count"] or k["private_segment_fixed_size"]}
    assert not bad, bad
    assert all(k["group_segment_fixed_size"] <= 16384 for k in rows)
