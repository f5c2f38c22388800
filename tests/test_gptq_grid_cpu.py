"""The grid form of the GPTQ block kernel without a GPU: the symbol, what hipcc emitted for it, its argument checks (which all
run before any device call), and the oracle, which does not export it, keeping gptq() on the column loop."""

import ctypes
import sys

import pytest
import torch

import parity_cases

from conftest import HIP_SO, ROOT, load_oracle
from fastforward_amd import _cabi, ops
from fastforward_amd._cabi import FFQLibrary, Status
from helpers import same_with_nan

sys.path.insert(0, str(ROOT / "tools"))

import kernel_resources  # noqa: E402

NAME = "ffq_gptq_block_grid"


def test_the_hip_library_exports_the_grid_entry_point():
    assert hasattr(ctypes.CDLL(str(HIP_SO)), NAME)
    assert NAME in _cabi.DEVICE_ONLY and NAME in _cabi.SIGNATURES
    assert FFQLibrary(HIP_SO).ffq_gptq_block_grid is not None


def test_the_grid_kernels_spill_nothing_and_fit_in_lds():
    if kernel_resources.readelf() is None or not kernel_resources.DEFAULT_LIBRARY.exists():
        pytest.skip("llvm-readelf or the built library is missing")
    rows = {str(k["name"]): k for k in kernel_resources.kernel_resources() if "gptq_block_grid_kernel" in str(k["name"]) or "gptq_refit_kernel" in str(k["name"])}
    assert len(rows) == 2, sorted(rows)
    for name, k in rows.items():
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (name, k)
        assert k["group_segment_fixed_size"] <= 160 * 1024, (name, k)


# every call below fails (or returns early) in the argument checks: the addresses are never dereferenced
FAKE = 1 << 20


def _call(lib, rows=64, cols=128, col0=0, block_cols=64, tile=(1, 32), refit=1, weights=FAKE, quantized=FAKE, errors=FAKE,
          hinv=FAKE, hinv_stride=128, scale=FAKE, offset=None, order=None):
    return lib.ffq_gptq_block_grid(weights, quantized, errors, rows, cols, col0, block_cols, hinv, hinv_stride, scale, offset,
                                   tile[0], tile[1], order, refit, 1, 1, 4.0, None)


@pytest.mark.parametrize(
    "kwargs,status",
    [
        (dict(rows=-1), Status.ERR_ARG),
        (dict(col0=-32), Status.ERR_ARG),
        (dict(tile=(1, -32)), Status.ERR_ARG),
        (dict(block_cols=129), Status.ERR_DTYPE),
        (dict(rows=0), Status.OK),
        (dict(block_cols=0), Status.OK),
        (dict(weights=None), Status.ERR_ARG),
        (dict(quantized=None), Status.ERR_ARG),
        (dict(errors=None), Status.ERR_ARG),
        (dict(hinv=None), Status.ERR_ARG),
        (dict(scale=None), Status.ERR_ARG),
        (dict(tile=(1, 48)), Status.ERR_TILE_DIVIDE),
        (dict(tile=(3, 32)), Status.ERR_TILE_DIVIDE),
        (dict(tile=(0, 32)), Status.ERR_TILE_DIVIDE),
        (dict(col0=96), Status.ERR_ARG),             # block past the last column
        (dict(hinv_stride=32), Status.ERR_ARG),       # block past Hinv
        (dict(cols=1 << 31, tile=(1, 1)), Status.ERR_ARG),
    ],
)
def test_argument_checks_need_no_device(kwargs, status):
    lib = FFQLibrary(HIP_SO)
    assert _call(lib, **kwargs) == status
    if status != Status.OK:
        assert lib.ffq_last_error()


def test_the_oracle_has_no_grid_entry_point():
    lib = load_oracle()
    assert lib.ffq_gptq_block_grid is None and not lib.is_device
    assert lib.ffq_gptq_block is not None


def test_ops_declines_under_the_oracle(oracle_backend):
    w = torch.randn(8, 64)
    args = (w, torch.zeros_like(w), torch.zeros_like(w), 0, 32, torch.eye(64), torch.ones(8, 2), None, (1, 32), 4.0)
    assert ops.gptq_block_grid(*args) is False


@pytest.mark.parametrize("name", ["group16_asym_4bit", "channel0_sym_3bit_actorder", "channel1_sym_4bit"])
def test_gptq_on_the_cpu_still_equals_the_reference(name, oracle_backend):
    (case,) = [c for c in parity_cases.golden("g13_gptq.pt") if c["name"] == name]
    layer = parity_cases.run_gptq_case(case, "cpu", fused=True)
    assert same_with_nan(layer.weight.detach(), case["result"]), name
    assert same_with_nan(layer.weight_quantizer.scale.detach(), case["scale"]), name


def test_device_only_entry_points_may_be_missing_from_a_host_library_only(monkeypatch):
    monkeypatch.setitem(_cabi.SIGNATURES, "ffq_not_exported_anywhere", (ctypes.c_int, []))
    monkeypatch.setattr(_cabi, "DEVICE_ONLY", _cabi.DEVICE_ONLY | {"ffq_not_exported_anywhere"})
    assert FFQLibrary(load_oracle().path).ffq_not_exported_anywhere is None
    with pytest.raises(ImportError, match="ffq_not_exported_anywhere"):
        FFQLibrary(HIP_SO)
