"""GPTQ through the grid form of the block kernel (ffq_gptq_block_grid) on an MI355X.

Grouped (PerBlock / PerTile), per-input-channel (PerChannel(1)) and act-order weight quantizers take one launch per block
(plus one refit launch for grouped weights without act-order) instead of the column loop. The loop is the yardstick: on the
same device and inputs the fused result must equal it bit for bit (weight, scale, offset).
"""

import pytest
import torch

import fastforward_amd as ff
import parity_cases

from fastforward_amd.quantization import gptq as gptq_module
from helpers import same_with_nan

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _backend(hip_backend):
    yield


def _granularity(name):
    if name == "tile4x32":
        return ff.PerTile((4, 32))
    if name == "channel1":
        return ff.PerChannel(1)
    return ff.PerBlock(block_dims=1, block_sizes=int(name[1:]), per_channel_dims=0)


# name: (rows, cols, granularity, bits, symmetric, block)
CASES = {
    "g16_asym4_ragged": (300, 208, "g16", 4, False, 64),       # 3 full blocks + a 16-column one; rows not a multiple of 64 / 256
    "g32_sym4": (200, 224, "g32", 4, True, 64),
    "g48_asym3_straddle64": (136, 240, "g48", 3, False, 64),   # groups straddle 64-column blocks
    "g48_sym8_straddle32": (72, 240, "g48", 8, True, 32),      # and 32-column blocks
    "g128_sym4_block32": (130, 384, "g128", 4, True, 32),      # a group wider than the block
    "g128_asym8_ragged": (257, 384, "g128", 8, False, 112),    # 112-column blocks, the last one 48 wide
    "tile4x32_asym4": (260, 160, "tile4x32", 4, False, 64),
    "tile4x32_sym3": (68, 192, "tile4x32", 3, True, 32),
    "channel1_sym4": (300, 200, "channel1", 4, True, 64),
    "channel1_asym3": (96, 136, "channel1", 3, False, 32),
}


def _inputs(rows, cols, seed):
    gen = torch.Generator().manual_seed(seed)
    weight = torch.randn(rows, cols, generator=gen) * 0.05
    acts = [torch.randn(2, 24, cols, generator=gen) * (1.0 + torch.rand(cols, generator=gen)) for _ in range(2)]
    return weight, acts


def _run(weight, acts, granularity, bits, symmetric, block, actorder, fused):
    layer = torch.nn.Linear(weight.shape[1], weight.shape[0], bias=False)
    with torch.no_grad():
        layer.weight.copy_(weight)
    ff.quantize_model(layer)
    layer.to(DEV)
    layer.weight_quantizer = ff.nn.LinearQuantizer(bits, granularity=granularity, symmetric=symmetric, device=DEV)
    with torch.no_grad(), ff.strict_quantization(False):
        gptq_module.gptq(layer, [((a.to(DEV),), {}) for a in acts], block_size=block, actorder=actorder, fused=fused)
    return layer


def _case(name, actorder, fused, weight=None):
    rows, cols, gran, bits, symmetric, block = CASES[name]
    w, acts = _inputs(rows, cols, seed=sum(map(ord, name)))
    return _run(w if weight is None else weight, acts, _granularity(gran), bits, symmetric, block, actorder, fused)


def _assert_same(fused, loop, what):
    assert torch.equal(fused.weight.detach().cpu(), loop.weight.detach().cpu()), what
    fq, lq = fused.weight_quantizer, loop.weight_quantizer
    assert same_with_nan(fq.scale.detach().cpu(), lq.scale.detach().cpu()), what
    assert (fq.offset is None) == (lq.offset is None), what
    if fq.offset is not None:
        assert same_with_nan(fq.offset.detach().cpu(), lq.offset.detach().cpu()), what


def _assert_on_grid(layer, what):
    """Every weight is a point of the final quantizer's grid: each group was refitted before any of its columns was snapped."""
    with torch.no_grad(), ff.strict_quantization(False):
        again = layer.weight_quantizer(layer.weight).dequantize()
    assert torch.equal(again.detach().cpu(), layer.weight.detach().cpu()), what


@pytest.mark.parametrize("actorder", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_equals_the_column_loop(name, actorder):
    fused = _case(name, actorder, fused=True)
    loop = _case(name, actorder, fused=False)
    _assert_same(fused, loop, (name, actorder))
    _assert_on_grid(fused, (name, actorder))


@pytest.mark.parametrize("actorder", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_grouped_weights_never_take_the_column_loop(name, actorder, monkeypatch):
    def refuse(self, start, stop):
        raise AssertionError(f"column loop taken for columns {start}:{stop}")

    monkeypatch.setattr(gptq_module._Sweep, "block_column_by_column", refuse)
    _case(name, actorder, fused=True)


def test_one_sided_refit_is_decided_per_group():
    """Symmetric, allow_one_sided: group 0 is all non-negative (the first refit sees it unchanged), the others are not. Only
    group 0 switches to the one-sided grid (offset -int_min); the decision is not shared across groups."""
    rows, cols = 192, 128
    w, acts = _inputs(rows, cols, seed=11)
    w[:, :32] = w[:, :32].abs() + 0.01
    layers = [_run(w, acts, _granularity("g32"), 4, True, 64, False, fused) for fused in (True, False)]
    _assert_same(layers[0], layers[1], "one-sided")
    _assert_on_grid(layers[0], "one-sided")
    offset = layers[0].weight_quantizer.offset.detach().cpu().view(rows, cols // 32)
    assert bool((offset[:, 0] == 8).all()) and bool((offset[:, 1:] == 0).all()), offset


@pytest.mark.parametrize("name", ["group16_asym_4bit", "channel1_sym_4bit"])
def test_g13_grouped_fixtures_on_the_device(name, monkeypatch):
    (case,) = [c for c in parity_cases.golden("g13_gptq.pt") if c["name"] == name]
    loop = parity_cases.run_gptq_case(case, DEV, fused=False)
    monkeypatch.setattr(gptq_module._Sweep, "block_column_by_column", lambda *a: pytest.fail("column loop taken"))
    fused = parity_cases.run_gptq_case(case, DEV, fused=True)
    _assert_same(fused, loop, name)
    _assert_on_grid(fused, name)


def test_no_host_sync_per_column_or_group(monkeypatch):
    """The host round trips of a fused grouped run do not grow with the number of columns or groups."""
    counts = {"n": 0}
    item, boolean = torch.Tensor.item, torch.Tensor.__bool__

    def counted_item(self):
        counts["n"] += self.is_cuda
        return item(self)

    def counted_bool(self):
        counts["n"] += self.is_cuda
        return boolean(self)

    monkeypatch.setattr(torch.Tensor, "item", counted_item)
    monkeypatch.setattr(torch.Tensor, "__bool__", counted_bool)
    seen = {}
    for cols in (512, 1024):
        for actorder in (False, True):
            w, acts = _inputs(256, cols, seed=cols)
            counts["n"] = 0
            _run(w, acts, _granularity("g32"), 4, True, 128, actorder, fused=True)
            seen[(cols, actorder)] = counts["n"]
    assert seen[(512, False)] == seen[(1024, False)] and seen[(512, True)] == seen[(1024, True)], seen


@pytest.mark.parametrize("actorder", [False, True])
@pytest.mark.parametrize("group", [32, 128])
@pytest.mark.parametrize("rows", [4096, 14336])
def test_full_size_w4_grouped(rows, group, actorder):
    cols = 4096
    gen = torch.Generator(device=DEV).manual_seed(rows + group)
    weight = (torch.randn(rows, cols, generator=gen, device=DEV) * 0.02).cpu()
    acts = [torch.randn(4, 256, cols, generator=gen, device=DEV) for _ in range(2)]
    layers = [_run(weight, acts, _granularity(f"g{group}"), 4, True, 128, actorder, fused) for fused in (True, False)]
    _assert_same(layers[0], layers[1], (rows, group, actorder))
    _assert_on_grid(layers[0], (rows, group, actorder))


def test_refits_on_the_device_move_the_parameter_versions(monkeypatch):
    """Code caches key on the quantizer parameters' `_version` (llama.py): a refit written by the kernel must move it, as the
    loop's indexed writes do."""
    rows, cols, gran, bits, symmetric, block = CASES["g32_sym4"]
    w, acts = _inputs(rows, cols, seed=5)
    layer = torch.nn.Linear(cols, rows, bias=False)
    with torch.no_grad():
        layer.weight.copy_(w)
    ff.quantize_model(layer)
    layer.to(DEV)
    layer.weight_quantizer = ff.nn.LinearQuantizer(bits, granularity=_granularity(gran), symmetric=symmetric, device=DEV)
    seen = []
    launch = gptq_module.ops.gptq_block_grid

    def recording(*args, **kwargs):
        q = layer.weight_quantizer
        seen.append((q.scale._version, q.offset._version))
        return launch(*args, **kwargs)

    monkeypatch.setattr(gptq_module.ops, "gptq_block_grid", recording)
    with torch.no_grad(), ff.strict_quantization(False):
        gptq_module.gptq(layer, [((a.to(DEV),), {}) for a in acts], block_size=block)
    q = layer.weight_quantizer
    assert seen and q.scale._version > seen[-1][0] and q.offset._version > seen[-1][1], (seen, q.scale._version, q.offset._version)
