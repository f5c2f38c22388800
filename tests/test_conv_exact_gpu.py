"""Every convolution kernel on drawn geometries against exact sums, on the MI355X (tests/conv_exact.py; docs/parity.md, "Order-free
convolutions"): power-of-two scales, integer offsets and codes small enough that every step of the affine epilogue is an integer
below 2^24 times a power of two, so the fp32 result is the float64 ATen convolution of the dequantized operands bit for bit — in any
summation order, with or without FMA. The fp32 output is that value, bf16 / fp16 its one rounding, the re-quantizing epilogue's codes
``clamp(rne(round_to(y, y_dt) / s - o))`` in float64 with a power-of-two scale that puts exact halves inside the code range.

One test per family, a block of 8 of its 64 draws per id. The draws alternate between the ``ops`` entry on raw codes (part of them
channels-last) and the ``ff.nn.functional`` operator on QuantizedTensors; 1-D draws reach the 2-D entry points as H = KH = 1. Every
launch is counted: a silent fallback or a declined draw fails the test. The last draw of a block runs twice and reproduces itself.
A draw that fails is a bug in the kernel or its host prologue: it is fixed there and the draw stays below the sweep as a named
regression case (``check(family, index, launches)`` runs one draw); none has failed so far."""

import pytest
import torch

import conv_exact

from conv_exact import BLOCK, FAMILIES, N_DRAWS
from fastforward_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BLOCKS = range(N_DRAWS // BLOCK)


@pytest.fixture(autouse=True)
def _inference():
    """Inference, as the models run: under grad mode the quantizers' learnable parameters send every call to the chain."""
    with torch.no_grad():
        yield


@pytest.fixture()
def launches(monkeypatch):
    """{entry: number of calls} of the four convolution wrappers of fastforward_amd.ops"""
    counts = {family.entry: 0 for family in FAMILIES.values()}
    for name in counts:
        real = getattr(ops, name)

        def counted(*a, _real=real, _name=name, **k):
            counts[_name] += 1
            return _real(*a, **k)

        monkeypatch.setattr(ops, name, counted)
    return counts


def run(c):
    """The draw's output on the device, as a plain tensor: the ``ops`` entry on raw codes or the functional call on QuantizedTensors."""
    if c.draw.route == "ops":
        return conv_exact.run_ops(c, DEV, ops)
    out = conv_exact.run_functional(c, DEV)
    if c.draw.mode == "int8":
        assert isinstance(out, conv_exact.ff.QuantizedTensor), str(c.draw)
        return out.raw_data
    return out


def check(family, index, launches):
    """One draw: one counted launch of the family's entry point (and of no other), the expected tensor bit for bit."""
    c = conv_exact.case(family, index)
    before = dict(launches)
    got = run(c)
    entry = FAMILIES[family].entry
    assert launches == {**before, entry: before[entry] + 1}, f"{c.draw}: launches {before} -> {launches}"
    got = got.cpu()
    assert got.is_contiguous() and torch.equal(got, c.expected), f"{c.draw}: {conv_exact.first_difference(got, c.expected)}"
    return c, got


def sweep(family, block, launches):
    for index in range(block * BLOCK, (block + 1) * BLOCK):
        c, got = check(family, index, launches)
    again = run(c).cpu()
    assert torch.equal(again, got), f"{c.draw}, the second call: {conv_exact.first_difference(again, got)}"
    assert launches[FAMILIES[family].entry] == BLOCK + 1 and sum(launches.values()) == BLOCK + 1


@pytest.mark.parametrize("block", BLOCKS)
def test_conv1d_and_conv2d_draws_are_exact(block, launches):
    sweep("conv", block, launches)


@pytest.mark.parametrize("block", BLOCKS)
def test_conv3d_draws_are_exact(block, launches):
    sweep("conv3d", block, launches)


@pytest.mark.parametrize("block", BLOCKS)
def test_conv_transpose1d_and_conv_transpose2d_draws_are_exact(block, launches):
    sweep("conv_transpose", block, launches)


@pytest.mark.parametrize("block", BLOCKS)
def test_depthwise_conv1d_and_conv2d_draws_are_exact(block, launches):
    sweep("depthwise", block, launches)
