"""The order-free convolution cases of tests/conv_exact.py without a GPU: every draw of the committed seeds keeps the bound that makes
its result exact in fp32, is a call the family's predicate and entry point take, has the float64 ATen convolution as its value — which
the fp32 host chain (``ff.nn.functional`` on host QuantizedTensors: dequantize, ATen's fp32 convolution, the output quantizer)
reproduces bit for bit —, and the 64 draws of a family together cover what docs/parity.md lists."""

import math

import pytest
import torch

import conv_exact

from conv_exact import FAMILIES, LIMIT, N_DRAWS, REAL
from fastforward_amd import fused_conv, fused_conv3d, fused_conv_transpose, fused_depthwise

KERNELS = {"conv": fused_conv.KERNELS, "conv3d": fused_conv3d.KERNELS, "conv_transpose": fused_conv_transpose.KERNELS,
           "depthwise": fused_depthwise.KERNELS}


@pytest.fixture(autouse=True)
def _inference():
    with torch.no_grad():
        yield


@pytest.mark.parametrize("family", list(FAMILIES))
def test_every_draw_keeps_the_bound_and_the_documented_limits(family):
    rule = FAMILIES[family]
    draws = conv_exact.draws(family)
    assert len(draws) == N_DRAWS and [d.index for d in draws] == list(range(N_DRAWS))
    for d in draws:
        R = d.reduction
        assert d.A in (16, 32, 64, 128) and R * (d.A ** 2 + abs(d.ox) * d.A + d.owmax * d.A + abs(d.ox) * d.owmax) < LIMIT, str(d)
        assert d.bound < LIMIT, str(d)  # ... with the bias's 128
        assert d.dims in rule.functional and 1 <= d.B <= 3 and max(d.size) <= rule.extent[d.dims], str(d)
        assert d.positions * d.OC <= conv_exact.MAX_OUTPUTS and min(d.out_size) >= 1, str(d)
        assert all(1 <= k <= 5 and 1 <= s <= 4 and 1 <= dil <= 3 and 0 <= p <= dil * (k - 1) + 2
                   for k, s, p, dil in zip(d.kernel, d.stride, d.padding, d.dilation)), str(d)
        if rule.kind == "transposed":
            want = tuple((n - 1) * s - 2 * p + dil * (k - 1) + op + 1
                         for n, k, s, p, dil, op in zip(d.size, d.kernel, d.stride, d.padding, d.dilation, d.output_padding))
            assert all(0 <= op < max(s, dil) for op, s, dil in zip(d.output_padding, d.stride, d.dilation)), str(d)
            assert max(want) <= rule.extent[d.dims], str(d)
        else:
            want = tuple((n + 2 * p - dil * (k - 1) - 1) // s + 1 for n, k, s, p, dil in zip(d.size, d.kernel, d.stride, d.padding, d.dilation))
            assert not any(d.output_padding)
        assert d.out_size == want, str(d)
        if rule.kind == "depthwise":
            assert d.C > 1 and d.OC % d.C == 0 and d.OC // d.C in (1, 2, 3) and d.taps <= fused_depthwise.MAX_TAPS, str(d)
        else:
            assert d.C * d.taps <= fused_conv.MAX_REDUCTION, str(d)
        assert not d.channels_last or (d.route == "ops" and d.C % 16 == 0), str(d)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_the_predicate_takes_every_draw(family, monkeypatch):
    """With the device check out of the way (the rules read no memory): no draw is declined."""
    monkeypatch.setattr("fastforward_amd.fused_conv._on_device", lambda *t: True)
    rule = FAMILIES[family]
    for index in range(N_DRAWS):
        c = conv_exact.case(family, index)
        d = c.draw
        dt = REAL[d.y_dt if d.mode == "int8" else d.mode]
        granularity = conv_exact.ff.PerChannel(rule.oc_axis) if len(d.b) > 1 else conv_exact.ff.PerTensor()
        xq = conv_exact.quantized(c.x_codes, c.x_scale, c.x_offset, conv_exact.ff.PerTensor(), dt)
        wq = conv_exact.quantized(c.w_codes, c.w_scale, c.w_offset, granularity, dt)
        geometry = dict(stride=d.stride, padding=d.padding, dilation=d.dilation)
        if rule.kind == "transposed":
            geometry["output_padding"] = d.output_padding
        assert KERNELS[family].supported(d.dims, input=xq, weight=wq, bias=None if c.bias is None else c.bias.to(dt), groups=d.groups,
                                         output_quantizer=None, strict_quantization=False, **geometry), str(d)


@pytest.mark.parametrize("block", range(N_DRAWS // conv_exact.BLOCK))
@pytest.mark.parametrize("family", list(FAMILIES))
def test_the_float64_value_is_exact_in_fp32_and_the_host_chain_gives_it(family, block):
    for index in range(block * conv_exact.BLOCK, (block + 1) * conv_exact.BLOCK):
        c = conv_exact.case(family, index)
        d = c.draw
        assert int(c.x_codes.min()) >= -d.A and int(c.x_codes.max()) < d.A and int(c.w_codes.min()) >= -d.A and int(c.w_codes.max()) < d.A
        assert c.w_offset is None or float(c.w_offset.abs().max()) == d.owmax
        # y is an integer below 2^24 times sx * sw[n]: fp32 holds it
        unit = (c.x_scale.double() * c.w_scale.double()).reshape(1, -1, *[1] * d.dims)
        integer = c.y / unit
        assert torch.equal(integer, torch.round(integer)) and float(integer.abs().max()) < LIMIT, str(d)
        assert torch.equal(c.y.float().double(), c.y), str(d)
        if c.bias is not None:
            for dt in REAL.values():
                assert torch.equal(c.bias.to(dt).double(), c.bias_m * c.x_scale.double() * c.w_scale.double()), str(d)
        host = conv_exact.run_functional(c, "cpu", torch.float32, fused_output=False)
        assert host.dtype == torch.float32 and torch.equal(host, c.y.float()), f"{d}: {conv_exact.first_difference(host, c.y.float())}"
        assert c.expected.shape == c.y.shape and c.expected.dtype == (torch.int8 if d.mode == "int8" else REAL[d.mode])
        if d.mode == "int8":
            lo, hi = conv_exact.code_range(d.bits)
            scale, offset = float(c.out_scale), 0.0 if c.out_offset is None else float(c.out_offset)
            assert math.log2(scale) == round(math.log2(scale)) and offset == round(offset), str(d)
            assert lo <= int(c.expected.min()) and int(c.expected.max()) <= hi, str(d)
            if d.y_dt == "f32":  # the host chain's own output quantizer (A1 in fp32) on the same value
                codes = conv_exact.output_quantizer(c, "cpu")(host)
                assert torch.equal(codes.raw_data, c.expected), f"{d}: {conv_exact.first_difference(codes.raw_data, c.expected)}"


def _count(draws, what):
    return sum(1 for d in draws if what(d))


@pytest.mark.parametrize("family", list(FAMILIES))
def test_the_draws_cover_what_the_kernels_branch_on(family):
    rule = FAMILIES[family]
    draws = conv_exact.draws(family)
    counts = {d.index: conv_exact.tap_counts(d) for d in draws}
    covered = {
        "a position with no tap inside the image": _count(draws, lambda d: any(min(axis) == 0 for axis in counts[d.index])),
        "more than 128 output positions": _count(draws, lambda d: d.positions > 128),
        "OC above 128": _count(draws, lambda d: d.OC > 128),
        "an output extent of 1 on some axis": _count(draws, lambda d: min(d.out_size) == 1),
        "|ox| > 127": _count(draws, lambda d: abs(d.ox) > 127),
        **{f"output mode {mode}": _count(draws, lambda d, mode=mode: d.mode == mode) for mode in conv_exact.MODES},
    }
    if rule.pads_channels:
        covered["taps * Cp not a multiple of 64"] = _count(draws, lambda d: d.taps * ((d.C + 15) // 16 * 16) % 64 != 0)
    if rule.kind == "transposed":
        covered["a phase without a tap"] = _count(draws, conv_exact.phase_without_tap)
        covered["gcd(stride, dilation) > 1"] = _count(draws, lambda d: any(math.gcd(s, dil) > 1 for s, dil in zip(d.stride, d.dilation)))
        assert _count(draws, lambda d: any(d.output_padding)) >= 8
    if rule.kind == "depthwise":
        assert {d.OC // d.C for d in draws} == {1, 2, 3}
    assert all(n >= 8 for n in covered.values()), covered
    assert _count(draws, lambda d: d.positions > 256) >= 2
    assert {127, 128, 129} <= {d.OC for d in draws}
    # the forms the routes rotate over, each on both routes; both ranks; channels-last codes
    for route in ("ops", "functional"):
        mine = [d for d in draws if d.route == route]
        assert len(mine) == N_DRAWS // 2
        assert {d.x_form for d in mine} == {d.w_form for d in mine} == {"none", "zero", "real"}
        assert {len(d.b) > 1 for d in mine} == {False, True} and {d.dims for d in mine} == set(rule.functional)
        assert {d.mode for d in mine} == set(conv_exact.MODES) and {d.bias is None for d in mine} == {False, True}
    requant = [d for d in draws if d.mode == "int8"]
    assert {d.bits for d in requant} == {4, 8} and {d.out_offset for d in requant} == {False, True} and {d.y_dt for d in requant} == set(REAL)
    assert {d.owmax for d in draws} == {0, 5, 32} and {d.ox for d in draws} >= {0, 200, -200}
    assert _count(draws, lambda d: d.channels_last) >= 4
    assert _count(draws, lambda d: d.A < 128) >= 1 or rule.kind == "depthwise"
    # the re-quantizing draws: exact halves strictly inside the code range (rne decides the code), and codes on both clamps
    cases = [conv_exact.case(family, d.index) for d in requant]
    assert sum(1 for c in cases if c.ties > 0) >= 8, [c.ties for c in cases]
    assert sum(1 for c in cases if len(torch.unique(c.expected)) > 2) >= 8
    assert sum(1 for c in cases if {int(c.expected.min()), int(c.expected.max())} == set(conv_exact.code_range(c.draw.bits))) >= 4
