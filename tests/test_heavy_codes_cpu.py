"""The operand patterns of tests/heavy_codes.py earn their place, without a GPU: on ``low`` and ``mirror`` every wrong form of
the fp32 epilogue that today's uniform-code tests cannot see (an FMA-contracted chain, a reordered sum, a truncating int -> float
conversion, the exact sum rounded once) differs from the stated chain on at least 1 % of the outputs — a condition on the INPUTS,
not on any kernel; ``ties`` holds at least 1000 exact halfway accumulators. The restated expectations themselves are checked on
host memory: the linear against the C oracle (its double-precision restatement of the reference chain), the convolutions — for
which neither the oracle nor the package has a host kernel — against the float64 value of the same affine operands."""

import pytest
import torch

import heavy_codes as hc

from fastforward_amd import ops

M = N = 64
K = 4096


@pytest.fixture(scope="module")
def terms():
    out = {}
    for pattern in ("low", "mirror"):
        o = hc.operands(pattern, M, N, K)
        acc = hc.accumulator64(o.xq, o.wq)
        out[pattern] = (o, acc, hc.terms64(acc, o.xq, o.wq, o.ox, o.ow))
    return out


@pytest.mark.parametrize("pattern", ["low", "mirror"])
def test_every_term_is_heavy_and_the_sum_is_light(pattern, terms):
    _, _, (a, p1, p2, p3) = terms[pattern]
    assert float(a.abs().min()) >= 2**24
    for t in (a, p1, p2, p3):
        assert 2.0e7 < float(t.abs().min()) and float(t.abs().max()) < 5.0e7
    # (mirror: -(-128) becomes 127, so code + offset is 8 where low has -9, and the sum is a little larger than low's 4e5)
    assert float((a + p1 + p2 + p3).abs().max()) <= (4.0e5 if pattern == "low" else 2.0**19)


@pytest.mark.parametrize("pattern", ["low", "mirror"])
def test_each_wrong_epilogue_differs_on_at_least_one_percent_of_the_outputs(pattern, terms):
    o, acc, (a, p1, p2, p3) = terms[pattern]
    stated = hc.restated_v(acc, o.xq, o.wq, o.ox, o.ow)
    counts = {name: int((v != stated).sum()) for name, v in hc.wrong_epilogues(a, p1, p2, p3).items()}
    print(pattern, counts)
    assert len(counts) == 5
    for name, count in counts.items():
        assert count >= 0.01 * stated.numel(), f"{pattern}: {name} differs on {count} of {stated.numel()} outputs only"
    # ... and through the scales: the fp32 outputs differ, not only v
    y = hc.restated_linear(acc, o.xq, o.wq, o.sx, o.ox, o.sw, o.ow)
    scale = o.sx.reshape(-1, 1) * o.sw.reshape(1, -1)
    for name, v in hc.wrong_epilogues(a, p1, p2, p3).items():
        assert int((scale * v != y).sum()) >= 0.01 * y.numel(), name


@pytest.mark.parametrize("pattern", ["low", "mirror"])
def test_the_stated_chain_stays_within_the_sum_of_its_half_ulps(pattern, terms):
    o, acc, (a, p1, p2, p3) = terms[pattern]
    error = (hc.restated_v(acc, o.xq, o.wq, o.ox, o.ow).double() - (a + p1 + p2 + p3)).abs()
    assert bool((error <= hc.rounding_bound(a, p1, p2, p3)).all())
    assert float(error.max()) > 0  # the regime: the chain does round


def test_ties_census():
    xq, wq = hc.codes("ties", M, N, K)
    acc = hc.accumulator64(xq, wq)
    low_band = (acc >= 2**24) & (acc < 2**25) & (acc % 2 == 1)
    high_band = (acc >= 2**25) & (acc < 2**26) & (acc % 4 == 2)
    assert int(low_band.sum()) >= 300 and int(high_band.sum()) >= 300
    assert int(low_band.sum() + high_band.sum()) >= 1000
    halfway = low_band | high_band
    assert bool((acc.float().double() != acc)[halfway].all())  # each of them rounds
    # both directions occur: round-half-even goes up for some and down for others
    assert bool((acc.float().double() > acc)[halfway].any()) and bool((acc.float().double() < acc)[halfway].any())


def test_saturated_holds_every_sign_pairing():
    xq, wq = hc.codes("saturated", M, N, K)
    assert set(xq.unique().tolist()) == set(wq.unique().tolist()) == {-128, 127}
    pairs = {(int(xq[m, K - 1]), int(wq[n, K - 1])) for m in range(4) for n in range(8)}
    assert pairs == {(-128, -128), (-128, 127), (127, -128), (127, 127)}
    assert float(hc.accumulator64(xq, wq).abs().max()) >= 2**25


def test_patterns_are_deterministic():
    for pattern in hc.PATTERNS:
        a, b = hc.codes(pattern, 5, 9, 2048), hc.codes(pattern, 5, 9, 2048)
        assert a[0].dtype == torch.int8 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- the linear on host memory against the C oracle -----------------------------------------------------------------------------------
def _oracle_tolerance(o, acc, sx, ox, sw, ow, bias):
    """|oracle - restated| in fp32 out. The oracle dequantizes both operands in fp32 — (q + o) is exact, the product with the scale
    rounds once: relative 2^-24 each — sums the products in double and rounds once; the restated chain carries rounding_bound on v,
    two roundings of (sx * sw) * v and one of the bias add. Derived from the formats; nothing here is measured."""
    a, p1, p2, p3 = hc.terms64(acc, o.xq, o.wq, ox, ow)
    zero = torch.zeros(1)
    oxr = (zero if ox is None else torch.round(ox)).double().reshape(-1, 1)
    owr = (zero if ow is None else torch.round(ow)).double().reshape(-1, 1)
    absdot = (o.xq.double() + oxr).abs() @ (o.wq.double() + owr).abs().T
    scale = sx.double().reshape(-1, 1) * sw.double().reshape(1, -1)
    y = scale * (a + p1 + p2 + p3)
    b = torch.zeros(1, dtype=torch.float64) if bias is None else bias.double()[None, :]
    return scale * (2.0**-23 * absdot + hc.rounding_bound(a, p1, p2, p3)) * (1 + 2.0**-20) + 2.0**-21 * (y.abs() + b.abs())


@pytest.mark.parametrize("pattern", hc.PATTERNS)
@pytest.mark.parametrize("m,n,k", [(64, 64, 4096), (65, 72, 4112), (1, 8, 4096)], ids=str)
def test_restated_linear_against_the_oracle(pattern, m, n, k, oracle_backend):
    o = hc.operands(pattern, m, n, k)
    acc = hc.accumulator64(o.xq, o.wq)
    bias = (torch.arange(n, dtype=torch.float32) % 13 - 6.0) * 0.37
    variants = [(False, "native", None), (True, "real", bias), (False, "zero", None)]
    for per_token, ow_kind, b in variants:
        sx, ox, sw, ow = hc.parameters(pattern, m, n, per_token=per_token, ow_kind=ow_kind)
        want = hc.restated_linear(acc, o.xq, o.wq, sx, ox, sw, ow, b)
        got = ops.linear_w8a8(o.xq, o.wq, sx, ox, sw, ow, bias=b, out_dtype=torch.float32)
        if ox is None and ow is None and b is None:  # unit scales: the oracle's double sum is the exact integer, rounded once
            assert torch.equal(got, want) and torch.equal(got, acc.float())
        else:
            excess = (got.double() - want.double()).abs() - _oracle_tolerance(o, acc, sx, ox, sw, ow, b)
            assert float(excess.max()) <= 0, f"{pattern} per_token={per_token} ow={ow_kind}: {float(excess.max()):.3g} beyond the bound"


def test_the_oracle_refuses_a_contraction_past_int32(oracle_backend):
    """The C ABI's bound (include/ffq.h): K <= 131071, as the library's — checked before the oracle touches `out`."""
    n, k = 2, 131072
    xq, wq = torch.full((1, k), -128, dtype=torch.int8), torch.full((n, k), -128, dtype=torch.int8)
    one = torch.ones(1)
    with pytest.raises(RuntimeError, match="int32 accumulator"):
        ops.linear_w8a8(xq, wq, one, None, one, None, out_dtype=torch.float32)
    got = ops.linear_w8a8(xq[:, :131056], wq[:, :131056], one, None, one, None, out_dtype=torch.float32)
    assert got.tolist() == [[float(2**31 - 2**18)] * n]


def test_the_dispatcher_declines_a_contraction_past_int32():
    from fastforward_amd import fused_conv, fused_linear

    assert fused_linear.MAX_CONTRACTION == fused_conv.MAX_REDUCTION == 131071
    assert 2**14 * 131071 < 2**31 <= 2**14 * 131072


# ---- the restated convolutions against float64 ----------------------------------------------------------------------------------------
CONVS = [
    (False, 1, 512, 40, (6, 7), (3, 3), (1, 1), (1, 1)),
    (False, 1, 512, 40, (6, 7), (3, 3), (2, 2), (1, 1)),
    (False, 1, 1024, 40, (1, 9), (1, 4), (1, 1), (0, 1)),
    (True, 1, 1024, 40, (3, 4), (4, 4), (2, 2), (1, 1)),
    (True, 1, 2048, 40, (1, 5), (1, 4), (1, 2), (0, 1)),
]


@pytest.mark.parametrize("pattern", ["low", "ties"])
@pytest.mark.parametrize("case", CONVS, ids=str)
def test_restated_convolution_against_float64(case, pattern):
    transposed, B, C, OC, spatial, kernel, stride, padding = case
    xc, wc = hc.conv_codes(pattern, B, C, OC, spatial, kernel, transposed=transposed)
    sx, ox, sw, ow = hc.parameters(pattern, 1, OC)
    y, (a, p1, p2, p3) = hc.restated_conv2d(xc, wc, sx, ox, sw, ow, None, stride, padding, transposed=transposed)
    assert float(a.abs().max()) >= 2**24
    # the same affine operands in float64: zero outside the image IS the real value 0, i.e. (code + offset) = 0 there
    xr = xc.double() + (0.0 if ox is None else float(torch.round(ox)))
    wr = wc.double() + (0.0 if ow is None else torch.round(ow).double().reshape((1, -1, 1, 1) if transposed else (-1, 1, 1, 1)))
    if transposed:
        exact = torch.nn.functional.conv_transpose2d(xr, wr, None, stride, padding)
    else:
        exact = torch.nn.functional.conv2d(xr, wr, None, stride, padding)
    assert torch.equal(exact, a + p1 + p2 + p3)  # the four terms are the affine product, per pixel, border windows included
    scale = sx.double().reshape(()) * sw.double().reshape(1, -1, 1, 1)
    bound = scale * hc.rounding_bound(a, p1, p2, p3) * (1 + 2.0**-20) + 2.0**-22 * (scale * exact).abs()
    assert bool(((y.double() - scale * exact).abs() <= bound).all())
    if pattern == "low" and not transposed and stride == (1, 1) and kernel == (3, 3):
        assert p3.unique().numel() >= 3  # cnt * ox * ow varies per pixel: corner, edge and interior windows
