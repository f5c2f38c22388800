"""The W8A8 depthwise convolution (csrc/ffq_depthwise.hip) on the MI355X.

* exact: with unit scales and no offsets the fp32 output is the integer accumulator, computed independently as a float64
  F.conv2d(groups=C) of the codes (exact below 2^53), at the smallest shapes that reach every branch of the kernel; with real scales
  and offsets it is the epilogue of include/ffq_depthwise.h restated with torch ops in the kernel's fp32 order;
* cross-kernel: every channel is ``ops.conv2d_w8a8`` on its one-channel slice bit for bit, and conv1d is the H = KH = 1 call;
* against the device reference chain (dequantize, F.conv2d(groups=C), the output quantizer): within the tolerances the linear is
  held to (tests/parity_cases.py::linear_tolerances), and the fused output quantizer's codes are A1 of the unfused value bit for bit;
* the G28 cases, layouts, views, declines, two converted models under graph capture, and the memory contract of the C entry point.

Every test counts the calls of ``ops.depthwise_conv2d_w8a8`` (and of ``ops.conv2d_w8a8``), so a silent fallback fails it."""

import contextlib

import pytest
import torch

import fastforward_amd as ff

from conftest import golden
from fastforward_amd import dispatcher, ops
from fastforward_amd._cabi import DType, Status
from fastforward_amd.nn import functional as F
from parity_cases import linear_tolerances
from test_depthwise_cpu import N_CASES, g28_quantizer, run_g28

pytestmark = pytest.mark.gpu
DEV = "cuda"
DW, GEMM = "depthwise_conv2d_w8a8", "conv2d_w8a8"


@pytest.fixture(autouse=True)
def _inference():
    """Inference, as the models run: under grad mode the quantizers' learnable parameters send every call to the chain."""
    with torch.no_grad():
        yield


@pytest.fixture()
def launches(monkeypatch):
    """{entry: number of calls} of ops.depthwise_conv2d_w8a8 and ops.conv2d_w8a8"""
    counts = {DW: 0, GEMM: 0}
    for name in counts:
        real = getattr(ops, name)

        def counted(*a, _real=real, _name=name, **k):
            counts[_name] += 1
            return _real(*a, **k)

        monkeypatch.setattr(ops, name, counted)
    return counts


@pytest.fixture()
def no_fused(monkeypatch):
    """A context in which the dispatcher has no kernel for conv1d / conv2d: the reference chain runs."""

    @contextlib.contextmanager
    def off():
        with monkeypatch.context() as m:
            for op in ("conv1d", "conv2d"):
                m.setitem(dispatcher._DISPATCHER, op, [])
            yield

    return off


def quantizer(lo, hi, symmetric=False, granularity=None, bits=8):
    q = ff.nn.LinearQuantizer(bits, symmetric=symmetric, granularity=granularity or ff.PerTensor(), quantized_dtype=torch.int8, device=DEV)
    q.quantization_range = (torch.as_tensor(lo, dtype=torch.float32, device=DEV), torch.as_tensor(hi, dtype=torch.float32, device=DEV))
    return q


def operands(B, C, M, spatial, k, dtype, positive=False, w_offset=False, per_channel=True, seed=0):
    """(input codes, weight codes) as QuantizedTensors: per-tensor asymmetric input [B, C, *spatial]; weights [C * M, 1, *k] per output
    channel (PerChannel(0)) or per tensor, symmetric or asymmetric with offsets."""
    g = torch.Generator().manual_seed(seed)
    OC = C * M
    x = torch.rand(B, C, *spatial, generator=g) * 3 + 0.25 if positive else torch.randn(B, C, *spatial, generator=g) * 1.5 + 0.3
    taps = 1
    for e in k:
        taps *= e
    w = torch.randn(OC, 1, *k, generator=g) * (0.5 / taps ** 0.5)
    x, w = x.to(DEV, dtype), w.to(DEV, dtype)
    xq = quantizer(x.float().min(), x.float().max())(x)
    if per_channel:
        wf = w.float().reshape(OC, -1)
        lo, hi = wf.amin(1).clamp(max=-1e-3), wf.amax(1).clamp(min=1e-3)
    else:
        lo, hi = w.float().min(), w.float().max()
    if w_offset:
        lo, hi = lo * 1.3, hi * 0.7  # a real zero-point
    wq = quantizer(lo, hi, symmetric=not w_offset, granularity=ff.PerChannel(0) if per_channel else None)(w)
    return xq, wq


def conv(dims, *args, **kwargs):
    return (F.conv1d if dims == 1 else F.conv2d)(*args, strict_quantization=False, **kwargs)


def pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def params(t):
    p = t.quantization_context.quantization_params
    return p.scale, p.offset


def codes(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-128, 128, shape, generator=g, dtype=torch.int8).to(DEV)


def accumulator64(xc, wc, stride, padding, dilation):
    """sum over the taps inside the image of x[b, n / M, ih, iw] * w[n, t], in float64 (exact), on the host: [B, C * M, OH, OW]."""
    return torch.nn.functional.conv2d(xc.cpu().double(), wc.cpu().double(), None, stride, padding, dilation, xc.shape[1])


# ---- exact ---------------------------------------------------------------------------------------------------------------------
# (C, M, (H, W), kernel, stride, padding, dilation, bias), B = 2 (planes cross the batch boundary). The kernel's branches: a lane owns
# 4 consecutive outputs, a block up to 16 x 16 lanes; stride_w == dil_w == 1 takes the dot4 form, anything else the byte form, and a
# patch above the LDS budget the unstaged form; W % 4 == 0 loads dwords; OW % 4 == 0 stores whole runs.
EXACT = [
    (3, 1, (5, 1), (3, 3), 1, 1, 1, False),                  # OW = 1
    (3, 1, (5, 7), (3, 3), 1, 1, 1, False),                  # OW = 7: one run and a tail
    (5, 1, (6, 9), (3, 3), 1, 1, 1, True),                   # OW = 9
    (3, 1, (20, 67), (3, 3), 1, 1, 1, False),                # OW = 67: a full block row of runs plus a tail, two tiles each way
    (3, 1, (18, 68), (3, 5), 1, (1, 2), 1, True),            # W % 4 == 0 and OW % 4 == 0: dword loads, whole-run stores
    (3, 1, (3, 3), (3, 3), 1, 1, 1, True),                   # every window is clipped
    (5, 1, (15, 13), (3, 3), 2, 1, 1, False),                # stride 2 on odd sizes (the byte form), OW = 7
    (3, 1, (16, 16), (3, 3), 2, 1, 1, True),                 # stride 2, OW = 8
    (3, 1, (12, 13), (3, 3), 1, 2, 3, False),                # dilation 3
    (3, 1, (6, 7), (3, 3), 1, 4, 1, True),                   # padding beyond the kernel: windows with no tap give the bias
    (5, 3, (9, 10), (3, 3), (2, 1), (1, 0), (1, 1), True),   # channel multiplier 3
    (3, 1, (33, 33), (31, 31), 1, 15, 1, False),             # RepLKNet's 31 x 31
    (2, 1, (40, 45), (32, 32), 1, 0, 1, False),              # 1024 taps
    (5, 1, (1, 70), (1, 31), 1, (0, 15), 1, True),           # conv1d k31 as H = KH = 1
    (3, 2, (1, 40), (1, 4), 1, (0, 3), 1, False),            # conv1d k4
    (3, 1, (1, 1500), (1, 4), 1, (0, 3), 1, False),          # a long row: 256 lanes along OW, two tiles
    (2, 1, (700, 700), (3, 3), 1, 0, 300, True),             # the patch exceeds the LDS budget: unstaged
    (2, 1, (810, 40), (3, 3), 1, 0, (400, 1), False),        # ... from the dot4 form's geometry
]


@pytest.mark.parametrize("shape", EXACT)
def test_unit_scales_give_the_integer_accumulator(shape, launches):
    C, M, spatial, k, s, p, d, with_bias = shape
    xc, wc = codes((2, C, *spatial), 1), codes((C * M, 1, *k), 2)
    one = torch.ones(1, device=DEV)
    bias = torch.randn(C * M, generator=torch.Generator().manual_seed(3)).to(DEV) if with_bias else None
    out = ops.depthwise_conv2d_w8a8(xc, wc, one, None, one, None, bias, s, p, d, out_dtype=torch.float32)
    assert launches[DW] == 1
    want = accumulator64(xc, wc, s, p, d).float()
    if with_bias:
        want = want + bias.cpu().reshape(1, -1, 1, 1)
    assert out.shape == want.shape and out.is_contiguous()
    assert torch.equal(out.cpu(), want)
    if p == 4:  # the corner windows have no tap inside the image
        assert torch.equal(out[:, :, 0, 0].cpu(), bias.cpu().expand(2, -1))


def _restated(xq, wq, bias, s, p, d):
    """include/ffq_depthwise.h's epilogue with torch ops in the kernel's fp32 order (on the host: IEEE fp32, no FMA)."""
    (sx, ox), (sw, ow) = params(xq), params(wq)
    xc, wc = xq.raw_data.cpu().double(), wq.raw_data.cpu().double()
    B, C = xc.shape[:2]
    OC = wc.shape[0]
    M = OC // C
    cv = lambda x, w, g: torch.nn.functional.conv2d(x, w, None, s, p, d, g)  # noqa: E731
    acc = cv(xc, wc, C)
    rsx = cv(xc, torch.ones(C, 1, *wc.shape[2:], dtype=torch.float64), C).repeat_interleave(M, 1)   # the codes under the taps of V(p)
    rsw = cv(torch.ones_like(xc), wc, C)                                                             # the weight codes over V(p)
    cnt = cv(torch.ones(B, 1, *xc.shape[2:], dtype=torch.float64), torch.ones(1, 1, *wc.shape[2:], dtype=torch.float64), 1)
    sx = sx.float().cpu().reshape(())
    ox = torch.round(ox.float().cpu().reshape(()))
    sw = sw.float().cpu().reshape(1, -1, 1, 1)
    ow = torch.round(ow.float().cpu()).reshape(1, -1, 1, 1)
    v = acc.float()
    v = v + ox * rsw.float()
    v = v + ow * rsx.float()
    v = v + cnt.float() * ox * ow
    y = (sx * sw) * v
    if bias is not None:
        y = y + bias.float().cpu().reshape(1, OC, 1, 1)
    return y, cnt


@pytest.mark.parametrize("positive", [False, True])
@pytest.mark.parametrize("geometry", [((3, 3), 1, 2, 1), ((3, 3), (2, 1), (1, 0), (1, 2)), ((5, 5), 2, 2, 1), ((1, 3), 1, (2, 2), 1)])
def test_the_affine_epilogue_is_the_stated_one(geometry, positive, launches):
    """Real weight offsets per channel, rne(x_offset) beyond int8 (the positive input), windows clipped down to one tap per axis
    and, with the (1, 3) kernel under row padding 2, windows with no tap at all: there y is the bias."""
    k, s, p, d = geometry
    xq, wq = operands(2, 5, 2, (9, 11), k, torch.float32, positive=positive, w_offset=True, seed=2)
    ox = float(torch.round(params(xq)[1]))
    assert ox != 0 and (not positive or abs(ox) > 127)
    assert bool((torch.round(params(wq)[1]) != 0).any())
    bias = torch.randn(10, device=DEV)
    out = conv(2, xq, wq, bias, s, p, d, 5)
    assert launches[DW] == 1 and launches[GEMM] == 0
    want, cnt = _restated(xq, wq, bias, pair(s), pair(p), pair(d))
    assert float(cnt.min()) < float(cnt.max()) and (k[0] != 1 or float(cnt.min()) == 0)
    assert torch.equal(out.cpu(), want)


# ---- cross-kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", [((3, 3), 1, 1, 1, 1), ((5, 3), (2, 1), (2, 1), (1, 2), 3), ((7, 7), 1, 3, 1, 2)])
def test_every_channel_is_the_implicit_gemm_on_its_slice_bit_for_bit(geometry, launches):
    k, s, p, d, M = geometry
    C, OC = 3, 3 * M
    xc, wc = codes((2, C, 13, 14), 4), codes((OC, 1, *k), 5)
    g = torch.Generator().manual_seed(6)
    xs, xo = torch.tensor([0.02], device=DEV), torch.tensor([-141.0], device=DEV)
    ws, wo = (torch.rand(OC, generator=g) * 1e-2 + 1e-3).to(DEV), torch.randint(-9, 10, (OC,), generator=g).float().to(DEV)
    bias = torch.randn(OC, generator=g).to(DEV, torch.bfloat16)
    os_, oo = torch.tensor([0.05], device=DEV), torch.tensor([7.0], device=DEV)
    forms = (dict(out_dtype=torch.bfloat16), dict(out_dtype=torch.float32), dict(out_dtype=torch.float16),
             dict(out_scale=os_, out_offset=oo, requant_from=torch.bfloat16), dict(out_scale=os_, requant_from=torch.float32))
    for extra in forms:
        got = ops.depthwise_conv2d_w8a8(xc, wc, xs, xo, ws, wo, bias, s, p, d, **extra)
        for c in range(C):
            n = slice(c * M, (c + 1) * M)
            want = ops.conv2d_w8a8(xc[:, c:c + 1], wc[n], xs, xo, ws[n], wo[n], bias[n], s, p, d, **extra)
            assert got.dtype == want.dtype and torch.equal(got[:, n], want), (extra, c)
    # per-tensor weight parameters
    got = ops.depthwise_conv2d_w8a8(xc, wc, xs, xo, ws[:1], wo[:1], None, s, p, d, out_dtype=torch.float32)
    want = torch.cat([ops.conv2d_w8a8(xc[:, c:c + 1], wc[c * M:(c + 1) * M], xs, xo, ws[:1], wo[:1], None, s, p, d, out_dtype=torch.float32)
                      for c in range(C)], 1)
    assert torch.equal(got, want)
    assert launches[DW] == len(forms) + 1 and launches[GEMM] == (len(forms) + 1) * C


@pytest.mark.parametrize("geometry", [(31, 1, 15, 1), (4, 1, 3, 1), (5, 2, 4, 3)])
def test_conv1d_is_the_one_row_2d_call_bit_for_bit(geometry, launches):
    k, s, p, d = geometry
    xq, wq = operands(2, 5, 2, (75,), (k,), torch.bfloat16, w_offset=True, seed=7)
    bias = torch.randn(10, device=DEV, dtype=torch.bfloat16)
    out_q = quantizer(-3.0, 3.0)
    value, quantized = conv(1, xq, wq, bias, s, p, d, 5), conv(1, xq, wq, bias, s, p, d, 5, output_quantizer=out_q)
    assert launches[DW] == 2 and launches[GEMM] == 0
    (xs, xo), (ws, wo) = params(xq), params(wq)
    args = (xq.raw_data.unsqueeze(2), wq.raw_data.unsqueeze(2), xs, xo, ws, wo, bias, (1, s), (0, p), (1, d))
    assert torch.equal(value, ops.depthwise_conv2d_w8a8(*args, out_dtype=torch.bfloat16).squeeze(2))
    os_, oo = out_q.scale, out_q.offset
    want = ops.depthwise_conv2d_w8a8(*args, out_scale=os_, out_offset=oo, requant_from=torch.bfloat16).squeeze(2)
    assert torch.equal(quantized.raw_data, want)


# ---- the sweep against the device reference chain ---------------------------------------------------------------------------------
# (dims, B, C, M, spatial, kernel, stride, padding, dilation, bias, positive input, per-channel weights, weight offsets)
SWEEP = [
    (2, 2, 16, 1, (14, 14), 3, 1, 1, 1, "plain", False, True, False),                  # MobileNet 3x3
    (2, 1, 24, 1, (15, 17), 3, 2, 1, 1, None, False, True, True),                      # stride 2
    (2, 2, 8, 1, (14, 14), 7, 1, 3, 1, "quantized", False, True, False),               # ConvNeXt 7x7
    (2, 2, 6, 1, (12, 12), 5, 1, 2, 1, "plain", True, False, True),                    # per-tensor weights with an offset
    (2, 2, 5, 1, (13, 13), 3, 1, 2, 2, None, True, True, False),                       # dilation
    (2, 1, 3, 1, (33, 33), 31, 1, 15, 1, "plain", False, True, True),                  # 31 x 31
    (2, 1, 7, 3, (11, 7), (1, 3), (1, 2), (0, 1), 1, "quantized", True, True, True),   # channel multiplier 3
    (2, 2, 3, 2, (9, 9), 2, 3, 0, 1, "plain", False, True, False),                     # stride above the kernel
    (2, 2, 8, 1, (6, 10), (5, 3), 1, "same", 1, "plain", False, False, False),         # 'same', symmetric
    (1, 2, 16, 1, (120,), 31, 1, 15, 1, "plain", False, True, True),                   # Conformer
    (1, 3, 12, 1, (64,), 4, 1, 3, 1, "quantized", False, False, True),                 # Mamba
    (1, 2, 6, 2, (50,), 5, 2, "valid", 2, None, True, True, False),
]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("case", range(len(SWEEP)))
def test_against_the_device_reference_chain(case, dtype, launches, no_fused):
    dims, B, C, M, spatial, k, stride, padding, dilation, bias_kind, positive, per_channel, w_offset = SWEEP[case]
    k = (k,) * dims if isinstance(k, int) else k
    xq, wq = operands(B, C, M, spatial, k, dtype, positive=positive, w_offset=w_offset, per_channel=per_channel, seed=case)
    if positive:
        assert abs(float(torch.round(params(xq)[1]))) > 127  # -ox does not fit int8
    bias = None
    if bias_kind is not None:
        bias = (torch.randn(C * M) * 0.2).to(DEV, dtype)
        if bias_kind == "quantized":
            bias = quantizer(-0.5, 0.5, symmetric=True)(bias)
    args = (xq, wq, bias, stride, padding, dilation, C)
    fused = conv(dims, *args)
    assert launches[DW] == 1
    with no_fused():
        chain = conv(dims, *args)
    assert launches[DW] == 1 and launches[GEMM] == 0
    assert fused.dtype == chain.dtype == dtype and fused.shape == chain.shape and fused.is_contiguous()
    atol, rtol = linear_tolerances(dtype)
    torch.testing.assert_close(fused.float(), chain.float(), atol=atol, rtol=rtol)
    # the output quantizer in the epilogue: A1 of the value the unfused launch returns, bit for bit
    out_q = quantizer(chain.float().min(), chain.float().max())
    quantized = conv(dims, *args, output_quantizer=out_q)
    assert launches[DW] == 2
    assert isinstance(quantized, ff.QuantizedTensor) and quantized.raw_data.dtype == torch.int8
    assert torch.equal(quantized.raw_data, out_q(fused).raw_data)
    assert torch.equal(quantized.dequantize(), out_q(fused).dequantize())


# ---- the reference's own outputs (G28) -----------------------------------------------------------------------------------------------
def _reference_share_against_float64(cases):
    """The share of output codes on which the reference's own bf16 chain (the fixture) differs from the same chain computed in
    float64 from the same operand codes and parameters: the room a faithful implementation has. From the fixture alone."""
    differ = total = 0
    for case in cases:
        if case["dtype"] != "torch.bfloat16":
            continue
        qs = {name: g28_quantizer(spec, case["params"][name]) for name, spec in case["slots"].items()}

        def real64(q, t):
            qt = q(t)
            p = qt.quantization_context.quantization_params
            shape = [1] * t.dim()
            if p.scale.numel() > 1:
                shape[0] = -1
            off = 0.0 if p.offset is None else torch.round(p.offset.double()).reshape(shape)
            return (qt.raw_data.double() + off) * p.scale.double().reshape(shape)

        x, w = real64(qs["input_quantizer"], case["x"]), real64(qs["weight_quantizer"], case["weight"])
        bias = None
        if case["bias"] is not None:
            bias = real64(qs["bias_quantizer"], case["bias"]) if case["bias_kind"] == "quantized" else case["bias"].double()
        op = torch.nn.functional.conv1d if case["dims"] == 1 else torch.nn.functional.conv2d
        y = op(x, w, bias, case["stride"], case["padding"], case["dilation"], case["groups"])
        out = case["params"]["output_quantizer"]
        codes64 = torch.clamp(torch.round(y / out["scale"].double() - torch.round(out["offset"].double())), -128, 127)
        differ += int((codes64 != case["codes"].double()).sum())
        total += codes64.numel()
    return differ / total


def test_the_g28_cases_on_the_device(launches):
    """The reference's own outputs (computed on the CPU): the fused route's value within the linear's tolerance of them; the fused
    quantizer's codes equal to the reference's wherever the two values agree before A1, elsewhere as far apart as that difference
    allows (|code - code_ref| <= |y - y_ref| / s + 1: both are clamp(rne(y / s - o)) of their own y), and the share of codes that
    differ at all no larger than the share on which the reference's bf16 chain itself differs from float64."""
    cases = golden("g28_depthwise.pt")["conv"]
    assert len(cases) == N_CASES
    differ = total = 0
    for index, case in enumerate(cases):
        value, quantized = run_g28(case, DEV)
        assert launches[DW] == 2 * (index + 1) and launches[GEMM] == 0
        atol, rtol = linear_tolerances(case["value"].dtype)
        value = value.cpu()
        torch.testing.assert_close(value.float(), case["value"].float(), atol=atol, rtol=rtol)
        assert isinstance(quantized, ff.QuantizedTensor) and quantized.raw_data.shape == case["codes"].shape
        got = quantized.raw_data.cpu()
        same = value == case["value"]
        assert torch.equal(got[same], case["codes"][same]), index
        scale = case["params"]["output_quantizer"]["scale"].float().reshape(())
        apart = (got.float() - case["codes"].float()).abs()
        assert bool((apart <= (value.float() - case["value"].float()).abs() / scale + 1).all()), (index, float(apart.max()))
        differ += int((apart != 0).sum())
        total += apart.numel()
    cap = _reference_share_against_float64(cases)
    print(f"G28: {differ} of {total} codes differ from the reference's ({differ / total:.5f}); the reference's bf16 chain against float64: {cap:.5f}")
    assert differ / total <= cap


# ---- layouts ----------------------------------------------------------------------------------------------------------------------
def test_channels_last_input_gives_the_bits_of_its_nchw_copy(launches, no_fused):
    xq, wq = operands(3, 16, 1, (10, 9), (3, 3), torch.bfloat16, seed=5)
    out = conv(2, xq, wq, None, 1, 1, 1, 16)
    assert out.is_contiguous() and out.shape == (3, 16, 10, 9)
    with no_fused():
        chain = conv(2, xq, wq, None, 1, 1, 1, 16)
    assert out.stride() == chain.stride()
    out.view(3, -1)  # a later .view works as on the reference's output
    x_cl = xq.dequantize().to(memory_format=torch.channels_last)
    q = quantizer(-4.0, 5.0)
    a, b = conv(2, q(x_cl), wq, None, 1, 1, 1, 16), conv(2, q(x_cl.contiguous()), wq, None, 1, 1, 1, 16)
    assert a.is_contiguous() and torch.equal(a, b)
    held = xq.raw_data.to(memory_format=torch.channels_last)
    assert held.is_contiguous(memory_format=torch.channels_last) and not held.is_contiguous()
    xs, xo = torch.tensor([0.03], device=DEV), torch.tensor([-17.0], device=DEV)
    ws, wo = torch.rand(16, device=DEV) * 1e-2 + 1e-3, torch.full((16,), 2.0, device=DEV)
    os_ = torch.tensor([0.02], device=DEV)
    for extra in (dict(out_dtype=torch.float32), dict(out_scale=os_, requant_from=torch.float16)):
        got = ops.depthwise_conv2d_w8a8(held, wq.raw_data, xs, xo, ws, wo, None, 2, 1, 1, **extra)
        want = ops.depthwise_conv2d_w8a8(held.contiguous(), wq.raw_data, xs, xo, ws, wo, None, 2, 1, 1, **extra)
        assert got.is_contiguous() and torch.equal(got, want)
    assert launches[DW] == 7


def test_offset_and_strided_views_give_the_bits_of_their_contiguous_copies(launches):
    big_x, big_w = codes((3, 12, 11, 22), 9), codes((24, 2, 3, 6), 10)
    scale = torch.rand(16, device=DEV) * 1e-2 + 1e-3
    views = [(big_x[1:, 2:10, 1:9, 3:20], big_w[3:19, 1:, :, 1:4]),            # offset views: misaligned pointers, W = 17
             (big_x[:, ::2, :, ::2][:, :, :, :8][:, :4], big_w[::3, :1, :, ::2]),   # strided views
             (big_x[:, :8, :, :11].transpose(2, 3), big_w[:16, :1, :, :3].transpose(2, 3))]
    one = torch.ones(1, device=DEV)
    off = torch.tensor([3.0], device=DEV)
    for xv, wv in views:
        assert not xv.is_contiguous() and not wv.is_contiguous()
        OC = wv.shape[0]
        got = ops.depthwise_conv2d_w8a8(xv, wv, one, off, scale[:OC], None, None, 1, 1, 1, out_dtype=torch.float32)
        want = ops.depthwise_conv2d_w8a8(xv.contiguous(), wv.contiguous(), one, off, scale[:OC], None, None, 1, 1, 1, out_dtype=torch.float32)
        assert torch.equal(got, want)
        assert torch.equal(got.cpu(), (accumulator64(xv, wv, 1, 1, 1) + 3.0 * accumulator64(torch.ones_like(xv), wv, 1, 1, 1)).float()
                           * scale[:OC].cpu().reshape(1, -1, 1, 1))
    assert launches[DW] == 6


# ---- declines ---------------------------------------------------------------------------------------------------------------------
def test_what_the_predicate_declines_takes_the_chain(launches, no_fused):
    xq, wq = operands(2, 16, 1, (8, 8), (3, 3), torch.bfloat16, seed=6)
    w_pairs = quantizer(-0.3, 0.3, symmetric=True)(torch.randn(16, 8, 3, 3, device=DEV, dtype=torch.bfloat16) * 0.1)
    x = xq.dequantize()
    xq_pc = quantizer(x.float().amin((0, 2, 3)), x.float().amax((0, 2, 3)), granularity=ff.PerChannel(1))(x)
    x_long, w_long = operands(1, 2, 1, (1100,), (1025,), torch.bfloat16, seed=8)
    w_in = quantizer(torch.full((1,), -0.3), torch.full((1,), 0.3), symmetric=True, granularity=ff.PerChannel(1))(wq.dequantize())
    calls = [lambda: conv(2, xq, w_pairs, None, 1, 1, 1, 2),                  # groups = 2, C = 16
             lambda: conv(1, x_long, w_long, None, 1, 0, 1, 2),              # 1025 taps
             lambda: conv(2, xq_pc, wq, None, 1, 1, 1, 16),                  # per-channel activations
             lambda: conv(2, xq, w_in, None, 1, 1, 1, 16),                   # PerChannel(1) weights
             lambda: conv(2, x, wq, None, 1, 1, 1, 16)]                      # a plain float input (weight-only)
    got = [call() for call in calls]
    assert launches == {DW: 0, GEMM: 0}
    with no_fused():
        for value, call in zip(got, calls):
            assert torch.equal(value, call())
    with torch.enable_grad():
        conv(2, xq, wq, None, 1, 1, 1, 16)
    assert launches[DW] == 0
    conv(2, xq, wq, None, 1, 1, 1, 16)
    assert launches == {DW: 1, GEMM: 0}


# ---- converted models under graph capture -----------------------------------------------------------------------------------------
def _convnext_block():
    return torch.nn.Sequential(torch.nn.Conv2d(8, 8, 7, padding=3, groups=8), torch.nn.Conv2d(8, 16, 1))


def _mobilenet_block():
    return torch.nn.Sequential(torch.nn.Conv2d(8, 16, 1), torch.nn.Conv2d(16, 16, 3, stride=2, padding=1, groups=16, bias=False),
                               torch.nn.Conv2d(16, 8, 1))


def _plain(t):
    return t.dequantize() if isinstance(t, ff.QuantizedTensor) else t


@pytest.mark.parametrize("make,depthwise,gemm", [(_convnext_block, 1, 1), (_mobilenet_block, 1, 2)])
def test_graph_replay_of_a_converted_block_equals_eager(make, depthwise, gemm, launches):
    """quantize_model leaves QuantizedConv2d layers that pass `groups` through: the depthwise layer takes the new route, the 1 x 1
    layers the implicit GEMM, each layer's output quantizer inside its launch. A linear chain of launches, none reading device
    memory on the host."""
    torch.manual_seed(0)
    model = ff.quantize_model(make().to(DEV, torch.bfloat16), extra_conversion=ff.nn.quantized_conv_modules())
    act = lambda: ff.nn.LinearQuantizer(8, symmetric=False, quantized_dtype=torch.int8, device=DEV)  # noqa: E731
    model[0].input_quantizer = act()
    for layer in model:
        assert type(layer) is ff.nn.QuantizedConv2d
        layer.output_quantizer = act()
        layer.weight_quantizer = ff.nn.LinearQuantizer(8, granularity=ff.PerChannel(0), quantized_dtype=torch.int8, device=DEV)
    x = torch.randn(2, 8, 14, 14, device=DEV, dtype=torch.bfloat16)
    with ff.strict_quantization(False):
        with ff.estimate_ranges(model, ff.range_setting.running_minmax):
            model(x)
        before = dict(launches)
        eager = _plain(model(x)).clone()
        assert launches == {DW: before[DW] + depthwise, GEMM: before[GEMM] + gemm}
        static = x.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                model(static)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = _plain(model(static))
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(captured, eager)
    assert launches == {DW: before[DW] + 4 * depthwise, GEMM: before[GEMM] + 4 * gemm}


# ---- the memory contract of the C entry point ---------------------------------------------------------------------------------------
MARGIN = 4096


@pytest.mark.parametrize("requant", [False, True])
@pytest.mark.parametrize("geometry", [((19, 23), (3, 3), (1, 1), (1, 1), (1, 1)), ((18, 72), (5, 3), (1, 1), (2, 1), (1, 1)),
                                      ((19, 23), (3, 5), (2, 2), (1, 2), (1, 1)), ((820, 40), (3, 3), (1, 1), (0, 1), (400, 1))])
def test_guard_bands_around_the_output(geometry, requant, launches):
    """`out` sits inside a larger buffer filled with a poison byte; two runs with two poisons: the margins keep their poison (no
    stray write), and the runs agree on every output element (none left unwritten). The tail form (OW = 23), the whole-run
    stores (OW = 72), the byte form (OW = 12) and the unstaged form (OW = 40)."""
    (H, W), K, s, p, d = geometry
    B, C, M = 2, 5, 2
    OC = C * M
    xc, wc = codes((B, C, H, W), 12), codes((OC, 1, *K), 13)
    xs, xo = torch.tensor([0.03], device=DEV), torch.tensor([5.0], device=DEV)
    ws, wo = torch.rand(OC, device=DEV) * 1e-2 + 1e-3, torch.full((OC,), -3.0, device=DEV)
    os_ = torch.tensor([0.5], device=DEV)
    size = [(n + 2 * pi - di * (k - 1) - 1) // si + 1 for n, k, si, pi, di in zip((H, W), K, s, p, d)]
    out_bytes = B * OC * size[0] * size[1] * (1 if requant else 2)
    lib = ops._native.library()
    stream = torch.cuda.current_stream().cuda_stream
    results = []
    for poison in (0x5A, 0xA5):
        out_buf = torch.full((MARGIN + out_bytes + MARGIN,), poison, dtype=torch.uint8, device=DEV)
        rc = lib.ffq_depthwise_conv2d_w8a8(xc.data_ptr(), wc.data_ptr(), xs.data_ptr(), xo.data_ptr(), ws.data_ptr(), wo.data_ptr(), 1, None, 0,
                                           out_buf.data_ptr() + MARGIN, int(DType.I8 if requant else DType.BF16),
                                           os_.data_ptr() if requant else None, None, 8.0, int(DType.BF16) if requant else 0, B, C, M, H, W,
                                           *K, *s, *p, *d, stream)
        assert rc == Status.OK, lib.ffq_last_error()
        torch.cuda.synchronize()
        assert bool((out_buf[:MARGIN] == poison).all()) and bool((out_buf[MARGIN + out_bytes:] == poison).all())
        results.append(out_buf[MARGIN:MARGIN + out_bytes].clone())
    assert torch.equal(results[0], results[1])
    want = ops.depthwise_conv2d_w8a8(xc, wc, xs, xo, ws, wo, None, s, p, d, **(dict(out_scale=os_, requant_from=torch.bfloat16) if requant else {}))
    assert torch.equal(results[0], want.reshape(-1).view(torch.uint8))
    assert launches[DW] == 1
