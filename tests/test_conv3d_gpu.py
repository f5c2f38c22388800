"""The W8A8 3-D convolution (csrc/ffq_conv3d.hip) on the MI355X.

* exact: with unit scales and no offsets the fp32 output is the integer accumulator, computed independently as a float64 F.conv3d
  of the codes (exact below 2^53); D = KD = 1 is ``ops.conv2d_w8a8`` bit for bit; with real scales and offsets it is the epilogue
  of include/ffq_3d.h restated with torch ops in the kernel's fp32 order;
* against the device reference chain (dequantize, F.conv3d, the output quantizer): within the tolerances the linear is held to
  (tests/parity_cases.py::linear_tolerances), and the fused output quantizer's codes are A1 of the unfused value bit for bit;
* layouts, views, declines, graph capture, the G27 cases and the memory contract of the C entry point (local guard bands:
  tests/guards.py wraps the symbols of ``_cabi.SIGNATURES`` only).

Every test counts the calls of ``ops.conv3d_w8a8`` (and of ``ops.pool3d_quantize`` where it runs), so a silent fallback fails it."""

import contextlib

import pytest
import torch

import fastforward_amd as ff

from conftest import golden
from fastforward_amd import dispatcher, ops
from fastforward_amd._cabi import DType, Status
from fastforward_amd.nn import functional as F
from fastforward_amd.ops import conv as ops_conv
from parity_cases import linear_tolerances
from test_conv3d_cpu import run_g27_conv

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _inference():
    """Inference, as the models run: under grad mode the quantizers' learnable parameters send every call to the chain."""
    with torch.no_grad():
        yield


@pytest.fixture()
def launches(monkeypatch):
    """{entry: number of calls} of ops.conv3d_w8a8 and ops.pool3d_quantize"""
    counts = {"conv3d_w8a8": 0, "pool3d_quantize": 0}
    for name in counts:
        real = getattr(ops, name)

        def counted(*a, _real=real, _name=name, **k):
            counts[_name] += 1
            return _real(*a, **k)

        monkeypatch.setattr(ops, name, counted)
    return counts


@pytest.fixture()
def no_fused(monkeypatch):
    """A context in which the dispatcher has no kernel for conv3d / avg_pool3d: the reference chain runs."""

    @contextlib.contextmanager
    def off():
        with monkeypatch.context() as m:
            for op in ("conv3d", "avg_pool3d"):
                m.setitem(dispatcher._DISPATCHER, op, [])
            yield

    return off


def quantizer(lo, hi, symmetric=False, granularity=None, bits=8):
    q = ff.nn.LinearQuantizer(bits, symmetric=symmetric, granularity=granularity or ff.PerTensor(), quantized_dtype=torch.int8, device=DEV)
    q.quantization_range = (torch.as_tensor(lo, dtype=torch.float32, device=DEV), torch.as_tensor(hi, dtype=torch.float32, device=DEV))
    return q


def operands(B, C, OC, spatial, k, dtype, positive=False, w_offset=False, per_channel=True, seed=0):
    """(input codes, weight codes) as QuantizedTensors: per-tensor asymmetric input; weights [OC, C, *k] per output channel
    (PerChannel(0)) or per tensor, symmetric or asymmetric with offsets."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, C, *spatial, generator=g) * 3 + 0.25 if positive else torch.randn(B, C, *spatial, generator=g) * 1.5 + 0.3
    w = torch.randn(OC, C, *k, generator=g) * (0.5 / (C * k[0] * k[1] * k[2]) ** 0.5)
    x, w = x.to(DEV, dtype), w.to(DEV, dtype)
    xq = quantizer(x.float().min(), x.float().max())(x)
    if per_channel:
        wf = w.float().reshape(OC, -1)
        lo, hi = wf.amin(1), wf.amax(1)
    else:
        lo, hi = w.float().min(), w.float().max()
    if w_offset:
        lo, hi = lo * 1.3, hi * 0.7  # a real zero-point
    wq = quantizer(lo, hi, symmetric=not w_offset, granularity=ff.PerChannel(0) if per_channel else None)(w)
    return xq, wq


def conv(*args, **kwargs):
    return F.conv3d(*args, strict_quantization=False, **kwargs)


def triple(v):
    return (v,) * 3 if isinstance(v, int) else tuple(v)


def accumulator64(xc, wc, stride, padding, dilation):
    """sum over the taps inside the volume and over c of x[b, c, id, ih, iw] * w[n, c, t], in float64 (exact): [B, OC, OD, OH, OW]."""
    return torch.nn.functional.conv3d(xc.double(), wc.double(), None, stride, padding, dilation)


# ---- exact ---------------------------------------------------------------------------------------------------------------------
# (C, OC, (D, H, W), kernel, stride, padding, dilation), B = 2: channel padding (C = 3, 20), a ragged last k-step (27 taps x 16 B =
# 6.75 steps), 200 positions in two tiles that cross the batch boundary, partial channel tiles (OC = 40, 130), the patch embedding
EXACT = [
    (3, 40, (5, 9, 11), (3, 3, 3), (1, 2, 3), (1, 0, 2), 1),
    (20, 130, (4, 6, 7), (2, 1, 3), 1, 0, (2, 1, 2)),
    (16, 32, (5, 6, 7), (3, 3, 3), 1, 0, 1),
    (16, 64, (4, 28, 28), (2, 14, 14), (2, 14, 14), 0, 1),
]


@pytest.mark.parametrize("shape", EXACT)
def test_unit_scales_give_the_integer_accumulator(shape, launches):
    C, OC, spatial, k, s, p, d = shape
    g = torch.Generator().manual_seed(1)
    xc = torch.randint(-128, 128, (2, C, *spatial), generator=g, dtype=torch.int8).to(DEV)
    wc = torch.randint(-128, 128, (OC, C, *k), generator=g, dtype=torch.int8).to(DEV)
    one = torch.ones(1, device=DEV)
    out = ops.conv3d_w8a8(xc, wc, one, None, one, None, None, s, p, d, out_dtype=torch.float32)
    assert launches["conv3d_w8a8"] == 1
    assert torch.equal(out, accumulator64(xc, wc, s, p, d).float())


@pytest.mark.parametrize("geometry", [((3, 3), (2, 1), (1, 2), (1, 2)), ((1, 5), (1, 3), (0, 2), (1, 1))])
def test_depth_one_is_the_2d_convolution_bit_for_bit(geometry, launches):
    k, s, p, d = geometry
    g = torch.Generator().manual_seed(3)
    xc = torch.randint(-128, 128, (3, 20, 9, 13), generator=g, dtype=torch.int8).to(DEV)
    wc = torch.randint(-128, 128, (70, 20, *k), generator=g, dtype=torch.int8).to(DEV)
    xs, xo = torch.tensor([0.02], device=DEV), torch.tensor([-141.0], device=DEV)
    ws, wo = torch.rand(70, device=DEV) * 1e-2 + 1e-3, torch.randint(-9, 10, (70,), generator=g).float().to(DEV)
    bias = torch.randn(70, device=DEV, dtype=torch.bfloat16)
    os_, oo = torch.tensor([0.05], device=DEV), torch.tensor([7.0], device=DEV)
    for extra in (dict(out_dtype=torch.bfloat16), dict(out_dtype=torch.float32), dict(out_scale=os_, out_offset=oo, requant_from=torch.bfloat16)):
        got = ops.conv3d_w8a8(xc.unsqueeze(2), wc.unsqueeze(2), xs, xo, ws, wo, bias, (1, *s), (0, *p), (1, *d), **extra)
        want = ops.conv2d_w8a8(xc, wc, xs, xo, ws, wo, bias, s, p, d, **extra)
        assert got.dtype == want.dtype and torch.equal(got.squeeze(2), want)
    assert launches["conv3d_w8a8"] == 3


def _restated(xq, wq, bias, s, p, d):
    """include/ffq_3d.h's epilogue with torch ops in the kernel's fp32 order (on the host: IEEE fp32, no FMA)."""
    px, pw_ = xq.quantization_context.quantization_params, wq.quantization_context.quantization_params
    xc, wc = xq.raw_data.cpu().double(), wq.raw_data.cpu().double()
    OC, C = wc.shape[:2]
    B = xc.shape[0]
    cv = lambda x, w: torch.nn.functional.conv3d(x, w, None, s, p, d)  # noqa: E731
    acc = cv(xc, wc)
    ones = torch.ones(B, 1, *xc.shape[2:], dtype=torch.float64)
    rsx = cv(xc, torch.ones(1, C, *wc.shape[2:], dtype=torch.float64))     # [B, 1, ...]: the codes under the taps of V(p)
    rsw = cv(ones, wc.sum(1, keepdim=True))                                # [B, OC, ...]: the per-tap weight sums over V(p)
    cnt = C * cv(ones, torch.ones(1, 1, *wc.shape[2:], dtype=torch.float64))
    sx = px.scale.float().cpu().reshape(())
    ox = torch.round(px.offset.float().cpu().reshape(()))
    sw = pw_.scale.float().cpu().reshape(1, -1, 1, 1, 1)
    ow = torch.round(pw_.offset.float().cpu()).reshape(1, -1, 1, 1, 1)
    v = acc.float()
    v = v + ox * rsw.float()
    v = v + ow * rsx.float()
    v = v + cnt.float() * ox * ow
    y = (sx * sw) * v
    if bias is not None:
        y = y + bias.float().cpu().reshape(1, OC, 1, 1, 1)
    return y, cnt


@pytest.mark.parametrize("positive", [False, True])
@pytest.mark.parametrize("geometry", [((3, 3, 3), 1, 2, 1), ((3, 3, 3), (2, 1, 2), (2, 1, 0), (1, 2, 1)), ((1, 3, 3), 1, (2, 2, 2), 1)])
def test_the_affine_epilogue_is_the_stated_one(geometry, positive, launches):
    """Real weight offsets, rne(x_offset) beyond int8 (the positive input), windows clipped down to one tap per axis (padding 2
    under kernel 3) and, with the (1, 3, 3) kernel under depth padding 2, windows with no tap at all: there y is the bias."""
    k, s, p, d = geometry
    xq, wq = operands(2, 24, 40, (4, 7, 6), k, torch.float32, positive=positive, w_offset=True, seed=2)
    ox = float(torch.round(xq.quantization_context.quantization_params.offset))
    assert ox != 0 and (not positive or abs(ox) > 127)
    assert bool((torch.round(wq.quantization_context.quantization_params.offset) != 0).any())
    bias = torch.randn(40, device=DEV)
    out = conv(xq, wq, bias, s, p, d)
    assert launches["conv3d_w8a8"] == 1
    want, cnt = _restated(xq, wq, bias, triple(s), triple(p), triple(d))
    assert float(cnt.min()) < float(cnt.max()) and (k[0] != 1 or float(cnt.min()) == 0)
    assert torch.equal(out.cpu(), want)


# ---- the sweep against the device reference chain ---------------------------------------------------------------------------------
# (B, C, OC, spatial, kernel, stride, padding, dilation, bias, positive input, per-channel weights, weight offsets)
SWEEP = [
    (2, 16, 40, (4, 9, 11), 3, 1, 1, 1, "plain", False, True, False),
    (1, 3, 64, (6, 17, 15), 3, 2, 1, 1, None, False, True, True),                      # C = 3
    (2, 64, 130, (3, 7, 9), 1, 1, 0, 1, "quantized", False, True, False),              # OC not a multiple of 128
    (2, 80, 96, (4, 8, 7), 3, 2, 1, 1, "plain", True, False, True),                    # per-tensor weights with an offset
    (2, 16, 33, (5, 13, 13), 3, 1, 2, 2, None, True, True, False),                     # dilation
    (4, 16, 24, (4, 28, 28), (2, 14, 14), (2, 14, 14), 0, 1, "plain", False, True, True),   # the patch embedding
    (1, 64, 200, (3, 11, 7), (1, 3, 3), (1, 2, 1), (0, 1, 1), 1, "quantized", True, True, True),
    (2, 3, 17, (5, 9, 9), 2, 3, 0, 1, "plain", False, True, False),                    # stride above the kernel
    (2, 80, 144, (3, 6, 10), (3, 5, 3), 1, "same", 1, "plain", False, False, False),   # 'same', symmetric
    (2, 20, 48, (6, 6, 7), (2, 3, 3), (1, 2, 3), (1, 1, 2), (2, 1, 1), None, True, True, True),
    (3, 32, 32, (4, 8, 8), 3, 1, "valid", 1, "quantized", False, False, True),
    (2, 48, 70, (2, 5, 19), (2, 1, 5), 1, (1, 0, 4), (1, 1, 2), "plain", True, True, False),
]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("case", range(len(SWEEP)))
def test_against_the_device_reference_chain(case, dtype, launches, no_fused):
    B, C, OC, spatial, k, stride, padding, dilation, bias_kind, positive, per_channel, w_offset = SWEEP[case]
    xq, wq = operands(B, C, OC, spatial, triple(k), dtype, positive=positive, w_offset=w_offset, per_channel=per_channel, seed=case)
    if positive:
        assert abs(float(torch.round(xq.quantization_context.quantization_params.offset))) > 127  # -ox does not fit int8
    bias = None
    if bias_kind is not None:
        bias = (torch.randn(OC) * 0.2).to(DEV, dtype)
        if bias_kind == "quantized":
            bias = quantizer(-0.5, 0.5, symmetric=True)(bias)
    args = (xq, wq, bias, stride, padding, dilation, 1)
    fused = conv(*args)
    assert launches["conv3d_w8a8"] == 1
    with no_fused():
        chain = conv(*args)
    assert launches["conv3d_w8a8"] == 1
    assert fused.dtype == chain.dtype == dtype and fused.shape == chain.shape and fused.is_contiguous()
    atol, rtol = linear_tolerances(dtype)
    torch.testing.assert_close(fused.float(), chain.float(), atol=atol, rtol=rtol)
    # the output quantizer in the epilogue: A1 of the value the unfused launch returns, bit for bit
    out_q = quantizer(chain.float().min(), chain.float().max())
    codes = conv(*args, output_quantizer=out_q)
    assert launches["conv3d_w8a8"] == 2
    assert isinstance(codes, ff.QuantizedTensor) and codes.raw_data.dtype == torch.int8
    assert torch.equal(codes.raw_data, out_q(fused).raw_data)
    assert torch.equal(codes.dequantize(), out_q(fused).dequantize())


@pytest.mark.parametrize("index", range(16))
def test_the_g27_cases_on_the_device(index, launches):
    """The reference's own outputs (computed on the CPU): the fused route's value within the linear's tolerance of them, and the
    fused quantizer's codes as far from the reference's as that difference allows: both are clamp(rne(y / s - o)) of their own y,
    and each rounding moves a code by at most one half, so |code - code_ref| <= |y - y_ref| / s + 1."""
    case = golden("g27_conv3d.pt")["conv"][index]
    value, quantized = run_g27_conv(case, DEV)
    assert launches["conv3d_w8a8"] == 2
    atol, rtol = linear_tolerances(case["value"].dtype)
    torch.testing.assert_close(value.float().cpu(), case["value"].float(), atol=atol, rtol=rtol)
    assert isinstance(quantized, ff.QuantizedTensor) and quantized.raw_data.shape == case["codes"].shape
    scale = case["params"]["output_quantizer"]["scale"].float().reshape(())
    apart = (quantized.raw_data.cpu().float() - case["codes"].float()).abs()
    assert bool((apart <= (value.float().cpu() - case["value"].float()).abs() / scale + 1).all()), float(apart.max())


# ---- layouts ----------------------------------------------------------------------------------------------------------------------
def test_channels_last_3d_agrees_and_skips_the_input_half_of_the_layout_pass(launches, no_fused, monkeypatch):
    """Codes in channels_last_3d with C % 16 == 0 reach the GEMM as they are: the call hands the C entry point the tensor's own memory
    (no copy launch) with x_ndhwc set, whose workspace holds no NDHWC copy (the layout pass's input half is skipped) — the device
    pass over the input that the NCDHW call makes is the one launch fewer. (A LinearQuantizer answers a channels_last_3d input with
    contiguous codes, so through the functional both inputs take the NCDHW form and agree.)"""
    dense_copies, workspaces = [], []
    real_dense, real_ws = ops_conv._dense, ops_conv._workspace
    monkeypatch.setattr(ops_conv, "_dense", lambda t, *a, **k: (lambda r: (dense_copies.append(r.data_ptr() != t.data_ptr()), r)[1])(real_dense(t, *a, **k)))
    monkeypatch.setattr(ops_conv, "_workspace", lambda n, dev: (workspaces.append(n), real_ws(n, dev))[1])
    xq, wq = operands(3, 32, 48, (4, 10, 9), (3, 3, 3), torch.bfloat16, seed=5)
    out = conv(xq, wq, None, 1, 1)
    assert out.is_contiguous() and out.shape == (3, 48, 4, 10, 9)
    with no_fused():
        chain = conv(xq, wq, None, 1, 1)
    assert out.stride() == chain.stride()
    out.view(3, -1)  # a later .view works as on the reference's output
    x_cl = xq.dequantize().to(memory_format=torch.channels_last_3d)
    q = quantizer(-4.0, 5.0)
    xq_cl, xq_ncdhw = q(x_cl), q(x_cl.contiguous())
    assert torch.equal(xq_cl.raw_data.contiguous(), xq_ncdhw.raw_data)
    a, b = conv(xq_cl, wq, None, 1, 1), conv(xq_ncdhw, wq, None, 1, 1)
    assert a.is_contiguous() and torch.equal(a, b)
    # codes held in channels_last_3d, with real parameters, a bias and the fused output quantizer
    codes = xq_ncdhw.raw_data.to(memory_format=torch.channels_last_3d)
    assert codes.is_contiguous(memory_format=torch.channels_last_3d) and not codes.is_contiguous()
    xs, xo = torch.tensor([0.03], device=DEV), torch.tensor([-17.0], device=DEV)
    ws, wo = torch.rand(48, device=DEV) * 1e-2 + 1e-3, torch.full((48,), 2.0, device=DEV)
    bias = torch.randn(48, device=DEV)
    os_ = torch.tensor([0.02], device=DEV)
    lib = ops._native.library()
    x_bytes = 3 * 4 * 10 * 9 * 32
    for extra in (dict(out_dtype=torch.float32), dict(out_scale=os_, requant_from=torch.float16)):
        del dense_copies[:], workspaces[:]
        got = ops.conv3d_w8a8(codes, wq.raw_data, xs, xo, ws, wo, bias, 2, 1, 1, **extra)
        want = ops.conv3d_w8a8(codes.contiguous(), wq.raw_data, xs, xo, ws, wo, bias, 2, 1, 1, **extra)
        assert got.is_contiguous() and torch.equal(got, want)
        assert dense_copies == [False, False, False, False]                 # input and weight of both calls: the caller's memory
        assert workspaces == [lib.ffq_conv3d_w8a8_workspace_bytes(3, 32, 4, 10, 9, 48, 3, 3, 3, flag) for flag in (1, 0)]
        assert workspaces[1] - workspaces[0] == -(-x_bytes // 256) * 256
    assert launches["conv3d_w8a8"] == 7


def test_offset_and_strided_views_give_the_bits_of_their_contiguous_copies(launches):
    g = torch.Generator().manual_seed(9)
    big_x = torch.randint(-128, 128, (3, 40, 6, 9, 14), generator=g, dtype=torch.int8).to(DEV)
    big_w = torch.randint(-128, 128, (50, 40, 3, 3, 6), generator=g, dtype=torch.int8).to(DEV)
    scale = torch.rand(24, device=DEV) * 1e-2 + 1e-3
    views = [(big_x[1:, 4:36, 1:5, 1:8, 2:13], big_w[3:27, 4:36, :, :, 1:4]),       # offset views
             (big_x[:, ::2, :, :, ::2], big_w[1:49:2, ::2, :, :, ::2]),              # strided views
             (big_x[:, 8:40].transpose(3, 4), big_w[:24, 8:40].transpose(3, 4))]
    one = torch.ones(1, device=DEV)
    off = torch.tensor([3.0], device=DEV)
    for xv, wv in views:
        assert not xv.is_contiguous() and not wv.is_contiguous()
        got = ops.conv3d_w8a8(xv, wv, one, off, scale, None, None, 2, 1, 1, out_dtype=torch.float32)
        want = ops.conv3d_w8a8(xv.contiguous(), wv.contiguous(), one, off, scale, None, None, 2, 1, 1, out_dtype=torch.float32)
        assert torch.equal(got, want)
    assert launches["conv3d_w8a8"] == 6


# ---- declines ---------------------------------------------------------------------------------------------------------------------
def test_what_the_predicate_declines_takes_the_chain(launches, no_fused):
    xq, wq = operands(2, 16, 32, (4, 8, 8), (3, 3, 3), torch.bfloat16, seed=6)
    w_half = quantizer(-0.3, 0.3, symmetric=True)(torch.randn(32, 8, 3, 3, 3, device=DEV, dtype=torch.bfloat16) * 0.1)
    w = wq.dequantize()
    w_in = quantizer(w.float().amin((0, 2, 3, 4)), w.float().amax((0, 2, 3, 4)), symmetric=True, granularity=ff.PerChannel(1))(w)
    x = xq.dequantize()
    xq_pc = quantizer(x.float().amin((0, 2, 3, 4)), x.float().amax((0, 2, 3, 4)), granularity=ff.PerChannel(1))(x)
    w_even = quantizer(-0.3, 0.3, symmetric=True)(torch.randn(32, 16, 2, 3, 3, device=DEV, dtype=torch.bfloat16) * 0.1)
    x4 = quantizer(-4.0, 5.0)(x[0])
    calls = [lambda: conv(xq, w_half, None, 1, 1, 1, 2),                     # groups = 2
             lambda: conv(xq, w_in, None, 1, 1),                             # per-input-channel weights
             lambda: conv(xq_pc, wq, None, 1, 1),                            # per-channel activations
             lambda: conv(xq, w_even, None, 1, "same"),                      # 'same' with an even kernel: asymmetric padding
             lambda: conv(x4, wq, None, 1, 1),                               # an unbatched 4-D input
             lambda: conv(x, wq, None, 1, 1)]                                # a plain float input (weight-only)
    got = [call() for call in calls]
    assert launches["conv3d_w8a8"] == 0
    with no_fused():
        for value, call in zip(got, calls):
            assert torch.equal(value, call())
    with torch.enable_grad():
        conv(xq, wq, None, 1, 1)
    assert launches["conv3d_w8a8"] == 0
    conv(xq, wq, None, 1, 1)
    assert launches["conv3d_w8a8"] == 1


# ---- graph capture ----------------------------------------------------------------------------------------------------------------
def _plain(t):
    return t.dequantize() if isinstance(t, ff.QuantizedTensor) else t


def test_graph_replay_of_a_two_layer_block_equals_eager(launches):
    """conv3d -> avg_pool3d -> conv3d with every quantizer fixed: five launches of the two entry points per pass, none of which
    reads device memory on the host."""
    torch.manual_seed(0)
    w1 = (torch.randn(32, 16, 3, 3, 3, device=DEV) * 0.05).to(torch.bfloat16)
    w2 = (torch.randn(24, 32, 3, 3, 3, device=DEV) * 0.05).to(torch.bfloat16)
    b1 = (torch.randn(32, device=DEV) * 0.1).to(torch.bfloat16)
    q_in, q_mid, q_pool, q_out = quantizer(-4.0, 4.0), quantizer(-3.0, 3.0), quantizer(-3.0, 3.0), quantizer(-2.0, 2.0)
    w1q = quantizer(w1.float().reshape(32, -1).amin(1), w1.float().reshape(32, -1).amax(1), symmetric=True, granularity=ff.PerChannel(0))(w1)
    w2q = quantizer(w2.float().min(), w2.float().max(), symmetric=True)(w2)

    def block(x):
        h = conv(q_in(x), w1q, b1, 1, 1, output_quantizer=q_mid)
        h = F.avg_pool3d(h, 2, 2, output_quantizer=q_pool, strict_quantization=False)
        return conv(h, w2q, None, 1, 1, output_quantizer=q_out)

    x = torch.randn(2, 16, 8, 8, 8, device=DEV, dtype=torch.bfloat16)
    eager = _plain(block(x)).clone()
    assert launches == {"conv3d_w8a8": 2, "pool3d_quantize": 1} and eager.shape == (2, 24, 4, 4, 4)
    static = x.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            block(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _plain(block(static))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager)
    assert launches == {"conv3d_w8a8": 8, "pool3d_quantize": 4}


# ---- the memory contract of the C entry point ---------------------------------------------------------------------------------------
MARGIN = 4096


@pytest.mark.parametrize("requant", [False, True])
def test_guard_bands_around_the_output_and_the_workspace(requant, launches):
    """`out` and the workspace (exactly the queried size) sit inside larger buffers filled with a poison byte; two runs with two
    poisons: the margins keep their poison (no stray write), and the runs agree on every output element (none left unwritten, none
    computed from workspace bytes the call did not write itself)."""
    B, C, D, H, W, OC, K, s, p, d = 2, 20, 4, 6, 7, 130, (3, 2, 3), (1, 1, 2), (1, 0, 2), (1, 2, 1)
    g = torch.Generator().manual_seed(12)
    xc = torch.randint(-128, 128, (B, C, D, H, W), generator=g, dtype=torch.int8).to(DEV)
    wc = torch.randint(-128, 128, (OC, C, *K), generator=g, dtype=torch.int8).to(DEV)
    xs, xo = torch.tensor([0.03], device=DEV), torch.tensor([5.0], device=DEV)
    ws, wo = torch.rand(OC, device=DEV) * 1e-2 + 1e-3, torch.full((OC,), -3.0, device=DEV)
    os_ = torch.tensor([0.5], device=DEV)
    size = [(n + 2 * pi - di * (k - 1) - 1) // si + 1 for n, k, si, pi, di in zip((D, H, W), K, s, p, d)]
    numel = B * OC * size[0] * size[1] * size[2]
    out_bytes = numel * (1 if requant else 2)
    lib = ops._native.library()
    nbytes = lib.ffq_conv3d_w8a8_workspace_bytes(B, C, D, H, W, OC, *K, 0)
    assert nbytes == -(-B * D * H * W * 32 // 256) * 256 + -(-OC * 18 * 32 // 256) * 256 + -(-(OC * 18 + OC) * 4 // 256) * 256
    stream = torch.cuda.current_stream().cuda_stream
    results = []
    for poison in (0x5A, 0xA5):
        out_buf = torch.full((MARGIN + out_bytes + MARGIN,), poison, dtype=torch.uint8, device=DEV)
        ws_buf = torch.full((MARGIN + nbytes + MARGIN,), poison, dtype=torch.uint8, device=DEV)
        rc = lib.ffq_conv3d_w8a8(xc.data_ptr(), 0, wc.data_ptr(), xs.data_ptr(), xo.data_ptr(), ws.data_ptr(), wo.data_ptr(), 1, None, 0,
                                 out_buf.data_ptr() + MARGIN, int(DType.I8 if requant else DType.BF16), os_.data_ptr() if requant else None, None,
                                 8.0, int(DType.BF16) if requant else 0, B, C, D, H, W, OC, *K, *s, *p, *d, ws_buf.data_ptr() + MARGIN, nbytes, stream)
        assert rc == Status.OK, lib.ffq_last_error()
        torch.cuda.synchronize()
        for buf, inner in ((out_buf, out_bytes), (ws_buf, nbytes)):
            assert bool((buf[:MARGIN] == poison).all()) and bool((buf[MARGIN + inner:] == poison).all())
        results.append(out_buf[MARGIN:MARGIN + out_bytes].clone())
    assert torch.equal(results[0], results[1])
    want = ops.conv3d_w8a8(xc, wc, xs, xo, ws, wo, None, s, p, d, **(dict(out_scale=os_, requant_from=torch.bfloat16) if requant else {}))
    assert torch.equal(results[0], want.reshape(-1).view(torch.uint8))
    assert launches["conv3d_w8a8"] == 1
