"""The W8A8 convolution (csrc/ffq_conv.hip) on the MI355X.

* exact: with unit scales and no offsets the fp32 output is the integer accumulator, computed independently as F.unfold of the
  codes and a float64 matmul (exact below 2^53); with real scales and offsets it is the epilogue of include/ffq.h restated with
  torch ops in the kernel's fp32 order;
* against the device reference chain (dequantize, F.conv1d / F.conv2d, the output quantizer): within the tolerances the linear is
  held to (tests/parity_cases.py::linear_tolerances), and the fused output quantizer's codes are A1 of the unfused value bit for bit;
* layout, declines, graph capture and the full-size ResNet-50 / Whisper shapes.

Every test counts the calls of ``ops.conv2d_w8a8``, so a silent fallback fails it."""

import contextlib

import pytest
import torch

import fastforward_amd as ff

from fastforward_amd import dispatcher, ops
from fastforward_amd.nn import functional as F
from parity_cases import linear_tolerances
from test_conv_cpu import _plain, install_quantizers, quantize_cnn, tiny_cnn

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _inference():
    """Inference, as the models run: under grad mode the quantizers' learnable parameters send every call to the chain."""
    with torch.no_grad():
        yield


@pytest.fixture()
def launches(monkeypatch):
    """[number of calls of ops.conv2d_w8a8]"""
    count = [0]
    real = ops.conv2d_w8a8

    def counted(*a, **k):
        count[0] += 1
        return real(*a, **k)

    monkeypatch.setattr(ops, "conv2d_w8a8", counted)
    return count


@pytest.fixture()
def no_fused_conv(monkeypatch):
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


def operands(B, C, OC, spatial, k, dtype, positive=False, w_offset=False, seed=0):
    """(input codes, weight codes) as QuantizedTensors: per-tensor asymmetric input, per-output-channel weights (symmetric, or
    asymmetric with offsets)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, C, *spatial, generator=g) * 3 + 0.25 if positive else torch.randn(B, C, *spatial, generator=g) * 1.5 + 0.3
    w = torch.randn(OC, C, *k, generator=g) * (0.5 / (C * k[0] * (k[1] if len(k) > 1 else 1)) ** 0.5)
    x, w = x.to(DEV, dtype), w.to(DEV, dtype)
    xq = quantizer(x.float().min(), x.float().max())(x)
    wf = w.float().reshape(OC, -1)
    lo, hi = wf.amin(1), wf.amax(1)
    if w_offset:
        lo, hi = lo * 1.3, hi * 0.7  # a real zero-point per channel
    wq = quantizer(lo, hi, symmetric=not w_offset, granularity=ff.PerChannel(0))(w)
    return xq, wq


def conv(dims, *args, **kwargs):
    return (F.conv2d if dims == 2 else F.conv1d)(*args, strict_quantization=False, **kwargs)


def accumulator64(xc, wc, stride, padding, dilation):
    """sum_{t, c} x[b, c, ih, iw] * w[n, c, t] with code 0 outside the image, in float64 (exact): [B, OC, OH, OW]."""
    B = xc.shape[0]
    OC = wc.shape[0]
    kh, kw = wc.shape[2:]
    cols = torch.nn.functional.unfold(xc.double(), (kh, kw), dilation=dilation, padding=padding, stride=stride)  # [B, C kh kw, L]
    acc = wc.double().reshape(OC, -1) @ cols
    H, W = xc.shape[2:]
    OH = (H + 2 * padding[0] - dilation[0] * (kh - 1) - 1) // stride[0] + 1
    OW = (W + 2 * padding[1] - dilation[1] * (kw - 1) - 1) // stride[1] + 1
    return acc.reshape(B, OC, OH, OW)


# ---- exact ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 70, (13, 11), (7, 7), (2, 2), (3, 3), (1, 1)), (3, 80, 130, (9, 10), (3, 3), (1, 1), (1, 1), (2, 1)),
                                   (1, 64, 64, (8, 8), (1, 1), (2, 2), (0, 0), (1, 1)), (2, 16, 40, (1, 53), (1, 5), (1, 2), (0, 2), (1, 3))])
def test_unit_scales_give_the_integer_accumulator(shape, launches):
    B, C, OC, (H, W), k, s, p, d = shape
    g = torch.Generator().manual_seed(1)
    xc = torch.randint(-128, 128, (B, C, H, W), generator=g, dtype=torch.int8).to(DEV)
    wc = torch.randint(-128, 128, (OC, C, *k), generator=g, dtype=torch.int8).to(DEV)
    one = torch.ones(1, device=DEV)
    out = ops.conv2d_w8a8(xc, wc, one, None, one, None, None, s, p, d, out_dtype=torch.float32)
    assert launches[0] == 1
    assert torch.equal(out, accumulator64(xc, wc, s, p, d).float())


def _restated(xq, wq, bias, s, p, d):
    """include/ffq.h's epilogue with torch ops in the kernel's fp32 order (on the host: IEEE fp32, no FMA)."""
    px, pw_ = xq.quantization_context.quantization_params, wq.quantization_context.quantization_params
    xc, wc = xq.raw_data.cpu(), wq.raw_data.cpu()
    OC, C, kh, kw = wc.shape
    acc = accumulator64(xc, wc, s, p, d)
    B, _, OH, OW = acc.shape
    ones = torch.ones(B, 1, *xc.shape[2:], dtype=torch.float64)
    mask = torch.nn.functional.unfold(ones, (kh, kw), dilation=d, padding=p, stride=s)  # [B, taps, L]: 1 where the tap is inside
    rsx = torch.nn.functional.unfold(xc.double(), (kh, kw), dilation=d, padding=p, stride=s).sum(1).reshape(B, 1, OH, OW)
    tapsum = wc.double().sum(1).reshape(OC, kh * kw)
    rsw = (tapsum @ mask).reshape(B, OC, OH, OW)
    cnt = (C * mask.sum(1)).reshape(B, 1, OH, OW)
    sx = px.scale.float().cpu().reshape(())
    ox = torch.round(px.offset.float().cpu().reshape(()))
    sw = pw_.scale.float().cpu().reshape(1, OC, 1, 1)
    ow = torch.round(pw_.offset.float().cpu()).reshape(1, OC, 1, 1)
    v = acc.float()
    v = v + ox * rsw.float()
    v = v + ow * rsx.float()
    v = v + cnt.float() * ox * ow
    y = (sx * sw) * v
    if bias is not None:
        y = y + bias.float().cpu().reshape(1, OC, 1, 1)
    return y


@pytest.mark.parametrize("positive", [False, True])
def test_the_affine_epilogue_is_the_stated_one(positive, launches):
    xq, wq = operands(2, 24, 40, (9, 12), (3, 3), torch.float32, positive=positive, w_offset=True, seed=2)
    assert float(torch.round(xq.quantization_context.quantization_params.offset)) != 0
    bias = torch.randn(40, device=DEV)
    out = conv(2, xq, wq, bias, 2, 1, 1)
    assert launches[0] == 1
    assert torch.equal(out.cpu(), _restated(xq, wq, bias, (2, 2), (1, 1), (1, 1)))


# ---- the sweep against the device reference chain ---------------------------------------------------------------------------------
# (dims, B, C, OC, spatial, kernel, stride, dilation, padding, bias, dtype, positive input)
SWEEP = [
    (2, 2, 16, 40, (9, 11), 3, 1, 1, 1, "plain", torch.bfloat16, False),
    (2, 1, 3, 64, (17, 15), 7, 2, 1, 3, None, torch.bfloat16, False),
    (2, 2, 64, 130, (7, 9), 1, 1, 1, 0, "quantized", torch.float16, False),
    (2, 2, 80, 96, (8, 7), 5, 1, 1, "same", "plain", torch.bfloat16, True),
    (2, 2, 16, 33, (13, 13), 3, 2, 2, "valid", None, torch.float16, True),
    (2, 32, 16, 24, (5, 5), 3, 1, 1, 1, "plain", torch.bfloat16, False),
    (2, 1, 64, 200, (11, 7), 3, 2, 1, 1, "quantized", torch.bfloat16, True),
    (2, 2, 3, 17, (9, 9), 5, 1, 2, "same", None, torch.float32, False),
    (2, 2, 80, 144, (6, 10), 7, 1, 1, 3, "plain", torch.float16, False),
    (2, 32, 3, 20, (15, 13), 3, 2, 1, 0, "quantized", torch.float32, True),
    (1, 2, 80, 130, (37,), 3, 1, 1, 1, "plain", torch.bfloat16, False),
    (1, 2, 64, 96, (41,), 3, 2, 1, 1, None, torch.float16, True),
    (1, 1, 16, 40, (29,), 5, 1, 2, "same", "quantized", torch.bfloat16, False),
    (1, 32, 3, 20, (19,), 7, 2, 1, 3, "plain", torch.bfloat16, False),
    (1, 2, 80, 48, (31,), 1, 1, 1, "valid", "plain", torch.float32, False),
]


@pytest.mark.parametrize("w_offset", [False, True])
@pytest.mark.parametrize("case", range(len(SWEEP)))
def test_against_the_device_reference_chain(case, w_offset, launches, no_fused_conv):
    dims, B, C, OC, spatial, k, stride, dilation, padding, bias_kind, dtype, positive = SWEEP[case]
    xq, wq = operands(B, C, OC, spatial, (k,) * dims, dtype, positive=positive, w_offset=w_offset, seed=case)
    if positive:
        assert float(torch.round(xq.quantization_context.quantization_params.offset)) > 127  # -ox does not fit int8
    bias = None
    if bias_kind is not None:
        bias = (torch.randn(OC) * 0.2).to(DEV, dtype)
        if bias_kind == "quantized":
            bias = quantizer(-0.5, 0.5, symmetric=True)(bias)
    args = (xq, wq, bias, stride, padding, dilation)
    fused = conv(dims, *args)
    assert launches[0] == 1
    with no_fused_conv():
        chain = conv(dims, *args)
    assert launches[0] == 1
    assert fused.dtype == chain.dtype == dtype and fused.shape == chain.shape and fused.stride() == chain.stride()
    atol, rtol = linear_tolerances(dtype)
    torch.testing.assert_close(fused.float(), chain.float(), atol=atol, rtol=rtol)
    # the output quantizer in the epilogue: A1 of the value the unfused launch returns, bit for bit
    out_q = quantizer(chain.float().min(), chain.float().max())
    codes = conv(dims, *args, output_quantizer=out_q)
    assert launches[0] == 2
    assert isinstance(codes, ff.QuantizedTensor) and codes.raw_data.dtype == torch.int8
    assert torch.equal(codes.raw_data, out_q(fused).raw_data)
    assert torch.equal(codes.dequantize(), out_q(fused).dequantize())


# ---- layout -----------------------------------------------------------------------------------------------------------------------
def test_output_is_contiguous_nchw_and_channels_last_input_agrees(launches, no_fused_conv):
    xq, wq = operands(4, 32, 48, (10, 9), (3, 3), torch.bfloat16, seed=5)
    out = conv(2, xq, wq, None, 1, 1, 1)
    assert out.is_contiguous() and out.shape == (4, 48, 10, 9)
    with no_fused_conv():
        chain = conv(2, xq, wq, None, 1, 1, 1)
    assert out.stride() == chain.stride()
    out.view(4, -1)  # a later .view works as on the reference's output
    x_cl = xq.dequantize().to(memory_format=torch.channels_last)
    q = quantizer(-4.0, 5.0)
    xq_cl = q(x_cl)
    xq_nchw = q(x_cl.contiguous())
    assert torch.equal(xq_cl.raw_data.contiguous(), xq_nchw.raw_data)
    a, b = conv(2, xq_cl, wq, None, 1, 1, 1), conv(2, xq_nchw, wq, None, 1, 1, 1)
    assert a.is_contiguous() and torch.equal(a, b)
    codes = xq_nchw.raw_data.to(memory_format=torch.channels_last)
    one = torch.ones(1, device=DEV)
    assert torch.equal(ops.conv2d_w8a8(codes, wq.raw_data, one, None, one, None, out_dtype=torch.float32),
                       ops.conv2d_w8a8(codes.contiguous(), wq.raw_data, one, None, one, None, out_dtype=torch.float32))
    assert launches[0] == 5


# ---- declines ---------------------------------------------------------------------------------------------------------------------
def test_groups_and_per_channel_activations_take_the_chain(launches, no_fused_conv):
    xq, wq = operands(2, 16, 32, (8, 8), (3, 3), torch.bfloat16, seed=6)
    w_half = quantizer(-0.3, 0.3, symmetric=True)(torch.randn(32, 8, 3, 3, device=DEV, dtype=torch.bfloat16) * 0.1)
    grouped = conv(2, xq, w_half, None, 1, 1, 1, groups=2)
    x = xq.dequantize()
    lo, hi = x.float().amin((0, 2, 3)), x.float().amax((0, 2, 3))
    xq_pc = quantizer(lo, hi, granularity=ff.PerChannel(1))(x)
    per_channel = conv(2, xq_pc, wq, None, 1, 1, 1)
    assert launches[0] == 0
    with no_fused_conv():
        assert torch.equal(grouped, conv(2, xq, w_half, None, 1, 1, 1, groups=2))
        assert torch.equal(per_channel, conv(2, xq_pc, wq, None, 1, 1, 1))
    # plain float input (weight-only) with strict quantization off: the chain
    conv(2, x, wq, None, 1, 1, 1)
    assert launches[0] == 0


# ---- graph capture ----------------------------------------------------------------------------------------------------------------
def test_graph_replay_of_the_tiny_cnn_equals_eager(launches):
    model = quantize_cnn(tiny_cnn(DEV, torch.bfloat16))
    install_quantizers(model, DEV)
    x = torch.randn(4, 3, 8, 8, device=DEV, dtype=torch.bfloat16)
    with torch.no_grad(), ff.strict_quantization(False):
        with ff.estimate_ranges(model, ff.range_setting.running_minmax):
            model(x)
        before = launches[0]
        eager = _plain(model(x)).clone()
        assert launches[0] == before + 2
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


# ---- full size: ResNet-50 and Whisper encoder shapes, exact against the float64 accumulator ---------------------------------------------
# (B, C, OC, (H, W), (KH, KW), stride, padding)
FULL = [
    (32, 64, 64, (56, 56), (3, 3), (1, 1), (1, 1)),
    (32, 256, 64, (56, 56), (1, 1), (1, 1), (0, 0)),
    (32, 128, 128, (28, 28), (3, 3), (1, 1), (1, 1)),
    (32, 512, 128, (28, 28), (1, 1), (1, 1), (0, 0)),
    (32, 256, 256, (14, 14), (3, 3), (1, 1), (1, 1)),
    (32, 512, 512, (7, 7), (3, 3), (1, 1), (1, 1)),
    (32, 3, 64, (224, 224), (7, 7), (2, 2), (3, 3)),
    (32, 128, 128, (56, 56), (3, 3), (2, 2), (1, 1)),
    (32, 80, 384, (1, 3000), (1, 3), (1, 1), (0, 1)),
    (32, 384, 384, (1, 3000), (1, 3), (1, 2), (0, 1)),
]


@pytest.mark.parametrize("case", range(len(FULL)))
def test_full_size_shapes_are_exact(case, launches):
    B, C, OC, (H, W), k, s, p = FULL[case]
    g = torch.Generator(device=DEV).manual_seed(case)
    xc = torch.randint(-128, 128, (B, C, H, W), generator=g, device=DEV, dtype=torch.int8)
    wc = torch.randint(-128, 128, (OC, C, *k), generator=g, device=DEV, dtype=torch.int8)
    one = torch.ones(1, device=DEV)
    out = ops.conv2d_w8a8(xc, wc, one, None, one, None, None, s, p, (1, 1), out_dtype=torch.float32)
    assert launches[0] == 1
    for b in range(0, B, 4):  # the float64 accumulator four images at a time
        assert torch.equal(out[b:b + 4], accumulator64(xc[b:b + 4], wc, s, p, (1, 1)).float()), b


def test_grad_mode_with_learnable_quantizer_parameters_takes_the_chain(launches):
    xq, wq = operands(2, 16, 32, (8, 8), (3, 3), torch.bfloat16, seed=7)
    with torch.enable_grad():
        conv(2, xq, wq, None, 1, 1, 1)
    assert launches[0] == 0
    conv(2, xq, wq, None, 1, 1, 1)
    assert launches[0] == 1
