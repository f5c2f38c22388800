"""The W8A8 transposed convolution (csrc/ffq_conv_transpose.hip) on the MI355X.

* exact: with unit scales and no offsets the fp32 output is the integer accumulator, computed independently as a float64
  F.conv_transpose2d of the codes (exact below 2^53); with real scales and offsets it is the epilogue of include/ffq.h restated with
  torch ops in the kernel's fp32 order;
* against the device reference chain (dequantize, F.conv_transpose1d / F.conv_transpose2d, the output quantizer): within the
  tolerances the linear is held to (tests/parity_cases.py::linear_tolerances), and the fused output quantizer's codes are A1 of the
  unfused value bit for bit;
* layout, views, declines, graph capture, the G26 cases and the full-size U-Net / DCGAN / vocoder shapes.

Every test counts the calls of ``ops.conv_transpose2d_w8a8``, so a silent fallback fails it."""

import contextlib

import pytest
import torch

import fastforward_amd as ff

from conftest import golden
from fastforward_amd import dispatcher, ops
from fastforward_amd.nn import functional as F
from parity_cases import linear_tolerances
from test_conv_transpose_cpu import run_g26_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
CONVT = ff.nn.quantized_conv_transpose_modules()


@pytest.fixture(autouse=True)
def _inference():
    """Inference, as the models run: under grad mode the quantizers' learnable parameters send every call to the chain."""
    with torch.no_grad():
        yield


@pytest.fixture()
def launches(monkeypatch):
    """[number of calls of ops.conv_transpose2d_w8a8]"""
    count = [0]
    real = ops.conv_transpose2d_w8a8

    def counted(*a, **k):
        count[0] += 1
        return real(*a, **k)

    monkeypatch.setattr(ops, "conv_transpose2d_w8a8", counted)
    return count


@pytest.fixture()
def no_fused(monkeypatch):
    """A context in which the dispatcher has no kernel for conv_transpose1d / conv_transpose2d: the reference chain runs."""

    @contextlib.contextmanager
    def off():
        with monkeypatch.context() as m:
            for op in ("conv_transpose1d", "conv_transpose2d"):
                m.setitem(dispatcher._DISPATCHER, op, [])
            yield

    return off


def quantizer(lo, hi, symmetric=False, granularity=None, bits=8):
    q = ff.nn.LinearQuantizer(bits, symmetric=symmetric, granularity=granularity or ff.PerTensor(), quantized_dtype=torch.int8, device=DEV)
    q.quantization_range = (torch.as_tensor(lo, dtype=torch.float32, device=DEV), torch.as_tensor(hi, dtype=torch.float32, device=DEV))
    return q


def operands(B, C, OC, spatial, k, dtype, positive=False, w_offset=False, per_channel=True, seed=0):
    """(input codes, weight codes) as QuantizedTensors: per-tensor asymmetric input; weights [C, OC, *k] per output channel
    (PerChannel(1)) or per tensor, symmetric or asymmetric with offsets."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, C, *spatial, generator=g) * 3 + 0.25 if positive else torch.randn(B, C, *spatial, generator=g) * 1.5 + 0.3
    w = torch.randn(C, OC, *k, generator=g) * (0.5 / (C * k[0] * (k[1] if len(k) > 1 else 1)) ** 0.5)
    x, w = x.to(DEV, dtype), w.to(DEV, dtype)
    xq = quantizer(x.float().min(), x.float().max())(x)
    if per_channel:
        wf = w.float().transpose(0, 1).reshape(OC, -1)
        lo, hi = wf.amin(1), wf.amax(1)
    else:
        lo, hi = w.float().min(), w.float().max()
    if w_offset:
        lo, hi = lo * 1.3, hi * 0.7  # a real zero-point
    wq = quantizer(lo, hi, symmetric=not w_offset, granularity=ff.PerChannel(1) if per_channel else None)(w)
    return xq, wq


def convt(dims, *args, **kwargs):
    return (F.conv_transpose2d if dims == 2 else F.conv_transpose1d)(*args, strict_quantization=False, **kwargs)


def accumulator64(xc, wc, stride, padding, output_padding, dilation):
    """sum over the taps that reach the input and over c of x[b, c, ih, iw] * w[c, n, t], in float64 (exact): [B, OC, OH, OW]."""
    return torch.nn.functional.conv_transpose2d(xc.double(), wc.double(), None, stride, padding, output_padding, 1, dilation)


# ---- exact ---------------------------------------------------------------------------------------------------------------------
# (B, C, OC, (H, W), kernel, stride, padding, output_padding, dilation)
EXACT = [
    (2, 3, 70, (13, 11), (4, 4), (2, 2), (1, 1), (0, 0), (1, 1)),
    (3, 80, 130, (9, 10), (3, 3), (1, 1), (1, 1), (0, 0), (2, 1)),
    (1, 64, 64, (8, 8), (2, 2), (2, 2), (0, 0), (0, 0), (1, 1)),
    (2, 16, 40, (1, 53), (1, 16), (1, 8), (0, 4), (0, 0), (1, 1)),
    (2, 24, 33, (7, 6), (2, 2), (3, 3), (0, 0), (0, 0), (1, 1)),      # stride 3 / kernel 2: a third of the positions have no tap
    (2, 20, 48, (6, 7), (3, 3), (2, 3), (1, 2), (1, 2), (2, 3)),      # gcd(stride, dilation) > 1, output_padding
    (1, 16, 16, (5, 5), (3, 5), (8, 8), (2, 0), (7, 3), (1, 2)),      # 64 phases
]


@pytest.mark.parametrize("shape", EXACT)
def test_unit_scales_give_the_integer_accumulator(shape, launches):
    B, C, OC, (H, W), k, s, p, op, d = shape
    g = torch.Generator().manual_seed(1)
    xc = torch.randint(-128, 128, (B, C, H, W), generator=g, dtype=torch.int8).to(DEV)
    wc = torch.randint(-128, 128, (C, OC, *k), generator=g, dtype=torch.int8).to(DEV)
    one = torch.ones(1, device=DEV)
    out = ops.conv_transpose2d_w8a8(xc, wc, one, None, one, None, None, s, p, op, d, out_dtype=torch.float32)
    assert launches[0] == 1
    assert torch.equal(out, accumulator64(xc, wc, s, p, op, d).float())


def _restated(xq, wq, bias, s, p, op, d):
    """include/ffq.h's epilogue with torch ops in the kernel's fp32 order (on the host: IEEE fp32, no FMA)."""
    px, pw_ = xq.quantization_context.quantization_params, wq.quantization_context.quantization_params
    xc, wc = xq.raw_data.cpu().double(), wq.raw_data.cpu().double()
    C, OC, kh, kw = wc.shape
    B, _, H, W = xc.shape
    ct = lambda x, w: torch.nn.functional.conv_transpose2d(x, w, None, s, p, op, 1, d)  # noqa: E731
    acc = ct(xc, wc)
    ones = torch.ones(B, 1, H, W, dtype=torch.float64)
    rsx = ct(xc, torch.ones(C, 1, kh, kw, dtype=torch.float64))   # [B, 1, OH, OW]: the codes under the taps of V(p)
    rsw = ct(ones, wc.sum(0, keepdim=True))                       # [B, OC, OH, OW]: the per-tap weight sums over V(p)
    cnt = C * ct(ones, torch.ones(1, 1, kh, kw, dtype=torch.float64))
    sx = px.scale.float().cpu().reshape(())
    ox = torch.round(px.offset.float().cpu().reshape(()))
    sw = pw_.scale.float().cpu().reshape(1, -1, 1, 1)
    ow = torch.round(pw_.offset.float().cpu()).reshape(1, -1, 1, 1)
    v = acc.float()
    v = v + ox * rsw.float()
    v = v + ow * rsx.float()
    v = v + cnt.float() * ox * ow
    y = (sx * sw) * v
    if bias is not None:
        y = y + bias.float().cpu().reshape(1, OC, 1, 1)
    return y


@pytest.mark.parametrize("positive", [False, True])
@pytest.mark.parametrize("geometry", [((4, 4), 2, 1, 0, 1), ((2, 2), 3, 0, 0, 1), ((3, 3), (2, 3), (1, 2), (1, 2), (2, 3))])
def test_the_affine_epilogue_is_the_stated_one(geometry, positive, launches):
    k, s, p, op, d = geometry
    xq, wq = operands(2, 24, 40, (9, 12), k, torch.float32, positive=positive, w_offset=True, seed=2)
    ox = float(torch.round(xq.quantization_context.quantization_params.offset))
    assert ox != 0 and (not positive or abs(ox) > 127)
    assert bool((torch.round(wq.quantization_context.quantization_params.offset) != 0).any())
    bias = torch.randn(40, device=DEV)
    out = convt(2, xq, wq, bias, s, p, op, 1, d)
    assert launches[0] == 1
    pair = lambda v: (v, v) if isinstance(v, int) else v  # noqa: E731
    assert torch.equal(out.cpu(), _restated(xq, wq, bias, pair(s), pair(p), pair(op), pair(d)))


# ---- the sweep against the device reference chain ---------------------------------------------------------------------------------
# (dims, B, C, OC, spatial, kernel, stride, padding, output_padding, dilation, bias, dtype, positive input, per-channel weights)
SWEEP = [
    (2, 2, 16, 40, (9, 11), 2, 2, 0, 0, 1, "plain", torch.bfloat16, False, True),
    (2, 1, 3, 64, (17, 15), 4, 2, 1, 0, 1, None, torch.bfloat16, False, True),            # C = 3
    (2, 2, 64, 130, (7, 9), 1, 1, 0, 0, 1, "quantized", torch.float16, False, True),      # OC not a multiple of 128
    (2, 2, 80, 96, (8, 7), 3, 2, 1, 1, 1, "plain", torch.bfloat16, True, False),          # output_padding
    (2, 2, 16, 33, (13, 13), 3, 1, 2, 0, 2, None, torch.float16, True, True),             # dilation, stride 1
    (2, 32, 16, 24, (5, 5), 4, 2, 1, 0, 1, "plain", torch.bfloat16, False, True),
    (2, 1, 64, 200, (11, 7), 3, (2, 4), (1, 0), (1, 2), 2, "quantized", torch.bfloat16, True, True),  # empty phases
    (2, 2, 3, 17, (9, 9), 2, 3, 0, 0, 1, "plain", torch.float32, False, True),            # stride 3 / kernel 2
    (2, 2, 80, 144, (6, 10), 5, 3, 2, 2, 1, "plain", torch.float16, False, False),
    (2, 32, 3, 20, (15, 13), 3, 2, 0, 1, 1, "quantized", torch.float32, True, True),
    (2, 3, 32, 48, (7, 11), (3, 2), (2, 3), (1, 2), (1, 2), (2, 3), None, torch.bfloat16, False, True),
    (1, 2, 80, 130, (37,), 16, 8, 4, 0, 1, "plain", torch.bfloat16, False, True),         # vocoder k16 s8 p4
    (1, 2, 64, 96, (41,), 4, 2, 1, 0, 1, None, torch.float16, True, True),
    (1, 1, 16, 40, (29,), 4, 4, 0, 0, 1, "quantized", torch.bfloat16, False, False),
    (1, 32, 3, 20, (19,), 3, 2, 1, 1, 2, "plain", torch.bfloat16, False, True),           # empty phases, 1-D
    (1, 2, 80, 48, (31,), 2, 3, 0, 2, 1, "plain", torch.float32, False, True),            # stride 3 / kernel 2, 1-D
]


@pytest.mark.parametrize("w_offset", [False, True])
@pytest.mark.parametrize("case", range(len(SWEEP)))
def test_against_the_device_reference_chain(case, w_offset, launches, no_fused):
    dims, B, C, OC, spatial, k, stride, padding, output_padding, dilation, bias_kind, dtype, positive, per_channel = SWEEP[case]
    kernel = k if isinstance(k, tuple) else (k,) * dims
    xq, wq = operands(B, C, OC, spatial, kernel, dtype, positive=positive, w_offset=w_offset, per_channel=per_channel, seed=case)
    if positive:
        assert abs(float(torch.round(xq.quantization_context.quantization_params.offset))) > 127  # -ox does not fit int8
    bias = None
    if bias_kind is not None:
        bias = (torch.randn(OC) * 0.2).to(DEV, dtype)
        if bias_kind == "quantized":
            bias = quantizer(-0.5, 0.5, symmetric=True)(bias)
    args = (xq, wq, bias, stride, padding, output_padding, 1, dilation)
    fused = convt(dims, *args)
    assert launches[0] == 1
    with no_fused():
        chain = convt(dims, *args)
    assert launches[0] == 1
    assert fused.dtype == chain.dtype == dtype and fused.shape == chain.shape and fused.stride() == chain.stride()
    atol, rtol = linear_tolerances(dtype)
    torch.testing.assert_close(fused.float(), chain.float(), atol=atol, rtol=rtol)
    # the output quantizer in the epilogue: A1 of the value the unfused launch returns, bit for bit
    out_q = quantizer(chain.float().min(), chain.float().max())
    codes = convt(dims, *args, output_quantizer=out_q)
    assert launches[0] == 2
    assert isinstance(codes, ff.QuantizedTensor) and codes.raw_data.dtype == torch.int8
    assert torch.equal(codes.raw_data, out_q(fused).raw_data)
    assert torch.equal(codes.dequantize(), out_q(fused).dequantize())


@pytest.mark.parametrize("dims", [1, 2])
def test_tap_free_positions_equal_the_bias_exactly(dims, launches):
    """stride 3 / kernel 2: outputs o = 2 (mod 3) on an axis have no tap; there y is the bias alone, or 0 without one."""
    spatial, k = ((6, 7), (2, 2)) if dims == 2 else ((11,), (2,))
    xq, wq = operands(2, 16, 40, spatial, k, torch.float32, positive=True, w_offset=True, seed=11)
    bias = torch.randn(40, device=DEV)
    for b in (bias, None):
        out = convt(dims, xq, wq, b, 3)
        want = (bias if b is not None else torch.zeros(40, device=DEV)).reshape(1, 40, *([1] * dims))
        free = out[..., 2::3] if dims == 1 else out[:, :, 2::3, :]
        assert free.numel() and torch.equal(free, want.expand_as(free))
        if dims == 2:
            assert torch.equal(out[:, :, :, 2::3], want.expand_as(out[:, :, :, 2::3]))
    assert launches[0] == 2


@pytest.mark.parametrize("index", range(20))
def test_the_g26_cases_on_the_device(index, launches):
    """The reference's own outputs (computed on the CPU): the fused route's value within the linear's tolerance of them, and the
    fused quantizer's codes as far from the reference's as that difference allows: both are clamp(rne(y / s - o)) of their own y,
    and each rounding moves a code by at most one half, so |code - code_ref| <= |y - y_ref| / s + 1."""
    case = golden("g26_conv_transpose.pt")[index]
    value, quantized = run_g26_case(case, DEV)
    assert launches[0] == 2
    atol, rtol = linear_tolerances(case["value"].dtype)
    torch.testing.assert_close(value.float().cpu(), case["value"].float(), atol=atol, rtol=rtol)
    assert isinstance(quantized, ff.QuantizedTensor) and quantized.raw_data.shape == case["codes"].shape
    scale = case["params"]["output_quantizer"]["scale"].float().reshape(())
    apart = (quantized.raw_data.cpu().float() - case["codes"].float()).abs()
    assert bool((apart <= (value.float().cpu() - case["value"].float()).abs() / scale + 1).all()), float(apart.max())


# ---- layout -----------------------------------------------------------------------------------------------------------------------
def test_output_is_contiguous_nchw_and_channels_last_input_agrees(launches, no_fused):
    xq, wq = operands(4, 32, 48, (10, 9), (4, 4), torch.bfloat16, seed=5)
    out = convt(2, xq, wq, None, 2, 1)
    assert out.is_contiguous() and out.shape == (4, 48, 20, 18)
    with no_fused():
        chain = convt(2, xq, wq, None, 2, 1)
    assert out.stride() == chain.stride()
    out.view(4, -1)  # a later .view works as on the reference's output
    x_cl = xq.dequantize().to(memory_format=torch.channels_last)
    q = quantizer(-4.0, 5.0)
    xq_cl = q(x_cl)
    xq_nchw = q(x_cl.contiguous())
    assert torch.equal(xq_cl.raw_data.contiguous(), xq_nchw.raw_data)
    a, b = convt(2, xq_cl, wq, None, 2, 1), convt(2, xq_nchw, wq, None, 2, 1)
    assert a.is_contiguous() and torch.equal(a, b)
    codes = xq_nchw.raw_data.to(memory_format=torch.channels_last)
    one = torch.ones(1, device=DEV)
    assert torch.equal(ops.conv_transpose2d_w8a8(codes, wq.raw_data, one, None, one, None, stride=2, out_dtype=torch.float32),
                       ops.conv_transpose2d_w8a8(codes.contiguous(), wq.raw_data, one, None, one, None, stride=2, out_dtype=torch.float32))
    assert launches[0] == 5


def test_offset_and_strided_views_give_the_bits_of_their_contiguous_copies(launches):
    g = torch.Generator().manual_seed(9)
    big_x = torch.randint(-128, 128, (3, 40, 9, 14), generator=g, dtype=torch.int8).to(DEV)
    big_w = torch.randint(-128, 128, (40, 50, 3, 6), generator=g, dtype=torch.int8).to(DEV)
    scale = torch.rand(24, device=DEV) * 1e-2 + 1e-3
    views = [(big_x[1:, 4:36, 1:8, 2:13], big_w[4:36, 3:27, :, 1:4]),       # offset views
             (big_x[:, ::2, :, ::2], big_w[::2, 1:49:2, :, ::2]),            # strided views
             (big_x[:, 8:40].transpose(2, 3), big_w[8:40, :24].transpose(2, 3))]
    one = torch.ones(1, device=DEV)
    off = torch.tensor([3.0], device=DEV)
    for xv, wv in views:
        assert not xv.is_contiguous() and not wv.is_contiguous()
        got = ops.conv_transpose2d_w8a8(xv, wv, one, off, scale, None, None, 2, 1, 1, out_dtype=torch.float32)
        want = ops.conv_transpose2d_w8a8(xv.contiguous(), wv.contiguous(), one, off, scale, None, None, 2, 1, 1, out_dtype=torch.float32)
        assert torch.equal(got, want)
    assert launches[0] == 6


# ---- declines ---------------------------------------------------------------------------------------------------------------------
def test_what_the_predicates_decline_takes_the_chain(launches, no_fused):
    xq, wq = operands(2, 16, 32, (8, 8), (4, 4), torch.bfloat16, seed=6)
    w_half = quantizer(-0.3, 0.3, symmetric=True)(torch.randn(16, 16, 4, 4, device=DEV, dtype=torch.bfloat16) * 0.1)
    grouped = convt(2, xq, w_half, None, 2, 1, groups=2)
    w = wq.dequantize()
    w_in = quantizer(w.float().amin((1, 2, 3)), w.float().amax((1, 2, 3)), symmetric=True, granularity=ff.PerChannel(0))(w)
    per_input_channel = convt(2, xq, w_in, None, 2, 1)
    x = xq.dequantize()
    xq_pc = quantizer(x.float().amin((0, 2, 3)), x.float().amax((0, 2, 3)), granularity=ff.PerChannel(1))(x)
    per_channel = convt(2, xq_pc, wq, None, 2, 1)
    many_phases = convt(2, xq, wq, None, (8, 9))   # 72 phases: the rule of fused_conv_transpose.transposed_geometry
    assert launches[0] == 0
    with no_fused():
        assert torch.equal(grouped, convt(2, xq, w_half, None, 2, 1, groups=2))
        assert torch.equal(per_input_channel, convt(2, xq, w_in, None, 2, 1))
        assert torch.equal(per_channel, convt(2, xq_pc, wq, None, 2, 1))
        assert torch.equal(many_phases, convt(2, xq, wq, None, (8, 9)))
    # plain float input (weight-only) with strict quantization off: the chain
    convt(2, x, wq, None, 2, 1)
    assert launches[0] == 0
    convt(2, xq, wq, None, (8, 8))
    assert launches[0] == 1


def test_grad_mode_with_learnable_quantizer_parameters_takes_the_chain(launches):
    xq, wq = operands(2, 16, 32, (8, 8), (4, 4), torch.bfloat16, seed=7)
    with torch.enable_grad():
        convt(2, xq, wq, None, 2, 1)
    assert launches[0] == 0
    convt(2, xq, wq, None, 2, 1)
    assert launches[0] == 1


# ---- graph capture ----------------------------------------------------------------------------------------------------------------
def _plain(t):
    return t.dequantize() if isinstance(t, ff.QuantizedTensor) else t


def test_graph_replay_of_a_small_decoder_equals_eager(launches):
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.ConvTranspose2d(16, 32, 4, stride=2, padding=1), torch.nn.ReLU(),
                                torch.nn.ConvTranspose2d(32, 3, 2, stride=2)).to(DEV, torch.bfloat16)
    surrogates = ff.nn.surrogate_quantized_modules(model, extra_conversion=CONVT)
    model = ff.quantize_model(model, extra_conversion={**CONVT, **surrogates})
    assert type(model[0]) is ff.nn.QuantizedConvTranspose2d and type(model[2]) is ff.nn.QuantizedConvTranspose2d
    act = lambda: ff.nn.LinearQuantizer(8, symmetric=False, quantized_dtype=torch.int8, device=DEV)  # noqa: E731
    model[0].input_quantizer, model[1].input_quantizer, model[1].output_quantizer, model[2].output_quantizer = act(), act(), act(), act()
    for m in (model[0], model[2]):
        m.weight_quantizer = ff.nn.LinearQuantizer(8, granularity=ff.PerChannel(1), quantized_dtype=torch.int8, device=DEV)
    x = torch.randn(4, 16, 8, 8, device=DEV, dtype=torch.bfloat16)
    with torch.no_grad(), ff.strict_quantization(False):
        with ff.estimate_ranges(model, ff.range_setting.running_minmax):
            model(x)
        before = launches[0]
        eager = _plain(model(x)).clone()
        assert launches[0] == before + 2 and eager.shape == (4, 3, 32, 32)
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


# ---- full size: U-Net up-convolutions, a DCGAN generator and a vocoder stack, exact against the float64 accumulator --------------------
# (B, C, OC, (H, W), (KH, KW), stride, padding)
FULL = [
    (32, 1024, 512, (28, 28), (2, 2), (2, 2), (0, 0)),
    (32, 512, 256, (56, 56), (2, 2), (2, 2), (0, 0)),
    (32, 256, 128, (112, 112), (2, 2), (2, 2), (0, 0)),
    (32, 512, 256, (8, 8), (4, 4), (2, 2), (1, 1)),
    (32, 256, 128, (16, 16), (4, 4), (2, 2), (1, 1)),
    (32, 128, 64, (32, 32), (4, 4), (2, 2), (1, 1)),
    (32, 64, 3, (64, 64), (4, 4), (2, 2), (1, 1)),
    (32, 512, 256, (1, 256), (1, 16), (1, 8), (0, 4)),
    (32, 256, 128, (1, 2048), (1, 16), (1, 8), (0, 4)),
    (32, 128, 64, (1, 16384), (1, 4), (1, 2), (0, 1)),
]


@pytest.mark.parametrize("case", range(len(FULL)))
def test_full_size_shapes_are_exact(case, launches):
    B, C, OC, (H, W), k, s, p = FULL[case]
    g = torch.Generator(device=DEV).manual_seed(case)
    xc = torch.randint(-128, 128, (B, C, H, W), generator=g, device=DEV, dtype=torch.int8)
    wc = torch.randint(-128, 128, (C, OC, *k), generator=g, device=DEV, dtype=torch.int8)
    one = torch.ones(1, device=DEV)
    out = ops.conv_transpose2d_w8a8(xc, wc, one, None, one, None, None, s, p, (0, 0), (1, 1), out_dtype=torch.float32)
    assert launches[0] == 1
    for b in range(0, B, 4):  # the float64 accumulator four images at a time
        assert torch.equal(out[b:b + 4], accumulator64(xc[b:b + 4], wc, s, p, (0, 0), (1, 1)).float()), b
