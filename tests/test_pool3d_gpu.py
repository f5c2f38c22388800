"""The one-pass avg_pool3d kernel (csrc/ffq_pool3d.hip) on the MI355X, against the device reference chain — dequantize the input,
F.avg_pool3d, the output quantizer — that the generated fallback runs (reference _gen/fallback.py:579-612), with this package's
registration taken out of the dispatcher.

The value is bit for bit the chain's (ATen's one fp32 accumulator, its depth / rows / columns order, its one division by the window's
size and its one rounding) and the codes are the output quantizer applied to that value. Also here: one launch feeding two quantizers
without writing the value, the G27 cases, the argument errors with real device buffers, and the memory contract of the C entry point
(local guard bands: tests/guards.py wraps the symbols of ``_cabi.SIGNATURES`` only). Every test counts the calls of
``ops.pool3d_quantize``, so a silent fallback fails it."""

import contextlib
import ctypes

import pytest
import torch

import fastforward_amd as ff

from conftest import golden
from fastforward_amd import _cabi, dispatcher, fused_pool, ops
from fastforward_amd._cabi import DType, Status
from fastforward_amd.nn import functional as F
from test_conv3d_cpu import run_g27_pool
from test_elementwise_gpu import compare_with_chain, operand
from test_modules_gpu import act_quantizer

pytestmark = pytest.mark.gpu
DEV = "cuda"
FORMS = ("plain", "int8_tensor", "container_tensor", "int8_channel", "container_channel")
DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture(autouse=True)
def _inference():
    """Inference, as the models run: under grad mode the quantizers' learnable parameters send every call to the chain."""
    with torch.no_grad():
        yield


@pytest.fixture()
def launches(monkeypatch):
    """[number of calls of ops.pool3d_quantize]"""
    count = [0]
    real = ops.pool3d_quantize

    def counted(*a, **k):
        count[0] += 1
        return real(*a, **k)

    monkeypatch.setattr(ops, "pool3d_quantize", counted)
    return count


@pytest.fixture()
def chain(monkeypatch):
    """A context in which the dispatcher has none of this package's kernels for avg_pool3d: the reference chain runs."""

    @contextlib.contextmanager
    def off():
        with monkeypatch.context() as m:
            kept = [it for it in dispatcher._DISPATCHER.get("avg_pool3d", []) if getattr(it.fn, "__self__", None) is not fused_pool.KERNELS]
            m.setitem(dispatcher._DISPATCHER, "avg_pool3d", kept)
            yield

    return off


def pool_operand(x, form):
    """`x` [B, C, D, H, W] plain, or as codes with per-tensor or per-channel parameters in an int8 or value-dtype container."""
    if not form.endswith("_channel"):
        return operand(x, form)
    per = x.float().transpose(0, 1).reshape(x.shape[1], -1)
    lo, hi = per.amin(-1).clamp(max=-0.5), per.amax(-1).clamp(min=0.5)
    container = torch.int8 if form.startswith("int8") else x.dtype
    return act_quantizer(lo, hi, granularity=ff.PerChannel(1), container=container)(x)


# ---- the named cases ------------------------------------------------------------------------------------------------------------------
CASES = [
    ((2, 6, 7, 9, 10), dict(kernel_size=2, stride=2)),
    ((2, 6, 7, 9, 10), dict(kernel_size=3, stride=2, padding=1)),
    ((2, 6, 7, 9, 10), dict(kernel_size=3, stride=2, padding=1, count_include_pad=False)),
    ((2, 5, 5, 7, 9), dict(kernel_size=2, stride=2, padding=1, ceil_mode=True)),          # the last window would start in the padding
    ((2, 5, 5, 7, 9), dict(kernel_size=3, stride=2, padding=1, ceil_mode=True, count_include_pad=False)),
    ((3, 5, 4, 13, 11), dict(kernel_size=(1, 3, 2), stride=(1, 2, 1))),
    ((1, 3, 9, 33, 35), dict(kernel_size=(2, 3, 3), stride=(2, 1, 2), padding=(0, 1, 1))),  # more than one block
]


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", FORMS)
def test_equals_the_reference_chain(case, dtype, form, launches, chain):
    shape, kwargs = CASES[case]
    torch.manual_seed(70 + case)
    x = (torch.randn(shape, device=DEV) * 2).to(dtype)
    value = compare_with_chain(F.avg_pool3d, (pool_operand(x, form),), kwargs, act_quantizer(-3.0, 3.5), chain)
    assert launches[0] == 2 and value.is_contiguous()


def test_ceil_mode_drops_the_window_that_starts_in_the_padding():
    assert ops.pool.pooled_size(5, 2, 1, 2, 1, True) == 3 and ops.pool.pooled_size(7, 2, 1, 2, 1, True) == 4   # 4 and 5 before the rule


def test_eight_outputs_per_lane_with_a_tail(launches, chain):
    """More than 2^20 outputs take the kernel's 8-outputs-per-lane form; a result whose size is no multiple of 8 ends in a partial group."""
    torch.manual_seed(50)
    x = pool_operand((torch.randn(1, 3, 71, 73, 69, device=DEV) * 2).to(torch.bfloat16), "int8_channel")
    value = compare_with_chain(F.avg_pool3d, (x,), dict(kernel_size=3, stride=1, padding=1), act_quantizer(-3.0, 3.5), chain)
    assert value.numel() >= 2**20 and value.numel() % 8 and launches[0] == 2


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_launch_feeds_two_output_quantizers_without_the_value(dtype, launches):
    torch.manual_seed(41)
    x = (torch.randn(3, 5, 6, 13, 11, device=DEV) * 2).to(dtype)
    qs = [act_quantizer(-3.0, 3.5), act_quantizer(-1.0, 6.0)]
    pairs = [(q.scale, q.offset) for q in qs]
    with torch.no_grad():
        value, codes = ops.pool3d_quantize("avg", x, (3, 3, 3), (2, 2, 2), (1, 1, 1), quantizers=pairs)
        none, codes_only = ops.pool3d_quantize("avg", x, (3, 3, 3), (2, 2, 2), (1, 1, 1), quantizers=pairs, want_value=False)
        assert none is None and torch.equal(value, torch.nn.functional.avg_pool3d(x, 3, 2, 1))
        for q, c, only in zip(qs, codes, codes_only):
            assert torch.equal(c, q(value).raw_data) and torch.equal(only, c)
    assert launches[0] == 2


def test_declines_take_the_chain(launches, chain):
    torch.manual_seed(5)
    x = (torch.randn(2, 4, 6, 8, 8, device=DEV) * 2).to(torch.bfloat16)
    oq = act_quantizer(-3.0, 3.5)
    qx = act_quantizer(-4.0, 5.0)(x)
    calls = [lambda: F.avg_pool3d(x.float(), 2, 2, output_quantizer=oq, strict_quantization=False),                        # fp32 values
             lambda: F.avg_pool3d(qx.dequantize().to(memory_format=torch.channels_last_3d), 2, 2, output_quantizer=oq, strict_quantization=False),
             lambda: F.avg_pool3d(x[0], 2, 2, output_quantizer=oq, strict_quantization=False)]                             # unbatched
    got = [call() for call in calls]
    assert launches[0] == 0
    with chain():
        for value, call in zip(got, calls):
            want = call()
            assert torch.equal(value.raw_data, want.raw_data) and torch.equal(value.dequantize(), want.dequantize())
    with pytest.raises(RuntimeError):   # padding above half the kernel: declined, and ATen raises
        F.avg_pool3d(qx, 2, 2, 2, output_quantizer=oq, strict_quantization=False)
    assert launches[0] == 0
    with torch.no_grad():
        assert not fused_pool.avg_pool3d_predicate(input=qx, kernel_size=2, stride=2, output_quantizer=oq)  # no strict_quantization keyword
        assert fused_pool.avg_pool3d_predicate(input=qx, kernel_size=2, stride=2, output_quantizer=oq, strict_quantization=False)


# ---- G27 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(18))
def test_the_g27_pool_cases_on_the_device(index, launches):
    """The reference ran these in fp32 on the CPU (ATen's CPU avg_pool3d has no bf16 / fp16). In fp32 the call is declined (the kernel
    is built for bf16 / fp16 values) and the device chain answers within fp32 rounding of the reference: a window of n <= 27 values of
    magnitude <= m summed in another order differs by at most n * 2^-24 * n * m, far below atol = 1e-4 for m <= 9.
    With the input rounded to bf16 the fused route runs. Its distance from the fp32 reference: the input's rounding moves every value
    by at most 2^-9 * |x| (plain), or a code by at most one step (quantized: the scale, and A2 then rounds the dequantized value to
    bf16: 2^-9 * |x| again), and an average moves by no more than its inputs; the result's own rounding adds 2^-9 * |y| <= 2^-9 *
    max|x|. Hence atol = 2^-8 * max|x| + scale."""
    case = golden("g27_conv3d.pt")["pool"][index]
    value, quantized = run_g27_pool(case, DEV)
    assert launches[0] == 0
    torch.testing.assert_close(value.cpu(), case["value"], atol=1e-4, rtol=1e-5)
    apart = (quantized.raw_data.cpu().float() - case["codes"].float()).abs()
    assert float(apart.max()) <= 1
    value16, quantized16 = run_g27_pool(case, DEV, torch.bfloat16)
    assert launches[0] == 2 and value16.dtype == torch.bfloat16
    scale = float(case["params"]["input"]["scale"].max()) if case["slots"] else 0.0
    atol = 2.0**-8 * float(case["x"].abs().max()) + scale
    torch.testing.assert_close(value16.float().cpu(), case["value"], atol=atol, rtol=0)
    out_scale = float(case["out_params"]["scale"])
    apart = (quantized16.raw_data.cpu().float() - case["codes"].float()).abs()
    assert float(apart.max()) <= atol / out_scale + 1


# ---- argument errors with real buffers: nothing is launched, nothing is written ------------------------------------------------------
def test_argument_errors_leave_the_output_untouched(launches):
    x = torch.randn(2, 3, 6, 7, 8, device=DEV).to(torch.bfloat16)
    with pytest.raises(ValueError, match="pad should be at most half"):
        ops.pool3d_quantize("avg", x, (2, 2, 2), (2, 2, 2), (2, 0, 0))
    with pytest.raises(RuntimeError, match="mode is"):
        ops.pool3d_quantize("max", x, (2, 2, 2), (2, 2, 2))
    with pytest.raises(RuntimeError, match="positive"):
        ops.pool3d_quantize("avg", x, (2, 0, 2), (2, 2, 2))
    with pytest.raises(NotImplementedError):
        ops.pool3d_quantize("avg", x.float(), (2, 2, 2), (2, 2, 2))
    with pytest.raises(RuntimeError, match="5 dims|\\[B, C, D, H, W\\]"):
        ops.pool3d_quantize("avg", x[0], (2, 2, 2), (2, 2, 2))
    lib = ops._native.library()
    out = torch.full((2 * 3 * 3 * 3 * 4,), 7.0, device=DEV, dtype=torch.bfloat16)
    stream = torch.cuda.current_stream().cuda_stream

    def call(mode=0, size=(6, 7, 8), k=(2, 2, 2), s=(2, 2, 2), p=(0, 0, 0), ceil=0, out_size=(3, 3, 4), x_dt=DType.BF16, scale=None):
        return lib.ffq_pool3d_quantize(mode, x.data_ptr(), int(x_dt), scale, None, 0, int(DType.BF16), 6, *size, *k, *s, *p, ceil, *out_size,
                                       out.data_ptr(), None, stream)

    assert call(mode=2) == Status.ERR_ARG
    assert call(x_dt=DType.I8) == Status.ERR_DTYPE
    assert call(p=(2, 0, 0)) == Status.ERR_ARG
    assert call(out_size=(3, 4, 4)) == Status.ERR_ARG
    assert call(ceil=1) == Status.ERR_ARG          # ceil_mode gives [3, 4, 4]
    assert call(size=(6, 0, 8)) == Status.ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call() == Status.OK
    torch.cuda.synchronize()
    assert torch.equal(out.view(2, 3, 3, 3, 4), torch.nn.functional.avg_pool3d(x, 2, 2))
    assert launches[0] == 5   # the five wrapper calls above, each of which raised


# ---- the memory contract of the C entry point ---------------------------------------------------------------------------------------
MARGIN = 4096


@pytest.mark.parametrize("want_value", [True, False])
def test_guard_bands_around_the_value_and_the_codes(want_value):
    """The value and two code tensors sit inside larger buffers filled with a poison byte; two runs with two poisons: the margins keep
    their poison (no stray write) and the runs agree on every output element (none left unwritten). 2145 outputs: a tail of one."""
    torch.manual_seed(13)
    B, C, size, k, s, p = 1, 5, (5, 11, 13), (3, 3, 3), (2, 1, 1), (1, 1, 1)
    x = torch.randint(-128, 128, (B, C, *size), dtype=torch.int8).to(DEV)
    xs, xo = (torch.rand(C) * 0.05 + 0.01).to(DEV), torch.randint(-5, 6, (C,)).float().to(DEV)
    q_scale = [torch.tensor([0.05], device=DEV), torch.tensor([0.11], device=DEV)]
    out_size = [ops.pool.pooled_size(n, ki, pi, si) for n, ki, pi, si in zip(size, k, p, s)]
    numel = B * C * out_size[0] * out_size[1] * out_size[2]
    assert numel % 8
    lib = ops._native.library()
    stream = torch.cuda.current_stream().cuda_stream
    results = []
    for poison in (0x5A, 0xA5):
        bufs = [torch.full((MARGIN + n + MARGIN,), poison, dtype=torch.uint8, device=DEV) for n in (numel * 2, numel, numel)]
        fan = _cabi.FanOut.make(8.0, [t.data_ptr() for t in q_scale], [None, None], [b.data_ptr() + MARGIN for b in bufs[1:]])
        rc = lib.ffq_pool3d_quantize(1, x.data_ptr(), int(DType.I8), xs.data_ptr(), xo.data_ptr(), C, int(DType.F16), B * C, *size, *k, *s, *p, 0,
                                     *out_size, bufs[0].data_ptr() + MARGIN if want_value else None, ctypes.byref(fan), stream)
        assert rc == Status.OK, lib.ffq_last_error()
        torch.cuda.synchronize()
        for buf, inner in zip(bufs, (numel * 2, numel, numel)):
            assert bool((buf[:MARGIN] == poison).all()) and bool((buf[MARGIN + inner:] == poison).all())
        if not want_value:
            assert bool((bufs[0] == poison).all())
        results.append([b[MARGIN:MARGIN + n].clone() for b, n in zip(bufs, (numel * 2, numel, numel))])
    for a, b in zip(results[0][0 if want_value else 1:], results[1][0 if want_value else 1:]):
        assert torch.equal(a, b)
    value, codes = ops.pool3d_quantize("avg_exclude_pad", x, k, s, p, quantizers=[(q_scale[0], None), (q_scale[1], None)], dtype=torch.float16,
                                       dequant=(xs, xo))
    if want_value:
        assert torch.equal(results[0][0], value.reshape(-1).view(torch.uint8))
    assert torch.equal(results[0][1].view(torch.int8), codes[0].reshape(-1)) and torch.equal(results[0][2].view(torch.int8), codes[1].reshape(-1))
