"""MX formats on the MI355X (csrc/ffq_mx.hip): the quantizer and its inverse bit for bit against the host path, the linear on the
block-scaled MFMA against float64 — exactly on operands built so that fp32 holds every partial sum (tests/mx_cases.py), within the fp32
accumulation bound on ordinary data — and ``QuantizedLinear`` with ``MXQuantizer``s in its slots.

Every test runs with a counting proxy as the loaded library and states how often each ``ffq_mx_*`` entry point (and every other GEMM of the
library) ran, so a silent fallback fails it."""

import pytest
import torch

import fastforward_amd as ff
import guards
import mx_cases

from conftest import use_backend
from fastforward_amd import _host, _native, fused_mx, ops
from fastforward_amd.nn import functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DTYPE_IDS = ["bf16", "fp16", "fp32"]
FORMATS = ("e4m3", "e2m1")
COUNTED = ("ffq_mx_quantize", "ffq_mx_dequantize", "ffq_linear_mx", "ffq_linear_w8a8", "ffq_linear_wq", "ffq_bmm_w8a8", "ffq_linear_w8a8_multi")


class Counting:
    """The loaded library with the calls of COUNTED counted (its path differs from the shipped one's: every call takes the ctypes route)."""

    def __init__(self, real) -> None:
        self._real, self.path, self.backend_name = real, f"{real.path}#counted", real.backend_name
        self.counts = dict.fromkeys(COUNTED, 0)

    @property
    def is_device(self) -> bool:
        return self._real.is_device

    def check(self, status: int) -> None:
        self._real.check(status)

    def __getattr__(self, name: str):
        attr = getattr(self._real, name)
        if name not in COUNTED or attr is None:
            return attr

        def counted(*args):
            self.counts[name] += 1
            return attr(*args)

        return counted


@pytest.fixture(autouse=True)
def calls():
    """{entry point: number of calls} on the loaded library, for the test's duration."""
    lib = Counting(_native.library())
    with use_backend(lib):
        yield lib.counts


def only(calls, **want):
    assert calls == {**dict.fromkeys(COUNTED, 0), **{f"ffq_{k}": v for k, v in want.items()}}, calls


def bits_of(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same(a, b):
    """Bit-equal, or NaN in the same places."""
    return a.shape == b.shape and a.dtype == b.dtype and bool(((bits_of(a) == bits_of(b)) | (a.isnan() & b.isnan())).all())


def check_quantizer(x, fmt):
    """One launch with both containers (e2m1) against the host path on the same values."""
    want_codes, want_scales = _host.mx_quantize(x.cpu(), fmt)
    codes, packed, scales = ops.mx_quantize(x, fmt, codes=True, packed=fmt == "e2m1")
    assert codes.dtype == torch.uint8 and codes.shape == x.shape and scales.dtype == torch.uint8 and scales.shape == (*x.shape[:-1], x.shape[-1] // 32)
    assert torch.equal(scales.cpu(), want_scales), (fmt, tuple(x.shape), x.dtype)
    assert torch.equal(codes.cpu(), want_codes), (fmt, tuple(x.shape), x.dtype, (codes.cpu() != want_codes).nonzero()[:4])
    if fmt == "e2m1":
        assert packed.dtype == torch.uint8 and packed.shape == (*x.shape[:-1], x.shape[-1] // 2) and torch.equal(packed.cpu(), _host.mx_pack(want_codes))
    else:
        assert packed is None
    return codes, packed, scales


def special_blocks(dtype):
    """The named cases of tests/test_mx_cpu.py as one matrix: ties, -0.0, an all-zero block, subnormals, the largest binade, and a NaN, a
    +Inf and a -Inf block beside untouched ones."""
    x = torch.randn(8, 96, generator=torch.Generator().manual_seed(5)).to(dtype)
    x[0, :32] = 0.0
    x[0, 5] = -0.0
    ties = torch.tensor([6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 7.0, -0.25, -0.75, -5.0, -0.0, 17.0, 19.0, 448.0, 465.0, 2.0**-10])
    x[1, 32:64] = 0.0
    x[1, 32:32 + ties.numel()] = ties.to(dtype)
    x[2, 64:96] = 0.0
    x[2, 64:67] = torch.tensor([3e38, -1e38, 1.0]).to(dtype) if dtype != torch.float16 else torch.tensor([65504.0, -3e4, 1.0]).to(dtype)
    x[3, 40] = float("nan")
    x[4, 0] = float("inf")
    x[5, 95] = float("-inf")
    x[6, :32] = 0.0
    x[6, :3] = torch.tensor([2.0**-24, -(2.0**-24), 2.0**-20]).to(dtype)  # subnormals of fp16; tiny everywhere
    return x


# ---- the quantizer ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_bf16_pattern_equals_the_host_path(fmt, calls):
    check_quantizer(mx_cases.exhaustive_bf16().to(DEV), fmt)
    only(calls, mx_quantize=1)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_the_quantizer_equals_the_host_path(fmt, dtype, calls):
    launches = 0
    for rows, K in ((1, 32), (3, 96), (70, 64), (5, 4096)):
        g = torch.Generator().manual_seed(rows * K)
        x = (torch.randn(rows, K, generator=g) * torch.exp2(torch.randint(-12, 13, (rows, K // 32), generator=g).float()).repeat_interleave(32, 1)).to(dtype)
        check_quantizer(x.to(DEV), fmt)
        check_quantizer(x.to(DEV).reshape(rows, K // 32, 32), fmt)  # leading dimensions fold into rows
        launches += 2
    check_quantizer(special_blocks(dtype).to(DEV), fmt)
    only(calls, mx_quantize=launches + 1)


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_column_window_is_read_in_place(fmt, calls):
    wide = torch.randn(7, 256 + 72, generator=torch.Generator().manual_seed(9)).to(torch.bfloat16).to(DEV)
    for start in (0, 8, 64, 3):  # 16-byte aligned starts take the 16-byte loads, the last one the element form
        window = wide[:, start:start + 256]
        assert not window.is_contiguous() or start == 0
        pointer = window.data_ptr()
        codes, packed, scales = check_quantizer(window, fmt)
        assert window.data_ptr() == pointer
        dense = ops.mx_quantize(window.contiguous(), fmt)
        assert torch.equal(dense[0], codes) and torch.equal(dense[2], scales)
    only(calls, mx_quantize=8)


def test_both_containers_from_one_launch_equal_two_launches(calls):
    x = special_blocks(torch.bfloat16).to(DEV)
    both = ops.mx_quantize(x, "e2m1", codes=True, packed=True)
    only(calls, mx_quantize=1)
    codes_only = ops.mx_quantize(x, "e2m1", codes=True, packed=False)
    packed_only = ops.mx_quantize(x, "e2m1", codes=False, packed=True)
    assert codes_only[1] is None and packed_only[0] is None
    assert torch.equal(both[0], codes_only[0]) and torch.equal(both[1], packed_only[1])
    assert torch.equal(both[2], codes_only[2]) and torch.equal(both[2], packed_only[2])
    only(calls, mx_quantize=3)


# ---- dequantize -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_dequantize_equals_the_host_path(fmt, dtype, calls):
    launches = 0
    sources = [special_blocks(torch.float32), torch.randn(70, 64, generator=torch.Generator().manual_seed(1)) * 40.0,
               torch.randn(3, 4096, generator=torch.Generator().manual_seed(2)) * 1e-3]
    for x in sources:
        codes, scales = _host.mx_quantize(x, fmt)
        want = _host.mx_dequantize(codes, scales, fmt, dtype)
        got = ops.mx_dequantize(codes.to(DEV), scales.to(DEV), fmt, dtype)
        assert same(got.cpu(), want), (fmt, dtype, tuple(x.shape))
        launches += 1
        if fmt == "e2m1":
            got = ops.mx_dequantize(_host.mx_pack(codes).to(DEV), scales.to(DEV), fmt, dtype, packed=True)
            assert same(got.cpu(), want)
            launches += 1
    # every element code under the smallest, an ordinary, the largest and the NaN scale
    n = 256 if fmt == "e4m3" else 16
    every = (torch.arange(256) % n).to(torch.uint8).repeat(4, 1)
    scales = torch.tensor([0, 127, 254, 255], dtype=torch.uint8)[:, None].repeat(1, 8)
    assert same(ops.mx_dequantize(every.to(DEV), scales.to(DEV), fmt, dtype).cpu(), _host.mx_dequantize(every, scales, fmt, dtype))
    only(calls, mx_dequantize=launches + 1)


# ---- guard bands ------------------------------------------------------------------------------------------------------------------------------
def guarded(run):
    """`run()` with its outputs carved from an arena under two poisons: every guard keeps its poison, and the runs agree with each other
    and with an unguarded run on every output byte."""
    results = []
    for poison in (guards.POISON_A, guards.POISON_B):
        arena = guards.Arena(poison)
        with guards.capture(arena):
            out = [t for t in run() if t is not None]
        torch.cuda.synchronize()
        assert all(arena.find(t.data_ptr()) is not None for t in out), "the outputs were not allocated inside the arena"
        assert not arena.touched_guards(), arena.touched_guards()
        results.append([t.clone() for t in out])
    plain = [t for t in run() if t is not None]
    for a, b, c in zip(results[0], results[1], plain):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)) and torch.equal(a.view(torch.uint8), c.view(torch.uint8))


@pytest.mark.parametrize("case", ["quantize", "quantize-element-form", "dequantize", "linear-e4m3-e4m3", "linear-e4m3-e2m1", "linear-e2m1-e2m1"])
def test_guard_bands_around_every_output(case, calls):
    if case.startswith("quantize"):
        x = torch.randn(7, 96 + 8, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16).to(DEV)
        x = x[:, 1:97] if case.endswith("element-form") else x[:, :96].contiguous()
        guarded(lambda: ops.mx_quantize(x, "e2m1", codes=True, packed=True))
        guarded(lambda: ops.mx_quantize(x, "e4m3"))
        guarded(lambda: ops.mx_quantize(x.float(), "e2m1", codes=False, packed=True))
        return only(calls, mx_quantize=9)
    if case == "dequantize":
        codes, scales = (t.to(DEV) for t in _host.mx_quantize(torch.randn(7, 96, generator=torch.Generator().manual_seed(4)), "e2m1"))
        packed = _host.mx_pack(codes)
        for dtype in DTYPES:
            guarded(lambda: [ops.mx_dequantize(codes, scales, "e2m1", dtype)])
            guarded(lambda: [ops.mx_dequantize(packed, scales, "e2m1", dtype, packed=True)])
        return only(calls, mx_dequantize=18)
    a_fmt, w_fmt = case.split("-")[1:]
    c = mx_cases.exact_case(33, 129, 256, a_fmt, w_fmt)
    operands = device_operands(c, a_fmt, w_fmt)
    for dtype in DTYPES:
        guarded(lambda: [ops.linear_mx(*operands, bias=c["bias"].float().to(DEV), out_dtype=dtype)])
    only(calls, linear_mx=9)


# ---- the linear, exactly ----------------------------------------------------------------------------------------------------------------------
def gemm_codes(codes, fmt):
    return _host.mx_pack(codes) if fmt == "e2m1" else codes


def device_operands(c, a_fmt, w_fmt):
    return (gemm_codes(c["a_codes"], a_fmt).to(DEV), c["a_scales"].to(DEV), a_fmt, gemm_codes(c["w_codes"], w_fmt).to(DEV), c["w_scales"].to(DEV), w_fmt)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("pair", mx_cases.PAIRS, ids=["-".join(p) for p in mx_cases.PAIRS])
def test_the_linear_is_the_float64_product_rounded_once(pair, dtype, calls):
    """Operands of tests/mx_cases.py: asymmetric (A != W^T, scale codes differ per row and block), every partial sum exact in fp32. A
    swapped row / column, a wrong k order inside a block, a wrong nibble or a wrong scale byte cannot pass."""
    a_fmt, w_fmt = pair
    launches = 0
    for M, N, K in mx_cases.EXACT_SHAPES:
        c = mx_cases.exact_case(M, N, K, a_fmt, w_fmt)
        operands = device_operands(c, a_fmt, w_fmt)
        repeats = 2 if (M, N, K) == mx_cases.EXACT_SHAPES[-1] else 1
        for _ in range(repeats):
            out = ops.linear_mx(*operands, out_dtype=dtype)
            want = c["product"].to(torch.float32).to(dtype)  # (exact in fp32: one rounding)
            assert out.dtype == dtype and out.shape == (M, N)
            assert torch.equal(out.cpu(), want), ((M, N, K), (out.cpu() != want).nonzero()[:4], out.cpu().flatten()[:4], want.flatten()[:4])
            out = ops.linear_mx(*operands, bias=c["bias"].float().to(DEV), out_dtype=dtype)
            assert torch.equal(out.cpu(), c["with_bias"].to(torch.float32).to(dtype)), (M, N, K)
            launches += 2
        if dtype != torch.float32:  # a bias in the output's dtype: whole numbers (exact in bf16 and fp16)
            whole = c["bias"].round()
            out = ops.linear_mx(*operands, bias=whole.to(dtype).to(DEV), out_dtype=dtype)
            assert torch.equal(out.cpu(), (c["product"] + whole).to(torch.float32).to(dtype)), (M, N, K)
            launches += 1
    only(calls, linear_mx=launches)


# ---- the linear on ordinary data --------------------------------------------------------------------------------------------------------------
HALF_ULP = {torch.float32: 2.0**-24, torch.bfloat16: 2.0**-8, torch.float16: 2.0**-11}  # relative: 2^-p for p significand bits


def accumulation_bound(a64, w64, K, dtype):
    """Per output: K * 2^-23 * sum |a b| — fp32 accumulation of K terms, each step's error taken for truncation (a whole ulp) so that it
    holds whatever the instruction's internal rounding is — plus half an ulp of the output dtype at the largest value the accumulator can
    hold (fp16: at least half its subnormal step)."""
    spread = K * 2.0**-23 * (a64.abs() @ w64.abs().T)
    reference = a64 @ w64.T
    half = HALF_ULP[dtype] * (reference.abs() + spread)
    if dtype == torch.float16:
        half = half.clamp(min=2.0**-25)
    return reference, spread + half


def quantized_operands(M, N, K, a_fmt, w_fmt, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    w = (0.02 * torch.randn(N, K, generator=g)).to(torch.bfloat16).to(DEV)
    qa = ops.mx_quantize(x, a_fmt, codes=True, packed=a_fmt == "e2m1")
    qw = ops.mx_quantize(w, w_fmt, codes=True, packed=w_fmt == "e2m1")
    return qa, qw


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("pair", mx_cases.PAIRS, ids=["-".join(p) for p in mx_cases.PAIRS])
def test_the_linear_on_ordinary_data_is_inside_the_fp32_accumulation_bound(pair, dtype, calls):
    a_fmt, w_fmt = pair
    M, N, K = 70, 130, 512
    qa, qw = quantized_operands(M, N, K, a_fmt, w_fmt, 21)
    a64 = _host.mx_dequantize(qa[0].cpu(), qa[2].cpu(), a_fmt).double()
    w64 = _host.mx_dequantize(qw[0].cpu(), qw[2].cpu(), w_fmt).double()
    reference, bound = accumulation_bound(a64, w64, K, dtype)
    out = ops.linear_mx(qa[1] if a_fmt == "e2m1" else qa[0], qa[2], a_fmt, qw[1] if w_fmt == "e2m1" else qw[0], qw[2], w_fmt, out_dtype=dtype)
    error = (out.cpu().double() - reference).abs()
    print(f"{pair} {dtype}: largest error / bound = {float((error / bound).max()):.3g}")
    assert bool((error <= bound).all()), float((error / bound).max())
    only(calls, mx_quantize=2, linear_mx=1)


# ---- views and errors -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", mx_cases.PAIRS, ids=["-".join(p) for p in mx_cases.PAIRS])
def test_a_column_window_of_wider_matrices_equals_the_dense_call(pair, calls):
    a_fmt, w_fmt = pair
    qa, qw = quantized_operands(37, 70, 512, a_fmt, w_fmt, 31)
    a_codes, w_codes = (qa[1] if a_fmt == "e2m1" else qa[0]), (qw[1] if w_fmt == "e2m1" else qw[0])
    a_cols, w_cols = a_codes.shape[1] // 4, w_codes.shape[1] // 4  # the K window [128, 384)
    window = (a_codes[:, a_cols:3 * a_cols], qa[2][:, 4:12], a_fmt, w_codes[:, w_cols:3 * w_cols], qw[2][:, 4:12], w_fmt)
    assert not any(t.is_contiguous() for t in window if isinstance(t, torch.Tensor))
    dense = tuple(t.contiguous() if isinstance(t, torch.Tensor) else t for t in window)
    got, want = ops.linear_mx(*window), ops.linear_mx(*dense)
    assert got.shape == (37, 70) and torch.equal(bits_of(got), bits_of(want)) and bool(want.abs().sum() > 0)
    only(calls, mx_quantize=2, linear_mx=2)


def test_a_misaligned_operand_is_refused_before_any_launch(calls):
    c = mx_cases.exact_case(33, 129, 256, "e4m3", "e4m3")
    a, sa, _, w, sw, _ = device_operands(c, "e4m3", "e4m3")
    wide = torch.zeros(33, 256 + 16, dtype=torch.uint8, device=DEV)
    wide[:, 8:264] = a
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.linear_mx(wide[:, 8:264], sa, "e4m3", w, sw, "e4m3")  # rows 16-byte apart, the first one 8 bytes in
    wide_scales = torch.zeros(129, 12, dtype=torch.uint8, device=DEV)
    wide_scales[:, 2:10] = sw
    with pytest.raises(ValueError, match="4-byte aligned"):
        ops.linear_mx(a, sa, "e4m3", w, wide_scales[:, 2:10], "e4m3")
    with pytest.raises(ValueError, match="not covered"):
        ops.linear_mx(_host.mx_pack(a), sa, "e2m1", w, sw, "e4m3")
    only(calls, linear_mx=3)
    # no launch: the entry point itself, handed an output full of poison, returns the error and leaves every byte of it
    lib = _native.library()
    stream = torch.cuda.current_stream().cuda_stream
    for a_ptr, sw_ptr, words in ((a.data_ptr() + 8, sw.data_ptr(), "16-byte aligned"), (a.data_ptr(), sw.data_ptr() + 2, "4-byte aligned")):
        out = torch.full((33, 129), 0x7F7F7F7F, dtype=torch.int32, device=DEV)
        status = lib.ffq_linear_mx(a_ptr, 256, sa.data_ptr(), 8, 0, w.data_ptr(), 256, sw_ptr, 8, 0, None, 0, out.data_ptr(), int(ops._tag(torch.float32)), 33, 129, 256,
                                   stream)
        torch.cuda.synchronize()
        assert status == 7 and words in lib.ffq_last_error().decode() and bool((out == 0x7F7F7F7F).all())  # FFQ_ERR_ARG
    only(calls, linear_mx=5)
    assert torch.equal(ops.linear_mx(a, sa, "e4m3", w, sw, "e4m3").cpu(), c["product"].float())


@pytest.mark.parametrize("pair", mx_cases.PAIRS, ids=["-".join(p) for p in mx_cases.PAIRS])
def test_a_nan_scale_block_leaves_every_other_row_alone(pair, calls):
    a_fmt, w_fmt = pair
    g = torch.Generator().manual_seed(41)
    x = torch.randn(40, 256, generator=g).to(torch.bfloat16)
    w = (0.02 * torch.randn(50, 256, generator=g)).to(torch.bfloat16).to(DEV)
    dirty = x.clone()
    dirty[3, 100] = float("nan")
    dirty[35, 0] = float("inf")
    qw = ops.mx_quantize(w, w_fmt, codes=False, packed=True) if w_fmt == "e2m1" else ops.mx_quantize(w, w_fmt)
    outs = []
    for data in (x, dirty):
        qa = ops.mx_quantize(data.to(DEV), a_fmt, codes=a_fmt == "e4m3", packed=a_fmt == "e2m1")
        outs.append(ops.linear_mx(qa[1] if a_fmt == "e2m1" else qa[0], qa[2], a_fmt, qw[1] if w_fmt == "e2m1" else qw[0], qw[2], w_fmt))
        if data is dirty:
            assert int(qa[2][3, 3]) == 255 and int(qa[2][35, 0]) == 255 and int((qa[2] == 255).sum()) == 2
    clean, got = outs
    keep = [r for r in range(40) if r not in (3, 35)]
    assert torch.equal(bits_of(got[keep]), bits_of(clean[keep])) and not got[keep].isnan().any()
    assert bool(got[[3, 35]].isnan().all())  # every output that reads a block whose scale byte is 255 is NaN (include_mx/ffq_mx.h)
    print(f"{pair}: the rows that read a scale byte of 255: NaN outputs {int(got[[3, 35]].isnan().sum())} of {2 * 50}; samples {got[3, :3].tolist()}")
    only(calls, mx_quantize=3, linear_mx=2)


# ---- the module -------------------------------------------------------------------------------------------------------------------------------
def mx_layer(fmt_in, fmt_w, K=256, N=200, out=None, dtype=torch.bfloat16):
    torch.manual_seed(4)
    layer = ff.nn.QuantizedLinear(K, N)
    layer.input_quantizer = ff.nn.MXQuantizer(fmt_in)
    layer.weight_quantizer = ff.nn.MXQuantizer(fmt_w)
    if out is not None:
        layer.output_quantizer = out
    return layer.to(DEV).to(dtype)


@pytest.mark.parametrize("pair", [("e4m3", "e2m1"), ("e2m1", "e2m1")], ids=["e4m3-e2m1", "e2m1-e2m1"])
def test_a_quantized_linear_with_mx_quantizers_is_two_quantize_launches_and_one_gemm(pair, calls):
    fmt_in, fmt_w = pair
    layer = mx_layer(fmt_in, fmt_w)
    x = torch.randn(3, 11, 256, generator=torch.Generator().manual_seed(8)).to(torch.bfloat16).to(DEV)
    with torch.no_grad(), ff.strict_quantization(False):
        out = layer(x)
        only(calls, mx_quantize=2, linear_mx=1)
        qx, qw = layer.input_quantizer(x), layer.weight_quantizer(layer.weight)
        assert fused_mx.fused_linear_mx_predicate(input=qx, weight=qw, bias=layer.bias)
        px, pw = qx.quantization_context.quantization_params, qw.quantization_context.quantization_params
        assert qx.raw_data.dtype == torch.uint8 and qx.shape == x.shape and (px.packed is not None) == (fmt_in == "e2m1") and pw.packed is not None
        direct = ops.linear_mx((px.packed if fmt_in == "e2m1" else qx.raw_data).reshape(33, -1), px.scale.reshape(33, 8), fmt_in, pw.packed, pw.scale, fmt_w,
                               bias=layer.bias, out_dtype=torch.bfloat16)
        assert out.dtype == torch.bfloat16 and out.shape == (3, 11, 200) and torch.equal(bits_of(out.reshape(33, 200)), bits_of(direct))
        only(calls, mx_quantize=4, linear_mx=2)
        # inside the accumulation bound of the float chain's value (the bias, a bf16 number, is added in fp32 on both sides)
        a64 = _host.mx_dequantize(qx.raw_data.cpu(), px.scale.cpu(), fmt_in).double().reshape(33, 256)
        w64 = _host.mx_dequantize(qw.raw_data.cpu(), pw.scale.cpu(), fmt_w).double()
        reference, bound = accumulation_bound(a64, w64, 256, torch.bfloat16)
        bias64 = layer.bias.cpu().double()
        bound = bound + HALF_ULP[torch.bfloat16] * bias64.abs() + 2.0**-24 * (reference.abs() + bias64.abs())  # (the fp32 bias add, then the wider value's half ulp)
        assert bool(((out.reshape(33, 200).cpu().double() - (reference + bias64)).abs() <= bound).all())
        chain = torch.nn.functional.linear(qx.dequantize(), qw.dequantize(), layer.bias)
        assert chain.dtype == torch.bfloat16 and chain.shape == out.shape
        only(calls, mx_quantize=4, mx_dequantize=2, linear_mx=2)


def test_an_output_quantizer_runs_on_the_result_by_its_own_call(calls):
    out_q = ff.nn.LinearQuantizer(8)
    layer = mx_layer("e4m3", "e2m1", out=out_q)
    out_q.quantization_range = (-4.0, 4.0)
    layer = layer.to(DEV)
    x = torch.randn(33, 256, generator=torch.Generator().manual_seed(8)).to(torch.bfloat16).to(DEV)
    with torch.no_grad(), ff.strict_quantization(False):
        out = layer(x)
        only(calls, mx_quantize=2, linear_mx=1)
        layer.output_quantizer = ff.nn.QuantizerStub()
        unfused = layer(x)
        want = out_q(unfused)
    assert isinstance(out, ff.QuantizedTensor) and not isinstance(unfused, ff.QuantizedTensor)
    assert torch.equal(out.raw_data, want.raw_data) and torch.equal(bits_of(out.dequantize()), bits_of(want.dequantize()))
    only(calls, mx_quantize=4, linear_mx=2)


def test_an_uncovered_contraction_takes_the_float_chain(calls):
    layer = mx_layer("e4m3", "e2m1", K=96, N=40)
    x = torch.randn(9, 96, generator=torch.Generator().manual_seed(8)).to(torch.bfloat16).to(DEV)
    with torch.no_grad(), ff.strict_quantization(False):
        out = layer(x)
        only(calls, mx_quantize=2, mx_dequantize=2)
        qx, qw = layer.input_quantizer(x), layer.weight_quantizer(layer.weight)
        assert not fused_mx.fused_linear_mx_predicate(input=qx, weight=qw, bias=layer.bias)
        want = torch.nn.functional.linear(qx.dequantize(), qw.dequantize(), layer.bias)
    assert torch.equal(bits_of(out), bits_of(want))
    assert calls["ffq_linear_mx"] == 0 and calls["ffq_linear_w8a8"] == 0 and calls["ffq_linear_wq"] == 0


def test_the_layer_is_captured_in_a_graph_and_replayed(calls):
    layer = mx_layer("e4m3", "e2m1")
    x = torch.randn(33, 256, generator=torch.Generator().manual_seed(8)).to(torch.bfloat16).to(DEV)
    static = x.clone()
    with torch.no_grad(), ff.strict_quantization(False):
        eager = layer(x)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            layer(static)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = layer(static)
        only(calls, mx_quantize=6, linear_mx=3)
        for scale in (1.0, 0.5):
            static.copy_(x * scale)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(bits_of(captured), bits_of(layer(x * scale)))
        assert torch.equal(bits_of(layer(x)), bits_of(eager))
    only(calls, mx_quantize=12, linear_mx=6)  # the replays call no entry point


def test_an_e2m1_tensor_without_its_packed_image_is_declined(calls):
    """Quantized on the host and moved to the device: the codes and scales are there, the packed image of a device launch is not. The
    predicate declines (no packing pass behind the caller's back) and the float chain's bits come back."""
    x = torch.randn(9, 256, generator=torch.Generator().manual_seed(8)).to(torch.bfloat16)
    w = (0.02 * torch.randn(40, 256, generator=torch.Generator().manual_seed(9))).to(torch.bfloat16)
    q = ff.nn.MXQuantizer("e2m1")
    with torch.no_grad(), ff.strict_quantization(False):
        qx, qw = q(x).to(DEV), q(w).to(DEV)
        assert qx.quantization_context.quantization_params.packed is None and qx.is_cuda
        assert not fused_mx.fused_linear_mx_predicate(input=qx, weight=qw)
        assert not fused_mx.fused_linear_mx_predicate(input=q(x.to(DEV)), weight=qw) and fused_mx.fused_linear_mx_predicate(input=q(x.to(DEV)), weight=q(w.to(DEV)))
        out = F.linear(qx, qw, strict_quantization=False)
        assert torch.equal(bits_of(out), bits_of(torch.nn.functional.linear(qx.dequantize(), qw.dequantize())))
    assert calls["ffq_linear_mx"] == 0 and calls["ffq_mx_dequantize"] == 4 and calls["ffq_mx_quantize"] == 3
