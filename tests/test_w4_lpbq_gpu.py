"""LPBQ weights on the MI355X (csrc/ffq_lpbq.hip).

Everything here is integer-exact or a bit pattern: the compression against the host path and the reference's recorded outputs (G32),
the fused quantizer against the composition ``ops.quantize_by_tile`` -> ``* int_scale``, the expansion against ``unpack_int4 * int_scale``,
and the linear on weights built so that the int8 GEMM's result is the float64 product of the dequantized operands.

Every test runs with a counting proxy as the loaded library: the calls of the three new entry points and of ``ffq_linear_w8a8`` /
``ffq_linear_wq`` are counted, so a silent fallback fails it."""

import pytest
import torch

import fastforward_amd as ff
import guards

from conftest import golden, use_backend
from fastforward_amd import _native, ops
from fastforward_amd.nn import functional as F
from fastforward_amd.quantization import lpbq

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DTYPE_IDS = ["bf16", "fp16", "fp32"]
COUNTED = ("ffq_lpbq_compress_scales", "ffq_lpbq_quantize", "ffq_lpbq_expand", "ffq_linear_w8a8", "ffq_linear_wq")
SHAPES = [(1, 16, 16), (3, 80, 16), (2, 64, 32), (130, 256, 128), (5, 8320, 128), (4, 14336, 128)]  # (N, K, G)
G32 = golden("g32_lpbq.pt")


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


def scales_of(N, J, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(N, J, generator=g) * 0.1 + 1e-3


# ---- compression --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [2, 3, 4])
def test_compression_equals_the_host_path(bits, calls):
    for N, J in ((1, 1), (1, 2), (3, 5), (2, 64), (2, 65), (5, 112), (1, 1024)):
        s = scales_of(N, J, 100 * N + J)
        want_q, want_d = lpbq.compress_scales_host(s, 1, bits)
        q, d = ops.lpbq_compress_scales(s.to(DEV), bits)
        assert q.dtype == torch.uint8 and q.shape == (N, J) and d.dtype == torch.float32 and d.shape == (N,)
        assert torch.equal(q.cpu(), want_q) and torch.equal(bits_of(d.cpu()), bits_of(want_d)), (N, J)
        # a strided view of a wider scale matrix is read in place
        wide = torch.full((N, J + 7), 9.0, device=DEV)
        wide[:, 3:3 + J] = s.to(DEV)
        q2, d2 = ops.lpbq_compress_scales(wide[:, 3:3 + J], bits)
        assert torch.equal(q2, q) and torch.equal(bits_of(d2), bits_of(d))
    only(calls, lpbq_compress_scales=14)


def test_compression_equals_the_reference_on_g32(calls):
    """The recorded ``grouped_dynamic_quantize`` outputs for fp32 scales with blocks along dim 1: ties to even both ways, entries clamped
    to 1, constant rows."""
    records = [r for r in G32["compress"] if r["orientation"] == "rows" and r["dtype"] == "float32"]
    assert len(records) == 18
    for r in records:
        q, d = ops.lpbq_compress_scales(r["scales"].to(DEV), r["bits"])
        assert torch.equal(q.cpu(), r["q"]) and torch.equal(bits_of(d.cpu()), bits_of(r["d"])), (r["J"], r["bits"])
        q, d = lpbq.compress_scales(r["scales"].to(DEV), 1, r["bits"])   # the public route takes the kernel for these
        assert torch.equal(q.cpu(), r["q"]) and torch.equal(bits_of(d.cpu()), bits_of(r["d"]))
    only(calls, lpbq_compress_scales=36)
    # the other orientation and bf16 scales take the host path on the device tensors: the same recorded bits
    for r in [r for r in G32["compress"] if r["J"] == 65 and (r["orientation"] == "columns" or r["dtype"] == "bfloat16")]:
        q, d = lpbq.compress_scales(r["scales"].to(DEV), 1 if r["orientation"] == "rows" else 0, r["bits"])
        assert torch.equal(q.cpu(), r["q"]) and torch.equal(bits_of(d.cpu()), bits_of(r["d"]))
    only(calls, lpbq_compress_scales=36)


@pytest.mark.parametrize("bits", [2, 4])
def test_a_nan_row_and_a_zero_row_leave_the_others_alone(bits, calls):
    s = scales_of(6, 37, 3)
    clean_q, clean_d = ops.lpbq_compress_scales(s.to(DEV), bits)
    dirty = s.clone()
    dirty[1, 5] = float("nan")
    dirty[3] = 0.0
    dirty[4, 0] = float("inf")
    q, d = ops.lpbq_compress_scales(dirty.to(DEV), bits)
    keep = [0, 2, 5]
    assert torch.equal(q[keep], clean_q[keep]) and torch.equal(bits_of(d[keep]), bits_of(clean_d[keep]))
    assert int(q.min()) >= 1 and int(q.max()) <= 2**bits
    only(calls, lpbq_compress_scales=2)


# ---- the fused quantizer ----------------------------------------------------------------------------------------------------------------
def weight_and_scales(N, K, G, dtype, seed):
    """A weight with ordinary values and, in every row, exact ties ``(k + 0.5) * s`` (block 0 has a power-of-two scale, so they are exact
    in every dtype), values beyond both clamps, -0.0, NaN and both infinities; its block scales (fp32 [N, K / G])."""
    g = torch.Generator().manual_seed(seed)
    J = K // G
    s = torch.rand(N, J, generator=g) * 0.05 + 0.01
    s[:, 0] = 2.0**-5
    w = torch.randn(N, K, generator=g) * s.repeat_interleave(G, 1) * 3.0
    ties = (torch.arange(G) % 16 - 8 + 0.5) * 2.0**-5
    w[:, :G] = ties
    special = torch.tensor([100.0, -100.0, -0.0, float("nan"), float("inf"), float("-inf")])
    if K >= 2 * G:
        n = min(G, special.numel())
        w[:, G:G + n] = special[:n]
    else:
        w[:, -special.numel():] = special
    return w.to(dtype).to(DEV), s.to(DEV)


def composition(w, s, G, bits, requantize):
    """``ops.quantize_by_tile`` -> ``* q`` with the host path's q and d."""
    q, d = lpbq.compress_scales_host(s.cpu(), 1, bits)
    q, d = q.to(w.device), d.to(w.device)
    applied = d[:, None] * q.float() if requantize else s
    codes4 = ops.quantize_by_tile(w, applied.contiguous(), (1, G), bits, torch.int8)
    return (codes4.int() * q.int().repeat_interleave(G, 1)).to(torch.int8), d, q


def same_as_composition(got, want):
    codes8, d, q = got
    assert codes8.dtype == torch.int8 and codes8.is_contiguous() and torch.equal(codes8, want[0]), f"{int((codes8 != want[0]).sum())} codes differ"
    assert d.dtype == torch.float32 and torch.equal(bits_of(d), bits_of(want[1]))
    assert q is None or (q.dtype == torch.uint8 and torch.equal(q, want[2]))


@pytest.mark.parametrize("requantize", [False, True], ids=["calibrated", "requantize"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_quantize_equals_the_composition(shape, dtype, requantize, calls):
    N, K, G = shape
    w, s = weight_and_scales(N, K, G, dtype, N + K)
    want = composition(w, s, G, 4, requantize)
    same_as_composition(ops.lpbq_quantize(w, s, G, 4, requantize), want)
    same_as_composition(ops.lpbq_quantize(w, s, G, 4, requantize, want_int_scale=False), want)
    assert int(want[0].min()) >= -128 and int(want[0].max()) <= 112
    only(calls, lpbq_quantize=2)


@pytest.mark.parametrize("bits", [2, 3])
def test_quantize_at_two_and_three_bits(bits, calls):
    for shape in (SHAPES[1], SHAPES[3], SHAPES[4]):
        for requantize in (False, True):
            w, s = weight_and_scales(*shape, torch.bfloat16, bits)
            want = composition(w, s, shape[2], bits, requantize)
            same_as_composition(ops.lpbq_quantize(w, s, shape[2], bits, requantize), want)
            assert int(want[0].min()) >= -(2 ** (2 * bits - 1)) and int(want[0].max()) <= 2 ** (2 * bits - 1) - 2**bits
    only(calls, lpbq_quantize=6)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_quantize_reads_column_windows_in_place_and_takes_any_group(dtype, calls):
    """A column window of a wider matrix: row stride != K. Starting at a multiple of 16 bytes it is the group form; starting at an
    element offset that breaks the alignment it is the element form, and so is a group size 8 does not divide."""
    launches = 0
    for N, K, G in ((3, 256, 32), (2, 4096, 128)):
        w, s = weight_and_scales(N, K, G, dtype, K)
        wide_s = torch.full((N, K // G + 5), 7.0, device=DEV)
        wide_s[:, 2:2 + K // G] = s
        for start in (8, 3):
            wide = torch.full((N, K + 40), 55.0, device=DEV, dtype=dtype)
            wide[:, start:start + K] = w
            window = wide[:, start:start + K]
            assert window.stride(0) == K + 40 and (window.data_ptr() % 16 == 0) == (start == 8)
            for requantize in (False, True):
                same_as_composition(ops.lpbq_quantize(window, wide_s[:, 2:2 + K // G], G, 4, requantize), composition(w, s, G, 4, requantize))
                launches += 1
    for N, K, G in ((3, 96, 24), (2, 2400, 24), (2, 70, 1)):
        w, s = weight_and_scales(N, K, G, dtype, K)
        for requantize in (False, True):
            same_as_composition(ops.lpbq_quantize(w, s, G, 4, requantize), composition(w, s, G, 4, requantize))
            launches += 1
    only(calls, lpbq_quantize=launches)


# ---- expand ---------------------------------------------------------------------------------------------------------------------------------
def codes_and_int_scale(N, K, G, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 8, (N, K), generator=g, dtype=torch.int8).to(DEV), torch.randint(1, 17, (N, K // G), generator=g).to(torch.uint8).to(DEV)


@pytest.mark.parametrize("shape", SHAPES + [(3, 96, 24), (2, 70, 1)], ids=lambda s: "x".join(map(str, s)))
def test_expand_equals_unpack_times_int_scale(shape, calls):
    N, K, G = shape
    codes4, q = codes_and_int_scale(N, K, G, K)
    want = (codes4.int() * q.int().repeat_interleave(G, 1)).to(torch.int8)
    assert torch.equal(ops.lpbq_expand(codes4, q, G), want)
    launches = 1
    for block in (32, 16, 2):
        if (N * K) % block:
            continue
        packed = ops.pack_int4(codes4, block)
        assert torch.equal(ops.unpack_int4(packed, (N, K), torch.int8, block), codes4)
        assert torch.equal(ops.lpbq_expand(packed, q, G, shape=(N, K), block=block), want), block
        launches += 1
    assert launches >= 2
    # dense buffers at an address that is not 8-byte aligned: the element form
    shifted = torch.empty(N * K + 1, dtype=torch.int8, device=DEV)[1:].view(N, K).copy_(codes4)
    assert shifted.data_ptr() % 8 and torch.equal(ops.lpbq_expand(shifted, q, G), want)
    only(calls, lpbq_expand=launches + 1)


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


@pytest.mark.parametrize("case", ["compress", "quantize-group-wave", "quantize-group-workgroup", "quantize-element-wave", "quantize-element-workgroup",
                                  "quantize-misaligned", "expand-group", "expand-element", "expand-nibbles-group", "expand-nibbles-element"])
def test_guard_bands_around_every_output(case, calls):
    if case == "compress":
        s = scales_of(7, 37, 1).to(DEV)
        guarded(lambda: ops.lpbq_compress_scales(s, 3))
        return only(calls, lpbq_compress_scales=3)
    if case.startswith("quantize"):
        N, K, G = {"group-wave": (7, 136, 8), "group-workgroup": (3, 8208, 16), "element-wave": (7, 130, 10), "element-workgroup": (3, 8200, 25),
                   "misaligned": (5, 264, 8)}[case.removeprefix("quantize-")]
        w, s = weight_and_scales(N, K, G, torch.bfloat16, K)
        if case == "quantize-misaligned":
            wide = torch.zeros(N, K + 9, device=DEV, dtype=torch.bfloat16)
            wide[:, 1:1 + K] = w
            w = wide[:, 1:1 + K]
        guarded(lambda: ops.lpbq_quantize(w, s, G, 4, True))
        guarded(lambda: ops.lpbq_quantize(w, s, G, 4, False, want_int_scale=False))
        return only(calls, lpbq_quantize=6)
    N, K, G = (5, 136, 8) if case.endswith("group") else (5, 130, 10)
    codes4, q = codes_and_int_scale(N, K, G, 9)
    if "nibbles" in case:
        block = 16 if case.endswith("group") else 10
        packed = ops.pack_int4(codes4[:, :128].contiguous() if case.endswith("group") else codes4, block)
        shape = (N, 128) if case.endswith("group") else (N, K)
        guarded(lambda: [ops.lpbq_expand(packed, q[:, :shape[1] // G].contiguous(), G, shape=shape, block=block)])
    else:
        guarded(lambda: [ops.lpbq_expand(codes4, q, G)])
    only(calls, lpbq_expand=3)


# ---- the linear, exact by construction ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N", [64, 200])
@pytest.mark.parametrize("tokens", [1, 17, 300])
def test_the_linear_on_an_lpbq_weight_is_the_exact_product(tokens, N, dtype, calls):
    """x = int8 codes * 2^-3; w = c4 * q * d[n] with d[n] powers of two and q over 1 .. 16 (16 in every row), block scales q * d, which
    the compression returns exactly. Every accumulator stays below 2^24, so the int8 GEMM's fp32 result is the float64 product of the
    dequantized operands, and in bf16 that product rounded once."""
    K, G = 512, 32
    assert K * 127 * 128 < 2**24
    g = torch.Generator().manual_seed(tokens + N)
    x_codes = torch.randint(-127, 128, (tokens, K), generator=g)
    c4 = torch.randint(-8, 8, (N, K), generator=g)
    q = torch.randint(1, 17, (N, K // G), generator=g)
    q[:, 3] = 16
    d = 2.0 ** -(torch.arange(N) % 5 + 4).double()
    w = c4.double() * q.double().repeat_interleave(G, 1) * d[:, None]
    x = x_codes.double() * 2.0**-3
    assert torch.equal(w.to(dtype).double(), w) and torch.equal(x.to(dtype).double(), x)
    quantizer = ff.nn.LPBQLinearQuantizer(4, G, device=DEV)
    quantizer.quantization_range = (-torch.ones(N * K // G, device=DEV), torch.ones(N * K // G, device=DEV))
    with torch.no_grad():
        quantizer.scale.copy_((q.double() * d[:, None]).float().flatten())
        qw = quantizer(w.to(dtype).to(DEV))
        qx = ff.quantization.affine.quantize_per_tensor(x.to(dtype).to(DEV), torch.tensor([2.0**-3], device=DEV), None, 8, output_dtype=torch.int8)
        assert torch.equal(qw.raw_data.cpu().long(), c4 * q.repeat_interleave(G, 1)) and torch.equal(qx.raw_data.cpu().long(), x_codes)
        assert torch.equal(qw.quantization_context.quantization_params.scale.cpu().double(), d)
        only(calls, lpbq_quantize=1)
        with ff.strict_quantization(False):
            out = F.linear(qx, qw)
    want = (x @ w.t()).to(dtype)
    assert type(out) is torch.Tensor and out.dtype == dtype and out.shape == (tokens, N)
    assert torch.equal(out.cpu(), want)
    if dtype == torch.float32:
        assert torch.equal(out.cpu().double(), x @ w.t())
    only(calls, lpbq_quantize=1, linear_w8a8=1)


# ---- the module ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [32, 64])
def test_a_converted_quantized_linear_takes_the_int8_gemm_and_replays(G, calls):
    """Before the conversion the layer takes whatever route the unconverted weight has: ``ffq_linear_wq`` once where the weight-only
    GEMM covers the group size (``ffq_linear_wq_supported``: a multiple of 64 input channels, so G = 64), the reference's float chain
    where it does not (G = 32: no GEMM of this library at all). After it, both take the fused quantizer and the int8 GEMM."""
    torch.manual_seed(21)
    dtype = torch.bfloat16
    layer = torch.nn.Sequential(torch.nn.Linear(512, 256)).to(DEV).to(dtype)
    ff.quantize_model(layer)
    lin = layer[0]
    LQ = ff.nn.LinearQuantizer
    lin.input_quantizer = LQ(8, symmetric=False, quantized_dtype=torch.int8, device=DEV)
    lin.input_quantizer.quantization_range = (torch.tensor(-4.0, device=DEV), torch.tensor(4.0, device=DEV))
    lin.weight_quantizer = LQ(4, symmetric=True, allow_one_sided=False, granularity=ff.PerBlock(1, G, 0), quantized_dtype=torch.int8, device=DEV)
    blocks = lin.weight.detach().float().reshape(256, 512 // G, G)
    lin.weight_quantizer.quantization_range = (blocks.amin(-1).reshape(-1), blocks.amax(-1).reshape(-1))
    lin.output_quantizer = LQ(8, symmetric=False, quantized_dtype=torch.int8, device=DEV)
    lin.output_quantizer.quantization_range = (torch.tensor(-3.0, device=DEV), torch.tensor(3.0, device=DEV))
    x = torch.randn(4, 32, 512, device=DEV).to(dtype)
    with torch.no_grad(), ff.strict_quantization(False):
        before = lin(x)
        covered = bool(_native.library().ffq_linear_wq_supported(ops._tag(dtype), ops._tag(torch.int8), ops._tag(dtype), 128, 256, 512, G, 0))
        assert covered == (G % 64 == 0)
        only(calls, linear_wq=int(covered))
        old = lin.weight_quantizer
        assert lpbq.convert_model(layer) == ["0.weight_quantizer"] and lin.weight_quantizer.scale is old.scale
        for key in calls:
            calls[key] = 0
        after = lin(x)
        only(calls, lpbq_quantize=1, linear_w8a8=1)
        # ... which is F.linear on decompress(the 4-bit tensor), the output quantizer fused in the epilogue as for any W8A8 layer
        decompressed = lpbq.decompress(old(lin.weight))
        assert torch.equal(decompressed.raw_data, lin.weight_quantizer(lin.weight).raw_data)
        want = F.linear(lin.input_quantizer(x), decompressed, lin.bias, output_quantizer=lin.output_quantizer)
    assert isinstance(after, ff.QuantizedTensor) and isinstance(before, ff.QuantizedTensor) and after.raw_data.dtype == torch.int8
    assert torch.equal(after.raw_data, want.raw_data) and torch.equal(bits_of(after.dequantize()), bits_of(want.dequantize()))
    # the two routes quantize the same weight against scales that differ by the compression: the outputs are close, not equal
    assert float((after.dequantize().detach().float() - before.dequantize().detach().float()).abs().max()) < 0.5
    # captured and replayed with new inputs: bit-equal to eager
    static_x = x.clone()
    with torch.no_grad(), ff.strict_quantization(False):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            lin(static_x)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = lin(static_x)
        for seed in (1, 2):
            fresh = torch.randn(4, 32, 512, device=DEV, generator=torch.Generator(DEV).manual_seed(seed)).to(dtype)
            static_x.copy_(fresh)
            graph.replay()
            torch.cuda.synchronize()
            eager = lin(fresh)
            assert torch.equal(captured.raw_data, eager.raw_data) and bool(eager.raw_data.any())
    assert calls["ffq_linear_wq"] == 0
