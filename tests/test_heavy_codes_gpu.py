"""The int8 contractions where accumulators exceed 2^24 (tests/heavy_codes.py): every output bit of every entry point that shares
the fp32 epilogue of include/ffq.h against the restated chain — float64 accumulator, one IEEE fp32 operation per torch op, in the
order of the tail kernel of csrc/ffq_linear.hip. The uniform-code tests elsewhere keep every term an integer below 2^24, where any
order, any FMA contraction and any int -> float conversion give the same bits; here they do not (tests/test_heavy_codes_cpu.py
proves that of the inputs). Also the int32 headroom of the accumulator at K = 131056 and K = 131072."""

import contextlib
import functools

import pytest
import torch

import fastforward_amd as ff
import heavy_codes as hc

from fastforward_amd import _native, dispatcher, ops
from parity_cases import linear_tolerances

pytestmark = pytest.mark.gpu
DEV = "cuda"
REAL = (torch.float32, torch.bfloat16, torch.float16)


@pytest.fixture(autouse=True)
def _backend(hip_backend):
    with torch.no_grad():
        yield


@functools.lru_cache(maxsize=4)
def _case(pattern, m, n, k, seed=1):
    """(xq, wq, exact accumulator) — computed once, shared, never written."""
    xq, wq = hc.codes(pattern, m, n, k, DEV, seed)
    return xq, wq, hc.accumulator64(xq, wq)


def _same(got, want, tag):
    assert got.dtype == want.dtype and got.shape == want.shape, tag
    differ = int((got != want).sum())
    assert differ == 0, f"{tag}: {differ} of {want.numel()} outputs differ from the restated epilogue"


def _dtypes(want32):
    return REAL if float(want32.abs().max()) < 6.0e4 else REAL[:2]  # fp16 where |y| fits


def _bias(n):
    return (torch.arange(n, device=DEV, dtype=torch.float32) % 13 - 6.0).mul(0.37).to(torch.bfloat16)


# ---- the tail kernel -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", hc.PATTERNS)
@pytest.mark.parametrize("m,n,k", [(64, 64, 4096), (65, 72, 4112), (1, 8, 4096), (300, 130, 4096)], ids=str)
def test_tail_kernel(pattern, m, n, k):
    xq, wq, acc = _case(pattern, m, n, k)
    if pattern in ("low", "mirror") and (m, n, k) == (64, 64, 4096):
        assert float(acc.abs().min()) >= 2**24
    sums = wq.sum(1, dtype=torch.int32)
    for per_token in (False, True):
        for ow_kind in ("none", "zero", "real"):
            sx, ox, sw, ow = hc.parameters(pattern, m, n, DEV, per_token=per_token, ow_kind=ow_kind)
            for bias in (None, _bias(n)):
                want32 = hc.restated_linear(acc, xq, wq, sx, ox, sw, ow, bias)
                for dtype in _dtypes(want32):
                    for rowsum in (None, sums):
                        got = ops.linear_w8a8(xq, wq, sx, ox, sw, ow, bias=bias, out_dtype=dtype, w_rowsum=rowsum)
                        _same(got, want32.to(dtype), f"{pattern} {m}x{n}x{k} per_token={per_token} ow={ow_kind} bias={bias is not None} {dtype} rowsum={rowsum is not None}")


# ---- the persistent kernels: 2048 x 2048 is the 64-tile threshold ---------------------------------------------------------------------
P = 2048


@pytest.mark.parametrize("pattern", hc.PATTERNS)
@pytest.mark.parametrize("k", [4096, 4160])  # 4160 = 64 (mod 128): the launcher sends it to the tail kernel at this size
def test_persistent_plain(pattern, k):
    xq, wq, acc = _case(pattern, P, P, k)
    lib = _native.library()
    assert lib.ffq_linear_w8a8_takes_earlier(P, P, k) == (1 if k == 4096 else 0)
    sums = wq.sum(1, dtype=torch.int32)
    for per_token, ow_kind, with_bias in ((False, "none", False), (False, "real", True), (True, "real", False), (False, "zero", False), (True, "none", True)):
        sx, ox, sw, ow = hc.parameters(pattern, P, P, DEV, per_token=per_token, ow_kind=ow_kind)
        bias = _bias(P) if with_bias else None
        want32 = hc.restated_linear(acc, xq, wq, sx, ox, sw, ow, bias)
        for dtype in _dtypes(want32):
            tag = f"{pattern} K={k} per_token={per_token} ow={ow_kind} bias={with_bias} {dtype}"
            _same(ops.linear_w8a8(xq, wq, sx, ox, sw, ow, bias=bias, out_dtype=dtype), want32.to(dtype), tag)
            _same(ops.linear_w8a8(xq, wq, sx, ox, sw, ow, bias=bias, out_dtype=dtype, w_rowsum=sums), want32.to(dtype), tag + " rowsum")
        previous = lib.ffq_force_generic_kernels(1)  # the library's other-form switch: the int8 GEMM must not depend on it
        try:
            _same(ops.linear_w8a8(xq, wq, sx, ox, sw, ow, bias=bias, out_dtype=torch.float32), want32, f"{pattern} K={k} forced generic")
        finally:
            lib.ffq_force_generic_kernels(previous)


@pytest.mark.parametrize("pattern", ["low", "mirror", "ties"])
def test_persistent_multi_and_earlier(pattern):
    k = 4096
    xq, wq, acc = _case(pattern, P, P, k)
    sums = wq.sum(1, dtype=torch.int32)
    for per_token in (False, True):
        sx, ox, sw, _ = hc.parameters(pattern, P, P, DEV, per_token=per_token, ow_kind="none")
        want32 = hc.restated_linear(acc, xq, wq, sx, ox, sw, None)
        rows = (1024, 512, 512)
        for dtype in (torch.float32, torch.bfloat16):
            for rowsum in (None, sums):
                got = ops.linear_w8a8_multi(xq, wq, sx, ox, sw, rows, out_dtype=dtype, w_rowsum=rowsum)
                assert got is not None
                at = 0
                for out, r in zip(got, rows):
                    _same(out, want32[:, at:at + r].to(dtype), f"multi {pattern} rows {at}:{at + r} {dtype} per_token={per_token}")
                    at += r
    # codes of an earlier quantizer of the same tensor: read where the parameter pairs agree, `x_codes` where they do not
    junk = torch.zeros_like(xq)
    for ow_kind in ("none", "real"):
        sx, ox, sw, ow = hc.parameters(pattern, P, P, DEV, ow_kind=ow_kind)
        want32 = hc.restated_linear(acc, xq, wq, sx, ox, sw, ow)
        other = None if ox is None else ox + 1.0
        for dtype in (torch.float32, torch.bfloat16):
            same = ops.linear_w8a8_earlier(junk, (xq, sx.clone(), None if ox is None else ox.clone()), wq, sx, ox, sw, ow, out_dtype=dtype)
            _same(same, want32.to(dtype), f"earlier (equal parameters) {pattern} ow={ow_kind} {dtype}")
            differs = ops.linear_w8a8_earlier(xq, (junk, sx * 2, other), wq, sx, ox, sw, ow, out_dtype=dtype)
            _same(differs, want32.to(dtype), f"earlier (other parameters) {pattern} ow={ow_kind} {dtype}")


def _product(gate32, up32):
    return hc.restated_gated(gate32.to(torch.bfloat16), up32)


def _pair_of(product):
    return torch.stack([product.float().min(), product.float().max()])


@pytest.mark.parametrize("pattern", ["low", "mirror"])
def test_persistent_gated_estimating_and_gate_up(pattern):
    k = 4096
    xq, wg, acc_g = _case(pattern, P, P, k)
    _, wu = hc.codes(pattern, 8, P, k, DEV, seed=2)
    acc_u = hc.accumulator64(xq, wu)
    g = torch.Generator(device=DEV).manual_seed(3)
    gate = (torch.randn(P, P, device=DEV, generator=g) * 3).to(torch.bfloat16)
    initial = [-1, 0, 0, 0]
    for ow_kind in ("none", "zero", "real"):
        sx, ox, sw, ow = hc.parameters(pattern, P, P, DEV, ow_kind=ow_kind)
        up32 = hc.restated_linear(acc_u, xq, wu, sx, ox, sw, ow)
        want = hc.restated_gated(gate, up32)
        got, pair = ops.linear_w8a8_gated(xq, wu, sx, ox, sw, ow, gate, want_extrema=True)
        _same(got, want, f"gated {pattern} ow={ow_kind}")
        assert torch.equal(pair.float(), _pair_of(want)), (pair, _pair_of(want))
        _same(ops.linear_w8a8_gated(xq, wu, sx, ox, sw, ow, gate), want, f"gated {pattern} ow={ow_kind} (no extrema)")
    # gate + up while estimating: the one-launch route (equal parameters, no live weight offset) and the two-launch route
    sx, ox, sw, ow = hc.parameters(pattern, P, P, DEV, ow_kind="real")
    su = sw.flip(0).contiguous()
    routes = {
        "one_launch": ((sx, ox), (sx.clone(), ox.clone()), (sw, None), (su, None)),
        "zero_weight_offsets": ((sx, ox), (sx.clone(), ox.clone()), (sw, torch.zeros_like(sw)), (su, torch.zeros_like(su) + 0.25)),
        "different_offset": ((sx, ox), (sx.clone(), ox - 1.0), (sw, None), (su, None)),
        "weight_offsets": ((sx, ox), (sx.clone(), ox.clone()), (sw, ow), (su, ow.flip(0).contiguous())),
    }
    for name, (pg, pu, qg, qu) in routes.items():
        gate32 = hc.restated_linear(acc_g, xq, wg, pg[0], pg[1], qg[0], qg[1])
        up32 = hc.restated_linear(acc_u, xq, wu, pu[0], pu[1], qu[0], qu[1])
        want = _product(gate32, up32)
        got, pair = ops.mlp_gate_up_w8a8_estimating(xq, xq, wg, wu, pg, pu, qg, qu, want_extrema=True)
        _same(got, want, f"estimating {pattern} {name}")
        assert torch.equal(pair.float(), _pair_of(want)), name
        _same(ops.mlp_gate_up_w8a8_estimating(xq, xq, wg, wu, pg, pu, qg, qu), want, f"estimating {pattern} {name} (no extrema)")
    for words in ops._EXTREMA_WORDS.values():
        assert words.tolist() == initial
    # gate + up + SiLU * up + the down_proj input quantizer in one launch
    gate32 = hc.restated_linear(acc_g, xq, wg, sx, ox, sw, None)
    up32 = hc.restated_linear(acc_u, xq, wu, sx, ox, su, None)
    z = _product(gate32, up32)
    so, oo = torch.tensor([float(z.float().std()) / 40], device=DEV), torch.tensor([-11.0], device=DEV)
    for rowsums in ((None, None), (wg.sum(1, dtype=torch.int32), wu.sum(1, dtype=torch.int32))):
        codes = ops.mlp_gate_up_w8a8(xq, wg, wu, sx, ox, sw, su, so, oo, 8, gate_rowsum=rowsums[0], up_rowsum=rowsums[1])
        assert codes is not None
        _same(codes, ops.quantize_by_tile(z, so, z.shape, 8, torch.int8, oo), f"gate/up launch {pattern}")


# ---- the requantizing epilogue ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,k", [(300, 200, 4096), (P, P, 4096)], ids=str)
def test_requantizing_epilogue(m, n, k):
    xq, wq, acc = _case("low", m, n, k)
    for ow_kind in ("none", "real"):
        sx, ox, sw, ow = hc.parameters("low", m, n, DEV, ow_kind=ow_kind)
        y32 = hc.restated_linear(acc, xq, wq, sx, ox, sw, ow)
        spread = float(y32.std())
        for y_dt in (torch.bfloat16, torch.float32):
            for container in (torch.int8, torch.bfloat16):
                for so, oo in ((spread / 40, torch.tensor([-17.6], device=DEV)), (spread / 25, None)):
                    so = torch.tensor([so], device=DEV)
                    want = hc.restated_requant(y32, y_dt, so, oo, 8, container, ops.quantize_by_tile)
                    got = ops.linear_w8a8(xq, wq, sx, ox, sw, ow, out_dtype=container, out_scale=so, out_offset=oo, out_num_bits=8, requant_from=y_dt)
                    _same(got, want, f"requant {m}x{n} ow={ow_kind} y_dt={y_dt} {container}")
                    assert int(want.float().max() - want.float().min()) >= 7  # a real grid, not a saturated tensor


# ---- QuantizedTensors from codes: the dispatcher's routes -----------------------------------------------------------------------------
def _quantized(codes, scale, offset, dtype, axis=None):
    """A QuantizedTensor that HOLDS `codes` under the given parameters (dequantize dtype `dtype`)."""
    zeros = torch.zeros(codes.shape, device=codes.device, dtype=dtype)
    if axis is None:
        q = ff.quantization.affine.quantize_per_tensor(zeros, scale, offset, 8, torch.int8)
    else:
        q = ff.quantization.affine.quantize_per_channel(zeros, scale, offset, axis, 8, torch.int8)
    return ff.QuantizedTensor(codes, q.quantization_context)


@contextlib.contextmanager
def _without(monkeypatch, *names):
    """The dispatcher without a kernel for `names`: the package's reference chain runs (dequantize, the float op)."""
    with monkeypatch.context() as mp:
        for name in names:
            mp.setitem(dispatcher._DISPATCHER, name, [])
        yield


@pytest.mark.parametrize("pattern", ["low", "ties"])
def test_batched_matmul_and_bmm_through_the_dispatcher(pattern, monkeypatch):
    b, m, n, k = 3, 64, 64, 4096
    xq, wq = hc.codes(pattern, b * m, b * n, k, DEV)
    xq, wq = xq.reshape(b, m, k), wq.reshape(b, n, k)
    sx, ox, sw, ow = hc.parameters(pattern, m, n, DEV)
    sw1 = sw[:1].clone()
    ow1 = None if ow is None else ow[7:8].clone()
    want32 = torch.stack([hc.restated_linear(hc.accumulator64(xq[i], wq[i]), xq[i], wq[i], sx, ox, sw1.expand(n), None if ow1 is None else ow1.expand(n)) for i in range(b)])
    calls = []
    real = ops.bmm_w8a8
    monkeypatch.setattr(ops, "bmm_w8a8", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    for dtype in (torch.float32, torch.bfloat16):
        qx = _quantized(xq, sx, ox, dtype)
        qr = _quantized(wq.transpose(1, 2).contiguous(), sw1, ow1, dtype)
        with ff.strict_quantization(False):
            _same(ff.nn.functional.bmm(qx, qr), want32.to(dtype), f"bmm {pattern} {dtype}")
            _same(ff.nn.functional.matmul(qx, qr), want32.to(dtype), f"matmul {pattern} {dtype}")
    assert len(calls) == 4  # no silent fallback


# ---- convolutions ---------------------------------------------------------------------------------------------------------------------
# (name, transposed, B, C, OC, spatial, kernel, stride, padding)
CONVS = [
    ("conv2d_s1", False, 1, 512, 40, (6, 7), (3, 3), (1, 1), (1, 1)),
    ("conv2d_s2", False, 1, 512, 40, (6, 7), (3, 3), (2, 2), (1, 1)),
    ("conv1d", False, 1, 1024, 40, (1, 9), (1, 4), (1, 1), (0, 1)),
    ("conv_transpose2d", True, 1, 1024, 40, (3, 4), (4, 4), (2, 2), (1, 1)),
    ("conv_transpose1d", True, 1, 2048, 40, (1, 5), (1, 4), (1, 2), (0, 1)),
]


def _conv_call(transposed, xc, wc, sx, ox, sw, ow, bias, stride, padding, dtype):
    if transposed:
        return ops.conv_transpose2d_w8a8(xc, wc, sx, ox, sw, ow, bias, stride, padding, (0, 0), (1, 1), out_dtype=dtype)
    return ops.conv2d_w8a8(xc, wc, sx, ox, sw, ow, bias, stride, padding, (1, 1), out_dtype=dtype)


@pytest.mark.parametrize("pattern", ["low", "ties"])
@pytest.mark.parametrize("case", CONVS, ids=[c[0] for c in CONVS])
def test_convolutions(case, pattern):
    _, transposed, B, C, OC, spatial, kernel, stride, padding = case
    xc, wc = hc.conv_codes(pattern, B, C, OC, spatial, kernel, DEV, transposed=transposed)
    reached = False
    for ow_kind in ("native", "zero"):
        sx, ox, sw, ow = hc.parameters(pattern, 1, OC, DEV, ow_kind=ow_kind)
        for bias in (None, _bias(OC).float()):
            want32, terms = hc.restated_conv2d(xc, wc, sx, ox, sw, ow, bias, stride, padding, transposed=transposed)
            reached = reached or float(terms[0].abs().max()) >= 2**24
            for dtype in _dtypes(want32):
                got = _conv_call(transposed, xc, wc, sx, ox, sw, ow, bias, stride, padding, dtype)
                _same(got.cpu(), want32.to(dtype), f"{case[0]} {pattern} ow={ow_kind} bias={bias is not None} {dtype}")
    assert reached, "no accumulator of this case reaches 2^24"


# ---- the parity side ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["low", "mirror"])
@pytest.mark.parametrize("k", [4096, 14336])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=str)
def test_linear_stays_within_the_projects_tolerance_of_the_reference_chain(pattern, k, dtype, monkeypatch):
    m = n = 64
    xq, wq = hc.codes(pattern, m, n, k, DEV)
    sign = -1.0 if pattern == "mirror" else 1.0
    sx, ox = torch.tensor([0.02], device=DEV), torch.tensor([sign * 119.0], device=DEV)
    sw = torch.full((n,), 1e-3, device=DEV)
    ow = hc.parameters(pattern, m, n, DEV)[3]
    qx, qw = _quantized(xq, sx, ox, dtype), _quantized(wq, sw, ow, dtype, axis=0)
    with ff.strict_quantization(False):
        assert dispatcher.dispatch("linear", input=qx, weight=qw) is not None
        fused = ff.nn.functional.linear(qx, qw)
        with _without(monkeypatch, "linear"):
            assert dispatcher.dispatch("linear", input=qx, weight=qw) is None
            chain = ff.nn.functional.linear(qx, qw)
    _same(fused, hc.restated_linear(hc.accumulator64(xq, wq), xq, wq, sx, ox, sw, ow).to(dtype), f"dispatcher linear {pattern} K={k}")
    atol, rtol = linear_tolerances(dtype)
    print(f"{pattern} K={k} {dtype}: max |fused - chain| = {float((fused.float() - chain.float()).abs().max()):.4g}")
    torch.testing.assert_close(fused.float(), chain.float(), atol=atol, rtol=rtol)


@pytest.mark.parametrize("pattern", ["low", "mirror"])
@pytest.mark.parametrize("stride", [1, 2])
def test_conv2d_stays_within_the_projects_tolerance_of_the_reference_chain(pattern, stride, monkeypatch):
    dtype = torch.bfloat16
    B, C, OC, spatial, kernel = 1, 512, 40, (6, 7), (3, 3)
    xc, wc = hc.conv_codes(pattern, B, C, OC, spatial, kernel, DEV)
    sign = -1.0 if pattern == "mirror" else 1.0
    sx, ox = torch.tensor([0.02], device=DEV), torch.tensor([sign * 119.0], device=DEV)
    sw = torch.full((OC,), 1e-3, device=DEV)
    ow = hc.parameters(pattern, 1, OC, DEV)[3]
    qx, qw = _quantized(xc, sx, ox, dtype), _quantized(wc, sw, ow, dtype, axis=0)
    launches = []
    real = ops.conv2d_w8a8
    monkeypatch.setattr(ops, "conv2d_w8a8", lambda *a, **kw: launches.append(1) or real(*a, **kw))
    fused = ff.nn.functional.conv2d(qx, qw, None, stride, 1, 1, strict_quantization=False)
    assert len(launches) == 1
    with _without(monkeypatch, "conv1d", "conv2d"):
        chain = ff.nn.functional.conv2d(qx, qw, None, stride, 1, 1, strict_quantization=False)
    assert len(launches) == 1
    want32, _ = hc.restated_conv2d(xc, wc, sx, ox, sw, ow, None, (stride, stride), (1, 1))
    _same(fused.cpu(), want32.to(dtype), f"dispatcher conv2d {pattern} stride {stride}")
    atol, rtol = linear_tolerances(dtype)
    print(f"conv2d {pattern} stride {stride}: max |fused - chain| = {float((fused.float() - chain.float()).abs().max()):.4g}")
    torch.testing.assert_close(fused.float(), chain.float(), atol=atol, rtol=rtol)


@pytest.mark.parametrize("pattern", ["low", "mirror"])
def test_the_v_chain_stays_within_the_sum_of_its_half_ulps(pattern):
    """Unit scales make y = v: |v - v_exact| <= heavy_codes.rounding_bound, in float64 — for the tail kernel and the persistent one."""
    for m, n, k in ((64, 64, 4096), (P, P, 4096)):
        xq, wq, acc = _case(pattern, m, n, k)
        _, ox, _, ow = hc.parameters(pattern, m, n, DEV)
        one, ones = torch.ones(1, device=DEV), torch.ones(n, device=DEV)
        a, p1, p2, p3 = hc.terms64(acc, xq, wq, ox, ow)
        got = ops.linear_w8a8(xq, wq, one, ox, ones, ow, out_dtype=torch.float32)
        error, bound = (got.double() - (a + p1 + p2 + p3)).abs(), hc.rounding_bound(a, p1, p2, p3)
        assert bool((error <= bound).all()), f"{pattern} {m}x{n}x{k}: {int((error > bound).sum())} outputs beyond the bound, worst ratio {float((error / bound).max()):.3f}"


# ---- int32 headroom -----------------------------------------------------------------------------------------------------------------
def _constant(shape, value):
    return torch.full(shape, value, device=DEV, dtype=torch.int8)


def test_linear_at_the_edge_of_int32():
    """K = 131056 (the longest K % 16 == 0 the accumulator holds): all -128 on both sides is 2^31 - 2^18, exact in fp32."""
    n, k = 16, 131056
    one, ones = torch.ones(1, device=DEV), torch.ones(n, device=DEV)
    got = ops.linear_w8a8(_constant((1, k), -128), _constant((n, k), -128), one, None, ones, None, out_dtype=torch.float32)
    assert got.tolist() == [[float(2**31 - 2**18)] * n]
    got = ops.linear_w8a8(_constant((1, k), -128), _constant((n, k), 127), one, None, ones, None, out_dtype=torch.float32)
    assert got.tolist() == [[float(-128 * 127 * k)] * n]


@pytest.mark.parametrize("w_code,want", [(127, -127.0 * 2**24), (-128, 2.0**31)])
def test_linear_past_int32_is_refused_and_the_dispatcher_takes_the_chain(w_code, want, monkeypatch):
    """K = 131072: -128 x -128 sums to exactly 2^31, which int32 does not hold. The C entry point refuses the length before any
    launch (FFQ_ERR_DTYPE, `out` untouched), the dispatcher declines it, and the reference chain gives the exact value."""
    from fastforward_amd.ops._base import _ptr

    n, k = 16, 131072
    xq, wq = _constant((1, k), -128), _constant((n, k), w_code)
    one, ones = torch.ones(1, device=DEV), torch.ones(n, device=DEV)
    lib = _native.library()
    out = torch.full((1, n), 7.0, device=DEV)
    ws = torch.empty(lib.ffq_linear_w8a8_workspace_bytes(1, n, k), device=DEV, dtype=torch.uint8)
    rc = lib.ffq_linear_w8a8(_ptr(xq), _ptr(wq), None, _ptr(one), None, 0, _ptr(ones), None, 1, None, 0, _ptr(out), ops._tag(torch.float32),
                             None, None, 8.0, 0, 1, n, k, _ptr(ws), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 6 and bool((out == 7.0).all())
    with pytest.raises(RuntimeError, match="int32 accumulator"):
        ops.linear_w8a8(xq, wq, one, None, ones, None, out_dtype=torch.float32)
    with pytest.raises(RuntimeError, match="int32 accumulator"):
        ops.bmm_w8a8(xq[None], wq[None], one, None, one, None, out_dtype=torch.float32)
    qx, qw = _quantized(xq, one, None, torch.float32), _quantized(wq, ones, None, torch.float32, axis=0)
    assert dispatcher.dispatch("linear", input=qx, weight=qw) is None
    with ff.strict_quantization(False):
        got = ff.nn.functional.linear(qx, qw)
    assert got.tolist() == [[want] * n]


@pytest.mark.parametrize("transposed", [False, True], ids=["conv2d", "conv_transpose2d"])
def test_convolutions_at_the_edge_of_int32(transposed, monkeypatch):
    """C * KH * KW = 131072 (C = 8192, 4 x 4, one output pixel) is refused before any launch and the dispatcher takes the chain,
    which is exact; one channel fewer (131056 taps) runs, and all -128 on both sides gives 2^31 - 2^18."""
    oc = 16
    one, ones = torch.ones(1, device=DEV), torch.ones(oc, device=DEV)
    wshape = (lambda c: (c, oc, 4, 4)) if transposed else (lambda c: (oc, c, 4, 4))
    run = (lambda x, w: ops.conv_transpose2d_w8a8(x, w, one, None, ones, None, None, 1, 0, 0, 1, out_dtype=torch.float32)) if transposed else \
          (lambda x, w: ops.conv2d_w8a8(x, w, one, None, ones, None, None, 1, 0, 1, out_dtype=torch.float32))
    # the transposed convolution of a 4 x 4 image with a 4 x 4 filter: its output pixel (3, 3) sees all sixteen taps
    pick = (lambda y: y[0, :, 3, 3]) if transposed else (lambda y: y[0, :, 0, 0])
    c = 8191
    for w_code, want in ((-128, 128.0 * 128 * 16 * c), (127, -128.0 * 127 * 16 * c)):
        got = pick(run(_constant((1, c, 4, 4), -128), _constant(wshape(c), w_code)))
        assert got.tolist() == [want] * oc
    c = 8192
    fn = ff.nn.functional.conv_transpose2d if transposed else ff.nn.functional.conv2d
    name = "conv_transpose2d" if transposed else "conv2d"
    for w_code, want in ((127, -127.0 * 2**24), (-128, 2.0**31)):
        x, w = _constant((1, c, 4, 4), -128), _constant(wshape(c), w_code)
        with pytest.raises(RuntimeError, match="int32 accumulator"):
            run(x, w)
        qx, qw = _quantized(x, one, None, torch.float32), _quantized(w, ones, None, torch.float32, axis=1 if transposed else 0)
        assert dispatcher.dispatch(name, input=qx, weight=qw, strict_quantization=False) is None
        got = pick(fn(qx, qw, strict_quantization=False))
        assert got.tolist() == [want] * oc
