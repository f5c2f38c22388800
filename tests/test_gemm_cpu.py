"""The int8 GEMM family's host side without a GPU: what every C-ABI entry point of csrc/ffq_linear.hip answers from its argument
checks (status codes, in the order the checks run), the shape-class query, the workspace size queries, and what the wrappers of
ops/gemm.py raise or decline before a library call.

Every C call below ends in an argument check or an empty extent: the pointers are fake and nothing may launch. To keep that true
even where a check under test went missing, each helper's DEFAULT call already fails in the entry point's LAST check before its
first launch (noted at each helper), so a row whose own check did not fire still returns — with the wrong status — and launches nothing.
``ffq_mlp_gate_up_w8a8`` has no check behind its workspace check, so "needs no workspace -> not ERR_WORKSPACE" has no row for it (that
call would launch; tests/test_gemm_gpu.py runs it)."""

import ctypes

import pytest
import torch

import fastforward_amd as ff

from conftest import HIP_SO
from fastforward_amd._cabi import DType, FFQLibrary, Status

FAKE = 1 << 20  # 16-byte aligned, never dereferenced
P = (2048, 2048, 512)  # the persistent kernel's class (64 tiles of 256 x 256: the threshold)
T = (16, 128, 256)  # the tile ("tail") kernel's
BF16, I8, I32 = int(DType.BF16), int(DType.I8), int(DType.I32)


@pytest.fixture(scope="module")
def lib():
    return FFQLibrary(HIP_SO)


def _bytes(lib, nbytes, M, N, K):
    return lib.ffq_linear_w8a8_workspace_bytes(M, N, K) if nbytes is None else nbytes


# default: an output quantizer into an int32 container, which no instantiation writes -> ERR_DTYPE at the kernel dispatch (no row sum
# launch precedes it without weight offsets, with the weight row sums handed in, or below the persistent class)
def _linear(lib, shape=T, x=FAKE, w=FAKE, rowsum=None, xs=FAKE, xo=None, x_per_row=0, ws=FAKE, wo=None, w_per_row=0, bias=None, bias_dt=0, out=FAKE,
            out_dt=I32, out_scale=FAKE, bits=8.0, y_dt=BF16, workspace=FAKE, nbytes=None):
    M, N, K = shape
    return lib.ffq_linear_w8a8(x, w, rowsum, xs, xo, x_per_row, ws, wo, w_per_row, bias, bias_dt, out, out_dt, out_scale, None, bits, y_dt, M, N, K,
                               workspace, _bytes(lib, nbytes, M, N, K), None)


# default: a first matrix of 300 rows (no multiple of 256) -> ERR_DTYPE in the segment check, behind the workspace check
def _multi(lib, shape=P, rows=None, x=FAKE, w=FAKE, rowsum=None, xs=FAKE, xo=None, ws=FAKE, count=None, outs=(FAKE, FAKE, FAKE), out_dt=BF16,
           workspace=FAKE, nbytes=None, no_outs=False, no_rows=False):
    M, N, K = shape
    rows = (300, N - 300) if rows is None else rows
    count = len(rows) if count is None else count
    n = max(len(rows), 1)
    outs_c = None if no_outs else (ctypes.c_void_p * n)(*outs[:n])
    rows_c = None if no_rows else (ctypes.c_int64 * n)(*rows)
    return lib.ffq_linear_w8a8_multi(x, w, rowsum, xs, xo, 0, ws, count, outs_c, out_dt, M, rows_c, K, workspace, _bytes(lib, nbytes, M, N, K), None)


# default: no workspace, which this entry point always needs -> ERR_WORKSPACE, its last check
def _earlier(lib, shape=P, x=FAKE, ex=FAKE, es=FAKE, w=FAKE, rowsum=None, xs=FAKE, xo=None, ws=FAKE, wo=None, out=FAKE, out_dt=BF16, workspace=None,
             nbytes=None):
    M, N, K = shape
    return lib.ffq_linear_w8a8_earlier(x, ex, es, None, w, rowsum, xs, xo, ws, wo, 1, out, out_dt, M, N, K, workspace, _bytes(lib, nbytes, M, N, K), None)


# default: N = 2080 (N % 64 == 32; 8 x 9 tiles) -> ERR_DTYPE in the gated form's own check, behind the workspace check
def _gated(lib, shape=(2048, 2080, 512), x=FAKE, w=FAKE, rowsum=None, xs=FAKE, xo=None, ws=FAKE, wo=None, gate=FAKE, out=FAKE, workspace=FAKE,
           nbytes=None, words=None, pair=None):
    M, N, K = shape
    return lib.ffq_linear_w8a8_gated(x, w, rowsum, xs, xo, 0, ws, wo, 0, gate, out, M, N, K, workspace, _bytes(lib, nbytes, M, N, K), words, pair, None)


# default: as _linear (the row sums of a batched call with weight offsets are launched behind the workspace check only)
def _bmm(lib, shape=(4, 128, 128, 64), x=FAKE, w=FAKE, xs=FAKE, xo=None, ws=FAKE, wo=None, out=FAKE, out_dt=I32, out_scale=FAKE, bits=8.0, y_dt=BF16,
         workspace=FAKE, nbytes=None):
    B, M, N, K = shape
    nbytes = lib.ffq_bmm_w8a8_workspace_bytes(B, M, N, K) if nbytes is None else nbytes
    return lib.ffq_bmm_w8a8(x, w, xs, xo, ws, wo, out, out_dt, out_scale, None, bits, y_dt, B, M, N, K, workspace, nbytes, None)


# default: an activation offset without weight row sums and without a workspace -> ERR_WORKSPACE, its last check
def _gate_up(lib, shape=(256, 256, 256), x=FAKE, gw=FAKE, uw=FAKE, grs=None, urs=None, xs=FAKE, xo=FAKE, gs=FAKE, us=FAKE, codes=FAKE, out_scale=FAKE,
             bits=8.0, workspace=None, nbytes=None):
    M, N, K = shape
    nbytes = lib.ffq_mlp_gate_up_w8a8_workspace_bytes(M, N, K) if nbytes is None else nbytes
    return lib.ffq_mlp_gate_up_w8a8(x, gw, uw, grs, urs, xs, xo, gs, us, codes, out_scale, None, bits, M, N, K, workspace, nbytes, None)


# default: no workspace, which this entry point always needs -> ERR_WORKSPACE, its last check
def _estimating(lib, shape=P, xg=FAKE, xu=FAKE, gw=FAKE, uw=FAKE, xsg=FAKE, xsu=FAKE, gs=FAKE, us=FAKE, scratch=FAKE, product=FAKE, workspace=None,
                nbytes=None, words=None, pair=None):
    M, N, K = shape
    nbytes = lib.ffq_mlp_gate_up_w8a8_estimating_workspace_bytes(M, N, K) if nbytes is None else nbytes
    return lib.ffq_mlp_gate_up_w8a8_estimating(xg, xu, gw, uw, xsg, None, xsu, None, gs, None, us, None, scratch, product, M, N, K, workspace, nbytes,
                                               words, pair, None)


CALLS = {"linear": _linear, "multi": _multi, "earlier": _earlier, "gated": _gated, "bmm": _bmm, "gate_up": _gate_up, "estimating": _estimating}
REQUIRED = {  # the pointers each entry point refuses as NULL
    "linear": ("x", "w", "xs", "ws", "out"),
    "multi": ("x", "w", "xs", "ws"),
    "earlier": ("x", "ex", "es", "w", "xs", "ws", "out"),
    "gated": ("x", "w", "xs", "ws", "gate", "out"),
    "bmm": ("x", "w", "xs", "ws", "out"),
    "gate_up": ("x", "gw", "uw", "xs", "gs", "us", "codes", "out_scale"),
    "estimating": ("xg", "xu", "gw", "uw", "xsg", "xsu", "gs", "us", "scratch", "product"),
}
CODES = {  # the int8 operands read with 16-byte loads
    "linear": ("x", "w"), "multi": ("x", "w"), "earlier": ("x", "ex", "w"), "gated": ("x", "w"), "bmm": ("x", "w"), "gate_up": ("x", "gw", "uw"),
    "estimating": ("xg", "xu", "gw", "uw"),
}


def _with(shape, index, value):
    return tuple(value if i == index else v for i, v in enumerate(shape))


def _shape_of(name):
    return CALLS[name].__defaults__[0]


def _rows():
    rows = []
    for name in CALLS:
        shape = _shape_of(name)
        m, n, k = len(shape) - 3, len(shape) - 2, len(shape) - 1
        rows += [(name, dict(shape=_with(shape, i, -1)), Status.ERR_ARG) for i in range(len(shape))]
        rows += [(name, dict(shape=_with(shape, m, 0)), Status.OK)]
        if name != "multi":  # (its N is the sum of the matrices' rows, each of which it wants positive)
            rows += [(name, dict(shape=_with(shape, n, 0)), Status.OK)]
        rows += [(name, {p: None}, Status.ERR_ARG) for p in REQUIRED[name]]
        rows += [(name, dict(shape=_with(shape, i, 1 << 31)), Status.ERR_ARG) for i in (m, n, k)]
        rows += [(name, dict(shape=_with(shape, k, 131072)), Status.ERR_DTYPE), (name, dict(shape=_with(shape, k, 264)), Status.ERR_DTYPE)]
        rows += [(name, {p: FAKE + 8}, Status.ERR_DTYPE) for p in CODES[name]]
    # the output checks, where the entry point has the argument
    for name in ("linear", "bmm"):
        rows += [
            (name, dict(out_dt=I8, bits=11.0), Status.ERR_PRECISION),
            (name, dict(out_dt=I8, y_dt=I8), Status.ERR_DTYPE),
            (name, dict(out_dt=I8, y_dt=int(DType.F64)), Status.ERR_DTYPE),
            (name, dict(out_dt=I8, out_scale=None), Status.ERR_DTYPE),
        ]
    rows += [("multi", dict(out_dt=I8), Status.ERR_DTYPE), ("earlier", dict(out_dt=I8), Status.ERR_DTYPE), ("gate_up", dict(bits=11.0), Status.ERR_PRECISION),
             ("linear", dict(bias=FAKE, bias_dt=99), Status.ERR_ARG)]
    # the workspace: too small and NULL exactly where include/ffq.h says one is needed ...
    needed = [
        ("linear", dict(wo=FAKE)), ("linear", dict(shape=P, wo=FAKE)), ("linear", dict(shape=P, xo=FAKE)), ("linear", dict(shape=P, xo=FAKE, wo=FAKE, rowsum=FAKE)),
        ("multi", dict(xo=FAKE)), ("earlier", dict()), ("earlier", dict(rowsum=FAKE)), ("gated", dict(wo=FAKE)), ("gated", dict(xo=FAKE)),
        ("bmm", dict(wo=FAKE)), ("bmm", dict(xo=FAKE, wo=FAKE)), ("gate_up", dict()), ("gate_up", dict(grs=FAKE)), ("estimating", dict()),
    ]
    for name, change in needed:
        rows += [(name, dict(change, workspace=None), Status.ERR_WORKSPACE), (name, dict(change, workspace=FAKE, nbytes=255), Status.ERR_WORKSPACE)]
    # ... and the same calls where it says none is needed go on to the default's last check
    spared = [
        ("linear", dict()), ("linear", dict(xo=FAKE)), ("linear", dict(shape=P)), ("linear", dict(shape=P, xo=FAKE, rowsum=FAKE)),
        ("linear", dict(shape=(1792, 2048, 256), xo=FAKE)), ("multi", dict()), ("multi", dict(xo=FAKE, rowsum=FAKE)), ("gated", dict()),
        ("gated", dict(xo=FAKE, rowsum=FAKE)), ("bmm", dict()), ("bmm", dict(xo=FAKE)),
    ]
    for name, change in spared:
        rows += [(name, dict(change, workspace=None, nbytes=0), Status.ERR_DTYPE)]
    # one entry point's own
    rows += [
        ("gated", dict(shape=T), Status.ERR_DTYPE),                                    # below the persistent class
        ("gated", dict(shape=(1792, 2048, 256)), Status.ERR_DTYPE),                    # 56 tiles
        ("gated", dict(shape=(2048, 2080, 512)), Status.ERR_DTYPE),                    # N % 64 != 0
        ("gated", dict(gate=FAKE + 8), Status.ERR_DTYPE),
        ("gated", dict(words=FAKE), Status.ERR_ARG),
        ("gated", dict(pair=FAKE), Status.ERR_ARG),
        ("estimating", dict(words=FAKE), Status.ERR_ARG),
        ("estimating", dict(pair=FAKE), Status.ERR_ARG),
        # N = 2176 is 17 column tiles of 128 (the one-launch mode's) but 9 of 256, and the class counts 256 x 256 tiles: 4 x 9 and 7 x 9 < 64
        ("estimating", dict(shape=(1024, 2176, 512)), Status.ERR_DTYPE),
        ("estimating", dict(shape=(1792, 2176, 512)), Status.ERR_DTYPE),
        ("estimating", dict(shape=(2048, 2176, 512)), Status.ERR_WORKSPACE),           # 8 x 9 tiles, N % 128 == 0: taken (on to the default's last check)
        ("estimating", dict(shape=(2048, 2112, 512)), Status.ERR_DTYPE),               # N % 128 != 0
        ("estimating", dict(shape=(100, 1 << 20, 512)), Status.ERR_DTYPE),
        ("estimating", dict(shape=(1792, 2048, 256)), Status.ERR_DTYPE),
        ("estimating", dict(shape=(2048, 2048, 128)), Status.ERR_DTYPE),
        ("estimating", dict(scratch=FAKE + 8), Status.ERR_DTYPE),
        ("estimating", dict(product=FAKE + 8), Status.ERR_DTYPE),
        ("gate_up", dict(shape=(256, 192, 256)), Status.ERR_DTYPE),
        ("gate_up", dict(shape=(256, 256, 128)), Status.ERR_DTYPE),
        ("gate_up", dict(codes=FAKE + 8), Status.ERR_DTYPE),
        ("multi", dict(rows=(2048,)), Status.ERR_ARG),
        ("multi", dict(rows=(512, 512, 512, 512)), Status.ERR_ARG),
        ("multi", dict(no_outs=True), Status.ERR_ARG),
        ("multi", dict(no_rows=True), Status.ERR_ARG),
        ("multi", dict(outs=(FAKE, None, FAKE)), Status.ERR_ARG),
        ("multi", dict(rows=(2048, 0)), Status.ERR_ARG),
        ("multi", dict(outs=(FAKE, FAKE + 8, FAKE)), Status.ERR_DTYPE),
        ("multi", dict(rows=(256, 300, 1492)), Status.ERR_DTYPE),                      # a middle matrix of 300 rows
        ("multi", dict(shape=(100, 512, 256), rows=(256, 256)), Status.ERR_DTYPE),     # outside the persistent class
        ("earlier", dict(shape=T, workspace=FAKE), Status.ERR_DTYPE),
        ("earlier", dict(shape=(1792, 2048, 256), workspace=FAKE), Status.ERR_DTYPE),
        ("bmm", dict(shape=(65536, 16, 16, 64)), Status.ERR_ARG),
        ("bmm", dict(shape=(0, 128, 128, 64)), Status.OK),
    ]
    return rows


ROWS = _rows()


@pytest.mark.parametrize("name,change,status", ROWS, ids=[f"{n}-{i}" for i, (n, _, _) in enumerate(ROWS)])
def test_argument_checks_need_no_device(lib, name, change, status):
    assert CALLS[name](lib, **change) == status, (name, change)
    if status != Status.OK:
        assert lib.ffq_last_error()


@pytest.mark.parametrize("shape,takes", [((2048, 2048, 512), 1), ((1800, 2048, 256), 1), ((1792, 2048, 256), 0), ((2048, 2048, 192), 0), ((2048, 2048, 320), 0),
                                         ((127, 1 << 20, 256), 0), ((0, 2048, 512), 0), ((-1, 2048, 512), 0), ((2048, 0, 512), 0), ((2048, 2048, 0), 0),
                                         ((128, 1 << 14, 256), 1), ((1 << 14, 128, 256), 1), ((1 << 14, 127, 256), 0), ((2048, 2048, 128), 0)])
def test_the_persistent_shape_class(lib, shape, takes):
    assert lib.ffq_linear_w8a8_takes_earlier(*shape) == takes


def test_workspace_queries(lib):
    assert lib.ffq_linear_w8a8_workspace_bytes(2048, 2048, 512) == 16640  # (2048 + 2048 + 1) int32, rounded up to 256 bytes
    assert lib.ffq_linear_w8a8_workspace_bytes(16, 128, 256) == 768
    assert lib.ffq_bmm_w8a8_workspace_bytes(4, 128, 128, 64) == 4096
    assert lib.ffq_mlp_gate_up_w8a8_workspace_bytes(7, 256, 9) == 2048
    assert lib.ffq_mlp_gate_up_w8a8_estimating_workspace_bytes(2048, 2048, 512) == 33280  # 256 + 2 * 2048 * 4 + the linear's
    for m, n in ((-1, 2048), (2048, -1)):
        assert lib.ffq_linear_w8a8_workspace_bytes(m, n, 512) == 0
        assert lib.ffq_mlp_gate_up_w8a8_estimating_workspace_bytes(m, n, 512) == 0
    assert lib.ffq_mlp_gate_up_w8a8_workspace_bytes(2048, -1, 512) == 0
    for shape in ((-1, 128, 128, 64), (4, -1, 128, 64), (4, 128, -1, 64)):
        assert lib.ffq_bmm_w8a8_workspace_bytes(*shape) == 0


# ---- the wrappers of ops/gemm.py on host tensors, the oracle standing in for the library ------------------------------------------
M_, N_, K_ = 4, 8, 32


def _codes(*shape):
    return torch.zeros(shape, dtype=torch.int8)


ONE = torch.ones(1)


def _wrapper(name, **change):
    """Call wrapper `name` on small valid operands with `change` applied."""
    ops = ff.ops
    x, w, wn = _codes(M_, K_), _codes(N_, K_), torch.ones(N_)
    if name == "linear_w8a8":
        call = dict(x_codes=x, w_codes=w, x_scale=ONE, x_offset=None, w_scale=wn, w_offset=None)
    elif name == "linear_w8a8_multi":
        call = dict(x_codes=x, w_codes=_codes(512, K_), x_scale=ONE, x_offset=None, w_scale=torch.ones(512), rows=(256, 256))
    elif name == "linear_w8a8_earlier":
        call = dict(x_codes=x, earlier=(x.clone(), ONE, None), w_codes=w, x_scale=ONE, x_offset=None, w_scale=wn, w_offset=None)
    elif name == "linear_w8a8_gated":
        call = dict(x_codes=x, w_codes=w, x_scale=ONE, x_offset=None, w_scale=wn, w_offset=None, gate=torch.zeros(M_, N_, dtype=torch.bfloat16))
    elif name == "bmm_w8a8":
        call = dict(x_codes=_codes(2, M_, K_), w_codes=_codes(2, N_, K_), x_scale=ONE, x_offset=None, w_scale=ONE, w_offset=None)
    elif name == "mlp_gate_up_w8a8":
        call = dict(x_codes=_codes(M_, 256), gate_codes=_codes(128, 256), up_codes=_codes(128, 256), x_scale=ONE, x_offset=None, gate_scale=torch.ones(128),
                    up_scale=torch.ones(128), out_scale=ONE, out_offset=None)
    else:
        call = dict(x_codes_gate=_codes(2048, 256), x_codes_up=_codes(2048, 256), gate_codes=_codes(2048, 256), up_codes=_codes(2048, 256),
                    x_params_gate=(ONE, None), x_params_up=(ONE, None), gate_params=(torch.ones(2048), None), up_params=(torch.ones(2048), None))
    call.update(change)
    return getattr(ops, name)(**call)


SHAPE_TEXT = "mat1 and mat2 shapes cannot be multiplied (4x32 and (8, 16)^T)"
ROWSUM_TEXT = "w_rowsum must be a contiguous int32 tensor with 8 entries on the codes' device"
RAISES = [
    ("linear_w8a8", dict(x_codes=torch.zeros(M_, K_)), TypeError, "linear_w8a8 expects int8 codes"),
    ("linear_w8a8", dict(w_codes=torch.zeros(N_, K_)), TypeError, "linear_w8a8 expects int8 codes"),
    ("linear_w8a8", dict(w_codes=_codes(N_, 16)), RuntimeError, SHAPE_TEXT),
    ("linear_w8a8", dict(w_codes=_codes(2, N_, K_)), RuntimeError, "mat1 and mat2 shapes cannot be multiplied (4x32 and (2, 8, 32)^T)"),
    ("linear_w8a8", dict(w_rowsum=torch.zeros(N_, dtype=torch.int64)), RuntimeError, ROWSUM_TEXT),
    ("linear_w8a8", dict(w_rowsum=torch.zeros(N_ + 1, dtype=torch.int32)), RuntimeError, ROWSUM_TEXT),
    ("linear_w8a8", dict(w_rowsum=torch.zeros(2 * N_, dtype=torch.int32)[::2]), RuntimeError, ROWSUM_TEXT),
    ("linear_w8a8", dict(x_scale=torch.ones(2)), RuntimeError, "activation scale must have 1 or 4 entries, got 2"),
    ("linear_w8a8", dict(w_scale=torch.ones(2)), RuntimeError, "weight scale must have 1 or 8 entries, got 2"),
    ("linear_w8a8_multi", dict(x_codes=torch.zeros(M_, K_)), TypeError, "linear_w8a8_multi expects int8 codes"),
    ("linear_w8a8_multi", dict(w_rowsum=torch.zeros(512, dtype=torch.int64)), RuntimeError, ROWSUM_TEXT.replace(" 8 ", " 512 ")),
    ("linear_w8a8_multi", dict(w_rowsum=torch.zeros(511, dtype=torch.int32)), RuntimeError, ROWSUM_TEXT.replace(" 8 ", " 512 ")),
    ("linear_w8a8_earlier", dict(w_codes=torch.zeros(N_, K_)), TypeError, "linear_w8a8_earlier expects int8 codes"),
    ("linear_w8a8_earlier", dict(earlier=(torch.zeros(M_, K_), ONE, None)), TypeError, "linear_w8a8_earlier expects int8 codes"),
    ("linear_w8a8_earlier", dict(w_codes=_codes(N_, 16)), RuntimeError, SHAPE_TEXT),
    ("linear_w8a8_earlier", dict(earlier=(_codes(2, K_), ONE, None)), RuntimeError, "earlier codes of shape (2, 32) for activation codes of shape (4, 32)"),
    ("linear_w8a8_earlier", dict(w_rowsum=torch.zeros(N_, dtype=torch.int64)), RuntimeError, ROWSUM_TEXT),
    ("linear_w8a8_earlier", dict(w_rowsum=torch.zeros(N_ - 1, dtype=torch.int32)), RuntimeError, ROWSUM_TEXT),
    ("linear_w8a8_gated", dict(x_codes=torch.zeros(M_, K_)), TypeError, "linear_w8a8_gated expects int8 codes"),
    ("linear_w8a8_gated", dict(w_codes=_codes(N_, 16)), RuntimeError, SHAPE_TEXT),
    ("linear_w8a8_gated", dict(w_rowsum=torch.zeros(N_, dtype=torch.int64)), RuntimeError, ROWSUM_TEXT),
    ("linear_w8a8_gated", dict(w_rowsum=torch.zeros(N_ + 1, dtype=torch.int32)), RuntimeError, ROWSUM_TEXT),
    ("bmm_w8a8", dict(x_codes=torch.zeros(2, M_, K_)), TypeError, "bmm_w8a8 expects int8 codes of shape [B, M, K] and [B, N, K]"),
    ("bmm_w8a8", dict(w_codes=_codes(N_, K_)), TypeError, "bmm_w8a8 expects int8 codes of shape [B, M, K] and [B, N, K]"),
    ("bmm_w8a8", dict(w_codes=_codes(2, N_, 16)), RuntimeError, "batch1 and batch2 shapes cannot be multiplied ((2, 4, 32) and (2, 8, 16)^T)"),
    ("bmm_w8a8", dict(w_codes=_codes(3, N_, K_)), RuntimeError, "batch1 and batch2 shapes cannot be multiplied ((2, 4, 32) and (3, 8, 32)^T)"),
    ("bmm_w8a8", dict(x_scale=torch.ones(2)), RuntimeError, "bmm_w8a8 takes per-tensor parameters (one scale per operand)"),
    ("bmm_w8a8", dict(w_scale=torch.ones(2)), RuntimeError, "bmm_w8a8 takes per-tensor parameters (one scale per operand)"),
    ("mlp_gate_up_w8a8", dict(x_codes=torch.zeros(M_, 256)), TypeError, "mlp_gate_up_w8a8 expects int8 codes and equally shaped gate / up weights"),
    ("mlp_gate_up_w8a8", dict(up_codes=_codes(256, 256)), TypeError, "mlp_gate_up_w8a8 expects int8 codes and equally shaped gate / up weights"),
    ("mlp_gate_up_w8a8", dict(x_codes=_codes(M_, 128)), RuntimeError, "mat1 and mat2 shapes cannot be multiplied (4x128 and (128, 256)^T)"),
    ("mlp_gate_up_w8a8", dict(x_scale=torch.ones(2)), RuntimeError, "expected 1 parameter entries, got 2"),
    ("mlp_gate_up_w8a8", dict(gate_scale=torch.ones(2)), RuntimeError, "expected 128 parameter entries, got 2"),
    ("mlp_gate_up_w8a8", dict(gate_rowsum=torch.zeros(128, dtype=torch.int64)), RuntimeError,
     "row sums must be contiguous int32 tensors with 128 entries on the codes' device"),
    ("mlp_gate_up_w8a8", dict(up_rowsum=torch.zeros(127, dtype=torch.int32)), RuntimeError,
     "row sums must be contiguous int32 tensors with 128 entries on the codes' device"),
    ("mlp_gate_up_w8a8_estimating", dict(x_codes_up=torch.zeros(2048, 256)), TypeError,
     "mlp_gate_up_w8a8_estimating expects int8 codes, equally shaped gate / up weights and equally shaped activations"),
    ("mlp_gate_up_w8a8_estimating", dict(x_codes_up=_codes(1024, 256)), TypeError,
     "mlp_gate_up_w8a8_estimating expects int8 codes, equally shaped gate / up weights and equally shaped activations"),
    ("mlp_gate_up_w8a8_estimating", dict(x_codes_gate=_codes(2048, 512), x_codes_up=_codes(2048, 512)), RuntimeError,
     "mat1 and mat2 shapes cannot be multiplied (2048x512 and (2048, 256)^T)"),
]


@pytest.mark.parametrize("name,change,kind,text", RAISES, ids=[f"{r[0]}-{i}" for i, r in enumerate(RAISES)])
def test_the_wrappers_raise_as_before(oracle_backend, name, change, kind, text):
    with pytest.raises(kind) as caught:
        _wrapper(name, **change)
    assert type(caught.value) is kind and str(caught.value) == text


BF = torch.zeros(M_, N_, dtype=torch.bfloat16)
DECLINES = [
    # linear_w8a8_multi: the count, the output dtype, the stacked weight's shape, the matrices' rows, the parameter layouts
    ("linear_w8a8_multi", dict(rows=(512,))),
    ("linear_w8a8_multi", dict(rows=(128, 128, 128, 128))),
    ("linear_w8a8_multi", dict(out_dtype=torch.int8)),
    ("linear_w8a8_multi", dict(w_codes=_codes(512, 16))),
    ("linear_w8a8_multi", dict(w_codes=_codes(2, 256, K_))),
    ("linear_w8a8_multi", dict(rows=(256, 128))),
    ("linear_w8a8_multi", dict(rows=(512, 0))),
    ("linear_w8a8_multi", dict(rows=(300, 212))),
    ("linear_w8a8_multi", dict(x_scale=torch.ones(2))),
    ("linear_w8a8_multi", dict(w_scale=ONE)),
    # linear_w8a8_earlier: per-tensor activation parameters only, a real-valued output, the persistent class
    ("linear_w8a8_earlier", dict(x_scale=torch.ones(M_))),
    ("linear_w8a8_earlier", dict(x_scale=torch.ones(2))),
    ("linear_w8a8_earlier", dict(earlier=(_codes(M_, K_), torch.ones(M_), None))),
    ("linear_w8a8_earlier", dict(w_scale=torch.ones(2))),
    ("linear_w8a8_earlier", dict(out_dtype=torch.int8)),
    ("linear_w8a8_earlier", dict()),  # (4, 8, 32): outside ffq_linear_w8a8_takes_earlier
    # linear_w8a8_gated: the gate's dtype and shape, empty extents, the parameter layouts
    ("linear_w8a8_gated", dict(gate=BF.float())),
    ("linear_w8a8_gated", dict(gate=torch.zeros(M_, N_ + 1, dtype=torch.bfloat16))),
    ("linear_w8a8_gated", dict(gate=torch.zeros(N_, M_, dtype=torch.bfloat16))),
    ("linear_w8a8_gated", dict(x_codes=_codes(0, K_), gate=torch.zeros(0, N_, dtype=torch.bfloat16))),
    ("linear_w8a8_gated", dict(w_codes=_codes(0, K_), w_scale=ONE, gate=torch.zeros(M_, 0, dtype=torch.bfloat16))),
    ("linear_w8a8_gated", dict(x_scale=torch.ones(2))),
    ("linear_w8a8_gated", dict(w_scale=torch.ones(2))),
    # mlp_gate_up_w8a8: N % 128, K % 128, K >= 256
    ("mlp_gate_up_w8a8", dict(gate_codes=_codes(192, 256), up_codes=_codes(192, 256))),
    ("mlp_gate_up_w8a8", dict(x_codes=_codes(M_, 320), gate_codes=_codes(128, 320), up_codes=_codes(128, 320))),
    ("mlp_gate_up_w8a8", dict(x_codes=_codes(M_, 128), gate_codes=_codes(128, 128), up_codes=_codes(128, 128))),
    # mlp_gate_up_w8a8_estimating: the persistent class and N % 128, then the parameter layouts
    ("mlp_gate_up_w8a8_estimating", dict(x_codes_gate=_codes(1792, 256), x_codes_up=_codes(1792, 256))),  # 56 tiles
    ("mlp_gate_up_w8a8_estimating", dict(x_codes_gate=_codes(100, 256), x_codes_up=_codes(100, 256), gate_codes=_codes(1 << 14, 256),
                                         up_codes=_codes(1 << 14, 256))),  # M < 128
    ("mlp_gate_up_w8a8_estimating", dict(gate_codes=_codes(2112, 256), up_codes=_codes(2112, 256))),  # N % 128 != 0 inside the class
    ("mlp_gate_up_w8a8_estimating", dict(x_codes_gate=_codes(1024, 256), x_codes_up=_codes(1024, 256), gate_codes=_codes(2176, 256),
                                         up_codes=_codes(2176, 256))),  # N % 128 == 0, but 4 x 9 tiles of 256 x 256
    ("mlp_gate_up_w8a8_estimating", dict(x_codes_gate=_codes(2048, 128), x_codes_up=_codes(2048, 128), gate_codes=_codes(2048, 128),
                                         up_codes=_codes(2048, 128))),
    ("mlp_gate_up_w8a8_estimating", dict(x_codes_gate=_codes(2048, 320), x_codes_up=_codes(2048, 320), gate_codes=_codes(2048, 320),
                                         up_codes=_codes(2048, 320))),
    ("mlp_gate_up_w8a8_estimating", dict(x_params_gate=(torch.ones(2), None))),
    ("mlp_gate_up_w8a8_estimating", dict(x_params_up=(torch.ones(2048), None))),
    ("mlp_gate_up_w8a8_estimating", dict(gate_params=(ONE, None))),
    ("mlp_gate_up_w8a8_estimating", dict(up_params=(torch.ones(2), None))),
    ("mlp_gate_up_w8a8_estimating", dict(x_params_gate=(ONE, torch.zeros(2)))),
    ("mlp_gate_up_w8a8_estimating", dict(up_params=(torch.ones(2048), torch.zeros(1)))),
]


@pytest.mark.parametrize("name,change", DECLINES, ids=[f"{r[0]}-{i}" for i, r in enumerate(DECLINES)])
def test_the_wrappers_decline_as_before(oracle_backend, name, change):
    assert _wrapper(name, **change) is None
