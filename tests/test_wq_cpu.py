"""The weight-only GEMM family's host side without a GPU: the plan queries against a recorded table (tests/golden/wq_plan.json, taken
from the build before the host side was restated: tests/golden/gen_wq_plan.py), what the three C-ABI entry points of
csrc/ffq_wlinear.hip answer from their argument checks (status codes, in the order the checks run), and what the wrappers of
ops/wq.py raise or decline before a library call.

Every C call below ends in an argument check or an empty extent: the pointers are fake and nothing may launch. To keep that true
even where a check under test went missing, each helper's DEFAULT call already fails in the entry point's LAST check before its
first launch: a forced ``split=2`` without a workspace is FFQ_ERR_ARG in each of the three forms (the skinny form at (16, 128, 256),
the 128-column tiles at (300, 128, 1024), the 256-row tiles at (1024, 128, 1024))."""

import ctypes
import json

import pytest
import torch

import fastforward_amd as ff
import gen_wq_plan

from conftest import GOLDEN, HIP_SO
from fastforward_amd._cabi import DType, FFQLibrary, Status

FAKE = 1 << 20  # 16-byte aligned, never dereferenced
SKINNY, MID, TILES = (16, 128, 256), (300, 128, 1024), (1024, 128, 1024)
FORMS = {"skinny": SKINNY, "mid": MID, "tiles": TILES}
BF16, F32, I8, U8 = int(DType.BF16), int(DType.F32), int(DType.I8), int(DType.U8)
OK, NUMEL, DTYPE, ARG = Status.OK, Status.ERR_PARAM_NUMEL, Status.ERR_DTYPE, Status.ERR_ARG
NEEDS_SCRATCH = "bytes of workspace and a ticket buffer"  # the default's last check


@pytest.fixture(scope="module")
def lib():
    return FFQLibrary(HIP_SO)


def test_the_plan_is_the_recorded_one(lib):
    if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the table is the plan for 256 CUs")
    want = json.loads((GOLDEN / "wq_plan.json").read_text())
    cases = gen_wq_plan.grid()
    assert [tuple(r[:4]) for r in want] == cases and len(cases) == 2856
    got = gen_wq_plan.table(gen_wq_plan.bind(HIP_SO))
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, f"{len(wrong)} rows differ, the first (got, recorded): {wrong[0]}"


def test_the_plan_of_no_problem(lib):
    for M, N, K in ((0, 128, 256), (-1, 128, 256), (16, 0, 256), (16, 128, 64), (16, 128, 0)):
        for mlp in (0, 1):
            assert lib.ffq_linear_wq_split(M, N, K, mlp) == 1
            assert lib.ffq_linear_wq_tickets(M, N, K, mlp) == 0
            assert lib.ffq_linear_wq_slab_bytes(M, N, K, mlp, 4) == 0
        assert lib.ffq_linear_wq_workspace_bytes(M, N, K) == 0
        assert lib.ffq_mlp_gate_up_wq_workspace_bytes(M, N, K) == 0
    assert lib.ffq_mlp_gate_up_wq_workspace_bytes(4096, 192, 256) == 0  # N % 128 != 0


def _linear(lib, shape=SKINNY, x=FAKE, w=FAKE, w_dt=I8, pack_block=0, scale=FAKE, offset=None, numel=None, group=None, bias=None, bias_dt=0, out=FAKE,
            out_dt=BF16, workspace=None, nbytes=0, tickets=None, split=2):
    M, N, K = shape
    group = K if group is None else group
    numel = N * (K // group if group > 0 else 1) if numel is None else numel
    return lib.ffq_linear_wq(x, BF16, w, w_dt, pack_block, scale, offset, numel, group, bias, bias_dt, out, out_dt, M, N, K, workspace, nbytes, tickets,
                             split, None)


def _multi(lib, shape=SKINNY, rows=None, x=FAKE, codes=(FAKE, FAKE, FAKE), scales=(FAKE, FAKE, FAKE), offsets=(None, None, None), outs=(FAKE, FAKE, FAKE),
           count=None, per_row=1, group=None, split=2, no_rows=False):
    M, N, K = shape
    rows = (256, N) if rows is None else rows
    count = len(rows) if count is None else count
    n = max(len(rows), 1)
    ptrs = lambda values: (ctypes.c_void_p * n)(*values[:n])  # noqa: E731
    rows_c = None if no_rows else (ctypes.c_int64 * n)(*rows)
    return lib.ffq_linear_wq_multi(x, BF16, count, ptrs(codes), I8, 0, ptrs(scales), ptrs(offsets), per_row, K if group is None else group, ptrs(outs), BF16,
                                   M, rows_c, K, None, 0, None, split, None)


def _mlp(lib, shape=TILES, x=FAKE, gate=FAKE, up=FAKE, gs=FAKE, go=None, us=FAKE, uo=None, numel=None, group=None, out=FAKE, split=2):
    M, N, K = shape
    group = K if group is None else group
    numel = N * (K // group if group > 0 else 1) if numel is None else numel
    return lib.ffq_mlp_gate_up_wq(x, BF16, gate, up, I8, 0, gs, go, us, uo, numel, group, out, M, N, K, None, 0, None, split, None)


CALLS = {"linear": _linear, "multi": _multi, "mlp": _mlp}


def _with(shape, index, value):
    return tuple(value if i == index else v for i, v in enumerate(shape))


def _rows():
    rows = []
    for form, shape in FORMS.items():
        for name in ("linear", "multi"):
            rows += [(name, dict(shape=shape), ARG, NEEDS_SCRATCH)]  # the default itself, in each form
        rows += [
            ("linear", dict(shape=_with(shape, 0, -1)), ARG, "negative extent"),
            ("linear", dict(shape=_with(shape, 1, -1)), ARG, "negative extent"),
            ("linear", dict(shape=_with(shape, 2, -1)), ARG, "negative extent"),
            ("linear", dict(shape=shape, split=-1), ARG, "negative extent"),
            ("linear", dict(shape=_with(shape, 0, 0)), OK, None),
            ("linear", dict(shape=_with(shape, 1, 0)), OK, None),
            ("linear", dict(shape=_with(shape, 0, 0), x=None), OK, None),  # an empty problem before the NULL check
            ("linear", dict(shape=_with(shape, 2, 100)), DTYPE, "weight-only linear: needs bf16 activations"),
            ("linear", dict(shape=_with(shape, 2, 64)), DTYPE, "weight-only linear: needs bf16 activations"),
            ("linear", dict(shape=shape, out_dt=I8), DTYPE, "weight-only linear: needs bf16 activations"),
            ("linear", dict(shape=shape, w_dt=U8, pack_block=48), DTYPE, "weight-only linear: needs bf16 activations"),
            ("linear", dict(shape=shape, group=96), DTYPE, "weight-only linear: needs bf16 activations"),
            ("linear", dict(shape=shape, bias=FAKE, bias_dt=99), ARG, "bad bias dtype"),
            ("linear", dict(shape=shape, numel=shape[1] + 1), NUMEL, "parameters for"),
            ("linear", dict(shape=shape, numel=1, group=128), NUMEL, "one parameter pair needs group == K"),
            # two broken checks: the earlier one answers
            ("linear", dict(shape=_with(shape, 2, 100), x=None), ARG, "NULL buffer"),
            ("linear", dict(shape=_with(shape, 2, 100), x=FAKE + 8), DTYPE, "weight-only linear: needs bf16 activations"),
            ("linear", dict(shape=_with(shape, 2, 100), numel=3), DTYPE, "weight-only linear: needs bf16 activations"),
            ("linear", dict(shape=shape, x=FAKE + 8, bias=FAKE, bias_dt=99), DTYPE, "16-byte aligned"),
            ("linear", dict(shape=shape, bias=FAKE, bias_dt=99, numel=3), ARG, "bad bias dtype"),
            ("linear", dict(shape=shape, out=FAKE + 8, numel=3), DTYPE, "16-byte aligned"),
            ("linear", dict(shape=shape, numel=3, split=1 << 20), NUMEL, "parameters for"),
        ]
        rows += [("linear", dict(shape=shape, **{p: None}), ARG, "NULL buffer") for p in ("x", "w", "scale", "out")]
        rows += [("linear", dict(shape=shape, **{p: FAKE + 8}), DTYPE, "16-byte aligned") for p in ("x", "w", "out")]
    # a split above the form's maximum: 2 chunks of 128 / 16 super-steps of 64 / 256 CUs over 4 tail tiles and 16 super-steps over 2
    for name in ("linear", "multi"):
        rows += [
            (name, dict(shape=SKINNY, split=3), ARG, "(skinny form): split 3 exceeds the 2 chunks of 128 along K"),
            (name, dict(shape=MID, split=17), ARG, "(128-column tiles): split 17 exceeds the 16 super-steps of 64 along K"),
        ]
    rows += [
        ("linear", dict(shape=TILES, split=9), ARG, "weight-only linear: split 9 exceeds 8 "),
        ("multi", dict(shape=TILES, split=9), ARG, "weight-only linear: split 9 exceeds 8 "),  # 8 tiles: 256 / 8 slices by the CUs, 8 by K
        ("mlp", dict(split=9), ARG, "weight-only linear: split 9 exceeds 8 "),
        # ffq_linear_wq_multi
        ("multi", dict(rows=()), ARG, "1 to 3 weight matrices"),
        ("multi", dict(rows=(256, 256, 256, 128)), ARG, "1 to 3 weight matrices"),
        ("multi", dict(no_rows=True), ARG, "1 to 3 weight matrices"),
        ("multi", dict(shape=_with(SKINNY, 0, -1)), ARG, "negative extent"),
        ("multi", dict(rows=(256, 0)), ARG, "empty weight matrix"),
        ("multi", dict(rows=(300, 84)), DTYPE, "every weight matrix but the last needs a multiple of 256 rows"),
        ("multi", dict(rows=(256, 300, 84)), DTYPE, "every weight matrix but the last needs a multiple of 256 rows"),
        ("multi", dict(codes=(FAKE, None, FAKE)), ARG, "NULL buffer"),
        ("multi", dict(scales=(None, FAKE, FAKE)), ARG, "NULL buffer"),
        ("multi", dict(outs=(FAKE, None, FAKE)), ARG, "NULL buffer"),
        ("multi", dict(offsets=(FAKE, None, None)), ARG, "offsets for all weight matrices or for none"),
        ("multi", dict(offsets=(None, FAKE, None)), ARG, "offsets for all weight matrices or for none"),
        ("multi", dict(codes=(FAKE, FAKE + 8, FAKE)), DTYPE, "16-byte aligned"),
        ("multi", dict(outs=(FAKE + 8, FAKE, FAKE)), DTYPE, "16-byte aligned"),
        ("multi", dict(shape=_with(SKINNY, 0, 0)), OK, None),
        ("multi", dict(x=None), ARG, "NULL or misaligned activations"),
        ("multi", dict(x=FAKE + 8), ARG, "NULL or misaligned activations"),
        ("multi", dict(shape=_with(SKINNY, 2, 100)), DTYPE, "weight-only linear: needs bf16 activations"),
        ("multi", dict(per_row=0, group=128), NUMEL, "one parameter pair per matrix needs group == K"),
        # ... the earlier check answers
        ("multi", dict(rows=(256, 256, 256, 128), shape=_with(SKINNY, 0, -1)), ARG, "1 to 3 weight matrices"),
        ("multi", dict(rows=(300, 84), codes=(None, FAKE, FAKE)), DTYPE, "every weight matrix but the last needs a multiple of 256 rows"),
        ("multi", dict(rows=(300, 84), shape=_with(SKINNY, 0, 0)), DTYPE, "every weight matrix but the last needs a multiple of 256 rows"),
        ("multi", dict(codes=(FAKE, None, FAKE), offsets=(FAKE, None, None)), ARG, "NULL buffer"),
        ("multi", dict(offsets=(FAKE, None, None), outs=(FAKE, FAKE + 8, FAKE)), ARG, "offsets for all weight matrices or for none"),
        ("multi", dict(shape=_with(SKINNY, 0, 0), x=None), OK, None),
        ("multi", dict(x=None, shape=_with(SKINNY, 2, 100)), ARG, "NULL or misaligned activations"),
        ("multi", dict(shape=_with(SKINNY, 2, 100), per_row=0, group=50), DTYPE, "weight-only linear: needs bf16 activations"),
        ("multi", dict(per_row=0, group=128, split=3), NUMEL, "one parameter pair per matrix needs group == K"),
        # ffq_mlp_gate_up_wq
        ("mlp", dict(), ARG, NEEDS_SCRATCH),
        ("mlp", dict(shape=_with(TILES, 0, -1)), ARG, "negative extent"),
        ("mlp", dict(split=-1), ARG, "negative extent"),
        ("mlp", dict(shape=_with(TILES, 0, 0)), OK, None),
        ("mlp", dict(shape=_with(TILES, 1, 0)), OK, None),
        ("mlp", dict(go=FAKE), ARG, "gate and up need offsets both or neither"),
        ("mlp", dict(uo=FAKE), ARG, "gate and up need offsets both or neither"),
        ("mlp", dict(shape=_with(TILES, 1, 192)), DTYPE, "fused weight-only gate/up: needs N % 128 == 0 and what ffq_linear_wq needs"),
        ("mlp", dict(shape=_with(TILES, 2, 100)), DTYPE, "fused weight-only gate/up: needs N % 128 == 0 and what ffq_linear_wq needs"),
        ("mlp", dict(numel=7), NUMEL, "parameters for"),
        ("mlp", dict(numel=1, group=128), NUMEL, "one parameter pair needs group == K"),
        ("mlp", dict(shape=_with(TILES, 0, 0), x=None), OK, None),
        ("mlp", dict(x=None, go=FAKE), ARG, "NULL buffer"),
        ("mlp", dict(go=FAKE, shape=_with(TILES, 1, 192)), ARG, "gate and up need offsets both or neither"),
        ("mlp", dict(shape=_with(TILES, 1, 192), up=FAKE + 8), DTYPE, "fused weight-only gate/up"),
        ("mlp", dict(shape=_with(TILES, 1, 192), numel=7), DTYPE, "fused weight-only gate/up"),
        ("mlp", dict(up=FAKE + 8, numel=7), DTYPE, "16-byte aligned"),
        ("mlp", dict(numel=7, split=9), NUMEL, "parameters for"),
    ]
    rows += [("mlp", {p: None}, ARG, "NULL buffer") for p in ("x", "gate", "up", "gs", "us", "out")]
    rows += [("mlp", {p: FAKE + 8}, DTYPE, "16-byte aligned") for p in ("x", "gate", "up", "out")]
    return rows


ROWS = _rows()


@pytest.mark.parametrize("name,change,status,text", ROWS, ids=[f"{r[0]}-{i}" for i, r in enumerate(ROWS)])
def test_argument_checks_need_no_device(lib, name, change, status, text):
    assert CALLS[name](lib, **change) == status, (name, change)
    if status != OK:
        assert text in lib.ffq_last_error().decode(), (name, change)


def test_supported(lib):
    ok = lambda *a: lib.ffq_linear_wq_supported(*a)  # noqa: E731
    assert ok(BF16, I8, BF16, 16, 128, 256, 256, 0) == 1 and ok(BF16, I8, F32, 16, 128, 256, 64, 0) == 1
    assert ok(BF16, U8, BF16, 16, 128, 256, 128, 32) == 1 and ok(BF16, U8, BF16, 16, 128, 256, 128, 256) == 1
    for bad in ((F32, I8, BF16, 16, 128, 256, 256, 0), (BF16, I8, I8, 16, 128, 256, 256, 0), (BF16, BF16, BF16, 16, 128, 256, 256, 0),
                (BF16, I8, BF16, 0, 128, 256, 256, 0), (BF16, I8, BF16, 16, 128, 64, 64, 0), (BF16, I8, BF16, 16, 128, 160, 160, 0),
                (BF16, I8, BF16, 16, 128, 256, 0, 0), (BF16, I8, BF16, 16, 128, 256, 96, 0), (BF16, I8, BF16, 16, 128, 256, 32, 0),
                (BF16, I8, BF16, 1 << 31, 128, 256, 256, 0), (BF16, I8, BF16, 16, 128, 1 << 23, 1 << 23, 0), (BF16, I8, BF16, 16, 128, 256, 256, 128),
                (BF16, U8, BF16, 16, 128, 256, 256, 0), (BF16, U8, BF16, 16, 128, 256, 256, 16), (BF16, U8, BF16, 16, 128, 256, 256, 96),
                (BF16, U8, BF16, 16, 128, 256, 256, 512)):
        assert ok(*bad) == 0, bad


# ---- the wrappers of ops/wq.py on host tensors, the oracle standing in for the library --------------------------------------------
M_, K_ = 4, 128
PACKED_TEXT = "packed weights are the uint8 output of pack_int4 for an [N, K] weight"


def _codes(n, k=K_, dtype=torch.int8):
    return torch.zeros(n, k, dtype=dtype)


def _wrapper(name, **change):
    """Call wrapper `name` on small valid operands with `change` applied."""
    x = torch.zeros(M_, K_, dtype=torch.bfloat16)
    if name == "linear_wq":
        call = dict(x=x, w_codes=_codes(8), w_scale=torch.ones(8), w_offset=None)
    elif name == "linear_wq_multi":
        call = dict(x=x, w_codes=[_codes(256), _codes(8)], w_scales=[torch.ones(256), torch.ones(8)], w_offsets=[None, None])
    else:
        call = dict(x=x, gate_codes=_codes(128), up_codes=_codes(128), gate_scale=torch.ones(128), gate_offset=None, up_scale=torch.ones(128), up_offset=None)
    call.update(change)
    return getattr(ff.ops, name)(**call)


RAISES = [
    ("linear_wq", dict(w_codes=_codes(8, K_ // 2), pack_block=32), PACKED_TEXT),  # int8 where packed nibbles are announced
    ("linear_wq", dict(w_codes=_codes(3, 50, torch.uint8), pack_block=32), PACKED_TEXT),  # 300 codes are no rows of 128
    ("linear_wq", dict(w_codes=_codes(8, 64)), "mat1 and mat2 shapes cannot be multiplied (4x128 and 8x64^T)"),
    ("linear_wq", dict(w_codes=torch.zeros(8 * K_, dtype=torch.int8)), "linear_wq expects a [N, K] weight"),
    ("linear_wq", dict(w_offset=torch.zeros(3)), "scale has 8 entries, offset 3"),
    ("mlp_gate_up_wq", dict(gate_codes=_codes(128, K_ // 2), up_codes=_codes(128, K_ // 2), pack_block=32), PACKED_TEXT),
    ("mlp_gate_up_wq", dict(gate_codes=_codes(128, 64), up_codes=_codes(128, 64)), "mlp_gate_up_wq expects [N, K] weights"),
    ("mlp_gate_up_wq", dict(up_codes=_codes(256)), "gate and up weights differ in shape or dtype"),
    ("mlp_gate_up_wq", dict(up_codes=_codes(128, K_, torch.uint8)), "gate and up weights differ in shape or dtype"),
    ("mlp_gate_up_wq", dict(up_scale=torch.ones(1)), "gate and up parameters differ in count"),
    ("mlp_gate_up_wq", dict(gate_offset=torch.zeros(128), up_offset=torch.zeros(1)), "gate and up parameters differ in count"),
]


@pytest.mark.parametrize("name,change,text", RAISES, ids=[f"{r[0]}-{i}" for i, r in enumerate(RAISES)])
def test_the_wrappers_raise_as_before(oracle_backend, name, change, text):
    with pytest.raises(RuntimeError) as caught:
        _wrapper(name, **change)
    assert type(caught.value) is RuntimeError and str(caught.value) == text


DECLINES = [
    # (dtypes the oracle's ffq_linear_wq_supported declines too: it stands in for the library here and admits more than the kernels)
    ("linear_wq", dict(x=torch.zeros(M_, K_, dtype=torch.int32))),
    ("linear_wq", dict(x=torch.zeros(M_, K_, dtype=torch.float64))),
    ("linear_wq", dict(w_codes=_codes(8, K_, torch.int16))),
    ("linear_wq", dict(out_dtype=torch.int8)),
    ("linear_wq", dict(group=96)),
    ("linear_wq_multi", dict(w_codes=[_codes(256)], w_scales=[torch.ones(256)], w_offsets=[None])),  # one matrix
    ("linear_wq_multi", dict(w_codes=[_codes(256)] * 4, w_scales=[torch.ones(256)] * 4, w_offsets=[None] * 4)),
    ("linear_wq_multi", dict(w_scales=[torch.ones(256)])),
    ("linear_wq_multi", dict(w_codes=[_codes(300), _codes(84)], w_scales=[torch.ones(300), torch.ones(84)])),  # a ragged non-last matrix
    ("linear_wq_multi", dict(w_codes=[_codes(256, K_ // 2), _codes(8, K_ // 2)], pack_block=32)),  # packed, of the wrong dtype
    ("linear_wq_multi", dict(w_codes=[_codes(256), _codes(8, 64)])),  # K mismatch
    ("linear_wq_multi", dict(w_codes=[_codes(256), _codes(8, K_, torch.uint8)])),  # two dtypes
    ("linear_wq_multi", dict(x=torch.zeros(M_, K_, dtype=torch.int32))),
    ("linear_wq_multi", dict(w_offsets=[torch.zeros(256), None])),  # offsets for some
    ("linear_wq_multi", dict(w_scales=[torch.ones(256), torch.ones(1)])),  # two granularity kinds
    ("linear_wq_multi", dict(w_scales=[torch.ones(256), torch.ones(7)])),
    ("linear_wq_multi", dict(w_offsets=[torch.zeros(256), torch.zeros(7)])),
    ("linear_wq_multi", dict(w_scales=[torch.ones(1), torch.ones(1)], group=64)),  # one pair per matrix needs group == K
    ("mlp_gate_up_wq", dict(gate_codes=_codes(192), up_codes=_codes(192), gate_scale=torch.ones(192), up_scale=torch.ones(192))),  # N % 128
    ("mlp_gate_up_wq", dict(x=torch.zeros(M_, K_))),
    ("mlp_gate_up_wq", dict(gate_offset=torch.zeros(128))),  # offsets on one side only
    ("mlp_gate_up_wq", dict(group=96)),
]


@pytest.mark.parametrize("name,change", DECLINES, ids=[f"{r[0]}-{i}" for i, r in enumerate(DECLINES)])
def test_the_wrappers_decline_as_before(oracle_backend, name, change):
    assert _wrapper(name, **change) is None
