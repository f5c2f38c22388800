"""The launch routes of the quantizer core (csrc/ffq_quantize.hip, ffq_dequantize.hip, ffq_minmax.hip, ffq_pack.hip,
ffq_backward.hip), one small call per route and per side of each threshold, through the C ABI on device tensors.

``cases()`` is an ordered list of (name, call); ``call(lib)`` returns the output tensors of one launch sequence and
``digest(tensors)`` is the SHA-256 of their bytes. Inputs come from closed integer formulas (exact in bf16 / fp16 / fp32), so a
digest depends on the kernels and on nothing else; float inputs carry a NaN, +Inf, -Inf and -0.0. Outputs and workspaces are
pre-filled with a byte pattern, so bytes a route leaves unwritten are part of the digest. tests/golden/gen_quantizer_routes.py
records the digests, tests/test_quantizer_routes_gpu.py compares them."""

from __future__ import annotations

import ctypes
import hashlib

import torch

from fastforward_amd._cabi import Tiling

DEV = "cuda"
TAG = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2, torch.float64: 3, torch.int8: 4, torch.int16: 5, torch.int32: 6, torch.int64: 7,
       torch.uint8: 8}
SHORT = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16", torch.float64: "f64", torch.int8: "i8", torch.int16: "i16",
         torch.int32: "i32", torch.uint8: "u8"}
f32, bf16, f16, f64, i8, i16, i32, u8 = torch.float32, torch.bfloat16, torch.float16, torch.float64, torch.int8, torch.int16, torch.int32, torch.uint8


# ---- operands from closed formulas ---------------------------------------------------------------------------------------------------------
def _mix(n, seed):
    i = torch.arange(n, dtype=torch.int64)
    return (i * 40503 + (i >> 3) * 7 + (i >> 7) * 31 + seed * 977) % 255 - 127  # [-127, 127]: 7 bits, exact in every float type here


def data(n, dtype, seed=0, specials=True, lead=0):
    """n values m / 16 (|m| <= 127) with a NaN, +Inf, -Inf and -0.0 planted; lead > 0: a view that starts `lead` elements into its buffer"""
    x = _mix(n, seed).to(torch.float32) / 16
    if specials and n > 9 and dtype.is_floating_point:
        x[3], x[5], x[7], x[9] = float("nan"), float("inf"), float("-inf"), -0.0
    buf = torch.zeros(n + lead, dtype=dtype)
    buf[lead:] = x.to(dtype)
    return buf.to(DEV)[lead:]


def codes(n, dtype, seed=0, lo=-127, lead=0):
    buf = torch.zeros(n + lead, dtype=dtype)
    buf[lead:] = (_mix(n, seed).clamp(min=lo)).to(dtype)
    return buf.to(DEV)[lead:]


def scales(n, dtype=f32, seed=0):
    i = torch.arange(n, dtype=torch.int64)
    return (((i * 7 + seed) % 13 + 3).to(torch.float32) / 64).to(dtype).to(DEV)


def offsets(n, dtype=f32, seed=0):
    i = torch.arange(n, dtype=torch.int64)
    return (((i * 5 + seed) % 9 - 4).to(torch.float32) + 0.25).to(dtype).to(DEV)  # a fraction: the kernels round it


def blank(n, dtype, lead=0):
    """an output: every byte 0x5A before the call"""
    return torch.full(((n + lead) * torch.empty((), dtype=dtype).element_size(),), 0x5A, dtype=u8, device=DEV).view(dtype)[lead:]


def scratch(nbytes):
    return torch.full((max(int(nbytes), 16),), 0xFF, dtype=u8, device=DEV)


def ticket():
    return torch.zeros(4, dtype=i32, device=DEV)


def ptr(t):
    return None if t is None else t.data_ptr()


def tiling(shape, tile):
    return ctypes.byref(Tiling.make(shape, tile))


def numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def ntiles(shape, tile):
    return numel([s // t for s, t in zip(shape, tile)])


def ok(lib, status):
    assert status == 0, f"status {status}: {lib.ffq_last_error().decode()}"
    torch.cuda.synchronize()


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().view(u8).numpy().tobytes())
    return h.hexdigest()


# ---- A1 / A2 ---------------------------------------------------------------------------------------------------------------------------------
def affine(lib, quantize, shape, tile, din, dout, offset=True, bits=8.0, param_dt=f32, lead=0, broadcast=False):
    n, nt = numel(shape), ntiles(shape, tile)
    x = data(n, din, seed=n, lead=lead) if quantize else codes(n, din, seed=n, lead=lead)
    pn = 1 if broadcast else nt
    s, o = scales(pn, param_dt, seed=nt), (offsets(pn, param_dt, seed=nt) if offset else None)
    out = blank(n, dout, lead=lead)
    if quantize:
        ok(lib, lib.ffq_quantize_by_tile(ptr(x), TAG[din], ptr(s), TAG[param_dt], pn, ptr(o), TAG[param_dt], pn, tiling(shape, tile), bits, ptr(out), TAG[dout], None))
    else:
        ok(lib, lib.ffq_dequantize_by_tile(ptr(x), TAG[din], ptr(s), TAG[param_dt], pn, ptr(o), TAG[param_dt], pn, tiling(shape, tile), ptr(out), TAG[dout], None))
    return [out]


# (name, shape, tile): the layouts and the sizes at which the streaming route changes
AFFINE_SHAPES = [
    ("scalar", (4096,), (4096,)),                    # one tile, whole chunks, one block
    ("scalar two blocks + tail", (4805,), (4805,)),  # 300 chunks of 16 (600 of 8): two blocks, and a tail for the generic kernel
    ("scalar 12", (12,), (12,)),                     # no chunk of 16; one chunk of 8 and a tail
    ("scalar 7", (7,), (7,)),                        # no chunk at all: all generic
    ("rows 64", (8, 64), (1, 64)),                   # run % 16 == 0
    ("rows 24", (8, 24), (1, 24)),                   # run % 16 != 0, run % 8 == 0
    ("rows 12", (8, 12), (1, 12)),                   # run % 8 != 0: generic
    ("channel inner 32", (2, 4, 32), (2, 1, 32)),    # inner % 16 == 0
    ("channel inner 8", (2, 4, 8), (2, 1, 8)),       # inner % 16 != 0, inner % 8 == 0
    ("channel inner 5", (2, 4, 5), (2, 1, 5)),       # generic
    ("columns 40 x 16", (40, 16), (40, 1)),          # inner == 1, channels % 8 == 0: the columns kernel, 5 row groups
    ("columns 3 x 8", (3, 8), (3, 1)),               # one row group
    ("columns 16 x 12", (16, 12), (16, 1)),          # channels % 8 != 0: generic
    ("2-d tiles", (8, 8), (4, 4)),                   # N-d tile grid: generic
]


def affine_cases():
    out = []
    for quantize, name, ins, outs in ((True, "quantize", (bf16, f32, f16), (i8, bf16, i32, i16, f32, f16)), (False, "dequantize", (i8, i16, i32, bf16), (bf16, f32, f16))):
        for k, (what, shape, tile) in enumerate(AFFINE_SHAPES):
            for j, dout in enumerate(outs):
                din = ins[(k + j) % len(ins)]
                for offset in (True, False):
                    if (j + k) % 2 == int(offset) and j >= 2:
                        continue  # (the wide containers take each shape with or without an offset, alternating)
                    tag = f"{name} {SHORT[din]}->{SHORT[dout]} {what}{' offset' if offset else ''}"
                    out.append((tag, lambda lib, q=quantize, s=shape, t=tile, a=din, b=dout, o=offset: affine(lib, q, s, t, a, b, o)))
        a, b = (bf16, i8) if quantize else (i8, bf16)
        for offset in (True, False):
            suffix = " offset" if offset else ""
            out += [
                (f"{name} misaligned view{suffix}", lambda lib, q=quantize, a=a, b=b, o=offset: affine(lib, q, (4096,), (4096,), a, b, o, lead=1)),
                (f"{name} bf16 parameters{suffix}", lambda lib, q=quantize, a=a, b=b, o=offset: affine(lib, q, (8, 64), (1, 64), a, b, o, param_dt=bf16)),
                (f"{name} one parameter for 8 runs{suffix}", lambda lib, q=quantize, a=a, b=b, o=offset: affine(lib, q, (8, 64), (1, 64), a, b, o, broadcast=True)),
                (f"{name} one parameter for 16 columns{suffix}", lambda lib, q=quantize, a=a, b=b, o=offset: affine(lib, q, (40, 16), (40, 1), a, b, o, broadcast=True)),
                (f"{name} one parameter for 4 channels{suffix}", lambda lib, q=quantize, a=a, b=b, o=offset: affine(lib, q, (2, 4, 32), (2, 1, 32), a, b, o, broadcast=True)),
            ]
        if quantize:
            out += [
                ("quantize 4 bits", lambda lib: affine(lib, True, (8, 64), (1, 64), bf16, i8, True, bits=4.0)),
                ("quantize 3.5 bits", lambda lib: affine(lib, True, (8, 64), (1, 64), bf16, i8, True, bits=3.5)),  # fractional: generic
                ("quantize f64 data", lambda lib: affine(lib, True, (8, 64), (1, 64), f64, i8, True)),
            ]
    return out


# ---- min/max, A5 -----------------------------------------------------------------------------------------------------------------------------
def minmax(lib, shape, tile, dt, accumulate=False, with_ticket=False, lead=0):
    n, nt = numel(shape), ntiles(shape, tile)
    x = data(n, dt, seed=n + 1, lead=lead)
    mn, mx = (data(nt, dt, seed=5, specials=False), data(nt, dt, seed=6, specials=False)) if accumulate else (blank(nt, dt), blank(nt, dt))
    flags, tk = torch.zeros(1, dtype=i32, device=DEV), ticket() if with_ticket else None
    ws = scratch(lib.ffq_minmax_workspace_bytes(tiling(shape, tile), TAG[dt]))
    ok(lib, lib.ffq_minmax_by_tile(ptr(x), TAG[dt], tiling(shape, tile), ptr(mn), ptr(mx), int(accumulate), ptr(flags), ptr(ws), ws.numel(), ptr(tk), None))
    return [mn, mx, flags] + ([tk] if with_ticket else [])


def running_step(lib, shape, tile, dt, symmetric, with_ticket):
    n, nt = numel(shape), ntiles(shape, tile)
    x = data(n, dt, seed=n + 2, specials=False)
    mn, mx = data(nt, dt, seed=5, specials=False), data(nt, dt, seed=6, specials=False)
    flags, tk = torch.zeros(1, dtype=i32, device=DEV), ticket() if with_ticket else None
    s, o = blank(nt, f32), blank(nt, f32)
    ws = scratch(lib.ffq_minmax_workspace_bytes(tiling(shape, tile), TAG[dt]))
    ok(lib, lib.ffq_running_minmax_step(ptr(x), TAG[dt], tiling(shape, tile), ptr(mn), ptr(mx), ptr(flags), 8.0, int(symmetric), 1, ptr(s), 0, ptr(o), 0,
                                        ptr(ws), ws.numel(), ptr(tk), None))
    return [mn, mx, flags, s, o]


def range_params(lib, nt, dt, symmetric, one_sided, workspace=True, positive=False, out_dt=f32):
    lo = data(nt, dt, seed=11, specials=False)
    if positive:
        lo = lo.abs()
    hi = (lo.float() + scales(nt, f32, seed=3) * 64).to(dt)
    s, o = blank(nt, out_dt), blank(nt, out_dt)
    need = lib.ffq_parameters_for_range_workspace_bytes(nt, int(symmetric), int(one_sided))
    ws = scratch(need) if workspace and need else None
    ok(lib, lib.ffq_parameters_for_range(ptr(lo), ptr(hi), TAG[dt], nt, 8.0, int(symmetric), int(one_sided), ptr(s), TAG[out_dt], ptr(o), TAG[out_dt], ptr(ws),
                                         ws.numel() if ws is not None else 0, None))
    return [s, o]


def minmax_cases():
    out = []
    for dt in (bf16, f32):
        d = SHORT[dt]
        for acc in (False, True):
            a = " accumulate" if acc else ""
            out += [
                (f"minmax {d} scalar two launches{a}", lambda lib, dt=dt, acc=acc: minmax(lib, (5003,), (5003,), dt, acc)),
                (f"minmax {d} scalar ticket{a}", lambda lib, dt=dt, acc=acc: minmax(lib, (5003,), (5003,), dt, acc, with_ticket=True)),
                (f"minmax {d} rows split{a}", lambda lib, dt=dt, acc=acc: minmax(lib, (3, 1040), (1, 1040), dt, acc)),
                (f"minmax {d} columns{a}", lambda lib, dt=dt, acc=acc: minmax(lib, (40, 16), (40, 1), dt, acc)),
                (f"minmax {d} generic channels{a}", lambda lib, dt=dt, acc=acc: minmax(lib, (2, 4, 5), (2, 1, 5), dt, acc)),
                (f"minmax {d} misaligned rows{a}", lambda lib, dt=dt, acc=acc: minmax(lib, (6, 64), (1, 64), dt, acc, lead=1)),
            ]
        for chunks in (1, 2, 3, 5, 9, 17, 33, 64, 65):  # 1, 2, 4, ..., 64 lanes per tile; 65 chunks: the split kernel
            out.append((f"minmax {d} rows {chunks} chunks", lambda lib, dt=dt, c=chunks: minmax(lib, (6, 8 * c), (1, 8 * c), dt, c % 2 == 0)))
        out += [
            (f"minmax {d} scalar 5", lambda lib, dt=dt: minmax(lib, (5,), (5,), dt)),
            (f"minmax {d} scalar two blocks of the ticket form", lambda lib, dt=dt: minmax(lib, (8 * 256 * 8 + 8,), (8 * 256 * 8 + 8,), dt, with_ticket=True)),
            (f"minmax {d} rows 12", lambda lib, dt=dt: minmax(lib, (6, 12), (1, 12), dt)),
            (f"minmax {d} columns 3 x 8", lambda lib, dt=dt: minmax(lib, (3, 8), (3, 1), dt)),
            (f"minmax {d} columns 1100 x 8", lambda lib, dt=dt: minmax(lib, (1100, 8), (1100, 1), dt)),  # more than 64 row groups of 16: capped
        ]
    out += [
        ("minmax f16 rows 4 chunks", lambda lib: minmax(lib, (6, 32), (1, 32), f16)),
        ("minmax f64 rows", lambda lib: minmax(lib, (6, 64), (1, 64), f64)),
        ("minmax i8 scalar", lambda lib: minmax(lib, (4096,), (4096,), i8)),
    ]
    for sym in (False, True):
        s = "symmetric" if sym else "asymmetric"
        out += [
            (f"running step {s} one tile ticket", lambda lib, sym=sym: running_step(lib, (5003,), (5003,), bf16, sym, True)),
            (f"running step {s} one tile", lambda lib, sym=sym: running_step(lib, (5003,), (5003,), bf16, sym, False)),
            (f"running step {s} rows", lambda lib, sym=sym: running_step(lib, (6, 64), (1, 64), bf16, sym, True)),
        ]
    for nt in (1, 16, 8192, 8193):  # kRangeGridTiles = 8192: the grid form starts above it
        for sym, one in ((False, True), (True, True), (True, False)):
            tag = f"parameters {nt} tiles {'symmetric' if sym else 'asymmetric'}{' one-sided allowed' if one else ''}"
            out.append((tag, lambda lib, nt=nt, sym=sym, one=one: range_params(lib, nt, f32, sym, one)))
    out += [
        ("parameters 8193 tiles symmetric all positive", lambda lib: range_params(lib, 8193, f32, True, True, positive=True)),
        ("parameters 8193 tiles symmetric no scratch", lambda lib: range_params(lib, 8193, f32, True, True, workspace=False)),
        ("parameters 8193 tiles bf16 ranges", lambda lib: range_params(lib, 8193, bf16, True, True)),
        ("parameters 8193 tiles bf16 out", lambda lib: range_params(lib, 8193, f32, False, True, out_dt=bf16)),
        ("parameters 8193 tiles f64 ranges", lambda lib: range_params(lib, 8193, f64, True, True)),
        ("parameters 16 tiles all positive", lambda lib: range_params(lib, 16, bf16, True, True, positive=True)),
    ]
    return out


# ---- dynamic quantize and the running form -------------------------------------------------------------------------------------------------
SIGNS = ("mixed", "positive", "some rows positive")


def _signed(x, shape, signs):
    if signs == "positive":
        return x.abs()
    if signs == "some rows positive":
        rows = x.view(shape[0], -1)
        rows[::2] = rows[::2].abs()
    return x


def dynamic(lib, shape, tile, din, dout, symmetric=False, one_sided=True, with_ticket=True, signs="mixed", specials=False, lead=0):
    n, nt = numel(shape), ntiles(shape, tile)
    x = _signed(data(n, din, seed=n + 3, specials=specials, lead=lead), shape, signs)
    out, s, o, tk = blank(n, dout, lead=lead), blank(nt, f32), blank(nt, f32), ticket() if with_ticket else None
    ws = scratch(lib.ffq_quantize_dynamic_workspace_bytes(tiling(shape, tile), TAG[din]))
    ok(lib, lib.ffq_quantize_dynamic_by_tile(ptr(x), TAG[din], tiling(shape, tile), 8.0, int(symmetric), int(one_sided), ptr(out), TAG[dout], ptr(s), ptr(o),
                                             ptr(ws), ws.numel(), ptr(tk), None))
    return [out, s, o] + ([tk] if with_ticket else [])


def running_quantize(lib, shape, tile, din, dout, symmetric, signs="mixed"):
    n, nt = numel(shape), ntiles(shape, tile)
    x = _signed(data(n, din, seed=n + 4, specials=False), shape, signs)
    mn, mx = data(nt, din, seed=5, specials=False) / 8, data(nt, din, seed=6, specials=False) / 8
    if signs != "mixed":
        mn = mn.abs()
    out, s, o, tk, flags = blank(n, dout), blank(nt, f32), blank(nt, f32), ticket(), torch.zeros(1, dtype=i32, device=DEV)
    ok(lib, lib.ffq_running_minmax_quantize(ptr(x), TAG[din], tiling(shape, tile), ptr(mn), ptr(mx), ptr(flags), 8.0, int(symmetric), 1, ptr(s), ptr(o), ptr(out),
                                            TAG[dout], ptr(tk), None))
    return [out, s, o, mn, mx, flags, tk]


def dynamic_cases():
    out = []
    # the ladder of launch_dynamic_rows: a rung per chunk count 1, 2, 4, ..., 512, then 4 * kBlock = 1024; above it the composed route
    for chunks in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025):
        dout, e, rows = (i8, 16, 5) if chunks <= 33 else (bf16, 8, 2)
        out.append((f"dynamic {chunks} chunks bf16->{SHORT[dout]}", lambda lib, c=chunks, e=e, r=rows, d=dout: dynamic(lib, (r, e * c), (1, e * c), bf16, d, specials=c % 3 == 0)))
    for signs in SIGNS:  # the global one-sided question: guess, then settle
        out += [
            (f"dynamic symmetric {signs} 4 chunks", lambda lib, g=signs: dynamic(lib, (6, 64), (1, 64), bf16, i8, True, signs=g)),
            (f"dynamic symmetric {signs} 300 chunks", lambda lib, g=signs: dynamic(lib, (4, 2400), (1, 2400), f32, bf16, True, signs=g)),
            (f"dynamic symmetric {signs} no ticket", lambda lib, g=signs: dynamic(lib, (6, 64), (1, 64), bf16, i8, True, with_ticket=False, signs=g)),
            (f"dynamic symmetric {signs} one tile", lambda lib, g=signs: dynamic(lib, (5003,), (5003,), bf16, i8, True, signs=g)),
            (f"dynamic symmetric {signs} one tile no ticket", lambda lib, g=signs: dynamic(lib, (5003,), (5003,), bf16, i8, True, with_ticket=False, signs=g)),
            (f"running quantize symmetric {signs}", lambda lib, g=signs: running_quantize(lib, (6, 64), (1, 64), bf16, i8, True, g)),
            (f"running quantize symmetric {signs} 300 chunks", lambda lib, g=signs: running_quantize(lib, (4, 2400), (1, 2400), bf16, bf16, True, g)),
        ]
    out += [
        ("dynamic symmetric two-sided only", lambda lib: dynamic(lib, (6, 64), (1, 64), bf16, i8, True, one_sided=False, signs="positive")),
        ("dynamic one tile", lambda lib: dynamic(lib, (5003,), (5003,), bf16, i8)),
        ("dynamic one tile no ticket", lambda lib: dynamic(lib, (5003,), (5003,), f32, i8, with_ticket=False)),
        ("dynamic columns", lambda lib: dynamic(lib, (40, 16), (40, 1), bf16, i8)),
        ("dynamic misaligned rows", lambda lib: dynamic(lib, (6, 64), (1, 64), bf16, i8, lead=1)),
        ("dynamic run % 16", lambda lib: dynamic(lib, (6, 24), (1, 24), bf16, i8)),
        ("dynamic f16->f32 rows", lambda lib: dynamic(lib, (6, 64), (1, 64), f16, f32, specials=True)),
        ("dynamic bf16->i16 rows", lambda lib: dynamic(lib, (6, 64), (1, 64), bf16, i16)),
        ("running quantize asymmetric", lambda lib: running_quantize(lib, (6, 64), (1, 64), bf16, i8, False)),
        ("running quantize asymmetric f32 200 chunks", lambda lib: running_quantize(lib, (3, 1600), (1, 1600), f32, bf16, False)),
    ]
    return out


# ---- int4 ------------------------------------------------------------------------------------------------------------------------------------
def pack(lib, n, block, dt, lead=0):
    c = codes(n, dt, seed=block, lead=lead) if not dt.is_floating_point else (codes(n, i8, seed=block).clamp(-8, 7).to(dt))
    packed = blank(n // 2, u8)
    ok(lib, lib.ffq_pack_int4(ptr(c), TAG[dt], n, block, ptr(packed), None))
    back = blank(n, dt, lead=lead)
    ok(lib, lib.ffq_unpack_int4(ptr(packed), n, block, ptr(back), TAG[dt], None))
    return [packed, back]


def fused_int4(lib, shape, tile, block, dt, offset):
    n, nt = numel(shape), ntiles(shape, tile)
    x, s, o = data(n, dt, seed=block + n), scales(nt, seed=2) * 8, (offsets(nt, seed=2) if offset else None)
    packed = blank(n // 2, u8)
    ok(lib, lib.ffq_quantize_pack_int4(ptr(x), TAG[dt], ptr(s), nt, ptr(o), nt, tiling(shape, tile), block, ptr(packed), None))
    back = blank(n, dt)
    ok(lib, lib.ffq_unpack_dequantize_int4(ptr(packed), ptr(s), nt, ptr(o), nt, tiling(shape, tile), block, ptr(back), TAG[dt], None))
    return [packed, back]


def pack_cases():
    out = []
    for dt in (i8, bf16, f16, f32):
        out += [
            (f"pack {SHORT[dt]} words", lambda lib, dt=dt: pack(lib, 4096 + 64, 64, dt)),
            (f"pack {SHORT[dt]} block 8", lambda lib, dt=dt: pack(lib, 4096 + 8, 8, dt)),
            (f"pack {SHORT[dt]} block 12", lambda lib, dt=dt: pack(lib, 4092, 12, dt)),  # block % 8 != 0: generic
        ]
    out += [
        ("pack i8 off a word", lambda lib: pack(lib, 4096, 64, i8, lead=1)),  # a pointer off 4 bytes: generic
        ("pack bf16 off a word", lambda lib: pack(lib, 4096, 64, bf16, lead=1)),
        ("pack i32 codes", lambda lib: pack(lib, 4096, 64, i32)),  # no word kernel for this container
    ]
    for dt in (bf16, f16, f32):  # unpack + dequantize: 8 elements of each half per lane for 16-bit outputs, 16 for f32
        for offset in (True, False):
            suffix = " offset" if offset else ""
            out += [
                (f"fused int4 {SHORT[dt]} rows block 64{suffix}", lambda lib, dt=dt, o=offset: fused_int4(lib, (40, 64), (1, 64), 64, dt, o)),
                (f"fused int4 {SHORT[dt]} one tile block 32{suffix}", lambda lib, dt=dt, o=offset: fused_int4(lib, (4128,), (4128,), 32, dt, o)),
                (f"fused int4 {SHORT[dt]} rows 16 block 128{suffix}", lambda lib, dt=dt, o=offset: fused_int4(lib, (256, 16), (1, 16), 128, dt, o)),
            ]
    return out


# ---- backward --------------------------------------------------------------------------------------------------------------------------------
def backward(lib, shape, tile, dt, offset, lead=0, broadcast=False):
    n, nt = numel(shape), ntiles(shape, tile)
    x, g = data(n, dt, seed=n + 5, specials=False, lead=lead), data(n, dt, seed=n + 6, specials=False, lead=lead)
    pn = 1 if broadcast else nt
    s, o = scales(pn, seed=4), (offsets(pn, seed=4) if offset else None)
    dx, ds, do = blank(n, dt, lead=lead), blank(nt, f32), (blank(nt, f32) if offset else None)
    ws = scratch(lib.ffq_quantize_backward_workspace_bytes(tiling(shape, tile)))
    ok(lib, lib.ffq_quantize_by_tile_backward(ptr(x), ptr(g), TAG[dt], ptr(s), pn, ptr(o), pn, tiling(shape, tile), 4.0, ptr(dx), ptr(ds), ptr(do), ptr(ws),
                                              ws.numel(), None))
    return [dx, ds] + ([do] if offset else [])


BACKWARD_SHAPES = [
    ("small by tile", (8, 64), (1, 64)),                   # a few small tiles: one launch
    ("small, a lane per tile", (16, 8), (1, 8)),           # fewer than 64 elements per tile
    ("by tile, odd size", (3, 100), (1, 100)),             # numel % 8 != 0
    ("by tile, strided channels", (3, 100), (3, 1)),       # 100 tiles of 3 elements, not contiguous
    ("streaming, a chunk per part, 8 units", (2, 64), (1, 64)),       # per_block 0, finalize of <= 32 units
    ("streaming, a chunk per part, 32 units", (2, 256), (1, 256)),
    ("streaming, a chunk per part, 33 units", (2, 264), (1, 264)),    # the wide finalize
    ("streaming, a block per part", (2, 2048), (1, 2048)),            # per_block 1, one unit
    ("streaming, one tile", (4096,), (4096,)),                        # per_block 1, two units
]


def backward_cases():
    out = []
    for what, shape, tile in BACKWARD_SHAPES:
        for dt in (f32, bf16):
            for offset in (True, False):
                out.append((f"backward {SHORT[dt]} {what}{' offset' if offset else ''}", lambda lib, s=shape, t=tile, dt=dt, o=offset: backward(lib, s, t, dt, o)))
    out += [
        ("backward f16 streaming", lambda lib: backward(lib, (2, 2048), (1, 2048), f16, True)),
        ("backward bf16 misaligned", lambda lib: backward(lib, (2, 2048), (1, 2048), bf16, True, lead=1)),      # by tile
        ("backward bf16 one scale for two tiles", lambda lib: backward(lib, (2, 2048), (1, 2048), bf16, True, broadcast=True)),  # by tile
    ]
    return out


def cases():
    return affine_cases() + minmax_cases() + dynamic_cases() + pack_cases() + backward_cases()
