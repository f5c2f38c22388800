"""Generate quantizer_refusals.json: what the quantizer core's entry points answer to every call they refuse, word for word.

    python tests/golden/gen_quantizer_refusals.py <path to libffq_hip.so> [output file]

Run on the build of the commit whose statuses, check order and wording are to be pinned (the file in the tree was taken from the
parent of the commit that added it, before the host halves of ffq_quantize.hip, ffq_dequantize.hip, ffq_minmax.hip, ffq_pack.hip
and ffq_backward.hip were restated). One record per call of ``calls()``:

    {"call": "<entry point>: <what is wrong>", "status": <FFQ status>, "message": <the whole ffq_last_error() text, "" for FFQ_OK>}

Every call is answered on the host, before anything is launched: the buffers are made-up addresses that nothing reads (``A``:
16-byte aligned, ``A4``: 4-byte aligned only). A call named "a + b" breaks two rules at once: which of the two it
reports pins the order of the checks. tests/test_quantizer_refusals_cpu.py compares the tree with the file, record for record."""

from __future__ import annotations

import ctypes
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

F32, BF16, F16, F64, I8, I16, I32, I64, U8, BAD = 0, 1, 2, 3, 4, 5, 6, 7, 8, 99
A, A4, B, C, D, E, G = 0x10000, 0x10004, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
BIG = 1 << 40  # a workspace size that is never the reason


def T(shape, tile):
    from fastforward_amd._cabi import Tiling

    return ctypes.byref(Tiling.make(shape, tile))


def rank(ndim):
    from fastforward_amd._cabi import Tiling

    t = Tiling()
    t.ndim = ndim
    return ctypes.byref(t)


ONE = lambda: T((4, 64), (4, 64))       # one tile
ROWS = lambda: T((4, 64), (1, 64))      # four contiguous runs
CHAN = lambda: T((4, 64), (4, 1))       # one channel per column
EMPTY = lambda: T((0, 64), (1, 64))
NODIV = lambda: T((4, 6), (1, 4))


def _quantize(name, bits_first):
    """A1 and A2 share their prologue; A1 has num_bits and the container check, A2 the integer-only refusal."""
    def call(lib, data=A, ddt=BF16, scale=B, sdt=F32, sn=4, offset=None, odt=F32, on=4, tiling=ROWS, bits=8.0, out=C, out_dt=I8):
        if bits_first:
            return lib.ffq_quantize_by_tile(data, ddt, scale, sdt, sn, offset, odt, on, tiling(), bits, out, out_dt, None)
        return lib.ffq_dequantize_by_tile(data, ddt, scale, sdt, sn, offset, odt, on, tiling(), out, out_dt, None)

    q = dict(ddt=BF16, out_dt=I8) if bits_first else dict(ddt=I8, out_dt=BF16)
    rows = [
        ("tile does not divide", lambda lib: call(lib, tiling=NODIV, **q)),
        ("rank too large", lambda lib: call(lib, tiling=lambda: rank(99), **q)),
        ("negative rank", lambda lib: call(lib, tiling=lambda: rank(-1), **q)),
        ("tiling NULL", lambda lib: call(lib, tiling=lambda: None, **q)),
        ("negative extent", lambda lib: call(lib, tiling=lambda: T((-4, 64), (1, 64)), **q)),
        ("tile extent zero", lambda lib: call(lib, tiling=lambda: T((4, 64), (0, 64)), **q)),
        ("bad data tag", lambda lib: call(lib, **{**q, "ddt": BAD})),
        ("bad scale tag", lambda lib: call(lib, sdt=BAD, **q)),
        ("bad out tag", lambda lib: call(lib, **{**q, "out_dt": BAD})),
        ("bad offset tag", lambda lib: call(lib, offset=D, odt=BAD, **q)),
        ("bad offset tag without an offset", lambda lib: call(lib, odt=BAD, tiling=EMPTY, **q)),
        ("wrong scale count", lambda lib: call(lib, sn=3, **q)),
        ("wrong offset count", lambda lib: call(lib, offset=D, on=5, **q)),
        ("wrong scale count on one tile", lambda lib: call(lib, sn=3, tiling=ONE, **q)),
        ("wrong offset count on one tile", lambda lib: call(lib, sn=1, offset=D, on=2, tiling=ONE, **q)),
        ("empty tensor", lambda lib: call(lib, tiling=EMPTY, **q)),
        ("empty tensor + wrong scale count", lambda lib: call(lib, sn=3, tiling=EMPTY, **q)),
        ("NULL data", lambda lib: call(lib, data=None, **q)),
        ("NULL scale", lambda lib: call(lib, scale=None, **q)),
        ("NULL out", lambda lib: call(lib, out=None, **q)),
        ("bad tiling + bad data tag", lambda lib: call(lib, tiling=NODIV, **{**q, "ddt": BAD})),
        ("bad scale tag + wrong scale count", lambda lib: call(lib, sdt=BAD, sn=3, **q)),
        ("wrong scale count + wrong offset count", lambda lib: call(lib, sn=3, offset=D, on=5, **q)),
        ("wrong offset count + NULL data", lambda lib: call(lib, data=None, offset=D, on=5, **q)),
    ]
    if bits_first:
        rows += [
            ("container too small", lambda lib: call(lib, bits=16.0, **q)),
            ("container too small, 2-byte", lambda lib: call(lib, bits=19.0, ddt=BF16, out_dt=I16)),
            ("container too small, bf16", lambda lib: call(lib, bits=12.0, ddt=BF16, out_dt=BF16)),
            ("wrong scale count + container too small", lambda lib: call(lib, sn=3, bits=16.0, **q)),
            ("container too small + NULL data", lambda lib: call(lib, data=None, bits=16.0, **q)),
            ("empty tensor + container too small", lambda lib: call(lib, tiling=EMPTY, bits=16.0, **q)),
        ]
    else:
        rows += [
            ("integer-only", lambda lib: call(lib, ddt=I8, sdt=I32, out_dt=I32)),
            ("integer-only with an integer offset", lambda lib: call(lib, ddt=I8, sdt=I32, offset=D, odt=I8, out_dt=I32)),
            ("wrong scale count + integer-only", lambda lib: call(lib, ddt=I8, sdt=I32, sn=3, out_dt=I32)),
            ("integer-only + NULL data", lambda lib: call(lib, data=None, ddt=I8, sdt=I32, out_dt=I32)),
            ("empty tensor + integer-only", lambda lib: call(lib, ddt=I8, sdt=I32, out_dt=I32, tiling=EMPTY)),
        ]
    return [(f"{name}: {what}", fn) for what, fn in rows]


def _unless_same():
    def call(lib, data=A, dt=BF16, scale=B, offset=None, numel=256, bits=8.0, es=C, eo=None, out=D):
        return lib.ffq_quantize_by_tile_unless_same(data, dt, scale, offset, numel, bits, es, eo, out, None)

    rows = [
        ("negative extent", lambda lib: call(lib, numel=-1)),
        ("container too small", lambda lib: call(lib, bits=11.0)),
        ("empty tensor", lambda lib: call(lib, numel=0)),
        ("NULL data", lambda lib: call(lib, data=None)),
        ("NULL scale", lambda lib: call(lib, scale=None)),
        ("NULL earlier scale", lambda lib: call(lib, es=None)),
        ("NULL out", lambda lib: call(lib, out=None)),
        ("fractional bits", lambda lib: call(lib, bits=7.5)),
        ("ragged chunk", lambda lib: call(lib, numel=250)),
        ("misaligned data", lambda lib: call(lib, data=A4)),
        ("misaligned out", lambda lib: call(lib, out=A4)),
        ("integer data", lambda lib: call(lib, dt=I8)),
        ("too many chunks", lambda lib: call(lib, numel=16 << 32)),
        ("negative extent + container too small", lambda lib: call(lib, numel=-1, bits=11.0)),
        ("container too small + NULL data", lambda lib: call(lib, data=None, bits=11.0)),
        ("NULL data + misaligned out", lambda lib: call(lib, data=None, out=A4)),
        ("empty tensor + container too small", lambda lib: call(lib, numel=0, bits=11.0)),
    ]
    return [(f"ffq_quantize_by_tile_unless_same: {what}", fn) for what, fn in rows]


def _rows_rowsum():
    def call(lib, data=A, dt=BF16, scale=B, offset=None, rows=4, cols=1024, bits=8.0, codes=C, rowsum=D):
        return lib.ffq_quantize_rows_rowsum(data, dt, scale, offset, rows, cols, bits, codes, rowsum, None)

    rows = [
        ("negative rows", lambda lib: call(lib, rows=-1)),
        ("negative cols", lambda lib: call(lib, cols=-1024)),
        ("not bf16", lambda lib: call(lib, dt=F16)),
        ("cols % 1024", lambda lib: call(lib, cols=512)),
        ("container too small", lambda lib: call(lib, bits=11.0)),
        ("fractional bits", lambda lib: call(lib, bits=7.5)),
        ("no rows", lambda lib: call(lib, rows=0)),
        ("NULL data", lambda lib: call(lib, data=None)),
        ("NULL scale", lambda lib: call(lib, scale=None)),
        ("NULL codes", lambda lib: call(lib, codes=None)),
        ("NULL rowsum", lambda lib: call(lib, rowsum=None)),
        ("misaligned data", lambda lib: call(lib, data=A4)),
        ("misaligned codes", lambda lib: call(lib, codes=A4)),
        ("too many elements", lambda lib: call(lib, rows=1 << 26)),
        ("negative rows + not bf16", lambda lib: call(lib, rows=-1, dt=F16)),
        ("not bf16 + cols % 1024", lambda lib: call(lib, dt=F16, cols=512)),
        ("cols % 1024 + container too small", lambda lib: call(lib, cols=512, bits=11.0)),
        ("container too small + fractional bits", lambda lib: call(lib, bits=11.5)),
        ("fractional bits + NULL data", lambda lib: call(lib, bits=7.5, data=None)),
        ("NULL data + misaligned codes", lambda lib: call(lib, data=None, codes=A4)),
        ("misaligned data + too many elements", lambda lib: call(lib, data=A4, rows=1 << 26)),
    ]
    return [(f"ffq_quantize_rows_rowsum: {what}", fn) for what, fn in rows]


def _rows_batch():
    from fastforward_amd._cabi import RowsBatch

    def call(lib, count=2, bits=8.0, dt=BF16, null=False, **members):
        """members: field=(value of member 0, value of member 1); defaults describe two [4, 1024] weights with row sums."""
        if null:
            return lib.ffq_quantize_rows_batch(None, dt, None)
        b = RowsBatch()
        b.count, b.num_bits = count, bits
        fields = dict(data=(A, B), scale=(C, C), offset=(None, None), codes=(D, E), rows=(4, 4), cols=(1024, 1024), rowsum=(G, G))
        fields.update(members)
        for field, values in fields.items():
            for i, v in enumerate(values):
                getattr(b, field)[i] = v
        return lib.ffq_quantize_rows_batch(ctypes.byref(b), dt, None)

    rows = [
        ("NULL batch", lambda lib: call(lib, null=True)),
        ("negative count", lambda lib: call(lib, count=-1)),
        ("count too large", lambda lib: call(lib, count=9)),
        ("empty batch", lambda lib: call(lib, count=0)),
        ("not bf16", lambda lib: call(lib, dt=F32)),
        ("container too small", lambda lib: call(lib, bits=11.0)),
        ("fractional bits", lambda lib: call(lib, bits=7.5)),
        ("row sums for one member only", lambda lib: call(lib, rowsum=(G, None))),
        ("row sums and cols % 1024", lambda lib: call(lib, cols=(1024, 512), rows=(4, 8))),
        ("no rows", lambda lib: call(lib, rows=(4, 0))),
        ("cols % 16", lambda lib: call(lib, cols=(1024, 1000), rowsum=(None, None))),
        ("chunks % block", lambda lib: call(lib, rows=(4, 3), rowsum=(None, None))),
        ("NULL data in member 1", lambda lib: call(lib, data=(A, None))),
        ("NULL scale in member 0", lambda lib: call(lib, scale=(None, C))),
        ("NULL codes in member 1", lambda lib: call(lib, codes=(D, None))),
        ("misaligned data", lambda lib: call(lib, data=(A, A4))),
        ("misaligned codes", lambda lib: call(lib, codes=(A4, E))),
        ("too many elements", lambda lib: call(lib, rows=(4, 1 << 33))),
        ("empty batch + not bf16", lambda lib: call(lib, count=0, dt=F32)),
        ("not bf16 + container too small", lambda lib: call(lib, dt=F32, bits=11.0)),
        ("container too small + fractional bits", lambda lib: call(lib, bits=11.5)),
        ("fractional bits + NULL data", lambda lib: call(lib, bits=7.5, data=(None, B))),
        ("row-sum mix + NULL data in the same member", lambda lib: call(lib, rowsum=(G, None), data=(A, None))),
        ("cols % 1024 + NULL data", lambda lib: call(lib, cols=(512, 1024), rows=(8, 4), data=(None, B))),
        ("ragged member + NULL data", lambda lib: call(lib, rows=(3, 4), data=(None, B))),
        ("NULL data + misaligned codes", lambda lib: call(lib, data=(None, B), codes=(A4, E))),
        ("NULL data in member 1 + misaligned data in member 0", lambda lib: call(lib, data=(A4, None))),
    ]
    return [(f"ffq_quantize_rows_batch: {what}", fn) for what, fn in rows]


def _minmax():
    def call(lib, data=A, dt=BF16, tiling=ROWS, mn=B, mx=C, acc=0, flags=None, ws=D, ws_bytes=BIG, ticket=None):
        return lib.ffq_minmax_by_tile(data, dt, tiling(), mn, mx, acc, flags, ws, ws_bytes, ticket, None)

    big_one = lambda: T((64, 64), (64, 64))
    rows = [
        ("tile does not divide", lambda lib: call(lib, tiling=NODIV)),
        ("bad data tag", lambda lib: call(lib, dt=BAD)),
        ("empty tensor", lambda lib: call(lib, tiling=EMPTY)),
        ("NULL data", lambda lib: call(lib, data=None)),
        ("NULL min", lambda lib: call(lib, mn=None)),
        ("NULL max", lambda lib: call(lib, mx=None)),
        ("workspace too small, one tile", lambda lib: call(lib, tiling=big_one, ws_bytes=8)),
        ("workspace NULL, one tile", lambda lib: call(lib, tiling=big_one, ws=None)),
        ("workspace too small, columns", lambda lib: call(lib, tiling=CHAN, ws_bytes=16)),
        ("workspace too small, generic", lambda lib: call(lib, dt=F64, ws_bytes=16)),
        ("workspace too small, misaligned rows", lambda lib: call(lib, data=A4, ws_bytes=16)),
        ("bad tiling + bad data tag", lambda lib: call(lib, tiling=NODIV, dt=BAD)),
        ("bad data tag + empty tensor", lambda lib: call(lib, dt=BAD, tiling=EMPTY)),
        ("empty tensor + NULL data", lambda lib: call(lib, tiling=EMPTY, data=None)),
        ("NULL data + workspace too small", lambda lib: call(lib, data=None, tiling=big_one, ws_bytes=8)),
    ]
    out = [(f"ffq_minmax_by_tile: {what}", fn) for what, fn in rows]

    def step(lib, data=A, dt=BF16, tiling=ROWS, mn=B, mx=C, flags=None, bits=8.0, sym=0, one=1, scale=D, sdt=F32, offset=E, odt=F32, ws=G,
             ws_bytes=BIG, ticket=None):
        return lib.ffq_running_minmax_step(data, dt, tiling(), mn, mx, flags, bits, sym, one, scale, sdt, offset, odt, ws, ws_bytes, ticket, None)

    rows = [
        ("NULL scale out", lambda lib: step(lib, scale=None)),
        ("bad scale tag", lambda lib: step(lib, sdt=BAD)),
        ("bad offset tag", lambda lib: step(lib, odt=BAD)),
        ("tile does not divide", lambda lib: step(lib, tiling=NODIV)),
        ("bad data tag", lambda lib: step(lib, dt=BAD)),
        ("empty tensor", lambda lib: step(lib, tiling=EMPTY)),
        ("NULL data", lambda lib: step(lib, data=None)),
        ("NULL min", lambda lib: step(lib, mn=None)),
        ("workspace too small", lambda lib: step(lib, tiling=big_one, ws_bytes=8)),
        ("NULL scale out + bad tiling", lambda lib: step(lib, scale=None, tiling=NODIV)),
        ("bad tiling + bad data tag", lambda lib: step(lib, tiling=NODIV, dt=BAD)),
        ("bad data tag + NULL data", lambda lib: step(lib, dt=BAD, data=None)),
    ]
    out += [(f"ffq_running_minmax_step: {what}", fn) for what, fn in rows]

    def fused(lib, data=A, dt=BF16, tiling=ROWS, mn=B, mx=C, flags=None, bits=8.0, sym=0, one=1, scale=D, offset=E, out=G, out_dt=I8, ticket=None):
        return lib.ffq_running_minmax_quantize(data, dt, tiling(), mn, mx, flags, bits, sym, one, scale, offset, out, out_dt, ticket, None)

    rows = [
        ("NULL data", lambda lib: fused(lib, data=None)),
        ("NULL min", lambda lib: fused(lib, mn=None)),
        ("NULL max", lambda lib: fused(lib, mx=None)),
        ("NULL scale out", lambda lib: fused(lib, scale=None)),
        ("NULL offset out", lambda lib: fused(lib, offset=None)),
        ("NULL out", lambda lib: fused(lib, out=None)),
        ("bad data tag", lambda lib: fused(lib, dt=BAD)),
        ("bad out tag", lambda lib: fused(lib, out_dt=BAD)),
        ("tile does not divide", lambda lib: fused(lib, tiling=NODIV)),
        ("empty tensor", lambda lib: fused(lib, tiling=EMPTY)),
        ("container too small", lambda lib: fused(lib, bits=11.0)),
        ("one tile", lambda lib: fused(lib, tiling=ONE)),
        ("strided channels", lambda lib: fused(lib, tiling=CHAN)),
        ("global question without ticket words", lambda lib: fused(lib, sym=1, one=1)),
        ("fractional bits", lambda lib: fused(lib, bits=7.5)),
        ("misaligned data", lambda lib: fused(lib, data=A4)),
        ("misaligned out", lambda lib: fused(lib, out=A4)),
        ("integer data", lambda lib: fused(lib, dt=I8)),
        ("int16 container", lambda lib: fused(lib, out_dt=I16)),
        ("run % chunk", lambda lib: fused(lib, tiling=lambda: T((4, 72), (1, 72)))),
        ("run longer than a block holds", lambda lib: fused(lib, tiling=lambda: T((2, 16 * 1025), (1, 16 * 1025)))),
        ("NULL data + bad data tag", lambda lib: fused(lib, data=None, dt=BAD)),
        ("bad out tag + bad tiling", lambda lib: fused(lib, out_dt=BAD, tiling=NODIV)),
        ("bad tiling + container too small", lambda lib: fused(lib, tiling=NODIV, bits=11.0)),
        ("empty tensor + container too small", lambda lib: fused(lib, tiling=EMPTY, bits=11.0)),
        ("container too small + one tile", lambda lib: fused(lib, bits=11.0, tiling=ONE)),
    ]
    out += [(f"ffq_running_minmax_quantize: {what}", fn) for what, fn in rows]

    def params(lib, mn=A, mx=B, rdt=F32, ntiles=4, bits=8.0, sym=0, one=1, scale=C, sdt=F32, offset=D, odt=F32, ws=None, ws_bytes=0):
        return lib.ffq_parameters_for_range(mn, mx, rdt, ntiles, bits, sym, one, scale, sdt, offset, odt, ws, ws_bytes, None)

    rows = [
        ("NULL min", lambda lib: params(lib, mn=None)),
        ("NULL max", lambda lib: params(lib, mx=None)),
        ("NULL scale out", lambda lib: params(lib, scale=None)),
        ("no tiles", lambda lib: params(lib, ntiles=0)),
        ("bad range tag", lambda lib: params(lib, rdt=BAD)),
        ("bad scale tag", lambda lib: params(lib, sdt=BAD)),
        ("bad offset tag", lambda lib: params(lib, odt=BAD)),
        ("NULL min + bad range tag", lambda lib: params(lib, mn=None, rdt=BAD)),
    ]
    out += [(f"ffq_parameters_for_range: {what}", fn) for what, fn in rows]

    def dyn(lib, data=A, dt=BF16, tiling=CHAN, bits=8.0, sym=0, one=1, out=B, out_dt=I8, scale=C, offset=D, ws=E, ws_bytes=BIG, ticket=None):
        return lib.ffq_quantize_dynamic_by_tile(data, dt, tiling(), bits, sym, one, out, out_dt, scale, offset, ws, ws_bytes, ticket, None)

    rows = [
        ("tile does not divide", lambda lib: dyn(lib, tiling=NODIV)),
        ("empty tensor", lambda lib: dyn(lib, tiling=EMPTY)),
        ("NULL data", lambda lib: dyn(lib, data=None)),
        ("NULL out", lambda lib: dyn(lib, out=None)),
        ("NULL scale out", lambda lib: dyn(lib, scale=None)),
        ("NULL offset out", lambda lib: dyn(lib, offset=None)),
        ("bad data tag", lambda lib: dyn(lib, dt=BAD)),
        ("bad out tag", lambda lib: dyn(lib, out_dt=BAD)),
        ("container too small", lambda lib: dyn(lib, bits=11.0)),
        ("workspace too small, strided channels", lambda lib: dyn(lib, ws_bytes=16)),
        ("workspace NULL, strided channels", lambda lib: dyn(lib, ws=None)),
        ("workspace too small, one tile with the global question", lambda lib: dyn(lib, tiling=ONE, sym=1, ws_bytes=16)),
        ("workspace too small, rows with the global question and no ticket", lambda lib: dyn(lib, tiling=ROWS, sym=1, ws_bytes=16)),
        ("workspace too small, fractional bits", lambda lib: dyn(lib, tiling=ROWS, bits=7.5, ws_bytes=16)),
        ("workspace too small, misaligned rows", lambda lib: dyn(lib, tiling=ROWS, data=A4, ws_bytes=16)),
        ("workspace too small, run % chunk", lambda lib: dyn(lib, tiling=lambda: T((4, 72), (1, 72)), ws_bytes=16)),
        ("workspace too small, run longer than a block holds", lambda lib: dyn(lib, tiling=lambda: T((2, 16 * 1025), (1, 16 * 1025)), ws_bytes=16)),
        ("workspace too small, int16 container", lambda lib: dyn(lib, tiling=ROWS, out_dt=I16, ws_bytes=16)),
        ("workspace too small, f64 data", lambda lib: dyn(lib, tiling=ROWS, dt=F64, out_dt=I8, ws_bytes=16)),
        ("bad tiling + NULL data", lambda lib: dyn(lib, tiling=NODIV, data=None)),
        ("empty tensor + NULL data", lambda lib: dyn(lib, tiling=EMPTY, data=None)),
        ("NULL data + bad data tag", lambda lib: dyn(lib, data=None, dt=BAD)),
        ("bad out tag + container too small", lambda lib: dyn(lib, out_dt=BAD, bits=11.0)),
        ("container too small + workspace too small", lambda lib: dyn(lib, bits=11.0, ws_bytes=16)),
    ]
    out += [(f"ffq_quantize_dynamic_by_tile: {what}", fn) for what, fn in rows]
    return out


def _pack():
    out = []
    for name in ("ffq_pack_int4", "ffq_unpack_int4"):
        def call(lib, codes=A, dt=I8, numel=256, block=64, packed=B, name=name):
            if name == "ffq_pack_int4":
                return lib.ffq_pack_int4(codes, dt, numel, block, packed, None)
            return lib.ffq_unpack_int4(packed, numel, block, codes, dt, None)

        rows = [
            ("bad codes tag", lambda lib, call=call: call(lib, dt=BAD)),
            ("odd block", lambda lib, call=call: call(lib, numel=255, block=51)),
            ("no block", lambda lib, call=call: call(lib, block=0)),
            ("negative block", lambda lib, call=call: call(lib, block=-64)),
            ("negative numel", lambda lib, call=call: call(lib, numel=-256)),
            ("numel % block", lambda lib, call=call: call(lib, numel=250)),
            ("empty tensor", lambda lib, call=call: call(lib, numel=0)),
            ("NULL codes", lambda lib, call=call: call(lib, codes=None)),
            ("NULL packed", lambda lib, call=call: call(lib, packed=None)),
            ("bad codes tag + odd block", lambda lib, call=call: call(lib, dt=BAD, block=51)),
            ("numel % block + NULL codes", lambda lib, call=call: call(lib, numel=250, codes=None)),
            ("empty tensor + NULL codes", lambda lib, call=call: call(lib, numel=0, codes=None)),
        ]
        out += [(f"{name}: {what}", fn) for what, fn in rows]
    for name in ("ffq_quantize_pack_int4", "ffq_unpack_dequantize_int4"):
        def call(lib, data=A, dt=BF16, scale=B, sn=4, offset=None, on=4, tiling=ROWS, block=64, packed=C, name=name):
            if name == "ffq_quantize_pack_int4":
                return lib.ffq_quantize_pack_int4(data, dt, scale, sn, offset, on, tiling(), block, packed, None)
            return lib.ffq_unpack_dequantize_int4(packed, scale, sn, offset, on, tiling(), block, data, dt, None)

        rows = [
            ("tile does not divide", lambda lib, call=call: call(lib, tiling=NODIV)),
            ("odd block", lambda lib, call=call: call(lib, block=51)),
            ("no block", lambda lib, call=call: call(lib, block=0)),
            ("numel % block", lambda lib, call=call: call(lib, block=96)),
            ("wrong scale count", lambda lib, call=call: call(lib, sn=3)),
            ("wrong offset count", lambda lib, call=call: call(lib, offset=D, on=5)),
            ("strided channels", lambda lib, call=call: call(lib, tiling=CHAN)),
            ("run % 16", lambda lib, call=call: call(lib, tiling=lambda: T((8, 64), (1, 8)), sn=64)),
            ("block % 32", lambda lib, call=call: call(lib, block=16)),
            ("empty tensor", lambda lib, call=call: call(lib, tiling=EMPTY)),
            ("NULL data", lambda lib, call=call: call(lib, data=None)),
            ("NULL scale", lambda lib, call=call: call(lib, scale=None)),
            ("NULL packed", lambda lib, call=call: call(lib, packed=None)),
            ("integer data", lambda lib, call=call: call(lib, dt=I8)),
            ("f64 data", lambda lib, call=call: call(lib, dt=F64)),
            ("misaligned data", lambda lib, call=call: call(lib, data=A4)),
            ("misaligned packed", lambda lib, call=call: call(lib, packed=A4)),
            ("bad tiling + odd block", lambda lib, call=call: call(lib, tiling=NODIV, block=51)),
            ("odd block + wrong scale count", lambda lib, call=call: call(lib, block=51, sn=3)),
            ("wrong scale count + strided channels", lambda lib, call=call: call(lib, sn=3, tiling=CHAN)),
            ("block % 32 + NULL data", lambda lib, call=call: call(lib, block=16, data=None)),
            ("NULL data + integer data", lambda lib, call=call: call(lib, data=None, dt=I8)),
            ("empty tensor + block % 32", lambda lib, call=call: call(lib, tiling=EMPTY, block=16)),
            ("empty tensor + NULL data", lambda lib, call=call: call(lib, tiling=EMPTY, data=None)),
        ]
        out += [(f"{name}: {what}", fn) for what, fn in rows]

    def gguf(lib, codes=A, scales=B, nblocks=4, fmt=4, out=C):
        return lib.ffq_pack_gguf_blocks(codes, scales, nblocks, fmt, out, None)

    rows = [
        ("bad format", lambda lib: gguf(lib, fmt=5)),
        ("negative block count", lambda lib: gguf(lib, nblocks=-1)),
        ("too many blocks", lambda lib: gguf(lib, nblocks=1 << 31)),
        ("no blocks", lambda lib: gguf(lib, nblocks=0)),
        ("NULL codes", lambda lib: gguf(lib, codes=None)),
        ("NULL scales", lambda lib: gguf(lib, scales=None)),
        ("NULL out", lambda lib: gguf(lib, out=None)),
        ("misaligned codes", lambda lib: gguf(lib, codes=A4)),
        ("misaligned out", lambda lib: gguf(lib, out=A4, fmt=8)),
        ("bad format + negative block count", lambda lib: gguf(lib, fmt=5, nblocks=-1)),
        ("too many blocks + NULL codes", lambda lib: gguf(lib, nblocks=1 << 31, codes=None)),
        ("NULL codes + misaligned out", lambda lib: gguf(lib, codes=None, out=A4)),
    ]
    return out + [(f"ffq_pack_gguf_blocks: {what}", fn) for what, fn in rows]


def _backward():
    def call(lib, data=A, grad=B, dt=BF16, scale=C, sn=4, offset=None, on=4, tiling=ROWS, bits=8.0, dinput=D, dscale=E, doffset=None, ws=G,
             ws_bytes=BIG):
        return lib.ffq_quantize_by_tile_backward(data, grad, dt, scale, sn, offset, on, tiling(), bits, dinput, dscale, doffset, ws, ws_bytes, None)

    stream = lambda: T((2, 4096), (1, 4096))  # two tiles: the streaming kernel and its workspace
    rows = [
        ("tile does not divide", lambda lib: call(lib, tiling=NODIV)),
        ("integer data", lambda lib: call(lib, dt=I8)),
        ("bad data tag", lambda lib: call(lib, dt=BAD)),
        ("wrong scale count", lambda lib: call(lib, sn=3)),
        ("wrong offset count", lambda lib: call(lib, offset=A, on=5)),
        ("empty tensor", lambda lib: call(lib, tiling=EMPTY)),
        ("NULL data", lambda lib: call(lib, data=None)),
        ("NULL output grad", lambda lib: call(lib, grad=None)),
        ("NULL scale", lambda lib: call(lib, scale=None)),
        ("NULL dinput", lambda lib: call(lib, dinput=None)),
        ("NULL dscale", lambda lib: call(lib, dscale=None)),
        ("doffset missing", lambda lib: call(lib, offset=A)),
        ("too many tiles", lambda lib: call(lib, tiling=lambda: T((1 << 31, 64), (1, 64)), sn=1 << 31)),
        ("workspace too small", lambda lib: call(lib, tiling=stream, sn=2, ws_bytes=16)),
        ("workspace NULL", lambda lib: call(lib, tiling=stream, sn=2, ws=None)),
        ("bad tiling + integer data", lambda lib: call(lib, tiling=NODIV, dt=I8)),
        ("integer data + wrong scale count", lambda lib: call(lib, dt=I8, sn=3)),
        ("wrong scale count + wrong offset count", lambda lib: call(lib, sn=3, offset=A, on=5)),
        ("wrong offset count + NULL data", lambda lib: call(lib, offset=A, on=5, data=None)),
        ("NULL data + doffset missing", lambda lib: call(lib, data=None, offset=A)),
        ("doffset missing + workspace too small", lambda lib: call(lib, tiling=stream, sn=2, on=2, offset=A, ws_bytes=16)),
        ("empty tensor + integer data", lambda lib: call(lib, tiling=EMPTY, dt=I8)),
        ("empty tensor + NULL data", lambda lib: call(lib, tiling=EMPTY, data=None)),
    ]
    return [(f"ffq_quantize_by_tile_backward: {what}", fn) for what, fn in rows]


def calls():
    return (_quantize("ffq_quantize_by_tile", True) + _quantize("ffq_dequantize_by_tile", False) + _unless_same() + _rows_rowsum() + _rows_batch()
            + _minmax() + _pack() + _backward())


def records(library_path):
    from fastforward_amd._cabi import FFQLibrary

    lib = FFQLibrary(library_path)
    out = []
    for name, call in calls():
        status = int(call(lib))
        out.append({"call": name, "status": status, "message": lib.ffq_last_error().decode() if status else ""})
    return out


if __name__ == "__main__":
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    out = pathlib.Path(sys.argv[2]) if len(sys.argv) > 2 else pathlib.Path(__file__).resolve().parent / "quantizer_refusals.json"
    rows = records(pathlib.Path(sys.argv[1]))
    out.write_text("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]\n")
    print(f"{len(rows)} records, {sum(r['status'] != 0 for r in rows)} refusals -> {out}")
    for r in rows:
        print(r["status"], r["call"], "|", r["message"][:100])
