"""Every stream-taking entry point of ``include/ffq.h`` under guard bands (tests/guards.py): no store outside an operand, inputs
left as they were, no unwritten output element, no dependence on workspace contents or on bytes outside an operand, ticket and
extrema words put back, workspaces as long as the size queries say. Small shapes at the edges of each family's kernels; at least
one case per family has an output of a whole number of 512-byte blocks, one an odd byte count; nothing exceeds 4 M elements.

Cases are data (``CASES``): ``build(device)`` returns ``(fn, inputs, inplace)``, so tests/test_guards_cpu.py runs the ones the C
oracle exports on host memory, and checks that ``GUARDED`` (the symbols the cases claim, each verified to be reached) and
``guards.EXEMPT`` partition ``_cabi.SIGNATURES``. The silu_mul table kernel (from 16.7 M elements) is out of reach of the
size cap and is not run here. Nothing is written outside an allocated buffer on purpose: the sensitivity test flips a guard byte
of the test's own arena buffer with a plain indexed write."""

from __future__ import annotations

import math

from dataclasses import dataclass
from typing import Callable

import pytest
import torch

from fastforward_amd import _native, ops

import guards

I8, U8, BF16, F16, F32 = torch.int8, torch.uint8, torch.bfloat16, torch.float16, torch.float32
NAME = {BF16: "bf16", F16: "fp16", F32: "fp32", I8: "i8"}


@dataclass(frozen=True)
class Case:
    id: str
    symbols: tuple[str, ...]  # entry points the case must reach (guards.check_call verifies it)
    build: Callable  # device -> (fn, inputs, inplace)
    host: bool = True  # the C oracle exports the symbols and the wrapper takes host tensors: also run by test_guards_cpu.py
    workspace_image: int = 0  # bytes the wrapper adds to a queried size by the header's rule (a forced two-pass weight image)


CASES: list[Case] = []


def case(id, symbols, host=True, workspace_image=0):
    def add(build):
        CASES.append(Case(id, tuple(symbols), build, host, workspace_image))
        return build
    return add


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def gen(dev, seed):
    return torch.Generator(dev).manual_seed(seed)


def real(dev, shape, dtype, seed, spread=3.0):
    x = torch.randn(shape, device=dev, generator=gen(dev, seed)) * spread
    if x.numel() >= 3:
        x.view(-1)[:3] = torch.tensor([0.0, -0.0, 1e-30], device=dev)
    return x.to(dtype)


def codes(dev, shape, seed, lo=-128, hi=128, dtype=I8):
    return torch.randint(lo, hi, shape, device=dev, generator=gen(dev, seed)).to(dtype)


def params(dev, n, seed, lo=0.02, hi=0.07):
    g = gen(dev, seed)
    return torch.rand(n, device=dev, generator=g) * (hi - lo) + lo, torch.randint(-3, 4, (n,), device=dev, generator=g).float()


def one(dev, scale=0.05, offset=1.0):
    """A per-tensor (scale, offset) pair."""
    return torch.tensor([scale], device=dev), torch.tensor([offset], device=dev)


def tiles(shape, tile):
    return math.prod(s // t for s, t in zip(shape, tile))


# ---- codec ------------------------------------------------------------------------------------------------------------------------
FLAT = [(1,), (7,), (8,), (15,), (16,), (17,), (24 * 64 + 1,), (256,)]  # (256 bf16: 512 bytes of codes-as-values exactly)
TILED = {"tensor": (24, 64), "channel": (1, 64), "block32": (1, 32), "tile4x16": (4, 16)}


def generic(fn, on):
    """`fn` with the streaming kernels switched off (ffq_force_generic_kernels), the setting put back whatever happens."""
    if not on:
        return fn

    def forced(*a):
        lib = _native.library()
        previous = lib.ffq_force_generic_kernels(1)
        try:
            return fn(*a)
        finally:
            lib.ffq_force_generic_kernels(previous)
    return forced


def codec_case(shape, tile, dtype, force, tag):
    n = tiles(shape, tile)
    contiguous_runs = tile[0] == 1 or n == 1  # (other tilings: backward takes the composite of tensor ops, which allocates on its own)

    def build(dev):
        x, grad = real(dev, shape, dtype, 1), real(dev, shape, dtype, 2, 1.0)
        scale, offset = params(dev, n, 3)
        cand_s, cand_o = torch.rand(3, n, device=dev, generator=gen(dev, 4)) * 0.05 + 0.02, torch.randint(-3, 4, (3, n), device=dev, generator=gen(dev, 5)).float()

        def fn(x, grad, scale, offset, cand_s, cand_o):
            out = [ops.quantize_by_tile(x, scale, tile, bits, od, offset) for bits in (8, 4, 3) for od in (I8, None)]
            out.append(ops.quantize_by_tile(x, scale, tile, 8, I8, None))
            out += [ops.dequantize_by_tile(out[0], scale, tile, offset, od) for od in (dtype, F32)]
            out.append(ops.dequantize_by_tile(out[1].to(dtype), scale, tile, None, None))
            out.append(ops.minmax_by_tile(x, tile))
            out += [ops.quantize_dynamic_by_tile(x, tile, 8, sym, side, I8) for sym, side in ((False, False), (True, False), (True, True))]
            out.append(ops.parameters_for_range(*out[-4], 8, False, False))
            if contiguous_runs:
                out.append(ops.quantize_by_tile_backward(x, grad, scale, tile, 4, offset))
                out.append(ops.grid_sqerror_by_tile(x, cand_s, cand_o, tile, 4))
            return out

        return generic(fn, force), (x, grad, scale, offset, cand_s, cand_o), ()

    symbols = ["ffq_quantize_by_tile", "ffq_dequantize_by_tile", "ffq_minmax_by_tile", "ffq_quantize_dynamic_by_tile", "ffq_parameters_for_range"]
    symbols += ["ffq_quantize_by_tile_backward"] if contiguous_runs else []
    case(f"codec-{tag}-{NAME[dtype]}-{'generic' if force else 'fast'}", symbols, host=not force)(build)  # (the oracle has one kernel family)


for force in (False, True):
    for shape in FLAT:
        codec_case(shape, shape, BF16, force, f"flat{shape[0]}")
    for shape in ((17,), (24 * 64 + 1,)):
        for dtype in (F16, F32):
            codec_case(shape, shape, dtype, force, f"flat{shape[0]}")
    for name, tile in TILED.items():
        for dtype in (BF16, F16, F32):
            codec_case((24, 64), tile, dtype, force, name)
    codec_case((3, 72), (1, 24), BF16, force, "rows-of-24")  # runs that are no multiple of 16 elements


@case("grid-sqerror-channel", ["ffq_grid_sqerror_by_tile"])
def _(dev):
    x = real(dev, (24, 64), BF16, 6)
    s, o = torch.rand(5, 24, device=dev, generator=gen(dev, 7)) * 0.05 + 0.02, torch.randint(-3, 4, (5, 24), device=dev, generator=gen(dev, 8)).float()
    into = torch.rand(5, 24, device=dev, generator=gen(dev, 9))
    return (lambda x, s, o, into: (ops.grid_sqerror_by_tile(x, s, o, (1, 64), 4), ops.grid_sqerror_by_tile(x, s, None, (1, 64), 4, out=into))), (x, s, o, into), (3,)


for sym, side in ((False, False), (True, False), (True, True)):
    for n in (1, 7, 8192 + 3):  # (above 8192 tiles: the grid form)
        @case(f"parameters-for-range-{n}-sym{int(sym)}-one{int(side)}", ["ffq_parameters_for_range"])
        def _(dev, n=n, sym=sym, side=side):
            lo, hi = -torch.rand(n, device=dev, generator=gen(dev, 10)) * 4, torch.rand(n, device=dev, generator=gen(dev, 11)) * 4
            if n > 2:
                lo[:3], hi[:3] = torch.tensor([0.0, 0.0, 1.0], device=dev), torch.tensor([0.0, 2.0, 3.0], device=dev)
            return (lambda lo, hi: ops.parameters_for_range(lo, hi, 8, sym, side)), (lo, hi), ()


for name, tile in TILED.items():
    for dtype in (BF16, F32):
        @case(f"running-minmax-{name}-{NAME[dtype]}", ["ffq_running_minmax_step", "ffq_minmax_by_tile"])
        def _(dev, tile=tile, dtype=dtype):
            n = tiles((24, 64), tile)
            x = real(dev, (24, 64), dtype, 12)
            rmin, rmax = torch.full((n,), 0.5, dtype=dtype, device=dev), torch.full((n,), 0.75, dtype=dtype, device=dev)
            amin, amax = rmin.clone(), rmax.clone()
            scale, offset = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
            flags = torch.zeros(1, dtype=torch.int32, device=dev)

            def fn(x, rmin, rmax, amin, amax, scale, offset, flags):
                ops._running_minmax_step(x, tile, rmin, rmax, flags, 8, False, False, scale, offset)
                ops.minmax_by_tile(x, tile, running_min=amin, running_max=amax, status_flags=flags)
                return None

            return fn, (x, rmin, rmax, amin, amax, scale, offset, flags), (1, 2, 3, 4, 5, 6, 7)


for name, tile in (("channel", (1, 64)), ("block32", (1, 32))):
    for sym, side in ((False, False), (True, True)):
        @case(f"running-minmax-quantize-{name}-sym{int(sym)}", ["ffq_running_minmax_quantize"], host=not sym)  # (the symmetric one-sided form takes a device ticket)
        def _(dev, tile=tile, sym=sym, side=side):
            n = tiles((24, 64), tile)
            x = real(dev, (24, 64), BF16, 13)
            rmin, rmax = torch.full((n,), 0.5, dtype=BF16, device=dev), torch.full((n,), 0.75, dtype=BF16, device=dev)
            scale, offset = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
            return (lambda x, rmin, rmax, scale, offset: ops.running_minmax_quantize(x, tile, rmin, rmax, None, 8, sym, side, scale, offset, I8)), (x, rmin, rmax, scale, offset), (1, 2, 3, 4)


for numel in (16, 48, 24 * 64):
    for dtype in (BF16, F32):
        @case(f"unless-same-{numel}-{NAME[dtype]}", ["ffq_quantize_by_tile_unless_same"])
        def _(dev, numel=numel, dtype=dtype):
            x = real(dev, (numel,), dtype, 14)
            (s, o), (es, eo) = one(dev, 0.03, 1.0), one(dev, 0.05, 1.0)  # (different parameters: the codes are written)
            return (lambda x, s, o, es, eo: ops.quantize_by_tile_unless_same(x, s, o, 8, es, eo)), (x, s, o, es, eo), ()


for rows in (1, 3):
    @case(f"rows-rowsum-{rows}x1024", ["ffq_quantize_rows_rowsum"])
    def _(dev, rows=rows):
        w = real(dev, (rows, 1024), BF16, 15, 0.05)
        s, o = params(dev, rows, 16, 0.0005, 0.001)
        return (lambda w, s, o: ops.quantize_rows_rowsum(w, s, o, 8)), (w, s, o), ()


@case("rows-batch-8-unequal", ["ffq_quantize_rows_batch"])
def _(dev):
    shapes = [(4, 1024), (8, 512), (16, 256), (4, 1024), (256, 16), (2, 2048), (1, 4096), (12, 1024)]
    ws = [real(dev, s, BF16, 17 + i, 0.05) for i, s in enumerate(shapes)]
    ps = [params(dev, s[0], 30 + i, 0.0005, 0.001) for i, s in enumerate(shapes)]
    return (lambda ws, ss, os_: ops.quantize_rows_batch(ws, ss, os_, 8)), (ws, [p[0] for p in ps], [p[1] for p in ps]), ()


@case("unless-same-same-parameters-writes-nothing", ["ffq_quantize_by_tile_unless_same"])
def _(dev):
    x = real(dev, (24 * 64,), BF16, 14)
    (s, o), (es, eo) = one(dev, 0.03, 1.0), one(dev, 0.03, 1.25)  # (the same scale bits and the same ROUNDED offset)

    def fn(x, s, o, es, eo):
        out = ops.quantize_by_tile_unless_same(x, s, o, 8, es, eo)
        assert out is not None
        if guards._PATCHED:  # the result is unwritten memory by contract: under the guards it must still hold the poison, every byte
            held = out.view(torch.uint8)
            assert bool((held == held[0]).all()) and int(held[0]) in (guards.POISON_A, guards.POISON_B), "codes were written for equal parameters"
        return None  # (nothing to compare between the runs; the guards, the inputs and the pointers are checked as ever)

    return fn, (x, s, o, es, eo), ()


# ---- packing ----------------------------------------------------------------------------------------------------------------------
for rows, cols in ((1, 32), (3, 64), (33, 32), (8, 128)):  # (8 x 128 nibbles: 512 bytes exactly)
    @case(f"int4-pack-unpack-{rows}x{cols}", ["ffq_pack_int4", "ffq_unpack_int4", "ffq_quantize_pack_int4", "ffq_unpack_dequantize_int4"])
    def _(dev, rows=rows, cols=cols):
        c = codes(dev, (rows, cols), 40, -8, 8)
        x = real(dev, (rows, cols), BF16, 41)
        (s, o), (sb, ob) = params(dev, rows, 42), params(dev, rows * cols // 32, 43)

        def fn(c, x, s, o, sb, ob):
            packed = ops.pack_int4(c, 32)
            qp = ops.quantize_pack_int4(x, s, (1, cols), o, 32)
            qb = ops.quantize_pack_int4(x, sb, (1, 32), None, 32)
            return [packed, ops.unpack_int4(packed, (rows, cols), I8, 32), ops.unpack_int4(packed, (rows, cols), BF16, 32), qp, qb,
                    ops.unpack_dequantize_int4(qp, s, (rows, cols), (1, cols), o, 32, BF16), ops.unpack_dequantize_int4(qb, sb, (rows, cols), (1, 32), None, 32, F32)]

        return fn, (c, x, s, o, sb, ob), ()


for blocks in (1, 33, 256):
    @case(f"gguf-blocks-{blocks}", ["ffq_pack_gguf_blocks"])
    def _(dev, blocks=blocks):
        c4, c8 = codes(dev, (blocks, 32), 44, -8, 8), codes(dev, (blocks, 32), 45)
        s = torch.rand(blocks, device=dev, generator=gen(dev, 46)) + 0.1
        return (lambda c4, c8, s: (ops.pack_q4_0_blocks(c4, s), ops.pack_q8_0_blocks(c8, s))), (c4, c8, s), ()


# ---- GPTQ -------------------------------------------------------------------------------------------------------------------------
def hinv(dev, n, seed):
    return torch.eye(n, device=dev) * 2 + torch.triu(torch.rand(n, n, device=dev, generator=gen(dev, seed)) * 0.1, 1)


for rows, cols, col0, block in ((1, 8, 0, 8), (5, 40, 32, 8), (16, 256, 128, 128)):  # (the smallest block; a ragged last block; a full one)
    @case(f"gptq-block-{rows}x{cols}-at{col0}", ["ffq_gptq_block"])
    def _(dev, rows=rows, cols=cols, col0=col0, block=block):
        w = real(dev, (rows, cols), F32, 50, 0.5)
        q, e = torch.zeros_like(w), torch.zeros_like(w)
        s, o = params(dev, rows, 51)
        return (lambda w, q, e, h, s, o: ops.gptq_block(w, q, e, col0, block, h, s, o, 4)), (w, q, e, hinv(dev, cols, 52), s, o), (1, 2)


for refit in (False, True):
    for rows, cols, col0, block, tile in ((2, 32, 0, 32, (1, 32)), (6, 96, 64, 32, (2, 32)), (16, 256, 128, 128, (1, 64))):
        @case(f"gptq-grid-{rows}x{cols}-at{col0}-refit{int(refit)}", ["ffq_gptq_block_grid"], host=False)
        def _(dev, rows=rows, cols=cols, col0=col0, block=block, tile=tile, refit=refit):
            w = real(dev, (rows, cols), F32, 53, 0.5)
            q, e = torch.zeros_like(w), torch.zeros_like(w)
            s, o = params(dev, (rows // tile[0]) * (cols // tile[1]), 54)
            order = torch.randperm(cols, device=dev, generator=gen(dev, 55))
            fn = lambda w, q, e, h, s, o, order: (ops.gptq_block_grid(w, q, e, col0, block, h, s, o, tile, 4, order, refit, False, False),  # noqa: E731
                                                  ops.gptq_block_grid(w, q, e, col0, block, h, s, None, tile, 4, None, refit, True, True))
            return fn, (w, q, e, hinv(dev, cols, 56), s, o, order), (1, 2, 4, 5)


# ---- int8 GEMMs -------------------------------------------------------------------------------------------------------------------
def w8a8(dev, M, N, K, seed):
    x, w = codes(dev, (M, K), seed), codes(dev, (N, K), seed + 1)
    (sx, ox), sw = one(dev, 0.02, 3.0), torch.rand(N, device=dev, generator=gen(dev, seed + 2)) * 0.01 + 0.001
    wo = torch.randint(-2, 3, (N,), device=dev, generator=gen(dev, seed + 3)).float()
    bias = real(dev, (N,), BF16, seed + 4, 1.0)
    return x, w, sx, ox, sw, wo, bias


for M in (1, 127, 129, 257):
    for N, K in ((1, 16), (16, 16), (272, 144), (256, 128)):
        @case(f"linear-w8a8-{M}x{N}x{K}", ["ffq_linear_w8a8"])
        def _(dev, M=M, N=N, K=K):
            x, w, sx, ox, sw, wo, bias = w8a8(dev, M, N, K, 60)
            os_, oo = one(dev, 0.5, -2.0)

            def fn(x, w, sx, ox, sw, wo, bias, os_, oo):
                return [ops.linear_w8a8(x, w, sx, ox, sw, None, bias), ops.linear_w8a8(x, w, sx, ox, sw, wo, None, F32),
                        ops.linear_w8a8(x, w, sx, None, sw, None, bias, I8, os_, oo, 8.0), ops.linear_w8a8(x, w, sx, ox, sw[:1].clone(), wo[:1].clone(), None, F16)]

            return fn, (x, w, sx, ox, sw, wo, bias, os_, oo), ()


for B, M, N, K in ((1, 1, 16, 16), (3, 20, 48, 64), (2, 129, 272, 144), (2, 128, 128, 128)):
    @case(f"bmm-w8a8-{B}x{M}x{N}x{K}", ["ffq_bmm_w8a8"])
    def _(dev, B=B, M=M, N=N, K=K):
        x, w = codes(dev, (B, M, K), 66), codes(dev, (B, N, K), 67)
        (s, o), (os_, oo) = one(dev, 0.02, 1.0), one(dev, 4.0, -2.0)
        return (lambda x, w, s, o, os_, oo: (ops.bmm_w8a8(x, w, s, o, s, None), ops.bmm_w8a8(x, w, s, o, s, o, F32), ops.bmm_w8a8(x, w, s, o, s, None, I8, os_, oo))), (x, w, s, o, os_, oo), ()


# _multi / _earlier / _gated / _estimating start at 64 tiles of 256 x 256 (M in {1, 127, 129, 257} is outside them): 8 x 8 tiles with a
# last row tile of ONE row, 3.67 M output elements
PERSISTENT = (7 * 256 + 1, 2048, 256)


@case("linear-w8a8-multi", ["ffq_linear_w8a8_multi"], host=False)
def _(dev):
    M, N, K = PERSISTENT
    x, w, sx, ox, sw, _, _ = w8a8(dev, M, N, K, 70)

    def fn(x, w, sx, ox, sw):
        got = ops.linear_w8a8_multi(x, w, sx, ox, sw, (768, 768, 512))
        assert got is not None, "linear_w8a8_multi declined the persistent kernel's own shape"
        return got

    return fn, (x, w, sx, ox, sw), ()


@case("linear-w8a8-earlier", ["ffq_linear_w8a8_earlier"], host=False)
def _(dev):
    M, N, K = PERSISTENT
    x, w, sx, ox, sw, wo, _ = w8a8(dev, M, N, K, 71)
    earlier = codes(dev, (M, K), 72)
    same, differs = one(dev, 0.02, 3.0), one(dev, 0.03, 3.0)

    def fn(x, earlier, w, sx, ox, sw, wo, same, differs):
        got = [ops.linear_w8a8_earlier(x, (earlier, *same), w, sx, ox, sw, wo), ops.linear_w8a8_earlier(x, (earlier, *differs), w, sx, ox, sw, None, F32)]
        assert all(g is not None for g in got), "linear_w8a8_earlier declined the persistent kernel's own shape"
        return got

    return fn, (x, earlier, w, sx, ox, sw, wo, same, differs), ()


@case("linear-w8a8-gated", ["ffq_linear_w8a8_gated"], host=False)
def _(dev):
    M, N, K = PERSISTENT
    x, w, sx, ox, sw, wo, _ = w8a8(dev, M, N, K, 73)
    gate = real(dev, (M, N), BF16, 74, 1.0)

    def fn(x, w, sx, ox, sw, wo, gate):
        got = [ops.linear_w8a8_gated(x, w, sx, ox, sw, wo, gate), ops.linear_w8a8_gated(x, w, sx, ox, sw, None, gate, want_extrema=True)]
        assert all(g is not None for g in got), "linear_w8a8_gated declined the persistent kernel's own shape"
        return got

    return fn, (x, w, sx, ox, sw, wo, gate), ()


for M, N, K in ((1, 128, 256), (129, 256, 384), (257, 128, 256)):
    @case(f"mlp-gate-up-w8a8-{M}x{N}x{K}", ["ffq_mlp_gate_up_w8a8"])
    def _(dev, M=M, N=N, K=K):
        x, g, u = codes(dev, (M, K), 75), codes(dev, (N, K), 76), codes(dev, (N, K), 77)
        (sx, ox), (so, oo) = one(dev, 0.02, 3.0), one(dev, 0.5, -20.0)
        gs, us = (torch.rand(N, device=dev, generator=gen(dev, 78 + i)) * 0.01 + 0.001 for i in range(2))

        def fn(x, g, u, sx, ox, gs, us, so, oo):
            got = ops.mlp_gate_up_w8a8(x, g, u, sx, ox, gs, us, so, oo)
            assert got is not None, "mlp_gate_up_w8a8 declined a shape inside its stated range"
            return got

        return fn, (x, g, u, sx, ox, gs, us, so, oo), ()


for equal in (True, False):
    @case(f"mlp-gate-up-w8a8-estimating-{'same' if equal else 'different'}-parameters", ["ffq_mlp_gate_up_w8a8_estimating"], host=False)
    def _(dev, equal=equal):
        M, N, K = PERSISTENT
        xg, xu, g, u = codes(dev, (M, K), 80), codes(dev, (M, K), 81), codes(dev, (N, K), 82), codes(dev, (N, K), 83)
        pg, pu = one(dev, 0.02, 3.0), one(dev, 0.02 if equal else 0.03, 3.0)
        gs, us = (torch.rand(N, device=dev, generator=gen(dev, 84 + i)) * 0.01 + 0.001 for i in range(2))

        def fn(xg, xu, g, u, pg, pu, gs, us):
            got = ops.mlp_gate_up_w8a8_estimating(xg, xu, g, u, pg, pu, (gs, None), (us, None), want_extrema=True)
            assert got is not None, "mlp_gate_up_w8a8_estimating declined the persistent kernel's own shape"
            return got

        return fn, (xg, xu, g, u, pg, pu, gs, us), ()


# ---- weight-only GEMMs ------------------------------------------------------------------------------------------------------------
def wq_weight(dev, N, K, group, seed, nibbles):
    lo, hi = (-8, 8) if nibbles else (-128, 128)
    w = codes(dev, (N, K), seed, lo, hi)
    n = N * (K // group)
    scale = torch.rand(n, device=dev, generator=gen(dev, seed + 1)) * 0.02 + 0.005
    offset = torch.randint(-2, 3, (n,), device=dev, generator=gen(dev, seed + 2)).float()
    return w, scale, offset


# M = 1, 7: the skinny forms; 129, 257: the 256-row tiles (one-wave and four-wave forms are the library's choice by shape); split > 1:
# slabs and tickets; K = 128 is the smallest the entry point takes; two_pass True: the image's scratch; False: the short workspace the header allows
WQ = [(1, 128, 128, 64), (7, 256, 256, 64), (129, 256, 256, 256), (257, 384, 320, 64), (33, 128, 1024, 128)]
for M, N, K, group in WQ:
    for nibbles in (False, True):
        for split, two_pass in ((0, None), (2, False), (0, True)):
            if split > 1 and K // 64 < 2 * split:
                continue  # (a forced split needs K / 64 >= 2 * split)
            @case(f"linear-wq-{M}x{N}x{K}-g{group}-{'nibbles' if nibbles else 'int8'}-split{split}-twopass{two_pass}", ["ffq_linear_wq"], workspace_image=N * K * 2 if two_pass else 0)
            def _(dev, M=M, N=N, K=K, group=group, nibbles=nibbles, split=split, two_pass=two_pass):
                x = real(dev, (M, K), BF16, 90, 0.5)
                w, s, o = wq_weight(dev, N, K, group, 91, nibbles)
                bias = real(dev, (N,), BF16, 94, 1.0)

                def fn(x, w, s, o, bias):
                    wk = ops.pack_int4(w, 32) if nibbles else w
                    got = [ops.linear_wq(x, wk, s, o, group, bias, None, 32 if nibbles else 0, two_pass, split), ops.linear_wq(x, wk, s, None, group, None, F32, 32 if nibbles else 0, two_pass, split)]
                    assert all(g is not None for g in got), "linear_wq declined a covered shape"
                    return got

                return fn, (x, w, s, o, bias), ()


for M in (5, 129):
    for split in (0, 2):
        @case(f"linear-wq-multi-and-mlp-{M}-split{split}", ["ffq_linear_wq_multi", "ffq_mlp_gate_up_wq"])
        def _(dev, M=M, split=split):
            K, group = 256, 64
            x = real(dev, (M, K), BF16, 95, 0.5)
            mats = [wq_weight(dev, n, K, group, 96 + 3 * i, True) for i, n in enumerate((256, 256, 128))]

            def fn(x, ws, ss, os_):
                multi = ops.linear_wq_multi(x, ws, ss, os_, group, split=split)
                mlp = ops.mlp_gate_up_wq(x, ws[0], ws[1], ss[0], os_[0], ss[1], os_[1], group, split=split)
                per_channel = ops.mlp_gate_up_wq(x, ws[0], ws[1], ss[0][::4].contiguous(), None, ss[1][::4].contiguous(), None, None, split=split)
                assert multi is not None and mlp is not None and per_channel is not None, "a covered weight-only shape was declined"
                return multi, mlp, per_channel

            return fn, (x, [m[0] for m in mats], [m[1] for m in mats], [m[2] for m in mats]), ()


# ---- producers and attention ------------------------------------------------------------------------------------------------------
for rows, cols in ((1, 64), (7, 80), (8, 256), (13, 1040)):  # (cols % 16 == 0 is the kernel's stated range)
    for dtype in (BF16,):  # (the fused producers are built for bf16 activations)
        @case(f"add-rmsnorm-and-silu-mul-{rows}x{cols}-{NAME[dtype]}", ["ffq_add_rmsnorm_quantize", "ffq_silu_mul_quantize"])
        def _(dev, rows=rows, cols=cols, dtype=dtype):
            x, d, r = real(dev, (rows, cols), dtype, 100), real(dev, (rows, cols), dtype, 101), real(dev, (rows, cols), dtype, 102)
            g = real(dev, (cols,), dtype, 103, 1.0)
            q1, q2, q3 = one(dev, 0.05, 1.0), one(dev, 0.02, -3.0), (one(dev, 0.1)[0], None)

            def fn(x, d, r, g, q1, q2, q3):
                return [ops.add_rmsnorm_quantize(x, d, g, 1e-5, [q1, q2, q3], want_norm=True), ops.add_rmsnorm_quantize(x, None, g, 1e-5, [q1]),
                        ops.add_rmsnorm_quantize(r, d, g, 1e-5, [q2], sum_inplace=True), ops.silu_mul_quantize(x, d, [q1, q3], want_product=True),
                        ops.silu_mul_quantize(x, d, [q2])]

            return fn, (x, d, r, g, q1, q2, q3), (2,)


for batch, seq, heads, kv in ((1, 1, 1, 1), (2, 7, 3, 3), (1, 33, 4, 2)):
    @case(f"rope-{batch}x{seq}x{heads}", ["ffq_rope_inplace"])
    def _(dev, batch=batch, seq=seq, heads=heads, kv=kv):
        q, k, k2 = real(dev, (batch, seq, heads * 64), BF16, 104), real(dev, (batch, seq, kv * 64), BF16, 105), real(dev, (batch, seq, kv * 64), BF16, 106)
        cos, sin = real(dev, (seq, 64), BF16, 107, 0.5), real(dev, (seq, 64), BF16, 108, 0.5)
        return (lambda q, k, k2, cos, sin: (ops.rope_(q, k, cos, sin, 64), ops.rope_(None, k2, cos, sin, 64))), (q, k, k2, cos, sin), (0, 1, 2)


for batch, seq, heads, kv, hd in ((1, 64, 1, 1, 128), (2, 128, 4, 2, 128), (3, 192, 3, 1, 128)):  # (head_dim 128 and seq % 64 == 0 are the kernel's stated range: no ragged length exists)
    @case(f"attention-{batch}x{seq}x{heads}over{kv}x{hd}", ["ffq_attention"])
    def _(dev, batch=batch, seq=seq, heads=heads, kv=kv, hd=hd):
        q, k, v = (real(dev, (batch, seq, h * hd), BF16, 110 + i, 0.5) for i, h in enumerate((heads, kv, kv)))
        cos, sin = real(dev, (seq, hd), BF16, 113, 0.5), real(dev, (seq, hd), BF16, 114, 0.5)
        quant = one(dev, 0.02, 1.0)
        fn = lambda q, k, v, cos, sin, quant: (ops.attention(q, k, v, hd, True, quant), ops.attention(q, k, v, hd, False, None),  # noqa: E731
                                               ops.attention(q, k, v, hd, True, quant, want_context=False, q_rope=(cos, sin)))
        return fn, (q, k, v, cos, sin, quant), ()


# ---- one-pass families (device only) ----------------------------------------------------------------------------------------------
def forms(dev, x, rows=None):
    """`x` plain, as int8 codes and as codes in the value dtype: (operand, dequant) triples; per-row parameters with `rows`."""
    s, o = one(dev, 0.05, 2.0)
    out = {"plain": (x, None), "int8": (codes(dev, x.shape, 120), (s, o)), "container": (codes(dev, x.shape, 121).to(x.dtype), (s, o))}
    if rows:
        out["int8-per-row"] = (codes(dev, x.shape, 122), params(dev, rows, 123))
    return out


QS = lambda dev: [one(dev, 0.05, 1.0), (one(dev, 0.02)[0], None)]  # noqa: E731  (two fused output quantizers)
ROWS = [(1, 8), (7, 40), (9, 264), (13, 1032), (8, 256)]  # rows no multiple of 8; (8, 256) bf16: 4096 bytes exactly

for rows, cols in ROWS:
    for dtype in (BF16, F16):
        for form in ("plain", "int8", "container", "int8-per-row"):
            @case(f"rowwise-{rows}x{cols}-{NAME[dtype]}-{form}", ["ffq_layer_norm_quantize", "ffq_softmax_quantize", "ffq_rms_norm_quantize", "ffq_pointwise_quantize",
                                                                    "ffq_activation_quantize", "ffq_unary_quantize", "ffq_sum_quantize", "ffq_cumsum_quantize"], host=False)
            def _(dev, rows=rows, cols=cols, dtype=dtype, form=form):
                x, dq = forms(dev, real(dev, (rows, cols), dtype, 124, 1.0), rows)[form]
                w, b = real(dev, (cols,), dtype, 125, 1.0), real(dev, (cols,), dtype, 126, 0.1)

                def fn(x, dq, w, b, qs):
                    kw = dict(dtype=dtype, dequant=dq)
                    out = [ops.layer_norm_quantize(x, cols, w, b, 1e-5, qs, **kw), ops.layer_norm_quantize(x, cols, None, None, 1e-5, (), **kw),
                           ops.softmax_quantize(x, qs, **kw), ops.rms_norm_quantize(x, w, 1e-6, qs, **kw)]
                    out += [ops.pointwise_quantize(op, x, qs, **kw) for op in ("relu", "silu")]
                    out += [ops.activation_quantize(op, x, qs, **kw) for op in ("sigmoid", "gelu", "gelu_tanh")]
                    out += [ops.unary_quantize(op, x, 1.7, qs, **kw) for op in ("exp", "sin", "cos", "pow")]
                    out += [ops.sum_quantize(x, d, qs, **kw) for d in (None, 0, 1)]
                    out += [ops.cumsum_quantize(x, d, qs, **kw) for d in (0, 1)]
                    out.append(ops.softmax_quantize(x, qs[:1], want_value=False, **kw))
                    return out

                return fn, (x, dq, w, b, QS(dev)), ()


for rows, cols in ((7, 40), (8, 256)):
    for op in ("add", "sub", "mul", "div"):
        @case(f"binary-{op}-{rows}x{cols}", ["ffq_binary_quantize"], host=False)
        def _(dev, rows=rows, cols=cols, op=op):
            a = real(dev, (rows, cols), BF16, 127, 1.0)
            b = (torch.rand(rows, cols, device=dev, generator=gen(dev, 128)) + 0.5).to(BF16)
            bias = (torch.rand(cols, device=dev, generator=gen(dev, 129)) + 0.5).to(BF16)
            ca, cb = codes(dev, (rows, cols), 130), codes(dev, (rows, cols), 131, 1, 100)
            pa, pb = one(dev, 0.05, 2.0), params(dev, rows, 132)

            def fn(a, b, bias, ca, cb, pa, pb, qs):
                return [ops.binary_quantize(op, a, b, qs), ops.binary_quantize(op, a, bias, qs, alpha=2 if op in ("add", "sub") else 1), ops.binary_quantize(op, a, 1.5, qs),
                        ops.binary_quantize(op, ca, cb, qs, dtype=BF16, a_dequant=pa, b_dequant=pb), ops.binary_quantize(op, ca.to(BF16), bias, (), dtype=BF16, a_dequant=pb)]

            return fn, (a, b, bias, ca, cb, pa, pb, QS(dev)), ()


for V, D, n in ((1, 16, 1), (50, 96, 42), (33, 256, 8)):
    @case(f"embedding-{V}x{D}-{n}", ["ffq_embedding_quantize"], host=False)
    def _(dev, V=V, D=D, n=n):
        table, table16 = codes(dev, (V, D), 133), codes(dev, (V, D), 134).to(BF16)
        ids = torch.randint(0, V, (n,), device=dev, generator=gen(dev, 135))
        (s1, o1), (sv, ov), (sg, og) = one(dev, 0.05, 2.0), params(dev, V, 136), params(dev, V * (D // 16), 137)

        def fn(table, table16, ids, s1, o1, sv, ov, sg, og, qs):
            return [ops.embedding_quantize(ids, table, s1, o1, False, D, BF16, qs), ops.embedding_quantize(ids.to(torch.int32), table, sv, ov, True, D, F16, qs),
                    ops.embedding_quantize(ids, table16, sg, None, True, 16, BF16, ())]

        return fn, (table, table16, ids, s1, o1, sv, ov, sg, og, QS(dev)), ()


POOLS = [((1, 3, 7, 7), (7, 7), (1, 1), (0, 0)), ((2, 5, 9, 11), (3, 3), (2, 2), (1, 1)), ((1, 16, 8, 8), (2, 2), (2, 2), (0, 0)), ((3, 2, 1, 13), (1, 3), (1, 2), (0, 1))]
for shape, kernel, stride, pad in POOLS:  # (the 7 x 7 head, odd maps, a 512-byte result, the 1-d pools as [B, C, 1, L])
    for form in ("plain", "int8", "container"):
        @case(f"pool-{'x'.join(map(str, shape))}-{form}", ["ffq_pool2d_quantize", "ffq_upsample_nearest_quantize"], host=False)
        def _(dev, shape=shape, kernel=kernel, stride=stride, pad=pad, form=form):
            x, dq = forms(dev, real(dev, shape, BF16, 138, 1.0))[form]
            per_channel = params(dev, shape[1], 139)

            def fn(x, dq, per_channel, qs):
                kw = dict(dtype=BF16, dequant=dq)
                out = [ops.pool2d_quantize(mode, x, kernel, stride, pad, (1, 1), ceil, qs, **kw) for mode in ("avg", "avg_exclude_pad", "max") for ceil in (False, True)]
                out += [ops.upsample_nearest_quantize(x, (shape[2] * 2, shape[3] * 3), None, m, qs, **kw) for m in ("nearest", "nearest-exact")]
                out.append(ops.upsample_nearest_quantize(x, (5, 3), None, "nearest", qs, **kw))
                if dq is not None:
                    out.append(ops.pool2d_quantize("max", x, kernel, stride, pad, (1, 1), False, qs, dtype=BF16, dequant=per_channel))
                return out

            return fn, (x, dq, per_channel, QS(dev)), ()


@case("cat-8-unequal-odd", ["ffq_cat_quantize"], host=False)
def _(dev):
    sizes = (1, 3, 5, 7, 9, 11, 13, 15)
    plain = [real(dev, (3, n, 5), BF16, 140 + i, 1.0) for i, n in enumerate(sizes)]
    mixed = [codes(dev, (3, n, 5), 150 + i) if i % 2 else plain[i] for i, n in enumerate(sizes)]
    dq = [one(dev, 0.03 + 0.01 * i, float(i)) if i % 2 else None for i in range(8)]

    def fn(plain, mixed, dq, qs):
        return [ops.cat_quantize(plain, 1, qs), ops.cat_quantize(plain, -2, ()), ops.cat_quantize(mixed, 1, qs, dtype=BF16, dequant=dq),
                ops.cat_quantize(plain + plain[:3], 1, qs[:1]), ops.cat_quantize([p.reshape(-1) for p in plain], 0, qs)]  # (11 inputs: two launches)

    return fn, (plain, mixed, dq, QS(dev)), ()


@case("cat-512-byte-rows", ["ffq_cat_quantize"], host=False)
def _(dev):
    xs = [real(dev, (4, 128), BF16, 160 + i, 1.0) for i in range(2)]
    return (lambda xs, qs: ops.cat_quantize(xs, 1, qs)), (xs, QS(dev)), ()


PADS = [("constant", (7, 9), (2, -3)), ("constant", (3, 7, 9), (-1, 2, 3, -2)), ("constant", (2, 3, 7, 9), (1, 1, -2, 3, 2, -1)), ("reflect", (5, 9), (3, 4)),
        ("reflect", (2, 3, 7, 9), (2, 1, 3, 0)), ("reflect", (1, 2, 4, 5, 6), (1, 2, 3, 1, 2, 0)), ("replicate", (5, 9), (3, 4)), ("replicate", (2, 3, 7, 9), (2, 1, 3, 0)),
        ("replicate", (1, 2, 4, 5, 6), (1, 2, 3, 1, 2, 0)), ("constant", (4, 60), (2, 2))]  # (the last: 4 x 64 bf16, 512 bytes)
for mode, shape, pad in PADS:
    @case(f"pad-{mode}-{'x'.join(map(str, shape))}-{'_'.join(map(str, pad))}", ["ffq_pad_quantize"], host=False)
    def _(dev, mode=mode, shape=shape, pad=pad):
        x = real(dev, shape, BF16, 170, 1.0)
        c, p = codes(dev, shape, 171), one(dev, 0.05, 2.0)
        return (lambda x, c, p, qs: [ops.pad_quantize(x, pad, mode, 1.5 if mode == "constant" else None, qs), ops.pad_quantize(c, pad, mode, None, qs[:1], dtype=BF16, dequant=p),
                                     ops.pad_quantize(c.to(BF16), pad, mode, None, (), dtype=BF16, dequant=p)]), (x, c, p, QS(dev)), ()


# ---- sdpa_quantize ----------------------------------------------------------------------------------------------------------------
SDPA_SLOTS = {"none": (), "output": ("output_quantizer",), "all": ("attn_scores_quantizer", "attn_mask_quantizer", "masked_scores_quantizer", "attn_weights_quantizer",
                                                                    "scaled_query_quantizer", "scaled_key_quantizer", "dropout_quantizer", "output_quantizer")}
for E in (64, 128):
    for L, S in ((1, 1), (1, 65), (63, 1), (65, 63), (64, 64)):
        for mask in ("none", "causal", "bool", "float"):
            @case(f"sdpa-E{E}-{L}x{S}-{mask}", ["ffq_sdpa_quantize"], host=False)
            def _(dev, E=E, L=L, S=S, mask=mask):
                g = torch.Generator().manual_seed(180)
                q, k, v = ((torch.randint(-8, 9, (1, 2, n, E), generator=g) * 2.0**-3).to(BF16).to(dev) for n in (L, S, S))
                k, v = k[:, :1].contiguous(), v[:, :1].contiguous()
                m = None
                if mask == "bool":
                    m = (torch.rand(L, S, generator=g) > 0.3).to(dev)
                    m[:, 0] = True
                elif mask == "float":
                    m = torch.randn(L, S, generator=g).to(BF16).to(dev)
                ps = {name: one(dev, 0.05, 1.0) for name in SDPA_SLOTS["all"]}

                def fn(q, k, v, m, ps):
                    out = []
                    for slots in SDPA_SLOTS.values():
                        quantizers = {name: (*ps[name], 8.0) for name in slots}
                        out.append(ops.sdpa_quantize(q, k, v, m, mask == "causal", None, float("-inf"), quantizers, want_codes="output_quantizer" in slots))
                    return out

                return fn, (q, k, v, m, ps), ()


for dtype, as_codes in ((F16, False), (BF16, True), (F16, True)):  # fp16 operands; q / k / v held as codes in the value dtype (deq_scale / deq_offset)
    for E, L, S, mask in ((64, 65, 63, "causal"), (128, 63, 65, "float"), (64, 1, 65, "bool"), (128, 129, 129, "causal-skip")):
        @case(f"sdpa-{NAME[dtype]}-{'codes' if as_codes else 'plain'}-E{E}-{L}x{S}-{mask}", ["ffq_sdpa_quantize"], host=False)
        def _(dev, dtype=dtype, as_codes=as_codes, E=E, L=L, S=S, mask=mask):
            g = torch.Generator().manual_seed(181)
            if as_codes:
                q, k, v = (torch.randint(-100, 101, (2, h, n, E), generator=g).to(dtype).to(dev) for h, n in ((4, L), (2, S), (2, S)))
            else:
                q, k, v = ((torch.randint(-8, 9, (2, h, n, E), generator=g) * 2.0**-3).to(dtype).to(dev) for h, n in ((4, L), (2, S), (2, S)))
            m = None
            if mask == "bool":
                m = (torch.rand(2, 1, L, S, generator=g) > 0.3).to(dev)
                m[..., 0] = True
            elif mask == "float":
                m = torch.randn(L, S, generator=g).to(dev)
            ps = {name: one(dev, 0.05, 1.0) for name in SDPA_SLOTS["all"]}
            dq = [one(dev, 0.01, 2.0), (one(dev, 0.012)[0], None), one(dev, 0.008, -1.0)] if as_codes else [None, None, None]

            def fn(q, k, v, m, ps, dq):
                out = []
                for slots in SDPA_SLOTS.values():
                    quantizers = {name: (*ps[name], 8.0) for name in slots}
                    out.append(ops.sdpa_quantize(q, k, v, m, mask.startswith("causal"), None, float("-inf"), quantizers, dq, want_codes="output_quantizer" in slots,
                                                 skip_above_diagonal=mask == "causal-skip"))
                return out

            return fn, (q, k, v, m, ps, dq), ()


# ---- convolutions -----------------------------------------------------------------------------------------------------------------
CONVS = [(1, 3, 1, 5, 5, 3, 1, 1, 1), (2, 16, 64, 9, 11, 3, 2, 1, 1), (1, 20, 129, 7, 6, 3, 1, 2, 2), (2, 16, 64, 8, 8, 1, 1, 0, 1), (1, 5, 129, 6, 7, (1, 3), (2, 1), (0, 1), 1)]
for B, C, OC, H, W, kernel, stride, pad, dil in CONVS:  # OC 1 / 64 / 129, C a multiple of 16 and not, (2, 64, 8, 8) fp32: whole 512-byte blocks
    for nhwc in (False, True):
        @case(f"conv2d-{B}x{C}x{H}x{W}-oc{OC}-{'nhwc' if nhwc else 'nchw'}", ["ffq_conv2d_w8a8"], host=False)
        def _(dev, B=B, C=C, OC=OC, H=H, W=W, kernel=kernel, stride=stride, pad=pad, dil=dil, nhwc=nhwc):
            kh, kw = (kernel, kernel) if isinstance(kernel, int) else kernel
            x, w = codes(dev, (B, C, H, W), 190, -20, 20), codes(dev, (OC, C, kh, kw), 191, -20, 20)
            if nhwc:
                x = x.contiguous(memory_format=torch.channels_last)
            (sx, ox), sw, (so, oo) = one(dev, 0.02, 3.0), torch.rand(OC, device=dev, generator=gen(dev, 192)) * 0.01 + 0.001, one(dev, 0.5, -2.0)
            bias = real(dev, (OC,), BF16, 193, 1.0)

            def fn(x, w, sx, ox, sw, so, oo, bias):
                return [ops.conv2d_w8a8(x, w, sx, ox, sw, None, bias, stride, pad, dil), ops.conv2d_w8a8(x, w, sx, ox, sw, None, None, stride, pad, dil, F32),
                        ops.conv2d_w8a8(x, w, sx, ox, sw, None, bias, stride, pad, dil, I8, so, oo)]

            return fn, (x, w, sx, ox, sw, so, oo, bias), ()


CONVTS = [(1, 3, 1, 4, 4, 3, 1, 0, 0, 1), (2, 16, 64, 5, 6, 3, 2, 1, 1, 1), (1, 20, 129, 4, 5, 2, 3, 0, 2, 1), (1, 16, 64, 4, 4, 1, 2, 0, 1, 1), (1, 5, 129, 3, 4, 3, 2, 1, 0, 2)]
for B, C, OC, H, W, kernel, stride, pad, outpad, dil in CONVTS:  # (kernel < stride: empty phases; output_padding; dilation)
    for nhwc in (False, True):
        @case(f"conv-transpose2d-{B}x{C}x{H}x{W}-oc{OC}-k{kernel}s{stride}-{'nhwc' if nhwc else 'nchw'}", ["ffq_conv_transpose2d_w8a8"], host=False)
        def _(dev, B=B, C=C, OC=OC, H=H, W=W, kernel=kernel, stride=stride, pad=pad, outpad=outpad, dil=dil, nhwc=nhwc):
            x, w = codes(dev, (B, C, H, W), 194, -20, 20), codes(dev, (C, OC, kernel, kernel), 195, -20, 20)
            if nhwc:
                x = x.contiguous(memory_format=torch.channels_last)
            (sx, ox), sw, (so, oo) = one(dev, 0.02, 3.0), torch.rand(OC, device=dev, generator=gen(dev, 196)) * 0.01 + 0.001, one(dev, 0.5, -2.0)
            bias = real(dev, (OC,), BF16, 197, 1.0)

            def fn(x, w, sx, ox, sw, so, oo, bias):
                return [ops.conv_transpose2d_w8a8(x, w, sx, ox, sw, None, bias, stride, pad, outpad, dil), ops.conv_transpose2d_w8a8(x, w, sx, ox, sw, None, None, stride, pad, outpad, dil, F32),
                        ops.conv_transpose2d_w8a8(x, w, sx, ox, sw, None, bias, stride, pad, outpad, dil, I8, so, oo)]

            return fn, (x, w, sx, ox, sw, so, oo, bias), ()


GUARDED = frozenset(s for c in CASES for s in c.symbols)  # what the cases claim; check_call verifies each claim in every case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_memory_contract(case):
    fn, inputs, inplace = case.build("cuda")
    guards.check_call(fn, inputs, inplace, case.symbols, workspace_image=case.workspace_image)


def test_a_flipped_guard_byte_is_flagged():
    """Sensitivity on the device without any fault: after a genuine guarded call, a plain indexed write by the test flips one guard
    byte of the test's own arena buffer; the verdict must name I1 (and nothing else)."""
    x, (s, o) = real("cuda", (24, 64), BF16, 1), one("cuda")
    fn = lambda x, s, o: ops.quantize_by_tile(x, s, (24, 64), 8, I8, o)  # noqa: E731
    run = guards.guarded_run(fn, (x, s, o), set(), _native.library(), guards.POISON_A)
    assert guards.verdict(run) == []
    out = next(b for b in run.arena.blocks if b.kind == "fresh")
    out.chunk[out.start + out.nbytes] ^= 0x55  # the first byte after the codes
    found = guards.verdict(run)
    assert len(found) == 1 and found[0].startswith("I1 ") and "+0 after" in found[0], found
