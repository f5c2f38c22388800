"""Timing of the preallocated KV cache on one MI355X: ``ops.kv_decode`` with every length equal to S against ``ops.sdpa_decode`` at the
same shape (both run the same kernels over the same ranges), and the in-place ``ops.kv_append`` of one token against the step it
replaces (the two quantizer calls + the code-level ``cat`` of K and V).

Each arm is captured as a graph of several calls and timed with device events around replays, so the figure is the kernels' time and
not the Python around each enqueue; the arms alternate within every round, and the median with the smallest and largest round is
printed as one JSON line per shape. ``--other-library PATH`` adds ``ops.sdpa_decode`` of another build of libffq_hip.so (the parent
commit's, for instance) as two further arms, first and last in every round: the same code at two places shows what the order does.

    python tools/kv_cache_time.py [--other-library PATH] [--keys 4096 32768]
"""

from __future__ import annotations

import argparse
import json
import pathlib
import statistics
import sys

import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import fastforward_amd as ff  # noqa: E402

from fastforward_amd import _native, ops  # noqa: E402
from fastforward_amd._cabi import FFQLibrary  # noqa: E402

DEV = "cuda"


def graphed(fn, reps):
    """`reps` calls of fn captured in one graph."""
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        for _ in range(reps):
            fn()
    return graph


def timed(graph, replays, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(replays):
        graph.replay()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / (replays * reps)  # us per call


def alternate(arms, reps, replays, rounds):
    graphs = {name: graphed(fn, reps) for name, fn in arms.items()}
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    samples = {name: [] for name in arms}
    for _ in range(rounds):
        for name, g in graphs.items():
            samples[name].append(timed(g, replays, reps))
    return {name: dict(median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2)) for name, v in samples.items()}


def quantizer(bits, scale, offset):
    q = ff.nn.LinearQuantizer(bits, symmetric=False, granularity=ff.PerTensor(), quantized_dtype=torch.int8, device=DEV)
    q.quantization_range = (torch.tensor(-1.0, device=DEV), torch.tensor(1.0, device=DEV))
    with torch.no_grad():
        q.scale.fill_(scale)
        q.offset.fill_(offset)
    return q


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--other-library", type=pathlib.Path, default=None)
    ap.add_argument("--keys", type=int, nargs="+", default=[4096, 32768])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    this = _native.library()
    other = FFQLibrary(args.other_library) if args.other_library else None

    def with_other(fn):
        def run():
            _native._LIB = other
            try:
                return fn()
            finally:
                _native._LIB = this
        return run

    B, HKV, G, E, dt = 8, 8, 4, 128, torch.bfloat16
    gen = torch.Generator().manual_seed(0)
    ks, vs = (torch.tensor([0.031], device=DEV), torch.tensor([3.0], device=DEV)), (torch.tensor([0.027], device=DEV), torch.tensor([-9.0], device=DEV))
    for S in args.keys:
        q = torch.randn(B, HKV * G, 1, E, generator=gen).to(dt).to(DEV)
        kc, vc = (torch.randint(-128, 128, (B, HKV, S, E), generator=gen).to(torch.int8).to(DEV) for _ in range(2))
        lens = torch.full((B,), S, dtype=torch.int32, device=DEV)
        deq = (None, ks, vs)

        def dense():
            return ops.sdpa_decode(q, kc, vc, dequant=deq)

        arms = {"kv_decode": lambda: ops.kv_decode(q, kc, vc, lens, dequant=deq), "sdpa_decode": dense}
        if other is not None:
            arms = {"sdpa_decode_other_first": with_other(dense), **arms, "sdpa_decode_other_last": with_other(dense)}
        same = all(torch.equal(fn(), dense()) for fn in arms.values())
        print(json.dumps(dict(what="decode", S=S, B=B, HKV=HKV, G=G, E=E, splits=ops.sdpa_decode_plan(B, HKV, S, G, E), bit_equal=same,
                              cache_bytes=2 * B * HKV * S * E, **alternate(arms, reps=20, replays=20, rounds=9))), flush=True)
        # the step's cache update: one in-place append of L = 1 against quantize + code-level cat of both tensors
        kq, vq = quantizer(8, 0.031, 3.0), quantizer(8, 0.027, -9.0)
        k_new, v_new = (torch.randn(B, HKV, 1, E, generator=gen).to(dt).to(DEV) for _ in range(2))
        pre_k, pre_v = (torch.zeros(B, HKV, S + 1, E, dtype=torch.int8, device=DEV) for _ in range(2))
        pre_k[:, :, :S], pre_v[:, :, :S] = kc, vc
        grown = torch.full((B,), S + 1, dtype=torch.int32, device=DEV)
        kp, vp = (kq.scale.detach(), kq.offset.detach(), 8.0), (vq.scale.detach(), vq.offset.detach(), 8.0)
        K, V = kq.wrap_codes(kc, dt), vq.wrap_codes(vc, dt)

        def cat_step():
            with torch.no_grad():
                return torch.cat([K, kq(k_new)], dim=2), torch.cat([V, vq(v_new)], dim=2)

        def append_step():
            grown.add_(0)  # (the caller's own length update; 0 keeps the position fixed over the repeats)
            ops.kv_append(k_new, v_new, pre_k, pre_v, grown, kp, vp)

        got = cat_step()
        append_step()
        same = torch.equal(got[0].raw_data, pre_k) and torch.equal(got[1].raw_data, pre_v)
        new_row_bytes = 2 * B * HKV * E * 3  # K and V: 2 bytes read + 1 written per element
        print(json.dumps(dict(what="append", S=S, bit_equal=same, append_bytes=new_row_bytes, cat_bytes=2 * 2 * B * HKV * S * E + new_row_bytes,
                              **alternate({"kv_append": append_step, "quantize_and_cat": cat_step}, reps=5, replays=20, rounds=7))), flush=True)
        del kc, vc, pre_k, pre_v, K, V, got
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
