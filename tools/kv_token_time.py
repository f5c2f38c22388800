"""Timing of the KV cache with per-token dynamic scales on one MI355X, by the procedure of tools/kv_cache_time.py: every arm is captured
as a graph of several calls and timed with device events around replays, the arms alternate within every round on one device in one
call, and the median with the smallest and largest round is printed as one JSON line per shape.

  decode   ``ops.kv_token_decode`` against ``ops.kv_decode`` over the same codes at B 8, H 32 / HKV 8, E 128 and E 64, every length
           equal to S. The per-row form reads 16 more bytes per key and kv head: +6.25 % of the K + V bytes at E = 128, +12.5 % at
           E = 64 (``extra_bytes_ratio``); ``ratio`` is the measured one, ``spread`` the largest (max - min) / median among the arms.
           ``--other-library PATH`` adds ``ops.kv_decode`` of another build of libffq_hip.so (the parent commit's) as two further arms,
           first and last in every round: the same kernel at two places shows what the order does, and ``dense_vs_other`` compares this
           build's dense decode with it.
  append   ``ops.kv_token_append`` against ``ops.kv_append`` for one new token (L = 1) and for a prompt of 512 rows.

    python tools/kv_token_time.py [--other-library PATH] [--keys 4096 32768] [--output profiles/kv_token_time.txt]
"""

from __future__ import annotations

import argparse
import json
import pathlib
import sys

import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from fastforward_amd import _native, ops  # noqa: E402
from fastforward_amd._cabi import FFQLibrary  # noqa: E402
from kv_cache_time import alternate  # noqa: E402

DEV = "cuda"


def spread(arms: dict) -> float:
    return round(max((a["max_us"] - a["min_us"]) / a["median_us"] for a in arms.values()), 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--other-library", type=pathlib.Path, default=None)
    ap.add_argument("--keys", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--output", type=pathlib.Path, default=ROOT / "profiles" / "kv_token_time.txt")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    this = _native.library()
    other = FFQLibrary(args.other_library) if args.other_library else None
    lines = []

    def emit(**record):
        lines.append(json.dumps(record))
        print(lines[-1], flush=True)

    def with_other(fn):
        def run():
            _native._LIB = other
            try:
                return fn()
            finally:
                _native._LIB = this
        return run

    B, HKV, G, dt = 8, 8, 4, torch.bfloat16
    gen = torch.Generator().manual_seed(0)
    ks, vs = (torch.tensor([0.031], device=DEV), torch.tensor([3.0], device=DEV)), (torch.tensor([0.027], device=DEV), torch.tensor([-9.0], device=DEV))
    for E in (128, 64):
        for S in args.keys:
            q = torch.randn(B, HKV * G, 1, E, generator=gen).to(dt).to(DEV)
            kc, vc = (torch.randint(-128, 128, (B, HKV, S, E), generator=gen).to(torch.int8).to(DEV) for _ in range(2))
            params = torch.tensor([0.031, 3.0, 0.027, -9.0], device=DEV).repeat(B, HKV, S, 1).contiguous()
            lens = torch.full((B,), S, dtype=torch.int32, device=DEV)
            deq = (None, ks, vs)

            def dense():
                return ops.kv_decode(q, kc, vc, lens, dequant=deq)

            arms = {"kv_token_decode": lambda: ops.kv_token_decode(q, kc, vc, params, lens), "kv_decode": dense}
            if other is not None:
                arms = {"kv_decode_other_first": with_other(dense), **arms, "kv_decode_other_last": with_other(dense)}
            same = all(torch.equal(fn(), dense()) for fn in arms.values())
            times = alternate(arms, reps=20, replays=20, rounds=9)
            extra = dict(ratio=round(times["kv_token_decode"]["median_us"] / times["kv_decode"]["median_us"], 4), extra_bytes_ratio=1 + 16 / (2 * E),
                         spread=spread(times))
            if other is not None:
                extra["dense_vs_other"] = round(2 * times["kv_decode"]["median_us"] / (times["kv_decode_other_first"]["median_us"] + times["kv_decode_other_last"]["median_us"]), 4)
            emit(what="decode", S=S, B=B, HKV=HKV, G=G, E=E, splits=ops.sdpa_decode_plan(B, HKV, S, G, E), bit_equal=same, cache_bytes=2 * B * HKV * S * E,
                 param_bytes=16 * B * HKV * S, **times, **extra)
            del q, params
            for L in (1, 512):
                k_new, v_new = (torch.randn(B, HKV, L, E, generator=gen).to(dt).to(DEV) for _ in range(2))
                grown = torch.full((B,), min(S, 2048) + L, dtype=torch.int32, device=DEV)
                store = torch.zeros(B, HKV, S + L, 4, device=DEV)
                pre_k, pre_v = (torch.zeros(B, HKV, S + L, E, dtype=torch.int8, device=DEV) for _ in range(2))
                kp, vp = (ks[0], ks[1], 8.0), (vs[0], vs[1], 8.0)
                arms = {"kv_token_append": lambda: ops.kv_token_append(k_new, v_new, pre_k, pre_v, store, grown, (8, False), (8, False)),
                        "kv_append": lambda: ops.kv_append(k_new, v_new, pre_k, pre_v, grown, kp, vp)}
                times = alternate(arms, reps=10, replays=20, rounds=9)
                emit(what="append", S=S, L=L, E=E, row_bytes=2 * B * HKV * L * E * 3, param_bytes=16 * B * HKV * L,
                     ratio=round(times["kv_token_append"]["median_us"] / times["kv_append"]["median_us"], 4), spread=spread(times), **times)
                del k_new, v_new, store, pre_k, pre_v
            del kc, vc
            torch.cuda.empty_cache()
    args.output.parent.mkdir(parents=True, exist_ok=True)
    args.output.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
