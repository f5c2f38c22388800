"""Timing of the paged KV cache with per-token dynamic scales on one MI355X, by the procedure of tools/kv_token_time.py: every arm is
captured as a graph of several calls and timed with device events around replays, the arms alternate within every round on one device
in one call, and the median with the smallest and largest round is printed as one JSON line per shape.

The shape is tools/kv_paged_time.py's: B 64, 32 query / 8 kv heads, E 128 and 64, capacity 4096, every length at the capacity; the pages
of every sequence are a seeded permutation of the pool.

  decode   ``ops.kv_paged_token_decode`` at P = 128 and P = 16 beside its three yardsticks on the same codes and (uniform) parameters:
           ``ops.kv_token_decode`` laid out densely, ``ops.kv_paged_decode`` at both page sizes, and ``ops.kv_decode``. From the bytes
           the new decode should take about the dense token time multiplied by the paged / dense ratio the static pair shows in the same
           run (``expected_us_P*``); ``margin`` is the largest (max - min) / median among the run's arms, and ``within_margin_P*`` says
           whether the measured median stays below expected * (1 + margin). ``--other-library PATH`` adds ``ops.kv_token_decode`` of
           another build of libffq_hip.so (the parent commit's) as two further arms, first and last in every round;
           ``token_vs_other`` compares this build's dense token decode with it.
  append   ``ops.kv_paged_token_append`` at both page sizes against ``ops.kv_token_append`` for one new token (L = 1) and for a prompt
           of 512 rows.

    python tools/kv_paged_token_time.py [--other-library PATH] [--batch 64] [--keys 4096] [--output profiles/kv_paged_token_time.txt]
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
from kv_cache_time import DEV, alternate  # noqa: E402
from kv_paged_time import pools_of  # noqa: E402
from kv_token_time import spread  # noqa: E402

PAGES = (128, 16)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--other-library", type=pathlib.Path, default=None)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--keys", type=int, default=4096)
    ap.add_argument("--output", type=pathlib.Path, default=ROOT / "profiles" / "kv_paged_token_time.txt")
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

    B, HKV, G, dt, cap = args.batch, 8, 4, torch.bfloat16, args.keys
    gen = torch.Generator().manual_seed(0)
    one = torch.tensor([0.031, 3.0, 0.027, -9.0], device=DEV)
    ks, vs = (one[0:1].clone(), one[1:2].clone()), (one[2:3].clone(), one[3:4].clone())
    deq = (None, ks, vs)
    for E in (128, 64):
        q = torch.randn(B, HKV * G, 1, E, generator=gen).to(dt).to(DEV)
        kc, vc = (torch.randint(-128, 128, (B, HKV, cap, E), generator=gen, dtype=torch.int8).to(DEV) for _ in range(2))
        params = one.repeat(B, HKV, cap, 1).contiguous()
        lens = torch.full((B,), cap, dtype=torch.int32, device=DEV)
        paged = {}
        for P in PAGES:
            perm = torch.randperm(B * (cap // P), generator=gen).to(DEV)
            paged[P] = (pools_of(kc, P, perm), pools_of(vc, P, perm), pools_of(params, P, perm), perm.view(B, cap // P).to(torch.int32).contiguous())

        def token():
            return ops.kv_token_decode(q, kc, vc, params, lens)

        arms = {"kv_decode": lambda: ops.kv_decode(q, kc, vc, lens, dequant=deq), "kv_token_decode": token}
        for P, (kp, vp, pp, table) in paged.items():
            arms[f"kv_paged_decode_P{P}"] = lambda kp=kp, vp=vp, table=table: ops.kv_paged_decode(q, kp, vp, lens, table, dequant=deq)
            arms[f"kv_paged_token_decode_P{P}"] = lambda kp=kp, vp=vp, pp=pp, table=table: ops.kv_paged_token_decode(q, kp, vp, pp, lens, table)
        if other is not None:
            arms = {"kv_token_decode_other_first": with_other(token), **arms, "kv_token_decode_other_last": with_other(token)}
        want = token()
        same = all(torch.equal(fn(), want) for fn in arms.values())
        times = alternate(arms, reps=20, replays=20, rounds=9)
        margin = spread(times)
        extra = dict(margin=margin)
        for P in PAGES:
            expected = times["kv_token_decode"]["median_us"] * times[f"kv_paged_decode_P{P}"]["median_us"] / times["kv_decode"]["median_us"]
            measured = times[f"kv_paged_token_decode_P{P}"]["median_us"]
            extra[f"expected_us_P{P}"] = round(expected, 2)
            extra[f"measured_over_expected_P{P}"] = round(measured / expected, 4)
            extra[f"within_margin_P{P}"] = measured <= expected * (1 + margin)
        if other is not None:
            both = times["kv_token_decode_other_first"]["median_us"] + times["kv_token_decode_other_last"]["median_us"]
            extra["token_vs_other"] = round(2 * times["kv_token_decode"]["median_us"] / both, 4)
        emit(what="decode", B=B, HKV=HKV, G=G, E=E, capacity=cap, splits=ops.sdpa_decode_plan(B, HKV, cap, G, E), bit_equal=same,
             code_bytes=2 * B * HKV * cap * E, param_bytes=16 * B * HKV * cap, **times, **extra)
        del q, arms
        for L in (1, 512):
            k_new, v_new = (torch.randn(B, HKV, L, E, generator=gen).to(dt).to(DEV) for _ in range(2))
            grown = torch.full((B,), min(cap, 2048) + L, dtype=torch.int32, device=DEV)
            arms = {"kv_token_append": lambda: ops.kv_token_append(k_new, v_new, kc, vc, params, grown, (8, False), (8, False))}
            for P, (kp, vp, pp, table) in paged.items():
                arms[f"kv_paged_token_append_P{P}"] = lambda kp=kp, vp=vp, pp=pp, table=table: ops.kv_paged_token_append(
                    k_new, v_new, kp, vp, pp, grown, table, (8, False), (8, False))
            times = alternate(arms, reps=10, replays=20, rounds=9)
            ratios = {f"ratio_P{P}": round(times[f"kv_paged_token_append_P{P}"]["median_us"] / times["kv_token_append"]["median_us"], 4) for P in PAGES}
            emit(what="append", B=B, HKV=HKV, L=L, E=E, capacity=cap, row_bytes=2 * B * HKV * L * E * 3, param_bytes=16 * B * HKV * L, spread=spread(times),
                 **ratios, **times)
            del k_new, v_new, arms
        del kc, vc, params, paged
        torch.cuda.empty_cache()
    args.output.parent.mkdir(parents=True, exist_ok=True)
    args.output.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
