"""What the block table costs the decode attention on one MI355X: ``ops.kv_paged_decode`` at page sizes 16 and 128 against
``ops.kv_decode`` on the same codes laid out densely, at the same split count, in one process.

The pages of every sequence are a seeded permutation of the pool (no two logical neighbours are physical neighbours by more than
chance), the lengths are all equal to the capacity or ragged between 512 and it. Each arm is captured as a graph of several calls and
timed with device events around replays (tools/kv_cache_time.py: the figure is the kernels' time, not the Python around each
enqueue); the arms alternate within every round, and the median with the smallest and largest round is printed as one JSON line per
shape. ``--other-library PATH`` adds ``ops.kv_decode`` of another build of libffq_hip.so (the parent commit's) as two further arms,
first and last in every round: the same code at two places shows what the order does, and the two builds' dense kernels are compared.

    python tools/kv_paged_time.py [--other-library PATH] [--batches 8 64] [--keys 4096]
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


def pools_of(dense: torch.Tensor, P: int, perm: torch.Tensor) -> torch.Tensor:
    """dense [B, H, C, E] cut into pages [B * C / P, H, P, E], page i of the row-major order stored at pool page perm[i]."""
    Bd, H, Cd, E = dense.shape
    pages = dense.view(Bd, H, Cd // P, P, E).permute(0, 2, 1, 3, 4).reshape(Bd * (Cd // P), H, P, E)
    pool = torch.empty_like(pages)
    pool[perm] = pages
    return pool


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--other-library", type=pathlib.Path, default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--keys", type=int, default=4096)
    ap.add_argument("--pages", type=int, nargs="+", default=[16, 128])
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

    HKV, G, E, dt, cap = 8, 4, 128, torch.bfloat16, args.keys
    gen = torch.Generator().manual_seed(0)
    deq = (None, (torch.tensor([0.031], device=DEV), torch.tensor([3.0], device=DEV)), (torch.tensor([0.027], device=DEV), torch.tensor([-9.0], device=DEV)))
    for Bt in args.batches:
        q = torch.randn(Bt, HKV * G, 1, E, generator=gen).to(dt).to(DEV)
        kc, vc = (torch.randint(-128, 128, (Bt, HKV, cap, E), generator=gen, dtype=torch.int8).to(DEV) for _ in range(2))
        paged = {}
        for P in args.pages:
            perm = torch.randperm(Bt * (cap // P), generator=gen).to(DEV)
            paged[P] = (pools_of(kc, P, perm), pools_of(vc, P, perm), perm.view(Bt, cap // P).to(torch.int32).contiguous())
        ragged = torch.randint(512, cap + 1, (Bt,), generator=gen).to(torch.int32)
        for name, host_lens in (("uniform", torch.full((Bt,), cap, dtype=torch.int32)), ("ragged", ragged)):
            lens = host_lens.to(DEV)

            def dense():
                return ops.kv_decode(q, kc, vc, lens, dequant=deq)

            arms = {"kv_decode": dense}
            for P, (kp, vp, table) in paged.items():
                arms[f"kv_paged_decode_P{P}"] = lambda kp=kp, vp=vp, table=table: ops.kv_paged_decode(q, kp, vp, lens, table, dequant=deq)
            if other is not None:
                arms = {"kv_decode_other_first": with_other(dense), **arms, "kv_decode_other_last": with_other(dense)}
            want = dense()
            same = all(torch.equal(fn(), want) for fn in arms.values())
            keys = int(host_lens.sum())
            print(json.dumps(dict(what="decode", lengths=name, B=Bt, HKV=HKV, G=G, E=E, capacity=cap, keys=keys, code_bytes=2 * keys * HKV * E,
                                  splits=ops.sdpa_decode_plan(Bt, HKV, cap, G, E), bit_equal=same, **alternate(arms, reps=20, replays=20, rounds=9))),
                  flush=True)
        del kc, vc, paged
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
