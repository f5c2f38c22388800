"""Generate wq_plan.json: what the plan queries of the weight-only GEMM answer on a machine without a GPU (the library then plans
for 256 CUs, the MI355X's count).

    python tests/golden/gen_wq_plan.py <path to libffq_hip.so> [output file]

Run on the build of the commit whose plan is to be pinned (the table in the tree was taken from the parent of the commit that added
it). One row per (M, N, K, mlp) of the grid below — it crosses every form boundary: 16 / 17, 32 / 33, 256 / 257 and 512 / 513 rows,
N = 8192, 1536 tokens with 144 tiles, 4096 tokens — mlp = 1 only where N % 128 == 0:

    [M, N, K, mlp, split, tickets, slab_bytes(split), slab_bytes(2), slab_bytes(4), workspace_bytes]

with workspace_bytes = ffq_mlp_gate_up_wq_workspace_bytes for mlp = 1, ffq_linear_wq_workspace_bytes otherwise.
tests/test_wq_cpu.py compares the library of the tree with the table, row for row.
"""

from __future__ import annotations

import ctypes
import json
import pathlib
import sys

MS = (1, 7, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 300, 512, 513, 1024, 1536, 2048, 3072, 4096, 8191)
NS = (128, 256, 1000, 1024, 4096, 6144, 8192, 14336, 28672)
KS = (128, 192, 256, 512, 1152, 4096, 8192, 14336)


def bind(path):
    lib = ctypes.CDLL(str(path))
    i64, i, sz = ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
    for name, res, args in (
        ("ffq_linear_wq_split", i64, [i64, i64, i64, i]),
        ("ffq_linear_wq_tickets", i64, [i64, i64, i64, i]),
        ("ffq_linear_wq_slab_bytes", sz, [i64, i64, i64, i, i64]),
        ("ffq_linear_wq_workspace_bytes", sz, [i64, i64, i64]),
        ("ffq_mlp_gate_up_wq_workspace_bytes", sz, [i64, i64, i64]),
    ):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def grid():
    return [(M, N, K, mlp) for M in MS for N in NS for K in KS for mlp in (0, 1) if not (mlp and N % 128)]


def row(lib, M, N, K, mlp):
    split = lib.ffq_linear_wq_split(M, N, K, mlp)
    workspace = lib.ffq_mlp_gate_up_wq_workspace_bytes(M, N, K) if mlp else lib.ffq_linear_wq_workspace_bytes(M, N, K)
    return [M, N, K, mlp, split, lib.ffq_linear_wq_tickets(M, N, K, mlp), lib.ffq_linear_wq_slab_bytes(M, N, K, mlp, split),
            lib.ffq_linear_wq_slab_bytes(M, N, K, mlp, 2), lib.ffq_linear_wq_slab_bytes(M, N, K, mlp, 4), workspace]


def table(lib):
    return [row(lib, *case) for case in grid()]


if __name__ == "__main__":
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    out = pathlib.Path(sys.argv[2]) if len(sys.argv) > 2 else pathlib.Path(__file__).resolve().parent / "wq_plan.json"
    rows = table(bind(sys.argv[1]))
    out.write_text("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]\n")
    print(f"{len(rows)} rows, {sum(r[4] > 1 for r in rows)} with a split above 1 -> {out}")
