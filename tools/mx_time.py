"""Timing of the MX kernels on one MI355X, by the procedure of tools/kv_token_time.py: every arm is captured as a graph of several calls and
timed with device events around replays, the arms alternate within every round on one device in one call, and the median with the
smallest and largest round is printed as one JSON line per shape.

  linear     ``ops.linear_mx`` for the three format pairs against ``ops.linear_w8a8`` (the int8 GEMM: this library's, whose source the MX
             work does not touch) at the four Llama-3-8B weight shapes with `--tokens` rows, bf16 output, no bias, operands quantized
             ahead of the timed region. ``ratio_*`` is that pair's median over ``w8a8``'s: the target for (e2m1, e2m1) is 1.0 or below.
  quantizer  ``ops.mx_quantize`` (e4m3 bytes; e2m1 bytes + packed; e2m1 packed only) beside plain A1 (``ops.quantize_by_tile`` into int8,
             per-tensor) on bf16 ``[8, 2048, 4096]`` and ``[14336, 4096]``: microseconds and ``fraction_of_8TBs`` = bytes moved / median /
             8e12 (each arm's own bytes: 2 per element in, its containers and scale bytes out).

    python tools/mx_time.py [--tokens 16384] [--output profiles/mx_time.txt]
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

from fastforward_amd import ops  # noqa: E402
from kv_cache_time import alternate  # noqa: E402
from kv_token_time import spread  # noqa: E402

DEV = "cuda"
SHAPES = {"q_o_proj": (4096, 4096), "k_v_proj": (1024, 4096), "gate_up_proj": (14336, 4096), "down_proj": (4096, 14336)}  # name -> (N, K)
PAIRS = (("e4m3", "e4m3"), ("e4m3", "e2m1"), ("e2m1", "e2m1"))


def gemm_operand(t: torch.Tensor, fmt: str):
    codes, packed, scales = ops.mx_quantize(t, fmt, codes=fmt == "e4m3", packed=fmt == "e2m1")
    return (packed if fmt == "e2m1" else codes), scales


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tokens", type=int, default=16384)
    ap.add_argument("--output", type=pathlib.Path, default=ROOT / "profiles" / "mx_time.txt")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    lines = []

    def emit(**record):
        lines.append(json.dumps(record))
        print(lines[-1], flush=True)

    dt = torch.bfloat16
    torch.manual_seed(0)
    M = args.tokens
    with torch.no_grad():
        for name, (N, K) in SHAPES.items():
            x = torch.randn(M, K, device=DEV).to(dt)
            w = (0.02 * torch.randn(N, K, device=DEV)).to(dt)
            xs, ws = x.float().abs().amax().reshape(1) / 127.0, (w.float().abs().amax(1) / 127.0).contiguous()
            xq = ops.quantize_by_tile(x, xs, x.shape, 8, torch.int8)
            wq = ops.quantize_by_tile(w, ws, (1, K), 8, torch.int8)
            held = {fmt: (gemm_operand(x, fmt), gemm_operand(w, fmt)) for fmt in ("e4m3", "e2m1")}
            arms = {"w8a8": lambda: ops.linear_w8a8(xq, wq, xs, None, ws, None, out_dtype=dt)}
            for fa, fw in PAIRS:
                (a, sa), (b, sb) = held[fa][0], held[fw][1]
                arms[f"{fa}_{fw}"] = lambda a=a, sa=sa, fa=fa, b=b, sb=sb, fw=fw: ops.linear_mx(a, sa, fa, b, sb, fw, out_dtype=dt)
            reference = torch.nn.functional.linear(x, w).float()
            error = {k: round(float((fn().float() - reference).abs().mean()), 5) for k, fn in arms.items()}
            times = alternate(arms, reps=3, replays=5, rounds=7)
            emit(what="linear", shape=name, tokens=M, N=N, K=K, ops=2 * M * N * K, mean_abs_error_vs_float=error,
                 **{f"ratio_{fa}_{fw}": round(times[f"{fa}_{fw}"]["median_us"] / times["w8a8"]["median_us"], 4) for fa, fw in PAIRS},
                 tera_ops={k: round(2 * M * N * K / (v["median_us"] * 1e-6) / 1e12, 1) for k, v in times.items()}, spread=spread(times), **times)
            del x, w, xq, wq, held, arms, reference
            torch.cuda.empty_cache()
        for shape in ((8, 2048, 4096), (14336, 4096)):
            x = (torch.randn(*shape, device=DEV) * 0.5).to(dt)
            n = x.numel()
            one = x.float().abs().amax().reshape(1) / 127.0
            arms = {"a1_int8": lambda: ops.quantize_by_tile(x, one, x.shape, 8, torch.int8),
                    "mx_e4m3": lambda: ops.mx_quantize(x, "e4m3"),
                    "mx_e2m1_both": lambda: ops.mx_quantize(x, "e2m1", codes=True, packed=True),
                    "mx_e2m1_packed": lambda: ops.mx_quantize(x, "e2m1", codes=False, packed=True)}
            nbytes = {"a1_int8": 3 * n, "mx_e4m3": 3 * n + n // 32, "mx_e2m1_both": 3 * n + n // 2 + n // 32, "mx_e2m1_packed": 2 * n + n // 2 + n // 32}
            times = alternate(arms, reps=10, replays=10, rounds=9)
            emit(what="quantizer", shape=list(shape), bytes=nbytes, fraction_of_8TBs={k: round(nbytes[k] / (v["median_us"] * 1e-6) / 8e12, 4) for k, v in times.items()},
                 spread=spread(times), **times)
            del x, arms
            torch.cuda.empty_cache()
    args.output.parent.mkdir(parents=True, exist_ok=True)
    args.output.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
