"""Timing of the LPBQ weight path on one MI355X, by the procedure of tools/kv_token_time.py: every arm is captured as a graph of several
calls and timed with device events around replays, the arms alternate within every round on one device in one call, and the median
with the smallest and largest round is printed as one JSON line per shape.

  layer      a ``QuantizedLinear`` (bf16, no bias, A8 per-tensor input quantizer, W4 weight quantizer with blocks of 128 input channels) at
             the four Llama-3-8B weight shapes with `--tokens` rows:
               wq             the unconverted layer: A1 of the input, A1 of the weight, ``ops.linear_wq`` on the dequantized input;
               lpbq           the same layer after ``quantization.lpbq.convert_model``: A1 of the input, ``ffq_lpbq_quantize``,
                              ``ops.linear_w8a8``;
               lpbq_held      the same layer with the weight held expanded: A1 of the input and the int8 GEMM only.
             ``ratio_lpbq`` / ``ratio_held`` are those arms' medians over ``wq``'s; ``spread`` is the largest (max - min) / median.
  quantizer  ``ops.lpbq_quantize`` against ``ops.quantize_by_tile`` (4 bits into int8, the same block scales) at [14336, 4096] bf16:
             both read 2 bytes and write 1 per element; ``fraction_of_8TBs`` is bytes / median / 8e12.

    python tools/lpbq_time.py [--tokens 16384] [--output profiles/lpbq_time.txt]
"""

from __future__ import annotations

import argparse
import copy
import json
import pathlib
import sys

import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import fastforward_amd as ff  # noqa: E402

from fastforward_amd import ops  # noqa: E402
from fastforward_amd.nn import functional as F  # noqa: E402
from fastforward_amd.quantization import lpbq  # noqa: E402
from kv_cache_time import alternate  # noqa: E402
from kv_token_time import spread  # noqa: E402

DEV = "cuda"
SHAPES = {"q_o_proj": (4096, 4096), "k_v_proj": (1024, 4096), "gate_up_proj": (14336, 4096), "down_proj": (4096, 14336)}  # name -> (N, K)
GROUP = 128


def make_layer(N: int, K: int, dtype: torch.dtype):
    model = torch.nn.Sequential(torch.nn.Linear(K, N, bias=False)).to(DEV).to(dtype)
    ff.quantize_model(model)
    layer = model[0]
    layer.input_quantizer = ff.nn.LinearQuantizer(8, symmetric=False, quantized_dtype=torch.int8, device=DEV)
    layer.input_quantizer.quantization_range = (torch.tensor(-4.0, device=DEV), torch.tensor(4.0, device=DEV))
    layer.weight_quantizer = ff.nn.LinearQuantizer(4, symmetric=True, allow_one_sided=False, granularity=ff.PerBlock(1, GROUP, 0), quantized_dtype=torch.int8,
                                                   device=DEV)
    blocks = layer.weight.detach().float().reshape(N, K // GROUP, GROUP)
    layer.weight_quantizer.quantization_range = (blocks.amin(-1).reshape(-1), blocks.amax(-1).reshape(-1))
    return model


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tokens", type=int, default=16384)
    ap.add_argument("--output", type=pathlib.Path, default=ROOT / "profiles" / "lpbq_time.txt")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    lines = []

    def emit(**record):
        lines.append(json.dumps(record))
        print(lines[-1], flush=True)

    dt = torch.bfloat16
    torch.manual_seed(0)
    with torch.no_grad(), ff.strict_quantization(False):
        for name, (N, K) in SHAPES.items():
            plain = make_layer(N, K, dt)
            converted = copy.deepcopy(plain)
            assert lpbq.convert_model(converted) == ["0.weight_quantizer"]
            x = torch.randn(args.tokens, K, device=DEV).to(dt)
            held = converted[0].weight_quantizer(converted[0].weight)
            arms = {"wq": lambda: plain[0](x), "lpbq": lambda: converted[0](x), "lpbq_held": lambda: F.linear(converted[0].input_quantizer(x), held)}
            error = {k: round(float((fn().float() - torch.nn.functional.linear(x, plain[0].weight).float()).abs().mean()), 5) for k, fn in arms.items()}
            times = alternate(arms, reps=3, replays=5, rounds=7)
            emit(what="layer", shape=name, tokens=args.tokens, N=N, K=K, group=GROUP, ops=2 * args.tokens * N * K, mean_abs_error_vs_float=error,
                 ratio_lpbq=round(times["lpbq"]["median_us"] / times["wq"]["median_us"], 4),
                 ratio_held=round(times["lpbq_held"]["median_us"] / times["wq"]["median_us"], 4), spread=spread(times), **times)
            del plain, converted, x, held, arms
            torch.cuda.empty_cache()
        N, K = SHAPES["gate_up_proj"]
        w = (torch.randn(N, K, device=DEV) * 0.02).to(dt)
        s = (w.float().reshape(N, K // GROUP, GROUP).abs().amax(-1) / 7.5).contiguous()
        arms = {"lpbq_quantize": lambda: ops.lpbq_quantize(w, s, GROUP, 4, False, want_int_scale=False),
                "lpbq_quantize_requantize": lambda: ops.lpbq_quantize(w, s, GROUP, 4, True, want_int_scale=False),
                "quantize_by_tile": lambda: ops.quantize_by_tile(w, s, (1, GROUP), 4, torch.int8)}
        times = alternate(arms, reps=10, replays=10, rounds=9)
        nbytes = N * K * 3 + N * (K // GROUP) * 4
        emit(what="quantizer", N=N, K=K, group=GROUP, bytes=nbytes, ratio=round(times["lpbq_quantize"]["median_us"] / times["quantize_by_tile"]["median_us"], 4),
             fraction_of_8TBs={k: round(nbytes / (v["median_us"] * 1e-6) / 8e12, 4) for k, v in times.items()}, spread=spread(times), **times)
    args.output.parent.mkdir(parents=True, exist_ok=True)
    args.output.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
