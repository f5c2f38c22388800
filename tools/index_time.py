"""Time the one-pass index_add / permute + quantize kernels (csrc/ffq_index.hip) against the reference's route — A2 of every
quantized input into a bf16 tensor, torch.index_add / a permuted view, A1 of the output quantizer — in one process on one device,
at one mixture-of-experts combine and one NCHW -> NHWC requantize. Each line: launches per call, microseconds per call
(hipGraph-replayed, the median of three medians, with their spread), and the algorithmic bytes of the FUSED call as a fraction of
8 TB/s. Run under `rocprofv3 --kernel-trace --stats` for the per-kernel times."""
import math
import pathlib
import statistics
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

from bench import event_time_ms  # noqa: E402
from fastforward_amd import ops  # noqa: E402

dev = "cuda"
bf16 = torch.bfloat16
s_a, o_a = torch.tensor([0.03], device=dev), torch.tensor([3.0], device=dev)
s_b, o_b = torch.tensor([0.02], device=dev), torch.tensor([-7.0], device=dev)
s_out, o_out = torch.tensor([0.05], device=dev), torch.tensor([-5.0], device=dev)
FAN = [(s_out, o_out)]


def line(name, launches, nbytes, fn):
    runs = sorted(event_time_ms(fn, iters=10, reps=4) for _ in range(3))
    ms = statistics.median(runs)
    frac = f"{nbytes / ms / 8e9:.3f} of 8 TB/s" if nbytes else ""
    print(f"{name:78s} {launches} launches {ms * 1e3:9.1f} us  (three runs: {runs[0] * 1e3:.1f} .. {runs[2] * 1e3:.1f})  {frac}", flush=True)


def a2(codes, s, o):
    return ops.dequantize_by_tile(codes, s, codes.shape, o, bf16)


def a1(value):
    return ops.quantize_by_tile(value, s_out, value.shape, 8, torch.int8, o_out)


# a top-2 combine: 4096 tokens of 4096 features, 8192 expert rows (every token twice), int8 codes in and out
tokens, hidden, rows = 4096, 4096, 8192
final = [torch.randint(-128, 128, (tokens, hidden), device=dev, dtype=torch.int8) for _ in range(2)]
expert = [torch.randint(-128, 128, (rows, hidden), device=dev, dtype=torch.int8) for _ in range(2)]
index = torch.randperm(rows, device=dev) % tokens
title = f"index_add dim 0 [{tokens}, {hidden}] += [{rows}, {hidden}] int8 -> int8"
line(f"{title} (fused)", 1, (tokens + rows + tokens) * hidden + 4 * 8 * rows,
     lambda r: ops.index_add_quantize(final[r % 2], 0, index, expert[r % 2], 1, quantizers=FAN, dtype=bf16, dequant=(s_a, o_a), source_dequant=(s_b, o_b), want_value=False))
line(f"{title} (A2 x 2, torch.index_add, A1)", 4, 0, lambda r: a1(torch.index_add(a2(final[r % 2], s_a, o_a), 0, index, a2(expert[r % 2], s_b, o_b))))
del final, expert

# NCHW -> NHWC under an output quantizer
shape, dims = (32, 256, 56, 56), (0, 2, 3, 1)
n = math.prod(shape)
xs = [torch.randint(-128, 128, shape, device=dev, dtype=torch.int8) for _ in range(2)]
title = f"permute {list(shape)} -> {list(dims)} int8 -> int8"
line(f"{title} (fused)", 1, n + n, lambda r: ops.permute_quantize(xs[r % 2], dims, quantizers=FAN, dtype=bf16, dequant=(s_a, o_a), want_value=False))
line(f"{title} (A2, permuted view, A1 of its dense copy)", 3, 0, lambda r: a1(a2(xs[r % 2], s_a, o_a).permute(dims).contiguous()))
ps = [(torch.randn(shape, device=dev) * 2).to(bf16) for _ in range(2)]
title = f"permute {list(shape)} -> {list(dims)} bf16 -> int8"
line(f"{title} (fused)", 1, 2 * n + n, lambda r: ops.permute_quantize(ps[r % 2], dims, quantizers=FAN, want_value=False))
line(f"{title} (permuted view, A1 of its dense copy)", 2, 0, lambda r: a1(ps[r % 2].permute(dims).contiguous()))
