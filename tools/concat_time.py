"""Time the one-pass cat / pad + quantize kernels (csrc/ffq_concat.hip) against the reference's route — A2 of every quantized input
into a bf16 tensor, torch.cat / F.pad, A1 of the output quantizer — in one process on one device, at the full-size shapes of
tests/test_concat_gpu.py. Each line: microseconds per call (hipGraph-replayed, the median of three medians, with their spread), and
the algorithmic bytes of the FUSED call (every input once, the codes once) as a fraction of 8 TB/s. Run under
`rocprofv3 --kernel-trace --stats` for the per-kernel times."""
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
TF = torch.nn.functional
s_a, o_a = torch.tensor([0.03], device=dev), torch.tensor([3.0], device=dev)
s_b, o_b = torch.tensor([0.02], device=dev), torch.tensor([-7.0], device=dev)
s_out, o_out = torch.tensor([0.05], device=dev), torch.tensor([-5.0], device=dev)
FAN = [(s_out, o_out)]


def line(name, nbytes, fn):
    runs = sorted(event_time_ms(fn, iters=10, reps=4) for _ in range(3))
    ms = statistics.median(runs)
    frac = f"{nbytes / ms / 8e9:.3f} of 8 TB/s" if nbytes else ""
    print(f"{name:72s} {ms * 1e3:9.1f} us  (three runs: {runs[0] * 1e3:.1f} .. {runs[2] * 1e3:.1f})  {frac}", flush=True)


def a2(codes, s, o):
    return ops.dequantize_by_tile(codes, s, codes.shape, o, bf16)


def a1(value):
    return ops.quantize_by_tile(value, s_out, value.shape, 8, torch.int8, o_out)


CAT = [("cat dim 1 (U-Net join)", (8, 64, 256, 256), (8, 64, 256, 256), 1), ("cat dim 1 (U-Net join)", (8, 512, 32, 32), (8, 512, 32, 32), 1),
       ("cat dim 2 (KV append)", (8, 8, 2047, 128), (8, 8, 1, 128), 2)]
PAD = [("pad reflect 3", (32, 3, 224, 224), (3, 3, 3, 3), "reflect"), ("pad constant 3", (32, 3, 224, 224), (3, 3, 3, 3), "constant"),
       ("pad constant (0, 0, 1, 0)", (8, 2048, 4096), (0, 0, 1, 0), "constant")]

for name, a, b, dim in CAT:
    n = math.prod(a) + math.prod(b)
    title = f"{name} {list(a)} + {list(b)}"
    xs = [[(torch.randn(s, device=dev) * 2).to(bf16) for s in (a, b)] for _ in range(2)]
    line(f"{title} bf16 -> int8 (fused)", 2 * n + n, lambda r: ops.cat_quantize(xs[r % 2], dim, quantizers=FAN, want_value=False))
    line(f"{title} bf16 -> int8 (torch.cat, A1)", 0, lambda r: a1(torch.cat(xs[r % 2], dim)))
    del xs
    qs = [[torch.randint(-128, 128, s, device=dev, dtype=torch.int8) for s in (a, b)] for _ in range(2)]
    deq = [(s_a, o_a), (s_b, o_b)]
    line(f"{title} int8 -> int8 (fused)", n + n, lambda r: ops.cat_quantize(qs[r % 2], dim, quantizers=FAN, dtype=bf16, dequant=deq, want_value=False))
    line(f"{title} int8 -> int8 (A2 x 2, torch.cat, A1)", 0, lambda r: a1(torch.cat([a2(qs[r % 2][0], s_a, o_a), a2(qs[r % 2][1], s_b, o_b)], dim)))
    del qs

for name, shape, pad, mode in PAD:
    n = math.prod(shape)
    out = math.prod(ops.concat.padded_shape(shape, pad))
    title = f"{name} {list(shape)}"
    xs = [(torch.randn(shape, device=dev) * 2).to(bf16) for _ in range(2)]
    line(f"{title} bf16 -> int8 (fused)", 2 * n + out, lambda r: ops.pad_quantize(xs[r % 2], pad, mode, quantizers=FAN, want_value=False))
    line(f"{title} bf16 -> int8 (F.pad, A1)", 0, lambda r: a1(TF.pad(xs[r % 2], pad, mode)))
    del xs
    qs = [torch.randint(-128, 128, shape, device=dev, dtype=torch.int8) for _ in range(2)]
    line(f"{title} int8 -> int8 (fused)", n + out, lambda r: ops.pad_quantize(qs[r % 2], pad, mode, quantizers=FAN, dtype=bf16, dequant=(s_a, o_a), want_value=False))
    line(f"{title} int8 -> int8 (A2, F.pad, A1)", 0, lambda r: a1(TF.pad(a2(qs[r % 2], s_a, o_a), pad, mode)))
    del qs
