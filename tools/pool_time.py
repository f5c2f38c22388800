"""Time the one-pass avg_pool1d / avg_pool2d / max_pool2d / nearest interpolate + quantize kernels (csrc/ffq_pool.hip) against the
reference's route — A2 of the quantized input into a bf16 tensor, the ATen op, A1 of the output quantizer — in one process on one
device, at the full-size shapes of tests/test_pool_gpu.py. Each line: microseconds per call (hipGraph-replayed, median), and the
algorithmic bytes of the FUSED call (the input once, the codes once) as a fraction of 8 TB/s. Run under
`rocprofv3 --kernel-trace --stats` for the per-kernel times."""
import math
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

from bench import event_time_ms  # noqa: E402
from fastforward_amd import ops  # noqa: E402

dev = "cuda"
bf16 = torch.bfloat16
TF = torch.nn.functional
s_a, o_a = torch.tensor([0.03], device=dev), torch.tensor([3.0], device=dev)
s_out, o_out = torch.tensor([0.05], device=dev), torch.tensor([-5.0], device=dev)
FAN = [(s_out, o_out)]


def line(name, nbytes, fn):
    ms = min(event_time_ms(fn, iters=10, reps=4) for _ in range(3))
    frac = f"{nbytes / ms / 8e9:.3f} of 8 TB/s" if nbytes else ""
    print(f"{name:64s} {ms * 1e3:9.1f} us  {frac}", flush=True)


def a2(codes):
    return ops.dequantize_by_tile(codes, s_a, codes.shape, o_a, bf16)


def a1(value):
    return ops.quantize_by_tile(value, s_out, value.shape, 8, torch.int8, o_out)


def pool(mode, k, s, p):
    return lambda x, **kw: ops.pool2d_quantize(mode, x if x.dim() == 4 else x.unsqueeze(-2), k, s, p, quantizers=FAN, want_value=False, **kw)


CASES = [  # name, shape, the fused call, the ATen op
    ("max_pool2d k3 s2 p1", (64, 64, 112, 112), pool("max", (3, 3), (2, 2), (1, 1)), lambda t: TF.max_pool2d(t, 3, 2, 1)),
    ("avg_pool2d k2 s2", (64, 128, 56, 56), pool("avg", (2, 2), (2, 2), (0, 0)), lambda t: TF.avg_pool2d(t, 2, 2)),
    ("avg_pool2d k7 s7", (64, 2048, 7, 7), pool("avg", (7, 7), (7, 7), (0, 0)), lambda t: TF.avg_pool2d(t, 7, 7)),
    ("avg_pool2d k56 s56 (global)", (64, 256, 56, 56), pool("avg", (56, 56), (56, 56), (0, 0)), lambda t: TF.avg_pool2d(t, 56, 56)),
    ("avg_pool1d k4 s4", (64, 512, 4096), pool("avg", (1, 4), (1, 4), (0, 0)), lambda t: TF.avg_pool1d(t, 4, 4)),
    ("interpolate nearest x2", (64, 256, 40, 40),
     lambda x, **kw: ops.upsample_nearest_quantize(x, (80, 80), (2.0, 2.0), quantizers=FAN, want_value=False, **kw), lambda t: TF.interpolate(t, scale_factor=2)),
]

for name, shape, fused, aten in CASES:
    n = math.prod(shape)
    xs = [(torch.randn(shape, device=dev) * 2).to(bf16) for _ in range(2)]
    out = aten(xs[0]).numel()
    line(f"{name} {list(shape)} bf16 -> int8 (fused)", 2 * n + out, lambda r: fused(xs[r % 2]))
    line(f"{name} {list(shape)} bf16 -> int8 (ATen op, A1)", 0, lambda r: a1(aten(xs[r % 2])))
    del xs
    qs = [torch.randint(-128, 128, shape, device=dev, dtype=torch.int8) for _ in range(2)]
    line(f"{name} {list(shape)} int8 -> int8 (fused)", n + out, lambda r: fused(qs[r % 2], dtype=bf16, dequant=(s_a, o_a)))
    line(f"{name} {list(shape)} int8 -> int8 (A2, ATen op, A1)", 0, lambda r: a1(aten(a2(qs[r % 2]))))
    del qs
