"""Time the one-pass LayerNorm / Embedding / ReLU / SiLU + quantize kernels (csrc/ffq_modules.hip) against the reference's
three-launch route — A2 of the quantized operand into a bf16 tensor, the ATen op, A1 of the output quantizer — in one process on
one device, at the full-size shapes of tests/test_modules_gpu.py. Each line: microseconds per call (hipGraph-replayed, median),
and the algorithmic bytes of the FUSED call as a fraction of 8 TB/s. Run under `rocprofv3 --kernel-trace --stats` for the
per-kernel times."""
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import torch.nn.functional as F  # noqa: E402

from bench import event_time_ms  # noqa: E402
from fastforward_amd import ops  # noqa: E402

dev = "cuda"
bf16 = torch.bfloat16
s_in, o_in = torch.tensor([0.03], device=dev), torch.tensor([3.0], device=dev)
s_out, o_out = torch.tensor([0.02], device=dev), torch.tensor([-5.0], device=dev)


def line(name, numel, bpe, fn):
    ms = min(event_time_ms(fn, iters=10, reps=4) for _ in range(3))
    frac = f"{numel * bpe / ms / 8e9:.3f} of 8 TB/s" if bpe else ""
    print(f"{name:58s} {ms * 1e3:9.1f} us  {frac}", flush=True)


def a2(codes, dtype=bf16):
    return ops.dequantize_by_tile(codes, s_in, codes.shape, o_in, dtype)


def a1(value):
    return ops.quantize_by_tile(value, s_out, value.shape, 8, torch.int8, o_out)


# LayerNorm [16384, 4096]: int8 codes in, int8 codes out (2 B / element), + the bf16 value (4 B / element)
rows, cols = 16384, 4096
xs = [torch.randint(-128, 128, (rows, cols), device=dev, dtype=torch.int8) for _ in range(2)]
w = (torch.rand(cols, device=dev) + 0.5).to(bf16)
b = (torch.randn(cols, device=dev) * 0.1).to(bf16)
n = rows * cols
line("layer_norm int8 -> int8 (fused)", n, 2, lambda r: ops.layer_norm_quantize(xs[r % 2], cols, w, b, 1e-5, [(s_out, o_out)], dtype=bf16, dequant=(s_in, o_in), want_value=False))
line("layer_norm int8 -> bf16 + int8 (fused)", n, 4, lambda r: ops.layer_norm_quantize(xs[r % 2], cols, w, b, 1e-5, [(s_out, o_out)], dtype=bf16, dequant=(s_in, o_in)))
line("layer_norm int8 -> int8 (A2, F.layer_norm, A1)", n, 0, lambda r: a1(F.layer_norm(a2(xs[r % 2]), (cols,), w, b, 1e-5)))
del xs

# ReLU / SiLU [16384, 16384]: bf16 in, int8 codes out (3 B / element)
ys = [(torch.randn(16384, 16384, device=dev) * 3).to(bf16) for _ in range(2)]
n = ys[0].numel()
for op, aten in (("relu", F.relu), ("silu", F.silu)):
    line(f"{op} bf16 -> int8 (fused)", n, 3, lambda r, op=op: ops.pointwise_quantize(op, ys[r % 2], [(s_out, o_out)], want_value=False))
    line(f"{op} bf16 -> int8 (F.{op}, A1)", n, 0, lambda r, aten=aten: a1(aten(ys[r % 2])))
del ys
yq = [torch.randint(-128, 128, (16384, 16384), device=dev, dtype=torch.int8) for _ in range(2)]
for op, aten in (("relu", F.relu), ("silu", F.silu)):
    line(f"{op} int8 -> int8 (fused)", n, 2, lambda r, op=op: ops.pointwise_quantize(op, yq[r % 2], [(s_out, o_out)], dtype=bf16, dequant=(s_in, o_in), want_value=False))
    line(f"{op} int8 -> int8 (A2, F.{op}, A1)", n, 0, lambda r, aten=aten: a1(aten(a2(yq[r % 2]))))
del yq

# Embedding: 16384 ids into [128256, 4096] int8, per-row parameters; int8 rows in, int8 codes out (2 B / element)
V, D = 128256, 4096
table = torch.randint(-127, 128, (V, D), device=dev, dtype=torch.int8)
scale = torch.rand(V, device=dev) * 0.01 + 1e-3
ids = [torch.randint(0, V, (16384,), device=dev) for _ in range(2)]
n = 16384 * D
line("embedding int8 rows -> int8 (fused)", n, 2, lambda r: ops.embedding_quantize(ids[r % 2], table, scale, None, True, D, bf16, [(s_out, o_out)], want_value=False))
line("embedding int8 rows -> int8 (A2 of the table, F.embedding, A1)", n, 0,
     lambda r: a1(F.embedding(ids[r % 2], ops.dequantize_by_tile(table, scale, (1, D), None, bf16))))
