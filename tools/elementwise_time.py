"""Time the one-pass add / sub / mul / div, softmax, sigmoid and GELU + quantize kernels (csrc/ffq_elementwise.hip) against the
reference's route — A2 of each quantized operand into a bf16 tensor, the ATen op, A1 of the output quantizer — in one process on one
device, at the full-size shapes of tests/test_elementwise_gpu.py. Each line: microseconds per call (hipGraph-replayed, median), and
the algorithmic bytes of the FUSED call as a fraction of 8 TB/s. Run under `rocprofv3 --kernel-trace --stats` for the per-kernel
times."""
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import torch.nn.functional as F  # noqa: E402

from bench import event_time_ms  # noqa: E402
from fastforward_amd import ops  # noqa: E402

dev = "cuda"
bf16 = torch.bfloat16
s_a, o_a = torch.tensor([0.03], device=dev), torch.tensor([3.0], device=dev)
s_b, o_b = torch.tensor([0.02], device=dev), torch.tensor([-7.0], device=dev)
s_out, o_out = torch.tensor([0.05], device=dev), torch.tensor([-5.0], device=dev)
s_p, o_p = torch.tensor([1.0 / 255], device=dev), torch.tensor([-128.0], device=dev)  # a [0, 1] output: probabilities


def line(name, numel, bpe, fn):
    ms = min(event_time_ms(fn, iters=10, reps=4) for _ in range(3))
    frac = f"{numel * bpe / ms / 8e9:.3f} of 8 TB/s" if bpe else ""
    print(f"{name:58s} {ms * 1e3:9.1f} us  {frac}", flush=True)


def a2(codes, s, o):
    return ops.dequantize_by_tile(codes, s, codes.shape, o, bf16)


def a1(value, s=s_out, o=o_out):
    return ops.quantize_by_tile(value, s, value.shape, 8, torch.int8, o)


# residual add [16384, 4096]: int8 + int8 codes with different scales -> int8 (3 B / element)
shape = (16384, 4096)
n = shape[0] * shape[1]
xa = [torch.randint(-128, 128, shape, device=dev, dtype=torch.int8) for _ in range(2)]
xb = [torch.randint(-128, 128, shape, device=dev, dtype=torch.int8) for _ in range(2)]
line("add int8 + int8 -> int8 (fused)", n, 3,
     lambda r: ops.binary_quantize("add", xa[r % 2], xb[r % 2], [(s_out, o_out)], dtype=bf16, a_dequant=(s_a, o_a), b_dequant=(s_b, o_b), want_value=False))
line("add int8 + int8 -> int8 (A2, A2, torch.add, A1)", n, 0, lambda r: a1(torch.add(a2(xa[r % 2], s_a, o_a), a2(xb[r % 2], s_b, o_b))))
del xa, xb

# bias add [16384, 4096] + [4096] bf16 -> int8 (3 B / element)
hs = [torch.randn(shape, device=dev).to(bf16) for _ in range(2)]
bias = torch.randn(shape[1], device=dev).to(bf16)
line("add bf16 + bias[4096] -> int8 (fused)", n, 3, lambda r: ops.binary_quantize("add", hs[r % 2], bias, [(s_out, o_out)], want_value=False))
line("add bf16 + bias[4096] -> int8 (torch.add, A1)", n, 0, lambda r: a1(torch.add(hs[r % 2], bias)))
del hs

# softmax [32768, 2048] bf16 -> int8 (3 B / element)
ss = [(torch.randn(32768, 2048, device=dev) * 3).to(bf16) for _ in range(2)]
n = ss[0].numel()
line("softmax bf16 -> int8 (fused)", n, 3, lambda r: ops.softmax_quantize(ss[r % 2], [(s_p, o_p)], want_value=False))
line("softmax bf16 -> int8 (F.softmax, A1)", n, 0, lambda r: a1(F.softmax(ss[r % 2], -1), s_p, o_p))
del ss

# sigmoid / GELU [16384, 16384]: bf16 -> int8 (3 B / element), int8 -> int8 (2 B / element)
ys = [(torch.randn(16384, 16384, device=dev) * 3).to(bf16) for _ in range(2)]
n = ys[0].numel()
acts = (("sigmoid", torch.sigmoid), ("gelu", F.gelu), ("gelu_tanh", lambda t: F.gelu(t, approximate="tanh")))
for op, aten in acts:
    line(f"{op} bf16 -> int8 (fused)", n, 3, lambda r, op=op: ops.activation_quantize(op, ys[r % 2], [(s_out, o_out)], want_value=False))
    line(f"{op} bf16 -> int8 (ATen op, A1)", n, 0, lambda r, aten=aten: a1(aten(ys[r % 2])))
del ys
yq = [torch.randint(-128, 128, (16384, 16384), device=dev, dtype=torch.int8) for _ in range(2)]
for op, aten in acts[:2]:
    line(f"{op} int8 -> int8 (fused)", n, 2, lambda r, op=op: ops.activation_quantize(op, yq[r % 2], [(s_out, o_out)], dtype=bf16, dequant=(s_a, o_a), want_value=False))
    line(f"{op} int8 -> int8 (A2, ATen op, A1)", n, 0, lambda r, aten=aten: a1(aten(a2(yq[r % 2], s_a, o_a))))
