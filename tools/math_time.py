"""Time the one-pass rms_norm, exp / sin / cos / pow, sum and cumsum + quantize kernels (csrc/ffq_math.hip) against the reference's
route — A2 of the quantized input into a bf16 tensor, the ATen op, A1 of the output quantizer — in one process on one device, at the
full-size shapes of tests/test_math_gpu.py. Each line: microseconds per call (hipGraph-replayed, median), and the algorithmic bytes of
the FUSED call as a fraction of 8 TB/s. Run under `rocprofv3 --kernel-trace --stats` for the per-kernel times."""
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

from bench import event_time_ms  # noqa: E402
from fastforward_amd import ops  # noqa: E402

dev = "cuda"
bf16 = torch.bfloat16
s_a, o_a = torch.tensor([0.03], device=dev), torch.tensor([3.0], device=dev)
s_out, o_out = torch.tensor([0.05], device=dev), torch.tensor([-5.0], device=dev)
s_sum, o_sum = torch.tensor([2.0], device=dev), torch.tensor([0.0], device=dev)  # a wide range for sums
EPS = torch.finfo(torch.float32).eps


def line(name, numel, bpe, fn):
    ms = min(event_time_ms(fn, iters=10, reps=4) for _ in range(3))
    frac = f"{numel * bpe / ms / 8e9:.3f} of 8 TB/s" if bpe else ""
    print(f"{name:58s} {ms * 1e3:9.1f} us  {frac}", flush=True)


def a2(codes, s, o):
    return ops.dequantize_by_tile(codes, s, codes.shape, o, bf16)


def a1(value, s=s_out, o=o_out):
    return ops.quantize_by_tile(value, s, value.shape, 8, torch.int8, o)


# rms_norm [16384, 4096] with a bf16 weight: bf16 -> int8 (3 B / element), int8 -> int8 (2 B / element)
shape = (16384, 4096)
n = shape[0] * shape[1]
w = (torch.randn(shape[1], device=dev) * 0.5 + 1).to(bf16)
hs = [torch.randn(shape, device=dev).to(bf16) for _ in range(2)]
line("rms_norm bf16 -> int8 (fused)", n, 3, lambda r: ops.rms_norm_quantize(hs[r % 2], w, EPS, [(s_out, o_out)], want_value=False))
line("rms_norm bf16 -> int8 (F.rms_norm, A1)", n, 0, lambda r: a1(torch.nn.functional.rms_norm(hs[r % 2], (shape[1],), w)))
# sum(-1), sum(0) [16384, 4096] bf16 -> int8 (2 B / input element)
line("sum(-1) bf16 -> int8 (fused)", n, 2, lambda r: ops.sum_quantize(hs[r % 2], -1, [(s_sum, o_sum)], want_value=False))
line("sum(-1) bf16 -> int8 (torch.sum, A1)", n, 0, lambda r: a1(torch.sum(hs[r % 2], -1), s_sum, o_sum))
line("sum(0) bf16 -> int8 (fused)", n, 2, lambda r: ops.sum_quantize(hs[r % 2], 0, [(s_sum, o_sum)], want_value=False))
line("sum(0) bf16 -> int8 (torch.sum, A1)", n, 0, lambda r: a1(torch.sum(hs[r % 2], 0), s_sum, o_sum))
line("sum() bf16 -> int8 (fused)", n, 2, lambda r: ops.sum_quantize(hs[r % 2], None, [(s_sum, o_sum)], want_value=False))
line("sum() bf16 -> int8 (torch.sum, A1)", n, 0, lambda r: a1(torch.sum(hs[r % 2]), s_sum, o_sum))
del hs
xq = [torch.randint(-128, 128, shape, device=dev, dtype=torch.int8) for _ in range(2)]
line("rms_norm int8 -> int8 (fused)", n, 2, lambda r: ops.rms_norm_quantize(xq[r % 2], w, EPS, [(s_out, o_out)], dtype=bf16, dequant=(s_a, o_a), want_value=False))
line("rms_norm int8 -> int8 (A2, F.rms_norm, A1)", n, 0, lambda r: a1(torch.nn.functional.rms_norm(a2(xq[r % 2], s_a, o_a), (shape[1],), w)))
del xq

# cumsum(-1) [4096, 4096] bf16 -> int8 (3 B / element), cumsum(0) for the column kernel
cs = [torch.randn(4096, 4096, device=dev).to(bf16) for _ in range(2)]
n = cs[0].numel()
line("cumsum(-1) bf16 -> int8 (fused)", n, 3, lambda r: ops.cumsum_quantize(cs[r % 2], -1, [(s_sum, o_sum)], want_value=False))
line("cumsum(-1) bf16 -> int8 (torch.cumsum, A1)", n, 0, lambda r: a1(torch.cumsum(cs[r % 2], -1), s_sum, o_sum))
line("cumsum(0) bf16 -> int8 (fused)", n, 3, lambda r: ops.cumsum_quantize(cs[r % 2], 0, [(s_sum, o_sum)], want_value=False))
line("cumsum(0) bf16 -> int8 (torch.cumsum, A1)", n, 0, lambda r: a1(torch.cumsum(cs[r % 2], 0), s_sum, o_sum))
del cs

# exp / sin / cos / pow(2) [16384, 16384] bf16 -> int8 (3 B / element)
ys = [(torch.randn(16384, 16384, device=dev) * 2).to(bf16) for _ in range(2)]
n = ys[0].numel()
unary = (("exp", 0.0, torch.exp), ("sin", 0.0, torch.sin), ("cos", 0.0, torch.cos), ("pow", 2.0, lambda t: torch.pow(t, 2)))
for op, e, aten in unary:
    name = f"{op}{'(2)' if op == 'pow' else ''}"
    line(f"{name} bf16 -> int8 (fused)", n, 3, lambda r, op=op, e=e: ops.unary_quantize(op, ys[r % 2], e, [(s_out, o_out)], want_value=False))
    line(f"{name} bf16 -> int8 (ATen op, A1)", n, 0, lambda r, aten=aten: a1(aten(ys[r % 2])))
del ys
