"""Time the W8A8 depthwise convolution (csrc/ffq_depthwise.hip, output quantizer fused) in one process on one device, interleaved
shape by shape: ConvNeXt-T's 7x7 ([32, 96, 56, 56]) and MobileNetV2's 3x3 at stride 1 and 2 ([32, 144, 56, 56]), against

  (a) the four-launch device chain the fallback runs — this project's A2 of the input codes and of the weight codes into bf16,
      F.conv2d(groups=C) in bf16 (the vendor's depthwise convolution), A1 of the output;
  (b) F.conv2d(groups=C) in bf16 alone.

Each line: microseconds per call (hipGraph-replayed, median of three), the ratios to the fused call, and the fused call's algorithmic
bytes (1 B per input element in, 1 B per output code out) over its time as a fraction of the 6.3 TB/s a streaming kernel reaches on
the MI355X. The inputs alternate between two buffers; at these sizes both stay in the 256 MiB Infinity Cache, so the fraction is of
the HBM RATE, not a claim that the bytes came from HBM. Run under `rocprofv3 --kernel-trace --stats -- python tools/depthwise_time.py`
(a run of its own) for the per-kernel medians."""
import pathlib
import statistics
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import torch.nn.functional as F  # noqa: E402

from bench import event_time_ms  # noqa: E402
from fastforward_amd import ops  # noqa: E402

dev = "cuda"
bf16 = torch.bfloat16
STREAM_TBPS = 6.3  # achievable HBM rate of a streaming kernel on the MI355X

# name, B, C, (H, W), kernel, stride, padding
CONVS = [
    ("ConvNeXt-T 56^2 x 96 k7 p3", 32, 96, (56, 56), (7, 7), (1, 1), (3, 3)),
    ("MobileNetV2 56^2 x 144 k3 s1 p1", 32, 144, (56, 56), (3, 3), (1, 1), (1, 1)),
    ("MobileNetV2 56^2 x 144 k3 s2 p1", 32, 144, (56, 56), (3, 3), (2, 2), (1, 1)),
]

s_x, o_x = torch.tensor([0.03], device=dev), torch.tensor([3.0], device=dev)
o_out, s_out = torch.tensor([-5.0], device=dev), torch.tensor([0.05], device=dev)


def timed(fn):
    return statistics.median(event_time_ms(fn, iters=10, reps=4) for _ in range(3)) * 1e3


def main() -> None:
    only = sys.argv[1:]
    print(f"{'shape':34s} {'fused':>9s} {'(a) A2+A2+op+A1':>16s} {'(b) op bf16':>13s} {'a/fused':>8s} {'b/fused':>8s} {'of 6.3 TB/s':>12s}")
    for name, B, C, size, k, s, p in CONVS:
        if only and not any(o in name for o in only):
            continue
        xs = [torch.randint(-128, 128, (B, C, *size), device=dev, dtype=torch.int8) for _ in range(2)]
        wc = torch.randint(-127, 128, (C, 1, *k), device=dev, dtype=torch.int8)
        s_w = torch.rand(C, device=dev) * 1e-3 + 1e-4
        tile = (1, 1, *k)
        xf = [ops.dequantize_by_tile(x, s_x, x.shape, o_x, bf16) for x in xs]
        wf = ops.dequantize_by_tile(wc, s_w, tile, None, bf16)

        def fused(r):
            return ops.depthwise_conv2d_w8a8(xs[r % 2], wc, s_x, o_x, s_w, None, None, s, p, (1, 1), out_scale=s_out, out_offset=o_out)

        def chain(r):
            x = ops.dequantize_by_tile(xs[r % 2], s_x, xs[0].shape, o_x, bf16)
            w = ops.dequantize_by_tile(wc, s_w, tile, None, bf16)
            y = F.conv2d(x, w, None, s, p, 1, C)
            return ops.quantize_by_tile(y, s_out, y.shape, 8, torch.int8, o_out)

        def plain(r):
            return F.conv2d(xf[r % 2], wf, None, s, p, 1, C)

        nbytes = xs[0].numel() + fused(0).numel()
        t_f, t_a, t_b = timed(fused), timed(chain), timed(plain)
        share = nbytes / (t_f * 1e-6) / (STREAM_TBPS * 1e12)
        print(f"{name:34s} {t_f:7.1f}us {t_a:14.1f}us {t_b:11.1f}us {t_a / t_f:8.2f} {t_b / t_f:8.2f} {share:12.3f}", flush=True)
        del xs, xf, wf


if __name__ == "__main__":
    main()
