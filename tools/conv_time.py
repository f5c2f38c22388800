"""Time the W8A8 convolution (csrc/ffq_conv.hip, output quantizer fused) against (a) the reference's route at its fastest — this
project's A2 of the input and weight codes into bf16, F.conv2d in bf16, A1 of the output — and (b) F.conv2d in bf16 alone, in one
process on one device, interleaved shape by shape, at eight ResNet-50 layers and two Whisper encoder layers (as conv1d), batch 32.

Each line: microseconds per call (hipGraph-replayed, median of three), and the fused call's share of peak as the measuring guide
defines it: the larger of (int8 ops / 5 POP/s) and (algorithmic bytes / 8 TB/s) over the measured time, naming the bound. Ops are
2 * B * OC * OH * OW * C * KH * KW (padded taps not counted); bytes are the input codes, the weight codes and the int8 output once.
Run under `rocprofv3 --kernel-trace --stats -- python tools/conv_time.py` (a run of its own) for the per-kernel medians."""
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import torch.nn.functional as F  # noqa: E402

from bench import event_time_ms  # noqa: E402
from fastforward_amd import ops  # noqa: E402

dev = "cuda"
bf16 = torch.bfloat16

# name, B, C, OC, (H, W), (KH, KW), stride, padding
SHAPES = [
    ("r50 56^2 64->64 3x3", 32, 64, 64, (56, 56), (3, 3), (1, 1), (1, 1)),
    ("r50 56^2 256->64 1x1", 32, 256, 64, (56, 56), (1, 1), (1, 1), (0, 0)),
    ("r50 28^2 128->128 3x3", 32, 128, 128, (28, 28), (3, 3), (1, 1), (1, 1)),
    ("r50 28^2 512->128 1x1", 32, 512, 128, (28, 28), (1, 1), (1, 1), (0, 0)),
    ("r50 14^2 256->256 3x3", 32, 256, 256, (14, 14), (3, 3), (1, 1), (1, 1)),
    ("r50 7^2 512->512 3x3", 32, 512, 512, (7, 7), (3, 3), (1, 1), (1, 1)),
    ("r50 stem 224^2 3->64 7x7 s2", 32, 3, 64, (224, 224), (7, 7), (2, 2), (3, 3)),
    ("r50 56^2 128->128 3x3 s2", 32, 128, 128, (56, 56), (3, 3), (2, 2), (1, 1)),
    ("whisper L3000 80->384 k3 p1", 32, 80, 384, (1, 3000), (1, 3), (1, 1), (0, 1)),
    ("whisper L3000 384->384 k3 s2 p1", 32, 384, 384, (1, 3000), (1, 3), (1, 2), (0, 1)),
]

s_x, o_x = torch.tensor([0.03], device=dev), torch.tensor([3.0], device=dev)
o_out, s_out = torch.tensor([-5.0], device=dev), torch.tensor([0.05], device=dev)


def timed(fn):
    return min(event_time_ms(fn, iters=10, reps=4) for _ in range(3)) * 1e3


def main() -> None:
    only = sys.argv[1:]
    print(f"{'shape':34s} {'fused':>9s} {'(a) A2+conv+A1':>15s} {'(b) conv bf16':>14s} {'a/fused':>8s} {'b/fused':>8s}  share of peak")
    for name, B, C, OC, (H, W), k, s, p in SHAPES:
        if only and not any(o in name for o in only):
            continue
        xs = [torch.randint(-128, 128, (B, C, H, W), device=dev, dtype=torch.int8) for _ in range(2)]
        wc = torch.randint(-127, 128, (OC, C, *k), device=dev, dtype=torch.int8)
        s_w = torch.rand(OC, device=dev) * 1e-3 + 1e-4
        xf = [ops.dequantize_by_tile(x, s_x, x.shape, o_x, bf16) for x in xs]
        wf = ops.dequantize_by_tile(wc, s_w, (1, *wc.shape[1:]), None, bf16)

        def fused(r):
            return ops.conv2d_w8a8(xs[r % 2], wc, s_x, o_x, s_w, None, None, s, p, (1, 1), out_scale=s_out, out_offset=o_out)

        def chain(r):
            x = ops.dequantize_by_tile(xs[r % 2], s_x, xs[0].shape, o_x, bf16)
            w = ops.dequantize_by_tile(wc, s_w, (1, *wc.shape[1:]), None, bf16)
            y = F.conv2d(x, w, None, s, p)
            return ops.quantize_by_tile(y, s_out, y.shape, 8, torch.int8, o_out)

        def plain(r):
            return F.conv2d(xf[r % 2], wf, None, s, p)

        t_f, t_a, t_b = timed(fused), timed(chain), timed(plain)
        out = fused(0)
        OH, OW = out.shape[2:]
        ops_n = 2 * B * OC * OH * OW * C * k[0] * k[1]
        bytes_n = B * C * H * W + OC * C * k[0] * k[1] + B * OC * OH * OW
        compute, memory = ops_n / (t_f * 1e-6) / 5e15, bytes_n / (t_f * 1e-6) / 8e12
        share = f"{max(compute, memory):.3f} ({'int8 ops' if compute >= memory else 'bytes'})"
        print(f"{name:34s} {t_f:7.1f}us {t_a:13.1f}us {t_b:12.1f}us {t_a / t_f:8.2f} {t_b / t_f:8.2f}  {share}", flush=True)
        del xs, xf, wf


if __name__ == "__main__":
    main()
