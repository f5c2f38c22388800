"""Time the W8A8 3-D convolution (csrc/ffq_conv3d.hip, output quantizer fused) and the one-pass avg_pool3d (csrc/ffq_pool3d.hip) in
one process on one device, interleaved shape by shape: four 3-D U-Net layers (k3 p1, batch 2), a ViViT / Qwen2-VL style patch
embedding (kernel = stride = (2, 14, 14), batch 32) and two k2 s2 pools, against

  (a) the three-launch device chain the fallback runs — this project's A2 of the codes into bf16, F.conv3d / F.avg_pool3d in bf16,
      A1 of the output;
  (b) F.conv3d / F.avg_pool3d in bf16 alone.

Each line: microseconds per call (hipGraph-replayed, median of three) and the ratios to the fused call. Run under
`rocprofv3 --kernel-trace --stats -- python tools/conv3d_time.py` (a run of its own) for the per-kernel medians."""
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

# name, B, C, OC, (D, H, W), kernel, stride, padding
CONVS = [
    ("unet 32^3 32->32 k3 p1", 2, 32, 32, (32, 32, 32), (3, 3, 3), (1, 1, 1), (1, 1, 1)),
    ("unet 16^3 64->64 k3 p1", 2, 64, 64, (16, 16, 16), (3, 3, 3), (1, 1, 1), (1, 1, 1)),
    ("unet 16^3 128->128 k3 p1", 2, 128, 128, (16, 16, 16), (3, 3, 3), (1, 1, 1), (1, 1, 1)),
    ("unet 8^3 256->256 k3 p1", 2, 256, 256, (8, 8, 8), (3, 3, 3), (1, 1, 1), (1, 1, 1)),
    ("patch embed 4x224^2 3->1280 k(2,14,14)", 32, 3, 1280, (4, 224, 224), (2, 14, 14), (2, 14, 14), (0, 0, 0)),
    ("patch embed 4x28^2 16->64 k(2,14,14)", 32, 16, 64, (4, 28, 28), (2, 14, 14), (2, 14, 14), (0, 0, 0)),
]
# name, B, C, (D, H, W)
POOLS = [
    ("avg_pool3d k2 s2 32^3 x 32", 2, 32, (32, 32, 32)),
    ("avg_pool3d k2 s2 16^3 x 128", 2, 128, (16, 16, 16)),
]

s_x, o_x = torch.tensor([0.03], device=dev), torch.tensor([3.0], device=dev)
o_out, s_out = torch.tensor([-5.0], device=dev), torch.tensor([0.05], device=dev)


def timed(fn):
    return statistics.median(event_time_ms(fn, iters=10, reps=4) for _ in range(3)) * 1e3


def main() -> None:
    only = sys.argv[1:]
    print(f"{'shape':42s} {'fused':>9s} {'(a) A2+op+A1':>14s} {'(b) op bf16':>13s} {'a/fused':>8s} {'b/fused':>8s}")
    for name, B, C, OC, size, k, s, p in CONVS:
        if only and not any(o in name for o in only):
            continue
        xs = [torch.randint(-128, 128, (B, C, *size), device=dev, dtype=torch.int8) for _ in range(2)]
        wc = torch.randint(-127, 128, (OC, C, *k), device=dev, dtype=torch.int8)
        s_w = torch.rand(OC, device=dev) * 1e-3 + 1e-4
        tile = (1, C, *k)
        xf = [ops.dequantize_by_tile(x, s_x, x.shape, o_x, bf16) for x in xs]
        wf = ops.dequantize_by_tile(wc, s_w, tile, None, bf16)

        def fused(r):
            return ops.conv3d_w8a8(xs[r % 2], wc, s_x, o_x, s_w, None, None, s, p, (1, 1, 1), out_scale=s_out, out_offset=o_out)

        def chain(r):
            x = ops.dequantize_by_tile(xs[r % 2], s_x, xs[0].shape, o_x, bf16)
            w = ops.dequantize_by_tile(wc, s_w, tile, None, bf16)
            y = F.conv3d(x, w, None, s, p)
            return ops.quantize_by_tile(y, s_out, y.shape, 8, torch.int8, o_out)

        def plain(r):
            return F.conv3d(xf[r % 2], wf, None, s, p)

        t_f, t_a, t_b = timed(fused), timed(chain), timed(plain)
        print(f"{name:42s} {t_f:7.1f}us {t_a:12.1f}us {t_b:11.1f}us {t_a / t_f:8.2f} {t_b / t_f:8.2f}", flush=True)
        del xs, xf, wf
    for name, B, C, size in POOLS:
        if only and not any(o in name for o in only):
            continue
        xs = [torch.randint(-128, 128, (B, C, *size), device=dev, dtype=torch.int8) for _ in range(2)]
        xf = [ops.dequantize_by_tile(x, s_x, x.shape, o_x, bf16) for x in xs]

        def fused(r):
            return ops.pool3d_quantize("avg", xs[r % 2], (2, 2, 2), (2, 2, 2), quantizers=[(s_out, o_out)], dtype=bf16, dequant=(s_x, o_x), want_value=False)

        def chain(r):
            x = ops.dequantize_by_tile(xs[r % 2], s_x, xs[0].shape, o_x, bf16)
            y = F.avg_pool3d(x, 2, 2)
            return ops.quantize_by_tile(y, s_out, y.shape, 8, torch.int8, o_out)

        def plain(r):
            return F.avg_pool3d(xf[r % 2], 2, 2)

        t_f, t_a, t_b = timed(fused), timed(chain), timed(plain)
        print(f"{name:42s} {t_f:7.1f}us {t_a:12.1f}us {t_b:11.1f}us {t_a / t_f:8.2f} {t_b / t_f:8.2f}", flush=True)
        del xs, xf


if __name__ == "__main__":
    main()
