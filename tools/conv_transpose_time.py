"""Time the W8A8 transposed convolution (csrc/ffq_conv_transpose.hip, output quantizer fused) in one process on one device,
interleaved shape by shape, at three U-Net up-convolutions, four DCGAN generator layers and three vocoder layers (as
conv_transpose1d), batch 32, against

  (a) the reference's route at its fastest — this project's A2 of the input and weight codes into bf16, F.conv_transpose2d in
      bf16, A1 of the output;
  (b) F.conv_transpose2d in bf16 alone;
  (c) for the k = 2s shapes and k = s shapes (k4 s2, k2 s2, k16 s8, k4 s2 1-D), ops.conv2d_w8a8 at the same MAC count: the same
      input, stride 1, a (KH / s_h) x (KW / s_w) filter and s_h * s_w * OC output channels — the pixel-shuffle equivalent. A
      phase-split kernel costs about 1x that call, a masked gather about s_h * s_w x.

Each line: microseconds per call (hipGraph-replayed, median of three) and the ratios to the fused call. Run under
`rocprofv3 --kernel-trace --stats -- python tools/conv_transpose_time.py` (a run of its own) for the per-kernel medians, which
give the reorder / GEMM split and the GEMM-to-GEMM ratio against (c): the shapes run one after another, so the trace's dispatches
of convt_* and conv_* kernels, taken in time order, fall into one group per shape."""
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

# name, B, C, OC, (H, W), (KH, KW), stride, padding
SHAPES = [
    ("unet 28^2 1024->512 k2 s2", 32, 1024, 512, (28, 28), (2, 2), (2, 2), (0, 0)),
    ("unet 56^2 512->256 k2 s2", 32, 512, 256, (56, 56), (2, 2), (2, 2), (0, 0)),
    ("unet 112^2 256->128 k2 s2", 32, 256, 128, (112, 112), (2, 2), (2, 2), (0, 0)),
    ("dcgan 8^2 512->256 k4 s2 p1", 32, 512, 256, (8, 8), (4, 4), (2, 2), (1, 1)),
    ("dcgan 16^2 256->128 k4 s2 p1", 32, 256, 128, (16, 16), (4, 4), (2, 2), (1, 1)),
    ("dcgan 32^2 128->64 k4 s2 p1", 32, 128, 64, (32, 32), (4, 4), (2, 2), (1, 1)),
    ("dcgan 64^2 64->3 k4 s2 p1", 32, 64, 3, (64, 64), (4, 4), (2, 2), (1, 1)),
    ("vocoder L256 512->256 k16 s8 p4", 32, 512, 256, (1, 256), (1, 16), (1, 8), (0, 4)),
    ("vocoder L2048 256->128 k16 s8 p4", 32, 256, 128, (1, 2048), (1, 16), (1, 8), (0, 4)),
    ("vocoder L16384 128->64 k4 s2 p1", 32, 128, 64, (1, 16384), (1, 4), (1, 2), (0, 1)),
]

s_x, o_x = torch.tensor([0.03], device=dev), torch.tensor([3.0], device=dev)
o_out, s_out = torch.tensor([-5.0], device=dev), torch.tensor([0.05], device=dev)


def timed(fn):
    return statistics.median(event_time_ms(fn, iters=10, reps=4) for _ in range(3)) * 1e3


def main() -> None:
    only = sys.argv[1:]
    print(f"{'shape':34s} {'fused':>9s} {'(a) A2+convT+A1':>16s} {'(b) convT bf16':>15s} {'(c) conv2d_w8a8':>16s} {'a/fused':>8s} {'b/fused':>8s} {'fused/c':>8s}")
    for name, B, C, OC, (H, W), k, s, p in SHAPES:
        if only and not any(o in name for o in only):
            continue
        xs = [torch.randint(-128, 128, (B, C, H, W), device=dev, dtype=torch.int8) for _ in range(2)]
        wc = torch.randint(-127, 128, (C, OC, *k), device=dev, dtype=torch.int8)
        s_w = torch.rand(OC, device=dev) * 1e-3 + 1e-4
        tile = (C, 1, *k)
        xf = [ops.dequantize_by_tile(x, s_x, x.shape, o_x, bf16) for x in xs]
        wf = ops.dequantize_by_tile(wc, s_w, tile, None, bf16)
        # (c): the same MACs as a stride-1 forward convolution
        kc = (k[0] // s[0], k[1] // s[1])
        w_same = torch.randint(-127, 128, (s[0] * s[1] * OC, C, *kc), device=dev, dtype=torch.int8)
        s_same = torch.rand(s[0] * s[1] * OC, device=dev) * 1e-3 + 1e-4

        def fused(r):
            return ops.conv_transpose2d_w8a8(xs[r % 2], wc, s_x, o_x, s_w, None, None, s, p, (0, 0), (1, 1), out_scale=s_out, out_offset=o_out)

        def chain(r):
            x = ops.dequantize_by_tile(xs[r % 2], s_x, xs[0].shape, o_x, bf16)
            w = ops.dequantize_by_tile(wc, s_w, tile, None, bf16)
            y = F.conv_transpose2d(x, w, None, s, p)
            return ops.quantize_by_tile(y, s_out, y.shape, 8, torch.int8, o_out)

        def plain(r):
            return F.conv_transpose2d(xf[r % 2], wf, None, s, p)

        def same_macs(r):
            return ops.conv2d_w8a8(xs[r % 2], w_same, s_x, o_x, s_same, None, None, (1, 1), (0, 0), (1, 1), out_scale=s_out, out_offset=o_out)

        t_f, t_a, t_b, t_c = timed(fused), timed(chain), timed(plain), timed(same_macs)
        print(f"{name:34s} {t_f:7.1f}us {t_a:14.1f}us {t_b:13.1f}us {t_c:14.1f}us {t_a / t_f:8.2f} {t_b / t_f:8.2f} {t_f / t_c:8.2f}", flush=True)
        del xs, xf, wf, w_same


if __name__ == "__main__":
    main()
