"""Time the one-pass unfold + quantize kernel (csrc/ffq_unfold.hip) against the reference's route in one process on one device,
interleaved layer by layer: the same ``ff.nn.functional.unfold`` call, with int8 codes in and an 8-bit output quantizer, once
with this package's registration (one launch: codes in, codes out) and once with the registration taken out of the dispatcher
(the fallback chain: A2 of the codes into bf16, ATen's im2col, A1 over the ``KH * KW`` times larger tensor). bf16 throughout.

  3x3 p1 and 7x7 s2 p3 on [32, 64, 56, 56] (im2col + GEMM convolutions), a 16x16 s16 patch extraction on [32, 3, 224, 224]
  (a ViT stem) and a 1-D window (1, 7) on [8, 512, 1, 4096].

Each line: microseconds per call (hipGraph-replayed, median of three), the ratio, and the fused call's algorithmic bytes (1 B per
input code in, 1 B per output code out) over its time as a fraction of 8 TB/s. The inputs alternate between two buffers; the smaller
layers stay in the 256 MiB Infinity Cache, so the fraction is of the HBM RATE, not a claim that the bytes came from HBM.
``python tools/unfold_time.py > profiles/unfold_time.txt`` writes the committed table."""
import contextlib
import pathlib
import statistics
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import fastforward_amd as ff  # noqa: E402

from bench import event_time_ms  # noqa: E402
from fastforward_amd import dispatcher, fused_unfold, ops  # noqa: E402

F = ff.nn.functional
dev = "cuda"
bf16 = torch.bfloat16
PEAK_TBPS = 8.0

# name, input shape, kernel_size, dilation, padding, stride
LAYERS = [
    ("3x3 p1        [32, 64, 56, 56]", (32, 64, 56, 56), 3, 1, 1, 1),
    ("7x7 s2 p3     [32, 64, 56, 56]", (32, 64, 56, 56), 7, 1, 3, 2),
    ("16x16 s16     [32, 3, 224, 224]", (32, 3, 224, 224), 16, 1, 0, 16),
    ("(1, 7)        [8, 512, 1, 4096]", (8, 512, 1, 4096), (1, 7), 1, 0, 1),
]


def quantizer(lo, hi):
    q = ff.nn.LinearQuantizer(8, symmetric=False, quantized_dtype=torch.int8, device=dev)
    q.quantization_range = (torch.tensor(lo, device=dev), torch.tensor(hi, device=dev))
    return q


@contextlib.contextmanager
def chain_only():
    """The dispatcher without this package's unfold kernel: the fallback chain runs."""
    kept = dispatcher._DISPATCHER["unfold"]
    dispatcher._DISPATCHER["unfold"] = [it for it in kept if getattr(it.fn, "__self__", None) is not fused_unfold.KERNELS]
    try:
        yield
    finally:
        dispatcher._DISPATCHER["unfold"] = kept


def timed(fn):
    return statistics.median(event_time_ms(fn, iters=10, reps=4) for _ in range(3)) * 1e3


def main() -> None:
    only = sys.argv[1:]
    q_in, q_out = quantizer(-4.0, 5.0), quantizer(-6.0, 7.0)
    launches = {"n": 0}
    real = ops.unfold_quantize

    def counted(*a, **k):
        launches["n"] += 1
        return real(*a, **k)

    ops.unfold_quantize = counted
    print(f"{'layer':34s} {'fused':>10s} {'chain A2+im2col+A1':>19s} {'chain/fused':>12s} {'MB moved':>9s} {'of 8 TB/s':>10s}")
    with torch.no_grad(), ff.strict_quantization(False):
        for name, shape, k, d, p, s in LAYERS:
            if only and not any(o in name for o in only):
                continue
            xs = [q_in((torch.randn(shape, device=dev) * 2).to(bf16)) for _ in range(2)]

            def call(r):
                return F.unfold(xs[r % 2], k, d, p, s, output_quantizer=q_out)

            before = launches["n"]
            out = call(0)
            assert launches["n"] == before + 1 and out.raw_data.dtype == torch.int8  # the fused route, codes out
            with chain_only():
                want = call(0)
                assert launches["n"] == before + 1 and torch.equal(want.raw_data, out.raw_data)  # the chain, and the same bits
                t_chain = timed(call)
            t_fused = timed(call)
            nbytes = xs[0].numel() + out.numel()
            share = nbytes / (t_fused * 1e-6) / (PEAK_TBPS * 1e12)
            print(f"{name:34s} {t_fused:8.1f}us {t_chain:17.1f}us {t_chain / t_fused:12.2f} {nbytes / 1e6:9.1f} {share:10.3f}", flush=True)
            del xs, out, want


if __name__ == "__main__":
    main()
