"""GPTQ on one Llama-3-8B-shaped linear: the one-launch-per-block kernels (fused) vs the reference's column loop.

    python tools/gptq_time.py [rows cols] [--granularity channel0|g32|g128|tile|channel1] [--actorder]

channel0 (default): 4-bit asymmetric per output channel (ffq_gptq_block). The others are 4-bit symmetric, block 128, through
ffq_gptq_block_grid: g32 / g128 = PerBlock groups of 32 / 128 input channels (refitted per group), tile = PerTile (4, 32),
channel1 = per input channel.
"""
import argparse, pathlib, sys, time
import torch
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import fastforward_amd as ff
from fastforward_amd.quantization.gptq import gptq

GRANULARITIES = {
    "channel0": (ff.PerChannel(0), False),
    "g32": (ff.PerBlock(block_dims=1, block_sizes=32, per_channel_dims=0), True),
    "g128": (ff.PerBlock(block_dims=1, block_sizes=128, per_channel_dims=0), True),
    "tile": (ff.PerTile((4, 32)), True),
    "channel1": (ff.PerChannel(1), True),
}

parser = argparse.ArgumentParser()
parser.add_argument("shape", nargs="*", type=int, default=[4096, 4096])
parser.add_argument("--granularity", choices=sorted(GRANULARITIES), default="channel0")
parser.add_argument("--actorder", action="store_true")
args = parser.parse_args()
granularity, symmetric = GRANULARITIES[args.granularity]

dev = "cuda"
torch.manual_seed(0)
n_out, n_in = args.shape
acts = [((torch.randn(4, 512, n_in, device=dev),), {}) for _ in range(2)]
for fused in (True, True, False, True, False):  # the first pass warms hipSOLVER / hipBLASLt up
    layer = torch.nn.Linear(n_in, n_out, bias=False, device=dev)
    ff.quantize_model(layer)
    layer.weight_quantizer = ff.nn.LinearQuantizer(4, granularity=granularity, symmetric=symmetric, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad(), ff.strict_quantization(False):
        gptq(layer, acts, actorder=args.actorder, fused=fused)
    torch.cuda.synchronize()
    print(f"{args.granularity}{' actorder' if args.actorder else ''} fused={fused}: {time.perf_counter() - t0:.3f} s for [{n_out}, {n_in}]")
