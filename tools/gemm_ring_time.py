"""Time the PLAIN launches of the W8A8 GEMM (bf16 out, per-tensor asymmetric activations, per-channel weights) at T tokens on the
Llama-3-8B and Llama-3-70B shapes, codes drawn like the forward's (clipped normal), hipGraph-replayed between HIP events.
One line per shape; FFQ_LIB selects a variant build (tools/build_variant.sh) for the A/B of tools/gemm_ring_ab.sh.
usage: [FFQ_LIB=tools/_exp/libffq_x.so] python tools/gemm_ring_time.py [T]"""
import os, pathlib, sys
import torch
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
from fastforward_amd import ops, _native
if os.environ.get("FFQ_LIB"):
    from fastforward_amd._cabi import FFQLibrary
    _native._LIB = FFQLibrary(os.environ["FFQ_LIB"])
from bench import event_time_ms

T = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
dev = "cuda"
SHAPES = (("8b q/o", 4096, 4096), ("8b k/v", 1024, 4096), ("8b gate/up", 14336, 4096), ("8b down", 4096, 14336),
          ("70b q/o", 8192, 8192), ("70b k/v", 1024, 8192), ("70b gate/up", 28672, 8192), ("70b down", 8192, 28672))
torch.manual_seed(0)
for name, n, k in SHAPES:
    xq = (torch.randn(T, k, device=dev) * 20).round().clamp(-128, 127).to(torch.int8)
    wq = (torch.randn(n, k, device=dev) * 30).round().clamp(-128, 127).to(torch.int8)
    sx, ox = torch.tensor([0.02], device=dev), torch.tensor([4.0], device=dev)
    sw = torch.rand(n, device=dev) * 0.001 + 0.0005
    rs = wq.sum(dim=1, dtype=torch.int32)  # the forward hands the row sums over: the GEMM launch alone is timed
    ms = event_time_ms(lambda r: ops.linear_w8a8(xq, wq, sx, ox, sw, None, out_dtype=torch.bfloat16, w_rowsum=rs), iters=5, reps=4)
    print(f"{name:12s} N={n:5d} K={k:5d} {ms:.4f} ms {2 * T * n * k / ms / 1e9:8.1f} TOP/s", flush=True)
    del xq, wq
