"""Time ff.nn.functional.scaled_dot_product_attention on its one-launch kernel (csrc/ffq_sdpa.hip) against the device math path
(nn/sdpa.py's scaled_dot_product_attention_math: the reference's chain, which is what runs without the kernel) and against
ops.attention (the Llama harness's unquantized flash kernel, D = 128, [B, S, H, D] layout) at the same unquantized shape. Each line:
milliseconds per call (device events around `iters` calls after warm-up, best of 3) and TFLOP/s of the fused call, with flops
4·L·S·D per (batch, head) for one pass and 6·L·S·D for two passes, halved under causal. Run under
`rocprofv3 --kernel-trace --stats` in a run of its own for the per-kernel times.

    python tools/sdpa_time.py [--quick]
"""
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import fastforward_amd as ff  # noqa: E402

from fastforward_amd import ops  # noqa: E402
from fastforward_amd.nn.sdpa import scaled_dot_product_attention_math  # noqa: E402

DEV = "cuda"
F = ff.nn.functional


def ms_per_call(fn, iters):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(3):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            fn()
        end.record()
        torch.cuda.synchronize()
        best = min(best, start.elapsed_time(end) / iters)
    return best


def quantizer(scale, offset=0.0):
    q = ff.nn.LinearQuantizer(8, symmetric=False, granularity=ff.PerTensor(), device=DEV)
    q.quantization_range = (torch.tensor(-1.0, device=DEV), torch.tensor(1.0, device=DEV))
    with torch.no_grad():
        q.scale.fill_(scale)
        q.offset.fill_(offset)
    return q


def quantizer_set(name):
    weights = dict(attn_weights_quantizer=quantizer(1 / 255, 128.0))
    if name == "none":
        return {}
    if name == "weights":
        return weights
    return dict(weights, scaled_query_quantizer=quantizer(0.02), scaled_key_quantizer=quantizer(0.02), attn_scores_quantizer=quantizer(0.1),
                attn_mask_quantizer=quantizer(0.5), masked_scores_quantizer=quantizer(0.2), dropout_quantizer=quantizer(2.0**-8, 128.0),
                output_quantizer=quantizer(0.02))


def main():
    quick = "--quick" in sys.argv
    shapes = [(1, 32, 32, 512), (8, 32, 32, 512), (1, 32, 32, 2048), (8, 32, 32, 2048), (1, 32, 8, 2048), (8, 32, 8, 2048), (1, 32, 32, 8192)]
    if quick:
        shapes = shapes[:3]
    D = 128
    print(f"{'B':>2} {'Hq/H':>6} {'L=S':>5} {'causal':>6} {'quantizers':>10} {'fused ms':>9} {'math ms':>9} {'speed-up':>8} {'attn ms':>8} "
          f"{'fused/attn':>10} {'TFLOP/s':>8}", flush=True)
    for B, H, HKV, L in shapes:
        gen = torch.Generator().manual_seed(0)
        qp = torch.randn(B, L, H, D, generator=gen).bfloat16().to(DEV)
        kp = torch.randn(B, L, HKV, D, generator=gen).bfloat16().to(DEV)
        vp = torch.randn(B, L, HKV, D, generator=gen).bfloat16().to(DEV)
        q, k, v = qp.transpose(1, 2), kp.transpose(1, 2), vp.transpose(1, 2)
        math_fits = B * H * L * L * 4 * 8 < 120e9  # the chain holds several fp32 [B, H, L, S] tensors at once
        for causal in (False, True):
            for qset in ("none", "weights", "all8"):
                qz = quantizer_set(qset)
                kw = dict(is_causal=causal, enable_gqa=HKV != H, strict_quantization=False, **qz)
                with torch.no_grad():
                    iters = 3 if L >= 8192 else 10
                    fused = ms_per_call(lambda: F.scaled_dot_product_attention(q, k, v, **kw), iters)
                    chain = ms_per_call(lambda: scaled_dot_product_attention_math(q, k, v, **kw), 2) if math_fits else float("nan")
                    attn = ms_per_call(lambda: ops.attention(qp.flatten(2), kp.flatten(2), vp.flatten(2), D, causal=causal), iters) if qset == "none" else float("nan")
                passes = 4 if qset == "none" else 6
                flops = passes * L * L * D * B * H / (2 if causal else 1)
                print(f"{B:>2} {f'{H}/{HKV}':>6} {L:>5} {str(causal):>6} {qset:>10} {fused:9.3f} {chain:9.3f} {chain / fused:8.1f} {attn:8.3f} "
                      f"{fused / attn:10.2f} {flops / fused / 1e9:8.1f}", flush=True)
        del qp, kp, vp, q, k, v
        torch.cuda.empty_cache()
    # what the scaled-key quantizer adds to a call (its codes written once by sdpa_key_codes_kernel), next to one A1 launch over K
    # (ops.quantize_by_tile: the floor of any pass that writes codes of K). Forming the codes per staged tile instead, in every query
    # block, added 0.47 ms (B = 1, L = 2048) to 4.9 ms (B = 1, L = 8192) on MI355X: docs/kernels.md.
    print(f"\n{'B':>2} {'Hq/H':>6} {'L=S':>5} {'weights ms':>10} {'+ scaled-K ms':>13} {'added ms':>19} {'A1 over K ms':>13}", flush=True)
    for B, H, HKV, L in [(1, 32, 32, 2048), (8, 32, 8, 2048), (8, 32, 32, 2048), (1, 32, 32, 8192)][: 1 if quick else 4]:
        gen = torch.Generator().manual_seed(0)
        q = torch.randn(B, L, H, D, generator=gen).bfloat16().to(DEV).transpose(1, 2)
        kp = torch.randn(B, L, HKV, D, generator=gen).bfloat16().to(DEV)
        v = torch.randn(B, L, HKV, D, generator=gen).bfloat16().to(DEV).transpose(1, 2)
        k = kp.transpose(1, 2)
        base = dict(enable_gqa=HKV != H, strict_quantization=False, **quantizer_set("weights"))
        iters = 3 if L >= 8192 else 10
        with torch.no_grad():
            plain = ms_per_call(lambda: F.scaled_dot_product_attention(q, k, v, **base), iters)
            keyed = ms_per_call(lambda: F.scaled_dot_product_attention(q, k, v, scaled_key_quantizer=quantizer(0.02), **base), iters)
            s_k, o_k = torch.tensor([0.02], device=DEV), torch.tensor([0.0], device=DEV)
            prepass = ms_per_call(lambda: ops.quantize_by_tile(kp, s_k, kp.shape, 8, torch.int8, o_k), iters)
        print(f"{B:>2} {f'{H}/{HKV}':>6} {L:>5} {plain:10.3f} {keyed:13.3f} {keyed - plain:19.3f} {prepass:13.3f}", flush=True)


if __name__ == "__main__":
    main()
