"""Time scaled_dot_product_attention for one new token over an int8 KV cache (csrc/ffq_sdpa_decode.hip) in one process on one device.

Three routes per shape (B in {1, 8}, 32 query heads on 8 kv heads, E = 128, bf16, L = 1, S in {2048, 8192, 32768}), on the same codes:

    decode   ff.nn.functional.scaled_dot_product_attention with K / V as int8 codes: the split-key kernels;
    math     nn/sdpa.py's scaled_dot_product_attention_math on the same int8 codes: what that call ran before these kernels;
    prefill  the one-launch kernel of csrc/ffq_sdpa.hip on the same codes held in a bf16 container.

Microseconds per call are device time: the calls of a route are captured into one hipGraph over `n` rotating copies of the cache
(n * bytes >= 512 MB where that fits in 64 copies, so a call does not find its codes in the caches from the call before), the graph is
replayed after a warm-up replay, and device events around the replays give the time (best of 3). The math path is timed eagerly
(device events around 3 calls after one warm-up call): it is milliseconds long and holds fp32 copies of the cache. GB/s is the
codes read once (B * 8 * S * 128 bytes for K and the same for V) over that time, beside the 6.29 TB/s copy ceiling of
docs/kernels.md.

    python tools/sdpa_decode_time.py            the table
    python tools/sdpa_decode_time.py --sweep    forced split counts per shape (ops.sdpa_decode(..., splits=n)) beside the rule's choice
"""
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import fastforward_amd as ff  # noqa: E402

from fastforward_amd import ops  # noqa: E402
from fastforward_amd.nn.sdpa import scaled_dot_product_attention_math  # noqa: E402
from fastforward_amd.quantization.affine import static  # noqa: E402

DEV = "cuda"
F = ff.nn.functional
H, HKV, E, L = 32, 8, 128, 1
SHAPES = [(B, S) for B in (1, 8) for S in (2048, 8192, 32768)]
CEILING = 6.29e12
K_PARAMS, V_PARAMS = (0.031, 3.0), (0.027, -9.0)


def codes(raw, params, container):
    scale, offset = (torch.tensor([p], dtype=torch.float32, device=DEV) for p in params)
    context = static.quantization_context(scale, offset, num_bits=8, output_dtype=container, dequantize_dtype=torch.bfloat16)
    return ff.QuantizedTensor(raw.to(container), context)


def graph_us(calls, replays=5):
    """Device microseconds per call of `calls` (a list of thunks), captured into one graph."""
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream), torch.no_grad():
        calls[0]()
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream), torch.no_grad():
        for call in calls:
            call()
    graph.replay()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(3):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(replays):
            graph.replay()
        end.record()
        torch.cuda.synchronize()
        best = min(best, start.elapsed_time(end) * 1e3 / (replays * len(calls)))
    return best


def eager_us(call, iters=3):
    with torch.no_grad():
        call()
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            call()
        end.record()
        torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters


def caches(B, S):
    """Rotating int8 copies of (K, V): >= 512 MB in all where 64 copies reach that."""
    nbytes = 2 * B * HKV * S * E
    n = max(2, min(64, -(-(512 << 20) // nbytes)))
    gen = torch.Generator(device=DEV).manual_seed(S + B)
    return [tuple(torch.randint(-128, 128, (B, S, HKV, E), generator=gen, device=DEV, dtype=torch.int8).transpose(1, 2) for _ in range(2)) for _ in range(n)]


def main():
    sweep = "--sweep" in sys.argv
    print(f"device: {torch.cuda.get_device_name(0)}; H/HKV = {H}/{HKV}, E = {E}, L = {L}, bf16; K / V codes int8, [B, S, HKV, E] seen transposed", flush=True)
    if sweep:
        counts = (1, 2, 4, 8, 16, 32, 64)
        print(f"{'B':>2} {'S':>6} {'rule':>5} " + " ".join(f"{f'n={n} us':>10}" for n in counts), flush=True)
    else:
        print(f"{'B':>2} {'S':>6} {'splits':>6} {'decode us':>10} {'GB/s':>7} {'of 6.29 TB/s':>12} {'math us':>10} {'math/decode':>11} {'prefill us':>10} {'prefill/decode':>14}", flush=True)
    for B, S in SHAPES:
        q = torch.randn(B, H, L, E, generator=torch.Generator().manual_seed(1)).bfloat16().to(DEV)
        pairs = caches(B, S)
        moved = 2 * B * HKV * S * E
        rule = ops.sdpa_decode_plan(B, HKV, S, L * H // HKV, E)
        deq = (None, *[tuple(torch.tensor([p], dtype=torch.float32, device=DEV) for p in params) for params in (K_PARAMS, V_PARAMS)])
        if sweep:
            times = []
            for n in counts:
                tiles = -(-S // 128)
                times.append(graph_us([lambda k=k, v=v: ops.sdpa_decode(q, k, v, dequant=deq, splits=n) for k, v in pairs]) if n <= tiles else float("nan"))
            print(f"{B:>2} {S:>6} {rule:>5} " + " ".join(f"{t:10.1f}" for t in times), flush=True)
            continue
        held = [(codes(k, K_PARAMS, torch.int8), codes(v, V_PARAMS, torch.int8)) for k, v in pairs]
        kw = dict(enable_gqa=True, strict_quantization=False)
        launched = [0]
        real = ops.sdpa_decode

        def counted(*a, **k):
            launched[0] += 1
            return real(*a, **k)

        ops.sdpa_decode = counted
        try:
            decode = graph_us([lambda k=k, v=v: F.scaled_dot_product_attention(q, k, v, **kw) for k, v in held])
        finally:
            ops.sdpa_decode = real
        assert launched[0] == len(held) + 1, "the decode kernels did not serve the call"
        math = eager_us(lambda: scaled_dot_product_attention_math(q, *held[0], **kw))
        wide = [(codes(k, K_PARAMS, torch.bfloat16), codes(v, V_PARAMS, torch.bfloat16)) for k, v in pairs[:4]]
        prefill = graph_us([lambda k=k, v=v: F.scaled_dot_product_attention(q, k, v, **kw) for k, v in wide], replays=2)
        rate = moved / (decode * 1e-6)
        note = "" if decode < math else "   <- NOT faster than the math path"
        print(f"{B:>2} {S:>6} {rule:>6} {decode:10.1f} {rate / 1e9:7.0f} {rate / CEILING:12.1%} {math:10.1f} {math / decode:11.1f} {prefill:10.1f} "
              f"{prefill / decode:14.1f}{note}", flush=True)
        del pairs, held, wide
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
