"""ff.nn.functional.scaled_dot_product_attention for a short query over int8 K / V codes on the MI355X: the split-key kernels of
csrc/ffq_sdpa_decode.hip against answers known by construction (tests/attention_exact.py), against the float64 attention of the
dequantized operands under the project's attention contract, and against the device math path (nn/sdpa.py), which is what the call ran
before these kernels. Every test counts the calls of ``ops.sdpa_decode`` and of ``ops.sdpa_quantize``: a served call makes exactly one
of the first and none of the second, so a silent fallback fails."""

import functools
import math

import pytest
import torch

import fastforward_amd as ff

import attention_exact as ax
import guards

from fastforward_amd import fused_sdpa_decode, ops
from fastforward_amd.exceptions import QuantizationError
from fastforward_amd.nn.sdpa import scaled_dot_product_attention_math
from fastforward_amd.ops import decode
from test_sdpa_decode_cpu import G31, as_codes, linear_quantizer, run_g31

pytestmark = pytest.mark.gpu
F = ff.nn.functional
DEV = "cuda"
CAP = decode.MAX_SPLITS
DTYPES = (torch.bfloat16, torch.float16)


@pytest.fixture
def launches(monkeypatch):
    count = {"decode": 0, "quantize": 0}
    real_decode, real_quantize = ops.sdpa_decode, ops.sdpa_quantize

    def counting_decode(*args, **kwargs):
        count["decode"] += 1
        return real_decode(*args, **kwargs)

    def counting_quantize(*args, **kwargs):
        count["quantize"] += 1
        return real_quantize(*args, **kwargs)

    monkeypatch.setattr(ops, "sdpa_decode", counting_decode)
    monkeypatch.setattr(ops, "sdpa_quantize", counting_quantize)
    return count


def served(launches, *args, **kwargs):
    """The call through ff.nn.functional: exactly one decode call, no call of the prefill kernel."""
    kwargs.setdefault("strict_quantization", False)
    before = dict(launches)
    with torch.no_grad():
        out = F.scaled_dot_product_attention(*args, **kwargs)
    assert launches["decode"] == before["decode"] + 1 and launches["quantize"] == before["quantize"], "the decode kernels did not serve the call"
    return out


def declined(launches, *args, **kwargs):
    """Zero launches of either kernel, and the math path's bits."""
    kwargs.setdefault("strict_quantization", False)
    before = dict(launches)
    torch.manual_seed(5)
    got = F.scaled_dot_product_attention(*args, **kwargs)
    assert dict(launches) == before, "a declined call reached a kernel"
    torch.manual_seed(5)
    want = scaled_dot_product_attention_math(*args, **kwargs)
    assert torch.equal(got, want)


def math_path(*args, **kwargs):
    kwargs.setdefault("strict_quantization", False)
    with torch.no_grad():
        return scaled_dot_product_attention_math(*args, **kwargs)


def meets_the_contract(got, want, ref, what=""):
    """The rule of tests/test_sdpa_gpu.py: the error against float64 is at most the device math path's own on the same call + 2^-9."""
    err_got = float((got.cpu().double() - ref).abs().max())
    err_math = float((want.cpu().double() - ref).abs().max())
    assert err_got <= err_math + 2.0**-9, f"{what}: {err_got:.3e} from float64, math path {err_math:.3e}"


def quantized(x, spec, container=torch.int8):
    with torch.no_grad():
        return linear_quantizer(spec, DEV, container)(x.to(DEV))


def random_operands(B, H, HKV, L, S, E, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, L, E, generator=gen).to(dtype).to(DEV)
    k = quantized(torch.randn(B, HKV, S, E, generator=gen).to(dtype), (8, 0.031, 3.0))
    v = quantized(torch.randn(B, HKV, S, E, generator=gen).to(dtype), (8, 0.027, -9.0))
    return q, k, v


def reference(q, k, v, **kw):
    deq = [t.dequantize() if isinstance(t, ff.QuantizedTensor) else t for t in (q, k, v)]
    return ax.reference64(*deq, **kw)


# ---- 1. known answers ---------------------------------------------------------------------------------------------------------------
ROWS = ((1, 1), (1, 4), (1, 8), (2, 4), (5, 1), (8, 4), (32, 1))  # (L, H / HKV)
KEYS = (1, 63, 64, 65, 129, 1000)
SPLITS = (0, 1, 2, 3, CAP)
V_OFFSETS = (0.0, 200.0, -200.0, 37.0)


def to_k_codes(k, scale, offset, dtype):
    """The pattern's keys (small integers times `scale`) as int8 codes c = k / scale - offset; refuses what does not fit."""
    c = k.double() / scale - offset
    assert bool((c == c.round()).all()) and float(c.min()) >= -128 and float(c.max()) <= 127
    return as_codes(c.to(torch.int8), scale, offset, dtype, DEV)


def drawn_v(shape, dtype, seed):
    """V = (c + o) * 2^-e rounded once to the dtype, c over all of [-128, 127]: (codes, scale, offset, the values in `dtype`)."""
    gen = ax.generator("decode_v", shape, str(dtype), seed)
    c = torch.randint(-128, 128, shape, generator=gen)
    c.view(-1)[:256] = torch.arange(-128, 128)[torch.randperm(256, generator=gen)][: c.numel()]  # every code at least once where there is room
    offset, e = V_OFFSETS[seed % 4], (0, 3, 7)[seed % 3]
    values = ((c.float() + offset) * 2.0**-e).to(dtype)
    return c.to(torch.int8), 2.0**-e, offset, values


@functools.lru_cache(maxsize=None)
def decode_patterns(L, G, S, E, dtype):
    """(pattern, K codes, V codes) of the four patterns at B = 2, HKV = 2, built once and left unchanged. The expectation and the
    bound are the module's own (``_onehot`` asserts r <= 2^-24 on the inputs, before any launch)."""
    shape = ax.Shape(2, 2 * G, 2, L, S, E)
    seed = L + 7 * G + S + E + DTYPES.index(dtype)
    out = []
    for base, (k_scale, k_offset) in ((ax.select(shape, dtype, causal=False), (1.0, 100.0)),
                                      (ax.staircase(shape, dtype, causal=L > 1), (1.0, 8.0)),
                                      (ax.mask_select(shape, dtype, ax.MASK_LEADS[seed % 3], mask_dtype=(None, torch.float32)[seed % 2]), (2.0**-2, -100.0))):
        vc, vs, vo, values = drawn_v((2, 2, S, E), dtype, seed + len(out))
        p = ax._onehot(base.name, shape, dtype, base.q.double(), base.k.double(), values, base.target, causal=base.causal, mask=base.mask, scale=base.scale)
        assert p.residual <= ax.RESIDUAL_LIMIT
        out.append((p, to_k_codes(base.k, k_scale, k_offset, dtype), as_codes(vc, vs, vo, dtype, DEV)))
    u = ax.uniform(shape, dtype, variant=seed % 2)
    out.append((u, to_k_codes(u.k, 2.0**-2, 100.0, dtype), as_codes((u.v.double() - 100.0).to(torch.int8), 1.0, 100.0, dtype, DEV)))
    return tuple(out)


@pytest.mark.parametrize("S", KEYS)
@pytest.mark.parametrize("L,G", ROWS, ids=[f"L{L}xG{G}" for L, G in ROWS])
def test_known_answers_at_every_split(launches, L, G, S):
    """select / staircase / uniform / mask_select with K and V handed in as int8 codes, E 64 and 128, bf16 and fp16, at the rule's
    split and at forced ones (a forced split may hold no key). Bounds: attention_exact's own (docs/numerics.md derives why the split
    form needs no further term)."""
    for E in (64, 128):
        for dtype in DTYPES:
            for p, kc, vc in decode_patterns(L, G, S, E, dtype):
                q = p.q.to(DEV)
                mask = None if p.mask is None else p.mask.to(DEV)
                first = served(launches, q, kc, vc, attn_mask=mask, is_causal=p.causal, scale=p.scale, enable_gqa=True)
                assert (why := ax.explain(p, first)) is None, why
                operands, dequant = zip(*(fused_sdpa_decode.KERNELS._dequant(t) for t in (q, kc, vc)))
                for splits in SPLITS:
                    got = ops.sdpa_decode(*operands, attn_mask=mask, is_causal=p.causal, scale=p.scale, dequant=dequant, dtype=dtype, splits=splits)
                    assert (why := ax.explain(p, got)) is None, f"splits={splits}: {why}"
                    if splits == 0:
                        assert torch.equal(got, first)


# ---- 2. the project's attention contract --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 17, 100, 1000, 4096])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("E", [64, 128])
def test_random_operands_meet_the_attention_contract(launches, S, dtype, E):
    q, k, v = random_operands(2, 8, 2, 1, S, E, dtype, seed=S * 3 + E)
    got = served(launches, q, k, v, enable_gqa=True)
    assert got.dtype == dtype and got.shape == (2, 8, 1, E)
    meets_the_contract(got, math_path(q, k, v, enable_gqa=True), reference(q, k, v), f"S={S}")


@pytest.mark.parametrize("container", [torch.int8, None], ids=["q_int8", "q_value_dtype"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_quantized_queries_in_either_container(launches, container, dtype):
    q, k, v = random_operands(2, 4, 2, 4, 300, 128, dtype, seed=9)
    qq = quantized(q, (8, 0.04, 5.0), container)
    assert qq.raw_data.dtype == (container or dtype)
    got = served(launches, qq, k, v, enable_gqa=True, scale=0.11)
    meets_the_contract(got, math_path(qq, k, v, enable_gqa=True, scale=0.11), reference(qq, k, v, scale=0.11))


# ---- 3. masks --------------------------------------------------------------------------------------------------------------------------
def test_a_fully_masked_row_is_exact_zeros_and_a_fully_masked_split_adds_nothing(launches):
    B, H, HKV, L, S, E = 2, 4, 2, 4, 300, 128
    q, k, v = random_operands(B, H, HKV, L, S, E, torch.bfloat16, seed=3)
    mask = torch.rand(B, H, L, S, generator=torch.Generator().manual_seed(3)) > 0.3
    mask[:, :, 2] = False                                 # a row without a key
    mask[:, :, :, 128:256] = False                        # the second of three forced splits (keys 128..255): all masked
    mask = mask.to(DEV)
    got = served(launches, q, k, v, attn_mask=mask, enable_gqa=True)
    want, ref = math_path(q, k, v, attn_mask=mask, enable_gqa=True), reference(q, k, v, mask=mask)
    assert torch.equal(got[:, :, 2], torch.zeros_like(got[:, :, 2])) and torch.equal(want[:, :, 2], got[:, :, 2])
    meets_the_contract(got, want, ref)
    operands, dequant = zip(*(fused_sdpa_decode.KERNELS._dequant(t) for t in (q, k, v)))
    assert decode.sdpa_decode_split_ranges(S, 3)[1] == (128, 256)
    for splits in (1, 3, CAP):
        forced = ops.sdpa_decode(*operands, attn_mask=mask, dequant=dequant, splits=splits)
        assert torch.equal(forced[:, :, 2], torch.zeros_like(forced[:, :, 2]))
        meets_the_contract(forced, want, ref, f"splits={splits}")


@pytest.mark.parametrize("lead", ["LS", "11LS", "B1LS", "BHLS"])
@pytest.mark.parametrize("mask_dtype", [torch.float32, None], ids=["fp32", "data_dtype"])
def test_float_masks_broadcast_over_their_leading_dims(launches, lead, mask_dtype):
    B, H, HKV, L, S, E = 2, 4, 2, 3, 200, 64
    dtype = torch.float16
    q, k, v = random_operands(B, H, HKV, L, S, E, dtype, seed=4)
    shape = {"LS": (L, S), "11LS": (1, 1, L, S), "B1LS": (B, 1, L, S), "BHLS": (B, H, L, S)}[lead]
    mask = (torch.randn(shape, generator=torch.Generator().manual_seed(len(lead))) * 2).to(mask_dtype or dtype)
    mask[..., 0, 5:9] = -math.inf
    mask = mask.to(DEV)
    got = served(launches, q, k, v, attn_mask=mask, enable_gqa=True)
    meets_the_contract(got, math_path(q, k, v, attn_mask=mask, enable_gqa=True), reference(q, k, v, mask=mask))


@pytest.mark.parametrize("S", [5, 8, 300])
def test_is_causal_is_the_math_paths_top_left_tril(launches, S):
    q, k, v = random_operands(2, 8, 2, 8, S, 128, torch.bfloat16, seed=S)
    got = served(launches, q, k, v, is_causal=True, enable_gqa=True)
    meets_the_contract(got, math_path(q, k, v, is_causal=True, enable_gqa=True), reference(q, k, v, causal=True))
    one = served(launches, q[:, :, :1], k, v, is_causal=True, enable_gqa=True)     # row 0 sees key 0 alone: V[0], rounded once
    groups = v.dequantize()[:, :, :1].repeat_interleave(4, 1)
    assert torch.equal(one, groups)


# ---- 4. the output quantizer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("splits_shape", [(300, 64), (1000, 128)])
def test_the_output_quantizer_runs_on_the_fp32_value(launches, dtype, splits_shape):
    S, E = splits_shape
    q, k, v = random_operands(2, 8, 2, 2, S, E, dtype, seed=S)
    bits, step, offset = 8, 2.0**-5, 3.0
    oq = linear_quantizer((bits, step, offset), DEV)
    got = served(launches, q, k, v, enable_gqa=True, output_quantizer=oq)
    assert type(got) is torch.Tensor and got.dtype == dtype
    units = got.cpu().double() / step
    assert torch.equal(units, units.round()), "an output is not a multiple of the scale"
    assert float((units - offset).min()) >= -2 ** (bits - 1) and float((units - offset).max()) <= 2 ** (bits - 1) - 1
    ref = reference(q, k, v)
    fake = (torch.clamp(torch.round(ref / step - offset), -2 ** (bits - 1), 2 ** (bits - 1) - 1) + offset) * step
    assert float((got.cpu().double() - fake).abs().max()) <= step


# ---- 5. views, at the ops level -------------------------------------------------------------------------------------------------------------
def test_views_are_taken_as_they_are(launches):
    B, H, HKV, L, S, E = 2, 8, 2, 1, 333, 128
    gen = torch.Generator().manual_seed(12)
    q = torch.randn(B, H, L, E, generator=gen).bfloat16().to(DEV)
    kc, vc = (torch.randint(-128, 128, (B, HKV, S, E), generator=gen).to(torch.int8).to(DEV) for _ in range(2))
    ks, vs = (torch.tensor([0.03], device=DEV), torch.tensor([4.0], device=DEV)), (torch.tensor([0.02], device=DEV), None)

    def run(qx, kx, vx):
        return ops.sdpa_decode(qx, kx, vx, dequant=(None, ks, vs))

    want = run(q, kc, vc)
    # the projections' layout [B, S, H, E], seen through .transpose(1, 2)
    qp, kp, vp = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (q, kc, vc))
    assert not kp.is_contiguous() and torch.equal(run(qp, kp, vp), want)
    # a [:, :, :S] slice of a longer int8 buffer (a pre-allocated cache)
    longer = [torch.full((B, HKV, S + 200, E), 77, dtype=torch.int8, device=DEV) for _ in range(2)]
    for buffer, codes in zip(longer, (kc, vc)):
        buffer[:, :, :S] = codes
    assert torch.equal(run(q, longer[0][:, :, :S], longer[1][:, :, :S]), want)
    # pointers offset by a multiple of 16 bytes
    flat = [torch.empty(t.numel() + 48, dtype=torch.int8, device=DEV) for t in (kc, vc)]
    shifted = [f[off:off + t.numel()].view(t.shape).copy_(t) for f, t, off in zip(flat, (kc, vc), (16, 48))]
    assert all(t.data_ptr() % 16 == 0 and t.data_ptr() % 512 != 0 for t in shifted) and torch.equal(run(q, *shifted), want)
    assert launches["decode"] == 4 and launches["quantize"] == 0
    # a misaligned pointer: the predicate declines, nothing is launched, the math path answers
    odd = torch.empty(kc.numel() + 16, dtype=torch.int8, device=DEV)[8:8 + kc.numel()].view(kc.shape).copy_(kc)
    assert odd.data_ptr() % 16 == 8
    k_odd, v_q = as_codes(odd, 0.03, 4.0, torch.bfloat16, DEV), as_codes(vc, 0.02, None, torch.bfloat16, DEV)
    assert not fused_sdpa_decode.sdpa_decode_predicate(query=q, key=k_odd, value=v_q, enable_gqa=True, strict_quantization=False)
    with torch.no_grad():
        declined(launches, q, k_odd, v_q, enable_gqa=True)
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            run(q, odd, vc)
    assert launches["decode"] == 5  # (the refused ops call above was counted, and launched nothing)


# ---- 6. declines ------------------------------------------------------------------------------------------------------------------------
def test_declines_reach_the_math_path(launches):
    bf = torch.bfloat16
    q, k, v = random_operands(1, 2, 2, 4, 40, 128, bf, seed=6)
    with torch.no_grad():
        q33 = torch.randn(1, 2, 33, 128, device=DEV).to(bf)
        declined(launches, q33, k, v)                                                               # 33 rows
        declined(launches, q, k, v, neg_inf=-1e4)                                                   # a finite neg_inf
        declined(launches, q, k, v, attn_weights_quantizer=linear_quantizer((8, 2.0**-8, 128.0), DEV))   # an active weights quantizer
        declined(launches, q, k, v.dequantize())                                                    # K int8 with V bf16
        declined(launches, q, k, quantized(v.dequantize(), (8, 0.027, -9.0), None))                 # ... and with V codes held in bf16
        pc = ff.nn.LinearQuantizer(8, granularity=ff.PerChannel(1), quantized_dtype=torch.int8, device=DEV)
        pc.quantization_range = (torch.full((2,), -3.0, device=DEV), torch.full((2,), 3.0, device=DEV))
        declined(launches, q, pc(k.dequantize()), v)                                                # per-channel K codes
        declined(launches, q, k, v, dropout_p=0.3)                                                  # dropout
        q96, k96, v96 = random_operands(1, 2, 2, 4, 40, 96, bf, seed=7)
        declined(launches, q96, k96, v96)                                                           # E = 96
    # a strict call: whatever the math path does with it (it raises: plain q under strict quantization), the kernels are not asked
    before = dict(launches)
    with torch.no_grad():
        with pytest.raises(QuantizationError) as theirs:
            scaled_dot_product_attention_math(q, k, v, strict_quantization=True)
        with pytest.raises(QuantizationError) as ours:
            F.scaled_dot_product_attention(q, k, v, strict_quantization=True)
    assert str(ours.value) == str(theirs.value) and dict(launches) == before
    # an operand that needs a gradient: declined; the math path then fails in the safe softmax's where(out=...) as the reference's does
    qg = q.clone().requires_grad_(True)
    assert not fused_sdpa_decode.sdpa_decode_predicate(query=qg, key=k, value=v, strict_quantization=False)
    with pytest.raises(RuntimeError, match="out=... arguments don't support automatic differentiation"):
        F.scaled_dot_product_attention(qg, k, v, strict_quantization=False)
    assert dict(launches) == before


# ---- 7. a decode loop -----------------------------------------------------------------------------------------------------------------------
def test_a_decode_loop_appends_codes_and_launches_once_per_step(launches):
    B, H, HKV, E, dtype = 2, 8, 2, 128, torch.bfloat16
    gen = torch.Generator().manual_seed(21)
    kq, vq = linear_quantizer((8, 0.031, 3.0), DEV, torch.int8), linear_quantizer((8, 0.027, -9.0), DEV, torch.int8)
    with torch.no_grad():
        K = kq(torch.randn(B, HKV, 59, E, generator=gen).to(dtype).to(DEV))
        V = vq(torch.randn(B, HKV, 59, E, generator=gen).to(dtype).to(DEV))
    for step in range(8):
        with torch.no_grad():
            k_new, v_new = (quant(torch.randn(B, HKV, 1, E, generator=gen).to(dtype).to(DEV)) for quant in (kq, vq))
            K, V = torch.cat([K, k_new], dim=2), torch.cat([V, v_new], dim=2)                       # the code-level cat: nothing is dequantized
        assert isinstance(K, ff.QuantizedTensor) and K.raw_data.dtype == torch.int8 and K.shape[2] == 60 + step
        q_t = torch.randn(B, H, 1, E, generator=gen).to(dtype).to(DEV)
        got = served(launches, q_t, K, V, enable_gqa=True)
        meets_the_contract(got, math_path(q_t, K, V, enable_gqa=True), reference(q_t, K, V), f"step {step}")
    assert launches["decode"] == 8 and K.shape[2] == 67


# ---- 8. graph capture -----------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_eager_result(launches):
    q, k, v = random_operands(2, 8, 2, 1, 1000, 128, torch.bfloat16, seed=8)
    oq = linear_quantizer((8, 2.0**-5, 0.0), DEV)
    kw = dict(enable_gqa=True, output_quantizer=oq, strict_quantization=False)
    with torch.no_grad():
        eager = F.scaled_dot_product_attention(q, k, v, **kw)
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            F.scaled_dot_product_attention(q, k, v, **kw)
        torch.cuda.current_stream().wait_stream(stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            captured = F.scaled_dot_product_attention(q, k, v, **kw)
        graph.replay()
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(captured, eager) and launches["decode"] == 3 and launches["quantize"] == 0


# ---- 9. guard bands -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splits", [0, 5])
@pytest.mark.parametrize("L,G,S,E", [(1, 4, 1000, 128), (5, 1, 65, 64), (8, 4, 300, 128)])
def test_guard_bands_around_the_output_and_the_workspace(launches, splits, L, G, S, E):
    """`out` and the workspace are carved from an arena (tests/guards.py) whose guards and fresh bodies hold a poison byte; two runs with
    two poisons: every guard keeps its poison (no stray write), and the runs agree with each other and with an unguarded run on every
    output byte (none left unwritten, none that depends on what the workspace held)."""
    gen = torch.Generator().manual_seed(S)
    q = torch.randn(2, 2 * G, L, E, generator=gen).bfloat16().to(DEV)
    kc, vc = (torch.randint(-128, 128, (2, 2, S, E), generator=gen).to(torch.int8).to(DEV) for _ in range(2))
    ks, vs = (torch.tensor([0.03], device=DEV), torch.tensor([4.0], device=DEV)), (torch.tensor([0.02], device=DEV), torch.tensor([-200.0], device=DEV))

    def run():
        return ops.sdpa_decode(q, kc, vc, dequant=(None, ks, vs), splits=splits)

    results = []
    for poison in (guards.POISON_A, guards.POISON_B):
        arena = guards.Arena(poison)
        with guards.capture(arena):
            out = run()
        torch.cuda.synchronize()
        fresh = [b for b in arena.blocks if b.kind == "fresh"]
        count = splits or ops.sdpa_decode_plan(2, 2, S, L * G, E)
        assert arena.find(out.data_ptr()) is not None and sorted(b.nbytes for b in fresh) == sorted([out.numel() * 2, ops.sdpa_decode_workspace_bytes(2, 2, L * G, E, count)])
        assert not arena.touched_guards(), arena.touched_guards()
        results.append(out.clone())
    plain = run()
    assert torch.equal(results[0].view(torch.int16), results[1].view(torch.int16)) and torch.equal(results[0].view(torch.int16), plain.view(torch.int16))
    assert launches["decode"] == 3


# ---- 10. G31 on the device ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(G31))
def test_the_reference_cases_on_the_device(launches, name):
    """The fixture's calls on the device, inside the attention contract of item 2: float64 attention of the dequantized operands."""
    case = G31[name]
    before = launches["decode"]
    got = run_g31(case, DEV)
    assert launches["decode"] == before + 1 and launches["quantize"] == 0
    want = run_g31(case, DEV, fn=scaled_dot_product_attention_math)
    ref = run_g31(case, DEV, fn=lambda q, k, v, attn_mask=None, is_causal=False, scale=None, **_: reference(q, k, v, mask=attn_mask, causal=is_causal, scale=scale))
    # (the math path returns its value in the dtype of q's CONTAINER — int8 for int8 q codes, as the reference does; the kernels return the data dtype)
    assert got.dtype == case["q"].dtype and got.shape == case["out"].shape and want.dtype == case["out"].dtype
    meets_the_contract(got, want, ref, name)
