"""ff.nn.functional.scaled_dot_product_attention on the MI355X: the one-launch kernel (csrc/ffq_sdpa.hip) against the device math
path (nn/sdpa.py's scaled_dot_product_attention_math, which is what the call runs with this registration taken out). Every case counts
the calls of ``ops.sdpa_quantize`` so that a silent fallback fails."""

import math

import pytest
import torch

import fastforward_amd as ff

from fastforward_amd import fused_sdpa, ops
from fastforward_amd.exceptions import QuantizationError
from fastforward_amd.nn.sdpa import QUANTIZER_NAMES, scaled_dot_product_attention_math

pytestmark = pytest.mark.gpu
F = ff.nn.functional
DEV = "cuda"


@pytest.fixture
def launches(monkeypatch):
    count = [0]
    real = ops.sdpa_quantize

    def counting(*args, **kwargs):
        count[0] += 1
        return real(*args, **kwargs)

    monkeypatch.setattr(ops, "sdpa_quantize", counting)
    return count


def quantizer(bits=8, scale=2.0**-4, offset=0.0):
    """A per-tensor LinearQuantizer with the given (power-of-two) scale and offset."""
    q = ff.nn.LinearQuantizer(bits, symmetric=False, granularity=ff.PerTensor(), device=DEV)
    q.quantization_range = (torch.tensor(-1.0, device=DEV), torch.tensor(1.0, device=DEV))
    with torch.no_grad():
        q.scale.fill_(scale)
        q.offset.fill_(offset)
    return q


def eight(weights_bits=8):
    """All eight quantizers, scales chosen for the operands of `exact_operands`: q / k codes hit the sums exactly, the probability
    quantizers cover [0, 1) (A2 = (code + 2^(bits-1)) * 2^-bits), the output covers |v|."""
    return dict(
        scaled_query_quantizer=quantizer(8, 2.0**-4),
        scaled_key_quantizer=quantizer(8, 2.0**-4),
        attn_scores_quantizer=quantizer(8, 2.0**-2),
        attn_mask_quantizer=quantizer(8, 2.0**-2),
        masked_scores_quantizer=quantizer(8, 2.0**-2),
        attn_weights_quantizer=quantizer(weights_bits, 2.0**-weights_bits, 2.0 ** (weights_bits - 1)),
        dropout_quantizer=quantizer(8, 2.0**-8, 128.0),
        output_quantizer=quantizer(8, 2.0**-5),
    )


def exact_operands(B, H, HKV, L, S, E, dtype=torch.bfloat16, gen=None):
    """Small integers times powers of two: every product and partial sum of the scores is exact in fp32 (order-free)."""
    gen = gen or torch.Generator().manual_seed(0)
    q = (torch.randint(-8, 9, (B, H, L, E), generator=gen) * 2.0**-3).to(dtype)
    k = (torch.randint(-8, 9, (B, HKV, S, E), generator=gen) * 2.0**-3).to(dtype)
    v = (torch.randint(-16, 17, (B, HKV, S, E), generator=gen) * 2.0**-4).to(dtype)
    return q.to(DEV), k.to(DEV), v.to(DEV)


def both(launches, q, k, v, **kw):
    kw.setdefault("strict_quantization", False)
    before = launches[0]
    with torch.no_grad():
        got = F.scaled_dot_product_attention(q, k, v, **kw)
        assert launches[0] == before + 1, "the fused kernel did not run"
        want = scaled_dot_product_attention_math(q, k, v, **kw)
    return got, want


def reference64(q, k, v, mask=None, causal=False, scale=None, gqa=False):
    q, k, v = q.double().cpu(), k.double().cpu(), v.double().cpu()
    if gqa:
        k = k.repeat_interleave(q.shape[1] // k.shape[1], 1)
        v = v.repeat_interleave(q.shape[1] // v.shape[1], 1)
    L, S, E = q.shape[-2], k.shape[-2], q.shape[-1]
    s = q @ k.transpose(-1, -2) * (1 / math.sqrt(E) if scale is None else scale)
    if causal:
        s = s.masked_fill(~torch.ones(L, S, dtype=torch.bool).tril(), -math.inf)
    if mask is not None:
        s = s.masked_fill(~mask.cpu(), -math.inf) if mask.dtype == torch.bool else s + mask.cpu().double()
    p = torch.softmax(s, -1).nan_to_num(0.0)
    return p @ v


@pytest.mark.parametrize("L,S", [(1, 1), (17, 17), (100, 17), (17, 100), (1000, 1000), (2048, 2048), (100, 1000)])
@pytest.mark.parametrize("E", [64, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("causal", [False, True])
def test_unquantized_probabilities_meet_the_attention_contract(launches, L, S, E, dtype, causal):
    """parity_cases.check_attention's contract: the error against float64 is no larger than the math path's own plus 2^-9."""
    if (L, S) == (2048, 2048) and E == 64 and dtype == torch.float16:
        pytest.skip("covered by the bf16 / E = 128 cases at this size")
    gen = torch.Generator().manual_seed(L * 7 + S)
    q, k, v = (torch.randn(2, 4, n, E, generator=gen).to(dtype).to(DEV) for n in (L, S, S))
    got, want = both(launches, q, k, v, is_causal=causal)
    assert got.dtype == dtype and got.shape == (2, 4, L, E)
    ref = reference64(q, k, v, causal=causal)
    err_got = float((got.cpu().double() - ref).abs().max())
    err_math = float((want.cpu().double() - ref).abs().max())
    assert err_got <= err_math + 2.0**-9, f"{err_got:.3e} from float64, math path {err_math:.3e}"


@pytest.mark.parametrize("L,S,causal", [(17, 17, False), (100, 1000, False), (1000, 100, True), (2048, 2048, True), (1, 17, True)])
@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_quantized_probabilities_differ_only_by_flipped_codes(launches, L, S, causal, bits, dtype):
    """Exact-sum operands: the score codes do not depend on the summation order, so the fused call and the chain agree on every
    masked score; p = exp(x - m) / l may differ by an ulp (summation order of l), which moves a weights code by one step
    s_w = 2^-bits on the rare element that sits at a rounding boundary. One flipped code moves an output by s_w * |v| <= s_w * max|V|;
    allowing two flips in one row bounds the deviation by 2 * s_w * max|V|. A flip changes one row's E outputs, and flips are
    rare: at most 2 % of the elements may differ."""
    q, k, v = exact_operands(1, 4, 4, L, S, 128, dtype)
    qz = dict(attn_weights_quantizer=quantizer(bits, 2.0**-bits, 2.0 ** (bits - 1)), scaled_query_quantizer=quantizer(8, 2.0**-4),
              scaled_key_quantizer=quantizer(8, 2.0**-4))
    got, want = both(launches, q, k, v, is_causal=causal, **qz)
    diff = (got.float() - want.float()).abs()
    bound = 2 * 2.0**-bits * float(v.float().abs().max())
    assert float(diff.max()) <= bound, f"{float(diff.max()):.3e} > {bound:.3e}"
    assert float((diff > 0).float().mean()) <= 0.02


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_all_eight_quantizers_and_fused_output_codes(launches, dtype):
    """With the output quantizer the call returns A2 of its codes in the query dtype: equal to the chain's wherever the chain's
    probabilities agree, and the codes (ops level) are exactly those behind the returned value."""
    q, k, v = exact_operands(2, 4, 2, 100, 300, 64, dtype)
    qz = eight()
    got, want = both(launches, q, k, v, is_causal=True, enable_gqa=True, **qz)
    step = float(qz["output_quantizer"].scale.detach())
    diff = (got.float() - want.float()).abs()
    assert float((diff > 0).float().mean()) <= 0.02 and float(diff.max()) <= 2 * 2.0**-8 * float(v.float().abs().max()) + step
    params = {n: (qz[n].scale, qz[n].offset, 8) for n in QUANTIZER_NAMES}
    value, codes = ops.sdpa_quantize(q, k, v, is_causal=True, quantizers=params, want_codes=True)
    assert torch.equal(value, got)
    deq = ((codes.float() + qz["output_quantizer"].offset.round()) * qz["output_quantizer"].scale).to(value.dtype)
    assert torch.equal(deq, value)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_query_and_key_offsets_beyond_the_exact_integers(launches, dtype):
    """Scaled-q / scaled-k quantizers whose range excludes 0: code + round(offset) runs to 327 (key) and -278 (query), beyond the 256
    integers bf16 holds exactly. The kernel contracts the codes and adds the offsets through row / key sums, so the scores stay the
    chain's (every term an integer times 2^-20, below 2^24 units: exact on both sides), and the result differs from the chain only by
    flipped weights codes: the bound of test_quantized_probabilities_differ_only_by_flipped_codes, 2 * s_w * max|V|."""
    q, k, v = exact_operands(1, 4, 2, 300, 200, 128, dtype)
    qz = dict(scaled_query_quantizer=quantizer(8, 2.0**-10, -150.0), scaled_key_quantizer=quantizer(8, 2.0**-10, 200.0),
              attn_weights_quantizer=quantizer(8, 2.0**-8, 128.0))
    got, want = both(launches, q, k, v, is_causal=True, enable_gqa=True, **qz)
    diff = (got.float() - want.float()).abs()
    assert float(diff.max()) <= 2 * 2.0**-8 * float(v.float().abs().max()) and float((diff > 0).float().mean()) <= 0.02


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("scale,offset,L,S", [(2.0**-9, 300.0, 100, 300), (2.0**-16, 40000.0, 8, 8), (2.0**-17, 100000.0, 8, 8),
                                              (2.0**-23, 5.0e6, 8, 8)])
def test_probability_offsets_beyond_the_exact_integers(launches, dtype, scale, offset, L, S):
    """A weights quantizer whose range excludes 0 (a calibration on rows without small probabilities): the integers code + offset
    reach 427, 40127, 100127 and 5000127 — beyond what bf16 (256) and fp16 (2048) hold, the fp16 ones beyond its largest finite
    value. The kernel feeds them to the MFMA in up to three exact parts. The chain's P V sums p_hat * v in fp32, which is exact in
    the first case (multiples of 2^-13 below 2^24 units) and rounds in the others by at most S * 2^-24 * sum|p_hat * v|
    <= S^2 * 2^-24 * max|V| (p_hat <= 1), and values that differ at all can round to neighbouring outputs in the query dtype (one ulp
    of max|out|: 2^-8 relative in bf16, 2^-11 in fp16); on top of that a flipped weights code moves an output by s_w * max|V| (two
    per row)."""
    q, k, v = exact_operands(1, 2, 2, L, S, 128, dtype)
    qz = dict(attn_weights_quantizer=quantizer(8, scale, offset), scaled_query_quantizer=quantizer(8, 2.0**-4),
              scaled_key_quantizer=quantizer(8, 2.0**-4))
    got, want = both(launches, q, k, v, **qz)
    vmax = float(v.float().abs().max())
    ulp = float(want.float().abs().max()) * (2.0**-8 if dtype == torch.bfloat16 else 2.0**-11)
    bound = 2 * scale * vmax + (0.0 if offset < 1000 else S * S * 2.0**-24 * vmax + ulp)
    diff = (got.float() - want.float()).abs()
    assert float(diff.max()) <= bound, f"{float(diff.max()):.3e} > {bound:.3e}"
    assert float((diff > 0).float().mean()) <= (0.02 if offset < 1000 else 1.0)


@pytest.mark.parametrize("quantized", [False, True])
def test_fully_masked_rows_are_exact_zeros(launches, quantized):
    q, k, v = exact_operands(1, 2, 2, 40, 70, 128)
    mask = torch.rand(40, 70, generator=torch.Generator().manual_seed(3)) > 0.3
    mask[5] = False
    mask[39] = False
    mask = mask.to(DEV)
    qz = dict(attn_weights_quantizer=quantizer(8, 2.0**-8, 128.0)) if quantized else {}
    got, want = both(launches, q, k, v, attn_mask=mask, **qz)
    assert torch.equal(got[:, :, 5], torch.zeros_like(got[:, :, 5])) and torch.equal(got[:, :, 39], torch.zeros_like(got[:, :, 39]))
    assert torch.equal(want[:, :, 5], got[:, :, 5])
    if not quantized:
        ref = reference64(q, k, v, mask=mask)
        assert float((got.cpu().double() - ref).abs().max()) <= float((want.cpu().double() - ref).abs().max()) + 2.0**-9


@pytest.mark.parametrize("mask_shape", [(1000, 1000), (1, 4, 1000, 1000), (2, 1, 1000, 1000)])
@pytest.mark.parametrize("kind", ["bool", "float"])
def test_broadcast_masks_and_gqa_on_strided_projections(launches, mask_shape, kind):
    """[B, S, H, D] projections seen through .transpose(1, 2): not copied; masks broadcast over their leading dims; 4 query heads on
    2 kv heads."""
    gen = torch.Generator().manual_seed(11)
    B, L, S, E = 2, 1000, 1000, 128
    qp = torch.randn(B, L, 4, E, generator=gen).bfloat16().to(DEV)
    kp = torch.randn(B, S, 2, E, generator=gen).bfloat16().to(DEV)
    vp = torch.randn(B, S, 2, E, generator=gen).bfloat16().to(DEV)
    q, k, v = qp.transpose(1, 2), kp.transpose(1, 2), vp.transpose(1, 2)
    m = torch.rand(mask_shape, generator=gen)
    mask = (m > 0.2) if kind == "bool" else (m * 4 - 2)
    mask = mask.to(DEV)
    got, want = both(launches, q, k, v, attn_mask=mask, enable_gqa=True, scale=0.1)
    ref = reference64(q, k, v, mask=mask.expand(B, 4, L, S), scale=0.1, gqa=True)
    assert float((got.cpu().double() - ref).abs().max()) <= float((want.cpu().double() - ref).abs().max()) + 2.0**-9


def test_quantized_operands_and_a_finite_neg_inf(launches):
    """q / k / v as per-tensor codes in bf16 (what q/k/v_proj output quantizers produce), dequantized in registers."""
    q, k, v = exact_operands(1, 2, 2, 64, 64, 128)
    qq, kq, vq = (quantizer(8, 2.0**-3)(t) for t in (q, k, v))
    qz = dict(attn_weights_quantizer=quantizer(8, 2.0**-8, 128.0), attn_mask_quantizer=quantizer(8, 2.0**-2))
    got, want = both(launches, qq, kq, vq, is_causal=True, neg_inf=-30.0, **qz)
    diff = (got.float() - want.float()).abs()
    assert float((diff > 0).float().mean()) <= 0.02 and float(diff.max()) <= 2 * 2.0**-8 * float(v.float().abs().max())


def _declined(launches, q, k, v, **kw):
    kw.setdefault("strict_quantization", False)
    before = launches[0]
    torch.manual_seed(5)
    got = F.scaled_dot_product_attention(q, k, v, **kw)
    assert launches[0] == before, "declined call reached the kernel"
    torch.manual_seed(5)
    want = scaled_dot_product_attention_math(q, k, v, **kw)
    assert torch.equal(got, want)


def test_declines_reach_the_math_path(launches):
    q, k, v = exact_operands(1, 2, 2, 33, 40, 128)
    with torch.no_grad():
        _declined(launches, q, k, v, dropout_p=0.3)
        pc = ff.nn.LinearQuantizer(8, granularity=ff.PerChannel(0), device=DEV)
        pc.quantization_range = (torch.full((1,), -1.0, device=DEV), torch.full((1,), 1.0, device=DEV))
        _declined(launches, q, k, v, attn_weights_quantizer=pc)
        q96, k96, v96 = exact_operands(1, 2, 2, 33, 40, 96)
        _declined(launches, q96, k96, v96)
        _declined(launches, q.float(), k.float(), v.float())
        with ff.sdpa_upcast(False):
            _declined(launches, q, k, v)
        _declined(launches, q, k[:, :1], v[:, :1])  # different head counts without enable_gqa
    w = quantizer(8, 2.0**-8, 128.0)
    with ff.estimate_ranges(w, ff.range_setting.running_minmax), torch.no_grad():
        _declined(launches, q, k, v, attn_weights_quantizer=w)
    # grad mode with an operand that needs a gradient: declined; the math path then fails in the safe softmax's where(out=...)
    # exactly as the reference's does
    qg = q.clone().requires_grad_(True)
    before = launches[0]
    assert not fused_sdpa.sdpa_predicate(query=qg, key=k, value=v, strict_quantization=False)
    with pytest.raises(RuntimeError, match="out=... arguments don't support automatic differentiation"):
        F.scaled_dot_product_attention(qg, k, v, strict_quantization=False)
    assert launches[0] == before


def test_strict_calls_follow_the_math_path(launches):
    """After the fp32 upcast a strict call on codes held in bf16 raises as the reference does; the kernel is never asked."""
    q, k, v = exact_operands(1, 2, 2, 16, 16, 128)
    qq, kq, vq = (quantizer(8, 2.0**-3)(t) for t in (q, k, v))
    with torch.no_grad(), pytest.raises(QuantizationError):
        F.scaled_dot_product_attention(qq, kq, vq, strict_quantization=True, **eight())
    assert launches[0] == 0


def test_graph_capture_replays_the_eager_result(launches):
    q, k, v = exact_operands(1, 4, 4, 256, 256, 128)
    qz = eight()
    with torch.no_grad():
        eager = F.scaled_dot_product_attention(q, k, v, is_causal=True, strict_quantization=False, **qz)
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            F.scaled_dot_product_attention(q, k, v, is_causal=True, strict_quantization=False, **qz)
        torch.cuda.current_stream().wait_stream(stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            captured = F.scaled_dot_product_attention(q, k, v, is_causal=True, strict_quantization=False, **qz)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(captured, eager)


def test_full_size_causal_with_all_eight_quantizers(launches):
    """B = 2, H = 32 on 8 kv heads, L = S = 2048, D = 128, causal, all eight quantizers: the chain on a sampled set of rows."""
    q, k, v = exact_operands(2, 32, 8, 2048, 2048, 128)
    qz = eight()
    before = launches[0]
    with torch.no_grad():
        got = F.scaled_dot_product_attention(q, k, v, is_causal=True, enable_gqa=True, strict_quantization=False, **qz)
    assert launches[0] == before + 1
    rows = torch.tensor([0, 1, 63, 64, 127, 128, 1000, 2047], device=DEV)
    for b, h in ((0, 0), (1, 31), (0, 17)):
        kv = h // 4
        with torch.no_grad():
            # causal rows see keys 0..row: the chain on those rows alone is the same computation (top-left tril per row)
            for r in rows.tolist():
                want = scaled_dot_product_attention_math(q[b:b + 1, h:h + 1, r:r + 1], k[b:b + 1, kv:kv + 1, :r + 1], v[b:b + 1, kv:kv + 1, :r + 1],
                                                         strict_quantization=False, **qz)
                diff = (got[b, h, r].float() - want[0, 0, 0].float()).abs()
                step = float(qz["output_quantizer"].scale.detach())
                assert float(diff.max()) <= 2 * 2.0**-8 * float(v.float().abs().max()) + step, (b, h, r)
