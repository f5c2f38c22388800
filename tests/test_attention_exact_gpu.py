"""The two attention kernels on the MI355X against answers known by construction (tests/attention_exact.py): ``attention_fwd_kernel``
behind ``ops.attention`` and the SDPA kernel behind ``ff.nn.functional.scaled_dot_product_attention``. The expectations and bounds
are the module's (derived there, proven on the CPU by tests/test_attention_exact_cpu.py); a failure names the first failing (batch,
head, row) and, for a one-hot pattern, the V row the kernel actually returned — a leak from above reads "key t + 1", a wrong kv head
or batch reads as such."""

import pytest
import torch

import attention_exact as ax
import fastforward_amd as ff

from conftest import use_backend
from fastforward_amd import ops

pytestmark = pytest.mark.gpu
F = ff.nn.functional
DEV = "cuda"


def check(p, got, expected=None, bound=None):
    text = ax.explain(p, got, expected, bound)
    assert text is None, text


# ---- ops.attention -------------------------------------------------------------------------------------------------------------------
def attention(p, **kw):
    q = p.q if p.q_in is None else p.q_in
    rope = None if p.rope is None else tuple(t.to(DEV) for t in p.rope)
    return ops.attention(ax.bsd(q).to(DEV), ax.bsd(p.k).to(DEV), ax.bsd(p.v).to(DEV), 128, causal=p.causal, q_rope=rope, softmax_scale=p.scale, **kw)


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("B,S,H,HKV", ax.ATTENTION_SHAPES)
def test_attention_returns_the_known_rows(B, S, H, HKV, causal):
    for p in ax.attention_patterns(B, S, H, HKV, causal):
        ctx, codes = attention(p)
        assert codes is None and ctx.dtype == torch.bfloat16 and tuple(ctx.shape) == (B, S, H * 128)
        check(p, ax.heads(ctx, 128))


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("B,S,H,HKV", ax.ROTATED_SHAPES)
def test_attention_rotates_each_query_row_by_its_own_table_row(B, S, H, HKV, causal):
    for p in ax.rotated_patterns(B, S, H, HKV, causal):
        ctx, _ = attention(p)
        check(p, ax.heads(ctx, 128))


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
def test_attention_applies_the_softmax_scale_once(causal):
    """Staircases whose step is wide enough only under the scale handed in: one breaks when it is applied twice, one when ignored."""
    for p in ax.scaled_patterns(ax.llama(*ax.SCALED_ATTENTION_SHAPE), torch.bfloat16, causal):
        ctx, _ = attention(p)
        check(p, ax.heads(ctx, 128))


@pytest.mark.parametrize("B,S,H,HKV", ax.QUANTIZED_SHAPES)
def test_attention_with_the_fused_quantizer(oracle_lib, B, S, H, HKV):
    """The context meets the bound whatever else the launch writes; the codes are the oracle's A1 of the context the launch returned
    (computed on the CPU); context only, codes only and both agree bit for bit."""
    scale, offset = torch.tensor([2.0**-3]), torch.tensor([3.0])  # |V| runs to 2^8: a part of the codes clamps
    quantizer = (scale.to(DEV), offset.to(DEV))
    for p in ax.attention_patterns(B, S, H, HKV, True)[:3]:
        ctx, codes = attention(p, quantizer=quantizer)
        check(p, ax.heads(ctx, 128))
        with use_backend(oracle_lib):
            want = ops.quantize_by_tile(ctx.cpu(), scale, ctx.shape, 8, torch.int8, offset)
        assert codes.dtype == torch.int8 and torch.equal(codes.cpu(), want), ax.first_mismatch(codes.cpu(), want)
        # both edges of the code range and its inside occur
        assert p.kind == "uniform" or (int(want.min()) == -128 and int(want.max()) == 127 and bool((want.int().abs() < 100).any()))
        only_ctx, none = attention(p)
        assert none is None and torch.equal(only_ctx, ctx)
        none, only_codes = attention(p, quantizer=quantizer, want_context=False)
        assert none is None and torch.equal(only_codes, codes)


# ---- scaled_dot_product_attention ------------------------------------------------------------------------------------------------------
@pytest.fixture
def launches(monkeypatch):
    count = [0]
    real = ops.sdpa_quantize

    def counting(*args, **kwargs):
        count[0] += 1
        return real(*args, **kwargs)

    monkeypatch.setattr(ops, "sdpa_quantize", counting)
    return count


def weights_quantizer():
    bits, scale, offset = ax.WEIGHTS_QUANTIZER
    q = ff.nn.LinearQuantizer(bits, symmetric=False, granularity=ff.PerTensor(), device=DEV)
    q.quantization_range = (torch.tensor(-1.0, device=DEV), torch.tensor(1.0, device=DEV))
    with torch.no_grad():
        q.scale.fill_(scale)
        q.offset.fill_(offset)
    return q


def sdpa(launches, p, q, k, v, quantized):
    """One call of the functional on the device; a call that does not reach the kernel fails."""
    kw = dict(attn_weights_quantizer=weights_quantizer()) if quantized else {}
    mask = None if p.mask is None else p.mask.to(DEV)
    before = launches[0]
    with torch.no_grad():
        got = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, is_causal=p.causal, scale=p.scale, enable_gqa=True, strict_quantization=False, **kw)
    assert launches[0] == before + 1, f"{p}: the fused kernel did not run"
    assert got.dtype == p.dtype and tuple(got.shape) == tuple(p.expected.shape)
    return got


def both_modes(launches, p, q, k, v):
    check(p, sdpa(launches, p, q, k, v, False))  # MODE 0: the online softmax
    check(p, sdpa(launches, p, q, k, v, True), *ax.weights_quantized(p))  # MODE 1: two passes, the weights codes


@pytest.mark.parametrize("kind", ax.SDPA_KINDS)
@pytest.mark.parametrize("L,S", ax.SDPA_LS)
def test_sdpa_returns_the_known_rows(launches, L, S, kind):
    for dtype in ax.SDPA_DTYPES:
        for p in ax.sdpa_patterns(L, S, kind, dtype):
            both_modes(launches, p, p.q.to(DEV), p.k.to(DEV), p.v.to(DEV))


@pytest.mark.parametrize("lead", ax.MASK_LEADS)
def test_sdpa_float_masks_broadcast_over_their_leading_dims(launches, lead):
    """Every leading shape of the mask, in both dtypes and on both head sizes, with the mask in the operands' dtype and in fp32."""
    for dtype, E, mask_dtype in ((torch.bfloat16, 128, None), (torch.float16, 64, torch.float32), (torch.float16, 128, None)):
        p = ax.mask_select(ax.Shape(2, 4, 2, 65, 129, E), dtype, lead, mask_dtype=mask_dtype)
        both_modes(launches, p, p.q.to(DEV), p.k.to(DEV), p.v.to(DEV))
        u = ax.masked_uniform(ax.Shape(2, 4, 2, 65, 129, E), dtype, 1, lead)
        both_modes(launches, u, u.q.to(DEV), u.k.to(DEV), u.v.to(DEV))


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("dtype", ax.SDPA_DTYPES)
def test_sdpa_applies_the_scale_once(launches, dtype, causal):
    """Staircases whose step is wide enough only under the `scale` handed in: one breaks when it is applied twice, one when ignored."""
    for p in ax.scaled_patterns(ax.SCALED_SDPA_SHAPE, dtype, causal):
        both_modes(launches, p, p.q.to(DEV), p.k.to(DEV), p.v.to(DEV))


@pytest.mark.parametrize("dtype", ax.SDPA_DTYPES)
def test_sdpa_on_transposed_views_of_the_projections(launches, dtype):
    """[B, S, H, E] projections seen through .transpose(1, 2): the kernel walks the strides, nothing is copied."""
    shape = ax.Shape(2, 4, 2, 130, 300, 128)
    for p in (ax.select(shape, dtype, True), ax.staircase(shape, dtype, False), ax.uniform(shape, dtype, 1, True)):
        q, k, v = (t.transpose(1, 2).contiguous().to(DEV).transpose(1, 2) for t in (p.q, p.k, p.v))
        assert not q.is_contiguous() and q.shape == p.q.shape
        both_modes(launches, p, q, k, v)
