"""The split-key decode kernels (csrc/ffq_sdpa_decode.hip) on the drawn cases of tests/decode_cases.py: answers known by construction in
every case's layout, container, mask form and split count; relations between two runs of the same kernel that must hold bit for bit
(docs/numerics.md, "Relations between two runs", has the reason for each); the attention contract on the same random operands; and a
cache growing across the 128- and 256-key edges. Every test counts the calls of ``ops.sdpa_decode`` and ``ops.sdpa_quantize``: nothing
falls back."""

import contextlib
import functools

import pytest
import torch

import fastforward_amd as ff

import attention_exact as ax
import decode_cases as dc

from fastforward_amd import ops
from test_sdpa_decode_cpu import as_codes, linear_quantizer
from test_sdpa_decode_gpu import launches, math_path, meets_the_contract, reference, served  # noqa: F401  (launches: the fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = dc.drawn()
EVERY = pytest.mark.parametrize("index", range(len(CASES)), ids=[f"{c.index:02d}" for c in CASES])


@functools.lru_cache(maxsize=None)
def _parameter(value):
    return torch.tensor([value], dtype=torch.float32, device=DEV)


def device_run(case):
    """``run`` of tests/decode_cases.py on the kernels, through ``ops.sdpa_decode``."""
    def run(q, k, v, *, mask=None, causal=False, splits=0, scale=None):
        dequant = tuple(None if c.scale is None else (_parameter(c.scale), None if c.offset is None else _parameter(c.offset)) for c in (q, k, v))
        return ops.sdpa_decode(q.raw, k.raw, v.raw, attn_mask=mask, is_causal=causal, scale=scale, dequant=dequant, dtype=case.dtype, splits=splits)

    return run


def quantized(c, dtype):
    return c.raw if c.scale is None else as_codes(c.raw, c.scale, c.offset, dtype, DEV)


def counted(launches, decode):
    assert launches == {"decode": decode, "quantize": 0}, launches


@contextlib.contextmanager
def named(case):
    """A failure names its case in full (the test ids carry the index alone)."""
    try:
        yield
    except AssertionError as failure:
        raise AssertionError(f"{case.id}: {failure}") from failure


# ---- a. known answers ---------------------------------------------------------------------------------------------------------------------------
def known_answers(launches, index):
    """a. The case's patterns in its layout, container, mask form and split count, through ``ops.sdpa_decode`` and, at the rule's split,
    through ``ff.nn.functional`` too."""
    case, run, calls = CASES[index], device_run(CASES[index]), 0
    with named(case):
        for known in dc.known(index):
            p = known.pattern
            q, k, v = dc.laid_out(case.layout, *(c.to(DEV) for c in known[1:]))
            mask = None if p.mask is None else dc.in_form(case, case.mask_form, p.mask.to(DEV))
            got = run(q, k, v, mask=mask, causal=p.causal, splits=case.splits, scale=p.scale)
            assert (why := ax.explain(p, got)) is None, why
            calls += 1
            if case.splits == 0:
                first = served(launches, *(quantized(c, case.dtype) for c in (q, k, v)), attn_mask=mask, is_causal=p.causal, scale=p.scale, enable_gqa=True)
                assert (why := ax.explain(p, first)) is None, why
                dc.same(first, got, "the call through ff.nn.functional against ops.sdpa_decode")
                calls += 1
        counted(launches, calls)


# ---- b. relations, bit for bit ----------------------------------------------------------------------------------------------------------------------
def relations(launches, index):
    """b. Every relation of tests/decode_cases.py on the case's random operands: a second launch; a row, a kv head and a batch alone;
    ``is_causal`` against the explicit trils; every mask form against the materialised mask; q in either container and plain; codes
    traded against the offset; every layout against its cloned contiguous operands."""
    case, run = CASES[index], device_run(CASES[index])
    with named(case):
        call = dc.call_of(case, DEV)
        full = call.full(run)
        dc.same(call.full(run), full, "two launches of the same call")
        b, head, _ = case.picks[0]
        calls = 2 + dc.row_alone(run, call, full)
        dc.kv_head_alone(run, call, full, head // case.G)
        dc.batch_alone(run, call, full, b)
        counted(launches, calls + 2)
        calls += 2 + dc.causal_is_tril(run, call)
        kind = case.mask if case.mask in dc.EXPLICIT else dc.EXPLICIT[index % 3]
        calls += dc.mask_forms(run, call, kind)
        counted(launches, calls)
        codes = dc.random_operands(case, q_container="int8")[0].to(DEV)
        assert torch.equal(dc.values(codes, case.dtype), quantized(codes, case.dtype).dequantize())  # (the plain tensor is q.dequantize())
        calls += dc.containers(run, call)
        trade = dc.call_of(dc.dataclasses.replace(case, q_container="int8"), DEV, trade=True)
        offsets = tuple(dc.TRADE_OFFSETS[(index + i) % 4] for i in range(3))
        calls += dc.code_offset_trade(run, trade, dc.TRADE_SHIFTS[index % 3], offsets)
        calls += dc.layouts_agree(run, call, full)
        counted(launches, calls)


# ---- c. the contract ------------------------------------------------------------------------------------------------------------------------------------
def held_to_the_contract(case, got, q, k, v, mask, causal, what=""):
    """`meets_the_contract` of tests/test_sdpa_decode_gpu.py. The math path gets int8 q codes in the data dtype's container (the same
    values): on an int8 container it returns truncated int8 values, which would make its own error, and so the allowance, meaningless."""
    if q.raw.dtype == torch.int8:
        q = dc.Coded(q.raw.to(case.dtype), q.scale, q.offset)
    operands = [quantized(c, case.dtype) for c in (q, k, v)]
    want = math_path(*operands, attn_mask=mask, is_causal=causal, enable_gqa=True)
    assert want.dtype == got.dtype
    meets_the_contract(got, want, reference(*operands, mask=mask, causal=causal), what)


def contract(launches, index):
    """c. The case's random operands against the float64 attention of the dequantized operands."""
    case = CASES[index]
    call = dc.call_of(case, DEV)
    got = call.full(device_run(case))
    counted(launches, 1)
    held_to_the_contract(case, got, call.q, call.k, call.v, call.mask, call.causal, case.id)
    counted(launches, 1)


@EVERY
def test_case(launches, index):
    """One drawn case: its known answers, every relation, the contract, each with its own count of launches from zero."""
    for part in (known_answers, relations, contract):
        launches.update(decode=0, quantize=0)
        part(launches, index)


# ---- d. a cache crossing tile edges --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", dc.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("start", [124, 252])
def test_cache_across_a_tile_edge(launches, start, dtype):
    """The decode loop from S = start + 1 to start + 7 (125..131: the workgroup step; 253..259: the shortest split), code-level cat,
    one launch per step; every step inside the contract and bit-equal to the call on a freshly built contiguous cache of the same codes."""
    B, HKV, G, E = 3, 3, 5, 128
    gen = ax.generator("decode_cases_cache", start, str(dtype))
    k_spec, v_spec = (8, 0.031, 3.0), (8, 0.027, -9.0)
    kq, vq = linear_quantizer(k_spec, DEV, torch.int8), linear_quantizer(v_spec, DEV, torch.int8)
    with torch.no_grad():
        K = kq(torch.randn(B, HKV, start, E, generator=gen).to(dtype).to(DEV))
        V = vq(torch.randn(B, HKV, start, E, generator=gen).to(dtype).to(DEV))
    chunks = [[K.raw_data.clone()], [V.raw_data.clone()]]
    case = dc.Case(-1, 1, G, B, HKV, start, E, dtype, "none", None, "plain", 0, "contiguous", 0, ())
    for step in range(7):
        with torch.no_grad():
            k_new, v_new = (quant(torch.randn(B, HKV, 1, E, generator=gen).to(dtype).to(DEV)) for quant in (kq, vq))
            K, V = torch.cat([K, k_new], dim=2), torch.cat([V, v_new], dim=2)
        chunks[0].append(k_new.raw_data.clone())
        chunks[1].append(v_new.raw_data.clone())
        S = start + 1 + step
        assert isinstance(K, ff.QuantizedTensor) and K.raw_data.dtype == torch.int8 and K.shape[2] == V.shape[2] == S
        q_t = torch.randn(B, HKV * G, 1, E, generator=gen).to(dtype).to(DEV)
        got = served(launches, q_t, K, V, enable_gqa=True)
        fresh = [torch.cat(c, dim=2).contiguous() for c in chunks]
        assert torch.equal(fresh[0], K.raw_data) and torch.equal(fresh[1], V.raw_data)
        again = served(launches, q_t, as_codes(fresh[0], *k_spec[1:], dtype, DEV), as_codes(fresh[1], *v_spec[1:], dtype, DEV), enable_gqa=True)
        dc.same(got, again, f"S = {S}: the appended cache against a freshly built one")
        held_to_the_contract(case, got, dc.Coded(q_t), dc.Coded(K.raw_data, *k_spec[1:]), dc.Coded(V.raw_data, *v_spec[1:]), None, False, f"S = {S}")
    counted(launches, 14)
