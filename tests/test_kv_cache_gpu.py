"""The preallocated int8 KV cache on the MI355X (csrc/ffq_kv_cache.hip, ffq_kv_decode in csrc/ffq_sdpa_decode.hip, ops/kv_cache.py,
nn/kv_cache.py).

Append: the cache starts as a sentinel pattern inside a guarded arena; after ONE launch exactly the rows ``lens[b] - L .. lens[b] - 1``
inside ``[0, S_max)`` hold ``ops.quantize_by_tile`` of the new rows (of ``ops.rope_`` of them, with tables), every other byte is
the sentinel and no guard byte moved. Decode: every batch row is bit-equal to ``ops.sdpa_decode`` on that row's own slice at the
same forced split count; operands whose answer is known by construction (tests/attention_exact.py), cut to every sequence's length,
give that answer exactly; random operands sit inside the attention contract of tests/test_sdpa_decode_gpu.py. The class: a ragged
decode loop, eager and replayed from one captured graph while the lengths move. Every test counts the calls of the C entry points
(one ``ffq_kv_append`` is one launch, one ``ffq_kv_decode`` the partial + combine pair): a silent fallback fails."""

import pytest
import torch

import fastforward_amd as ff

import guards
import kv_cache_cases as cases

from fastforward_amd import _native, ops
from kv_cache_cases import B, HKV, S_MAX
from test_sdpa_decode_gpu import math_path, meets_the_contract, reference

pytestmark = pytest.mark.gpu
F = ff.nn.functional
DEV = "cuda"
NAMES = ("ffq_kv_append", "ffq_kv_decode", "ffq_sdpa_decode")


@pytest.fixture
def entries(monkeypatch):
    """Calls of the three C entry points, counted on the loaded library itself."""
    lib = _native.library()
    count = dict.fromkeys(NAMES, 0)
    for name in NAMES:
        def counting(*args, _real=getattr(lib, name), _name=name):
            count[_name] += 1
            return _real(*args)
        monkeypatch.setattr(lib, name, counting)
    return count


def lens_tensor(lens):
    return torch.tensor(lens, dtype=torch.int32, device=DEV)


def scalars(scale, offset):
    return torch.tensor([scale], device=DEV), None if offset is None else torch.tensor([offset], device=DEV)


# ---- append ---------------------------------------------------------------------------------------------------------------------------
def new_rows(L, E, dtype, view, gen):
    """k_new / v_new [B, HKV, L, E] as `view` lays them out, with values on both clamps, on exact ties and not numbers at all."""
    def draw(centre, spread):
        x = torch.randn(B, HKV, L, E, generator=gen) * spread + centre
        x[0, 0, 0, :8] = torch.tensor([1e4, -1e4, float("inf"), -float("inf"), float("nan"), 0.0, -0.0, centre])
        x[-1, -1, -1, :4] = torch.tensor([0.5, 1.5, 2.5, -0.5]) * spread  # (ties of a power-of-two scale; plain values of the others)
        return x.to(dtype).to(DEV)

    k, v = draw(-9.3, 2.0), draw(40.0, 0.5)
    if view == "projection":    # the projection's [B, L, HKV * E] output seen as [B, L, HKV, E].transpose(1, 2)
        k, v = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (k, v))
        assert L == 1 or not k.is_contiguous()
    elif view == "strided":     # a window of a wider buffer: rows 16 bytes further apart, a pointer off the allocation's start
        wide = [torch.zeros(B, HKV, L + 2, E + 8, dtype=dtype, device=DEV) for _ in range(2)]
        k, v = (w[:, :, 1:L + 1, 8:].copy_(t) for w, t in zip(wide, (k, v)))
        assert k.stride(2) == E + 8 and k.data_ptr() % 16 == 0
    return k, v


def sentinel_caches(arena, layout, E):
    shape = (B, HKV, S_MAX, E) if layout == "bhse" else (B, S_MAX, HKV, E)
    plain = torch.full(shape, cases.SENTINEL, dtype=torch.int8, device=DEV)
    caches = [arena.adopt(plain, f"{name} cache") for name in ("k", "v")]
    return [t if layout == "bhse" else t.transpose(1, 2) for t in caches]


def expected_cache(codes, lens, L):
    want = torch.full((B, HKV, S_MAX, codes.shape[-1]), cases.SENTINEL, dtype=torch.int8, device=DEV)
    for b, n in enumerate(lens):
        for l, pos in cases.positions(n, L):
            want[b, :, pos] = codes[b, :, l]
    return want


def check_append(entries, dtype, E, L, lens, layout, view, k_spec, v_spec, rotated=None, seed=0):
    gen = torch.Generator().manual_seed(seed + L + E)
    k_new, v_new = new_rows(L, E, dtype, view, gen)
    arena = guards.Arena(guards.POISON_A)
    kc, vc = sentinel_caches(arena, layout, E)
    rope = None
    if rotated is not None:
        rope = tuple((torch.randn(S_MAX + 5, E, generator=gen)).to(dtype).to(DEV) for _ in range(2))
    before = entries["ffq_kv_append"]
    ops.kv_append(k_new, v_new, kc, vc, lens_tensor(lens), cases.params(k_spec, DEV), cases.params(v_spec, DEV), rope=rope)
    torch.cuda.synchronize()
    assert entries["ffq_kv_append"] == before + 1
    k_rows = k_new.contiguous() if rope is None else rotated(k_new, rope, lens, L)
    (ks, ko, kb), (vs, vo, vb) = cases.params(k_spec, DEV), cases.params(v_spec, DEV)
    want_k = expected_cache(ops.quantize_by_tile(k_rows, ks, k_rows.shape, kb, torch.int8, ko), lens, L)
    want_v = expected_cache(ops.quantize_by_tile(v_new.contiguous(), vs, v_new.shape, vb, torch.int8, vo), lens, L)
    assert torch.equal(kc, want_k), f"K: {int((kc != want_k).sum())} bytes differ"
    assert torch.equal(vc, want_v), f"V: {int((vc != want_v).sum())} bytes differ"
    assert not arena.touched_guards(), arena.touched_guards()


@pytest.mark.parametrize("view", ["contiguous", "projection", "strided"])
@pytest.mark.parametrize("layout", ["bhse", "bshe"])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_append_writes_exactly_its_rows(entries, dtype, layout, view):
    """8-bit K and 4-bit V with real offsets beyond int8; L = 1, 4, 5 over both length sets (below L, on the tile edges, past S_max)."""
    for E in cases.ES:
        for L in cases.LS:
            for lens in cases.LENS_SETS:
                check_append(entries, dtype, E, L, lens, layout, view, cases.K_SPEC, cases.V_SPEC)
    assert entries["ffq_kv_append"] == 12
    # exact ties of a power-of-two scale, and a quantizer without an offset
    check_append(entries, dtype, 128, 4, (4, 130, 385, 3, 384), layout, view, (8, 2.0, None), (4, 0.5, -2.0), seed=3)


def rope_reference_bf16(k_new, rope, lens, L):
    """``ops.rope_`` on the rows, each batch with the table rows of its own positions (a dropped row takes row 0: it is not compared)."""
    out = torch.empty_like(k_new.contiguous())
    for b, n in enumerate(lens):
        at = torch.tensor([min(max(n - L + l, 0), S_MAX - 1) for l in range(L)], device=DEV)
        flat = k_new[b].transpose(0, 1).reshape(1, L, -1).contiguous()          # [1, L, HKV * E]
        ops.rope_(None, flat, rope[0][at].contiguous(), rope[1][at].contiguous(), k_new.shape[-1])
        out[b] = flat.reshape(L, HKV, -1).transpose(0, 1)
    return out


def rope_reference_fp16(k_new, rope, lens, L):
    """ATen's ``x * cos + rotate_half(x) * sin`` in fp16."""
    out = torch.empty_like(k_new.contiguous())
    half = k_new.shape[-1] // 2
    for b, n in enumerate(lens):
        at = torch.tensor([min(max(n - L + l, 0), S_MAX - 1) for l in range(L)], device=DEV)
        x, cos, sin = k_new[b], rope[0][at], rope[1][at]
        out[b] = x * cos + torch.cat((-x[..., half:], x[..., :half]), dim=-1) * sin
    return out


@pytest.mark.parametrize("layout", ["bhse", "bshe"])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_append_rotates_k_at_each_rows_own_position(entries, dtype, layout):
    rotated = rope_reference_bf16 if dtype == torch.bfloat16 else rope_reference_fp16
    for E in cases.ES:
        for L, view in ((1, "projection"), (4, "contiguous"), (5, "strided")):
            for lens in cases.LENS_SETS:
                check_append(entries, dtype, E, L, lens, layout, view, (8, 0.11, 20.5), cases.V_SPEC, rotated=rotated, seed=11)
    assert entries["ffq_kv_append"] == 12


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_a_prompt_goes_through_the_same_call(entries, dtype):
    """L = 300 in one launch at ragged targets: whole in the cache, cut at its end, cut at its start."""
    gen = torch.Generator().manual_seed(5)
    L, E, lens = 300, 128, (300, 384, 450, 120, 0)
    k_new, v_new = (torch.randn(B, HKV, L, E, generator=gen).to(dtype).to(DEV) for _ in range(2))
    rope = tuple(torch.randn(S_MAX, E, generator=gen).to(dtype).to(DEV) for _ in range(2))
    arena = guards.Arena(guards.POISON_B)
    kc, vc = sentinel_caches(arena, "bshe", E)
    ops.kv_append(k_new, v_new, kc, vc, lens_tensor(lens), cases.params(cases.K_SPEC, DEV), cases.params(cases.V_SPEC, DEV), rope=rope)
    torch.cuda.synchronize()
    assert entries["ffq_kv_append"] == 1 and [len(cases.positions(n, L)) for n in lens] == [300, 300, 234, 120, 0]
    rotated = (rope_reference_bf16 if dtype == torch.bfloat16 else rope_reference_fp16)(k_new, rope, lens, L)
    (ks, ko, kb), (vs, vo, vb) = cases.params(cases.K_SPEC, DEV), cases.params(cases.V_SPEC, DEV)
    assert torch.equal(kc, expected_cache(ops.quantize_by_tile(rotated, ks, rotated.shape, kb, torch.int8, ko), lens, L))
    assert torch.equal(vc, expected_cache(ops.quantize_by_tile(v_new, vs, v_new.shape, vb, torch.int8, vo), lens, L))
    assert not arena.touched_guards(), arena.touched_guards()


# ---- decode -----------------------------------------------------------------------------------------------------------------------------
K_DEQ, V_DEQ = (0.031, 3.0), (0.027, -9.0)


def random_cache(E, seed):
    gen = torch.Generator().manual_seed(seed)
    return tuple(torch.randint(-128, 128, (B, HKV, S_MAX, E), generator=gen).to(torch.int8).to(DEV) for _ in range(2))


def rule_count(rows, E, plan_len=S_MAX):
    return ops.sdpa_decode_plan(B, HKV, plan_len, rows, E)


@pytest.mark.parametrize("G", cases.GROUPS)
@pytest.mark.parametrize("E", cases.ES)
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_every_batch_row_is_the_dense_kernel_on_its_own_slice(entries, dtype, E, G):
    """Bit for bit, at the same split count (the ranges are the same by construction): no mask against no mask, bottom-right causality
    against the equivalent bool mask; exact zeros where the dense entry refuses S = 0."""
    kc, vc = random_cache(E, seed=E + G)
    deq = (None, scalars(*K_DEQ), scalars(*V_DEQ))
    gen = torch.Generator().manual_seed(G)
    calls = 0
    for L in cases.LS:
        q = torch.randn(B, HKV * G, L, E, generator=gen).to(dtype).to(DEV)
        for lens in cases.LENS_SETS:
            device_lens = lens_tensor(lens)
            for causal in (False, True):
                for splits in cases.SPLITS:
                    got = ops.kv_decode(q, kc, vc, device_lens, is_causal=causal, dequant=deq, splits=splits)
                    calls += 1
                    count = splits or rule_count(L * G, E)
                    for b, n in enumerate(lens):
                        S = cases.clamp_len(n)
                        if S == 0:
                            assert torch.equal(got[b], torch.zeros_like(got[b])), (L, lens, causal, splits)
                            continue
                        mask = cases.bottom_right(L, S, DEV) if causal else None
                        dense = ops.sdpa_decode(q[b:b + 1], kc[b:b + 1, :, :S], vc[b:b + 1, :, :S], attn_mask=mask, dequant=deq, splits=count)
                        assert torch.equal(got[b:b + 1].view(torch.int16), dense.view(torch.int16)), (L, lens, b, causal, splits)
                        if causal and S < L:
                            assert torch.equal(got[b, :, :L - S], torch.zeros_like(got[b, :, :L - S]))
    assert entries["ffq_kv_decode"] == calls == 3 * 2 * 2 * 5


@pytest.mark.parametrize("L,G", [(1, 1), (1, 4), (4, 4), (5, 1), (5, 4)])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_known_answers_at_every_length_and_split(entries, dtype, L, G):
    """select / staircase / uniform cut to each sequence's own key count (kv_cache_cases.exact_case): the answer itself, under every
    split count, with and without bottom-right causality."""
    for E in cases.ES:
        for kind, causal in (("select", False), ("staircase", False), ("staircase", True), ("uniform", False), ("uniform", True)):
            for lens in cases.LENS_SETS:
                q, kc, vc, k_param, v_param, expected = cases.exact_case(kind, causal, L, G, E, dtype, lens)
                operands = [t.to(DEV) for t in (q, kc, vc)]
                deq = (None, scalars(*k_param), scalars(*v_param))
                for splits in cases.SPLITS:
                    got = ops.kv_decode(*operands, lens_tensor(lens), is_causal=causal, dequant=deq, splits=splits)
                    same = got.cpu().double() == expected
                    assert bool(same.all()), f"{kind} causal={causal} E={E} lens={lens} splits={splits}: {int((~same).sum())} elements differ, first at {(~same).nonzero()[0].tolist()}"
    assert entries["ffq_kv_decode"] == 2 * 5 * 2 * 5


@pytest.mark.parametrize("E", cases.ES)
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_random_operands_meet_the_attention_contract(entries, dtype, E):
    """The rule of tests/test_sdpa_decode_gpu.py, per sequence: the error against float64 attention of the dequantized slice is at most
    the device math path's own on the same call + 2^-9."""
    kq, vq = cases.quantizer((8, *K_DEQ), DEV), cases.quantizer((8, *V_DEQ), DEV)
    gen = torch.Generator().manual_seed(E)
    k_all, v_all = (torch.randn(B, HKV, S_MAX, E, generator=gen).to(dtype).to(DEV) for _ in range(2))
    with torch.no_grad():
        k_codes, v_codes = kq(k_all), vq(v_all)
    kc, vc = k_codes.raw_data, v_codes.raw_data
    deq = (None, (kq.scale.detach(), kq.offset.detach()), (vq.scale.detach(), vq.offset.detach()))
    for L, G, lens, causal in ((1, 4, cases.LENS_SETS[0], False), (4, 4, cases.LENS_SETS[1], True), (5, 1, cases.LENS_SETS[1], True)):
        q = torch.randn(B, HKV * G, L, E, generator=gen).to(dtype).to(DEV)
        got = ops.kv_decode(q, kc, vc, lens_tensor(lens), is_causal=causal, dequant=deq)
        for b, n in enumerate(lens):
            S = cases.clamp_len(n)
            if S == 0:
                continue
            k_b, v_b = kq.wrap_codes(kc[b:b + 1, :, :S], dtype), vq.wrap_codes(vc[b:b + 1, :, :S], dtype)
            mask = cases.bottom_right(L, S, DEV) if causal else None
            want = math_path(q[b:b + 1], k_b, v_b, attn_mask=mask, enable_gqa=True)
            meets_the_contract(got[b:b + 1], want, reference(q[b:b + 1], k_b, v_b, mask=mask), f"L={L} G={G} S={S}")
    assert entries["ffq_kv_decode"] == 3


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_the_output_quantizer_runs_on_the_fp32_value(entries, dtype):
    """The properties tests/test_sdpa_decode_gpu.py asks of the dense entry, per sequence: every output a multiple of the scale, inside
    the grid, within one step of the fake-quantized float64 attention."""
    E, L, G, lens = 128, 2, 4, cases.LENS_SETS[1]
    kc, vc = random_cache(E, seed=31)
    gen = torch.Generator().manual_seed(31)
    q = torch.randn(B, HKV * G, L, E, generator=gen).to(dtype).to(DEV)
    bits, step, offset = 8, 2.0**-5, 3.0
    for splits in (0, 3):
        got = ops.kv_decode(q, kc, vc, lens_tensor(lens), is_causal=True, dequant=(None, scalars(*K_DEQ), scalars(*V_DEQ)),
                            output_quantizer=(*scalars(step, offset), float(bits)), splits=splits)
        assert got.dtype == dtype
        units = got.cpu().double() / step
        assert torch.equal(units, units.round()), "an output is not a multiple of the scale"
        assert float((units - offset).min()) >= -2 ** (bits - 1) and float((units - offset).max()) <= 2 ** (bits - 1) - 1
        ref = cases.attend64(q, kc, vc, lens, (8, *K_DEQ), (8, *V_DEQ), causal=True)
        fake = (torch.clamp(torch.round(ref / step - offset), -2 ** (bits - 1), 2 ** (bits - 1) - 1) + offset) * step
        assert float((got.cpu().double() - fake).abs().max()) <= step
    assert entries["ffq_kv_decode"] == 2


@pytest.mark.parametrize("plan_len", [None, 1, 200, 1024])
def test_the_plan_hint_names_the_split_count_and_the_workspace_is_guarded(entries, plan_len):
    """``splits = 0`` takes ``sdpa_decode_plan`` at `plan_len` keys (S_max by default): seen in the workspace the call allocates inside a
    guarded arena (tests/guards.py), under two poisons; the result is the forced count's, whatever the workspace held."""
    Bp, Hp, S_max, E, L, G = 1, 2, 1024, 128, 2, 4
    assert [ops.sdpa_decode_plan(Bp, Hp, n, L * G, E) for n in (1, 200, 1024)] == [1, 1, 4]
    count = ops.sdpa_decode_plan(Bp, Hp, plan_len or S_max, L * G, E)
    gen = torch.Generator().manual_seed(2)
    q = torch.randn(Bp, Hp * G, L, E, generator=gen).bfloat16().to(DEV)
    kc, vc = (torch.randint(-128, 128, (Bp, Hp, S_max, E), generator=gen).to(torch.int8).to(DEV) for _ in range(2))
    lens, deq = lens_tensor([700]), (None, scalars(*K_DEQ), scalars(*V_DEQ))
    results = []
    for poison in (guards.POISON_A, guards.POISON_B):
        arena = guards.Arena(poison)
        with guards.capture(arena):
            out = ops.kv_decode(q, kc, vc, lens, is_causal=True, dequant=deq, plan_len=plan_len)
        torch.cuda.synchronize()
        fresh = sorted(b.nbytes for b in arena.blocks if b.kind == "fresh")
        assert fresh == sorted([out.numel() * 2, ops.sdpa_decode_workspace_bytes(Bp, Hp, L * G, E, count)]) and arena.find(out.data_ptr()) is not None
        assert not arena.touched_guards(), arena.touched_guards()
        results.append(out.clone())
    forced = ops.kv_decode(q, kc, vc, lens, is_causal=True, dequant=deq, splits=count)
    assert torch.equal(results[0].view(torch.int16), results[1].view(torch.int16)) and torch.equal(results[0].view(torch.int16), forced.view(torch.int16))
    assert entries["ffq_kv_decode"] == 3


# ---- the class --------------------------------------------------------------------------------------------------------------------------
def make_cache(dtype, E, layout="bshe", batch=B, max_len=S_MAX):
    kq, vq = cases.quantizer(cases.K_SPEC, DEV), cases.quantizer(cases.V_SPEC, DEV)
    return ff.nn.QuantizedKVCache(batch, HKV, max_len, E, kq, vq, dtype, DEV, layout=layout)


def step_inputs(E, dtype, G, steps, seed):
    gen = torch.Generator().manual_seed(seed)
    return [tuple(torch.randn(B, heads, 1, E, generator=gen).to(dtype).to(DEV) for heads in (HKV, HKV, HKV * G)) for _ in range(steps)]


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_a_ragged_decode_loop_eager_and_replayed_from_one_graph(entries, dtype):
    """The prompt goes in at per-batch lengths, then 12 steps of append + attend at L = 1, one launch of each per step. Step 6 is then
    captured ONCE and steps 6 .. 11 replayed from it with new inputs: the same outputs, lengths and cache as the eager loop, which no
    graph of the dense entry can give (its key count is frozen at capture)."""
    E, G, start = 128, 4, (0, 100, 127, 255, 380)  # (the last sequence runs past S_max after four steps: its rows are dropped)
    gen = torch.Generator().manual_seed(17)
    rope = tuple(torch.randn(S_MAX, E, generator=gen).to(dtype).to(DEV) for _ in range(2))
    prompt = tuple(torch.randn(B, HKV, max(start), E, generator=gen).to(dtype).to(DEV) for _ in range(2))
    inputs = step_inputs(E, dtype, G, 12, seed=18)

    eager = make_cache(dtype, E)
    eager.reset([n - max(start) for n in start])  # (append adds L = max(start) itself: sequence b keeps the prompt's last start[b] rows)
    eager.append(*prompt, rope=rope)
    assert eager.lengths.tolist() == list(start) and entries["ffq_kv_append"] == 1
    composed = make_cache(dtype, E)                # the same loop's cache through the composed route (lengths read on the host)
    composed.reset(start)
    ff.nn.kv_cache.composed_append(composed.k_cache, composed.v_cache, composed.lengths, *prompt, composed.key_quantizer, composed.value_quantizer, rope)
    snapshot = None
    outs = []
    for step, (k_t, v_t, q_t) in enumerate(inputs):
        if step == 6:
            snapshot = (eager.k_cache.clone(), eager.v_cache.clone(), eager.lengths.clone())
        eager.append(k_t, v_t, rope=rope)
        outs.append(eager.attend(q_t))
        composed.lengths.add_(1)
        ff.nn.kv_cache.composed_append(composed.k_cache, composed.v_cache, composed.lengths, k_t, v_t, composed.key_quantizer, composed.value_quantizer, rope)
    torch.cuda.synchronize()
    assert entries["ffq_kv_append"] == 13 and entries["ffq_kv_decode"] == 12 and eager.lengths.tolist() == [n + 12 for n in start]
    assert torch.equal(eager.k_cache, composed.k_cache) and torch.equal(eager.v_cache, composed.v_cache)
    deq = (None, *((quantizer.scale.detach(), quantizer.offset.detach()) for quantizer in (eager.key_quantizer, eager.value_quantizer)))
    for b, n in enumerate(eager.lengths.tolist()):  # the last step against the dense kernel on every sequence's own slice
        S = cases.clamp_len(n)
        dense = ops.sdpa_decode(inputs[-1][2][b:b + 1], eager.k_cache[b:b + 1, :, :S], eager.v_cache[b:b + 1, :, :S], dequant=deq, splits=rule_count(G, E))
        assert torch.equal(outs[-1][b:b + 1].view(torch.int16), dense.view(torch.int16)), b

    # ---- capture step 6 once, on a side stream, with static input buffers
    replayed = make_cache(dtype, E)
    replayed.k_cache.copy_(snapshot[0])
    replayed.v_cache.copy_(snapshot[1])
    replayed.lengths.copy_(snapshot[2])
    static = [t.clone() for t in inputs[6]]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):               # (a warm-up outside the capture, undone below)
        replayed.append(static[0], static[1], rope=rope)
        replayed.attend(static[2])
    torch.cuda.current_stream().wait_stream(stream)
    replayed.k_cache.copy_(snapshot[0])
    replayed.v_cache.copy_(snapshot[1])
    replayed.lengths.copy_(snapshot[2])
    before = dict(entries)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        replayed.append(static[0], static[1], rope=rope)
        captured = replayed.attend(static[2])
    assert entries["ffq_kv_append"] == before["ffq_kv_append"] + 1 and entries["ffq_kv_decode"] == before["ffq_kv_decode"] + 1
    assert replayed.lengths.tolist() == snapshot[2].tolist()                       # (a capture runs nothing)
    for i, step in enumerate(range(6, 12)):
        for buffer, new in zip(static, inputs[step]):
            buffer.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured.view(torch.int16), outs[step].view(torch.int16)), f"replay {i}"
        assert replayed.lengths.tolist() == [n + step + 1 for n in start]
    assert torch.equal(replayed.k_cache, eager.k_cache) and torch.equal(replayed.v_cache, eager.v_cache)
    assert entries["ffq_kv_append"] == before["ffq_kv_append"] + 1                 # (six replays, no further call)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.DTYPE_IDS)
def test_a_uniform_cache_goes_straight_into_scaled_dot_product_attention(entries, dtype):
    """``keys(S)`` / ``values(S)`` are tensors the fused decode route's predicate takes: one ``ffq_sdpa_decode`` call, and the bits of
    ``attend(is_causal=False)`` at the same split count."""
    E, G, S = 64, 4, 300
    cache = make_cache(dtype, E, layout="bhse")
    gen = torch.Generator().manual_seed(23)
    k, v = (torch.randn(B, HKV, S, E, generator=gen).to(dtype).to(DEV) for _ in range(2))
    q = torch.randn(B, HKV * G, 1, E, generator=gen).to(dtype).to(DEV)
    cache.append(k, v)
    assert cache.lengths.tolist() == [S] * B and entries["ffq_kv_append"] == 1
    with torch.no_grad():
        assert torch.equal(cache.keys(S).raw_data, cache.key_quantizer(k).raw_data) and torch.equal(cache.keys(S).dequantize(), cache.key_quantizer(k).dequantize())
        routed = F.scaled_dot_product_attention(q, cache.keys(S), cache.values(S), enable_gqa=True, strict_quantization=False)
    assert entries["ffq_sdpa_decode"] == 1 and entries["ffq_kv_decode"] == 0
    own = cache.attend(q, is_causal=False, splits=ops.sdpa_decode_plan(B, HKV, S, G, E))
    assert entries["ffq_kv_decode"] == 1 and torch.equal(own.view(torch.int16), routed.view(torch.int16))
