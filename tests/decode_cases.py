"""The drawn cases of the split-key decode attention (csrc/ffq_sdpa_decode.hip), their operands, views and mask forms, and the
bit-exact relations between two runs of the same kernel that tests/test_sdpa_decode_cases_cpu.py (on a pure-torch model of the
kernel's indexing) and tests/test_sdpa_decode_cases_gpu.py (on the device) share. A plain module: no test, no fixture.

:func:`drawn` returns the same list on every machine. The fields of a case are paired by index arithmetic, not drawn uniformly,
so that the coverage conditions hold (the CPU test asserts them): every value of every field occurs in at least three cases, each of
the five ``(L, G)`` with a non-power-of-two ``L`` and ``G > 1`` meets every mask kind, and every layout meets an explicit mask, int8
``q`` and a forced split count above one. What cannot be paired is drawn from ``attention_exact.generator("decode_cases", i)``: the
seed of the case's random operands and the three ``(batch, head, row)`` of the "row alone" relation.

Two constraints shape the pairing, none drops a value from the domain: ``batch_expand`` takes a ``(B, HKV)`` with ``B > 1`` and
``bshe`` one with ``HKV > 1`` (the next pair in the list that has it), since a stride over a dimension of size 1 is never stepped and
would claim nothing; the ``transposed`` mask form is given to cases with ``L > 1`` for the same reason. No value of the
domain below was dropped.

A run is ``run(q, k, v, *, mask=None, causal=False, splits=0) -> Tensor [B, H, L, E]`` with q / k / v as :class:`Coded` (the tensor
as handed over, a view included, and its ``(scale, offset)``, ``scale`` None for plain values). The relations take such a function, so
the CPU test can hand them a model with a planted indexing defect and see them fail."""

from __future__ import annotations

import dataclasses
import functools

from typing import Callable, NamedTuple

import torch

import attention_exact as ax

from fastforward_amd.ops import decode

ROWS = ((3, 5), (5, 6), (7, 4), (6, 5), (11, 2), (1, 32), (2, 16), (16, 2), (31, 1), (1, 1))  # (L, G = H / HKV)
FIRST_FIVE = ROWS[:5]  # L not a power of two together with G > 1: row / L and row % L are no shifts and masks
GROUPS = ((1, 1), (1, 2), (3, 1), (3, 3), (2, 4))  # (B, HKV)
KEYS = (31, 32, 33, 96, 97, 127, 128, 255, 256, 257, 383, 384, 385, 511, 513, 2049)
WIDTHS = (64, 128)
DTYPES = (torch.bfloat16, torch.float16)
MASKS = ("none", "causal", "bool", "float32", "float")  # "float": in the data dtype
EXPLICIT = MASKS[2:]
FORMS = ("LS", "B1LS", "1HLS", "BHLS", "transposed", "byte_offset")
CONTAINERS = ("plain", "int8", "dtype")
SPLITS = (0, 1, 2, 3, 7, decode.MAX_SPLITS)
LAYOUTS = ("contiguous", "bshe", "fused_kv", "cache_prefix", "batch_expand", "shifted")
CACHE_TAIL = 200  # keys behind a cache prefix, filled with 77
TRADE_SHIFTS = (-27, 1, 27)
TRADE_OFFSETS = (3.0, -9.0, 2.5, -0.5)

_BOOL_FORMS = ("byte_offset", "LS", "transposed", "byte_offset", "B1LS", "1HLS", "byte_offset", "BHLS", "transposed", "byte_offset")
_FLOAT_FORMS = ("LS", "B1LS", "1HLS", "BHLS", "transposed")


@dataclasses.dataclass(frozen=True)
class Case:
    index: int
    L: int
    G: int
    B: int
    HKV: int
    S: int
    E: int
    dtype: torch.dtype
    mask: str
    mask_form: str | None  # None without an explicit mask
    q_container: str
    splits: int
    layout: str
    seed: int
    picks: tuple[tuple[int, int, int], ...]  # (batch, head, row) of "row alone"

    @property
    def H(self) -> int:
        return self.HKV * self.G

    @property
    def rows(self) -> int:
        return self.L * self.G

    @property
    def shape(self) -> ax.Shape:
        return ax.Shape(self.B, self.H, self.HKV, self.L, self.S, self.E)

    @property
    def count(self) -> int:
        """The split count the call runs with, the rule's made explicit."""
        return self.splits or decode.sdpa_decode_plan(self.B, self.HKV, self.S, self.rows, self.E)

    @property
    def id(self) -> str:
        dt = "bf16" if self.dtype == torch.bfloat16 else "fp16"
        mask = self.mask if self.mask_form is None else f"{self.mask}[{self.mask_form}]"
        return f"{self.index:02d}-L{self.L}xG{self.G}-B{self.B}xK{self.HKV}-S{self.S}-E{self.E}-{dt}-{mask}-q_{self.q_container}-split{self.splits}-{self.layout}"


@functools.lru_cache(maxsize=None)
def _drawn(n: int) -> tuple[Case, ...]:
    out: list[Case] = []
    bools = floats = 0
    for i in range(n):
        t = i % 50
        if t < 25:
            (L, G), mask = FIRST_FIVE[t % 5], MASKS[t // 5]
        else:
            j = t - 25
            (L, G), mask = ROWS[5 + j % 5], MASKS[(j + j // 5) % 5]
        a, k = i % 6, i // 6
        layout, splits, container = LAYOUTS[a], SPLITS[(a + k) % 6], CONTAINERS[(a + 2 * k) % 3]
        at = (i + i // 5) % 5
        while (layout == "batch_expand" and GROUPS[at][0] == 1) or (layout == "bshe" and GROUPS[at][1] == 1):
            at = (at + 1) % 5
        B, HKV = GROUPS[at]
        form = None
        if mask == "bool":
            form = _BOOL_FORMS[bools % len(_BOOL_FORMS)]
            bools += 1
        elif mask in EXPLICIT:
            form = _FLOAT_FORMS[floats % len(_FLOAT_FORMS)]
            floats += 1
        if form == "transposed" and L == 1:
            form = "BHLS"
        gen = ax.generator("decode_cases", i)
        seed = int(torch.randint(0, 2**31 - 1, (1,), generator=gen))
        picks = tuple((int(torch.randint(0, B, (1,), generator=gen)), int(torch.randint(0, HKV * G, (1,), generator=gen)),
                       int(torch.randint(0, L, (1,), generator=gen))) for _ in range(3))
        out.append(Case(i, L, G, B, HKV, KEYS[(7 * i + i // 16) % 16], WIDTHS[(i // 2 + i // 5) % 2], DTYPES[(i + i // 6) % 2], mask, form, container, splits,
                        layout, seed, picks))
    return tuple(out)


def drawn(n: int = 48) -> list[Case]:
    return list(_drawn(n))


# ---- operands -----------------------------------------------------------------------------------------------------------------------------
class Coded(NamedTuple):
    raw: torch.Tensor  # as handed to the call: plain values, or codes in int8 or in the data dtype
    scale: float | None = None  # None: plain values
    offset: float | None = None

    def cut(self, *index: slice) -> "Coded":
        return Coded(self.raw[index], self.scale, self.offset)

    def to(self, device: str) -> "Coded":
        return Coded(self.raw.to(device), self.scale, self.offset)


def values(c: Coded, dtype: torch.dtype) -> torch.Tensor:
    """What the kernel contracts: plain values as they are, codes as ``(c + rne(o)) * s`` in fp32 rounded once to `dtype`."""
    if c.scale is None:
        return c.raw
    offset = torch.round(torch.tensor(c.offset or 0.0, dtype=torch.float32))
    return ((c.raw.float() + offset.to(c.raw.device)) * torch.tensor(c.scale, dtype=torch.float32, device=c.raw.device)).to(dtype)


def codes_of(x: torch.Tensor, scale: float, offset: float, container: torch.dtype = torch.int8) -> Coded:
    """`x` (multiples of `scale`) as codes ``c = x / scale - offset``; refuses what does not fit int8 (the premise of the known-answer
    tests: ``to_k_codes`` of tests/test_sdpa_decode_gpu.py)."""
    c = x.double() / scale - offset
    assert bool((c == c.round()).all()) and float(c.min()) >= -128 and float(c.max()) <= 127, "the values do not fit int8 codes"
    return Coded(c.to(container), scale, offset)


V_OFFSETS = (0.0, 200.0, -200.0, 37.0)


def drawn_v(shape: tuple[int, ...], dtype: torch.dtype, seed: int) -> tuple[Coded, torch.Tensor]:
    """V = (c + o) * 2^-e rounded once to the dtype with c over all of [-128, 127] (``drawn_v`` of tests/test_sdpa_decode_gpu.py): the
    codes and the values in `dtype`."""
    gen = ax.generator("decode_cases_v", shape, str(dtype), seed)
    c = torch.randint(-128, 128, shape, generator=gen)
    c.view(-1)[:256] = torch.arange(-128, 128)[torch.randperm(256, generator=gen)][: c.numel()]
    offset, e = V_OFFSETS[seed % 4], (0, 3, 7)[seed % 3]
    return Coded(c.to(torch.int8), 2.0**-e, offset), ((c.float() + offset) * 2.0**-e).to(dtype)


def _container(case: Case) -> torch.dtype:
    return case.dtype if case.q_container == "dtype" else torch.int8


class Known(NamedTuple):
    pattern: ax.Pattern
    q: Coded
    k: Coded
    v: Coded


_PATTERN_LEAD = {"LS": "LS", "transposed": "LS", "byte_offset": "LS", "B1LS": "B1LS", "1HLS": "1HLS", "BHLS": "1HLS"}


@functools.lru_cache(maxsize=None)
def known(index: int) -> tuple[Known, ...]:
    """The known-answer patterns of drawn case `index` on the host, built once and left unchanged: ``select`` and ``staircase`` (and
    ``uniform`` without a mask) for mask none / causal, ``mask_select`` for a float mask, ``masked_uniform`` for a bool one. K and V
    are int8 codes, V drawn over every code (:func:`drawn_v`); q goes into the case's container. Under ``batch_expand`` K and V are
    those of batch 0 in every batch and the expectations are built from the expanded values. A staircase whose q must fit int8 codes
    is the ``a = 1, scale = 32`` one (q = (1, 128, noise): codes at scale 1, offset 1), with the same step of 32 between scores."""
    case = drawn()[index]
    shape, dtype, plain = case.shape, case.dtype, case.q_container == "plain"
    expand = (lambda t: t[:1].expand(t.shape).contiguous()) if case.layout == "batch_expand" else (lambda t: t)
    group = (case.B, case.HKV, case.S, case.E)
    out: list[Known] = []

    def onehot(base: ax.Pattern, k_params: tuple[float, float], q_params: tuple[float, float]) -> None:
        v, v_values = drawn_v(group, dtype, case.seed + len(out))
        v, v_values = Coded(expand(v.raw), v.scale, v.offset), expand(v_values)
        k = expand(base.k.double())
        q = base.q.double()
        if base.name == "select":  # the query selects its target among the keys it is given
            q = ax.GAIN * k.repeat_interleave(case.G, 1).gather(2, base.target.unsqueeze(-1).expand(-1, -1, -1, case.E))
        p = ax._onehot(base.name, shape, dtype, q, k, v_values, base.target, causal=base.causal, mask=base.mask, scale=base.scale)
        assert p.residual <= ax.RESIDUAL_LIMIT
        out.append(Known(p, Coded(p.q) if plain else codes_of(p.q, *q_params, _container(case)), codes_of(p.k, *k_params), v))

    if case.mask in ("none", "causal"):
        causal = case.mask == "causal"
        onehot(ax.select(shape, dtype, causal=causal), (1.0, 100.0), (2.0, 3.0))
        stair = ax.staircase(shape, dtype, causal=causal) if plain else ax.staircase(shape, dtype, causal=causal, a=1, scale=32.0)
        onehot(stair, (1.0, 8.0), (1.0, 1.0))
    elif case.mask in ("float32", "float"):
        lead = _PATTERN_LEAD[case.mask_form]
        onehot(ax.mask_select(shape, dtype, lead, mask_dtype=torch.float32 if case.mask == "float32" else None), (2.0**-2, -100.0), (0.5, 5.0))
    if case.mask in ("none", "bool"):
        variant = case.index % 2
        u = ax.uniform(shape, dtype, variant) if case.mask == "none" else ax.masked_uniform(shape, dtype, variant, _PATTERN_LEAD[case.mask_form])
        u = dataclasses.replace(u, k=expand(u.k))
        q = Coded(u.q) if plain else codes_of(u.q, 0.5, 5.0, _container(case))
        out.append(Known(u, q, codes_of(u.k, 2.0**-2, 100.0), codes_of(u.v, 1.0, 100.0)))
    return tuple(out)


def random_operands(case: Case, trade: bool = False, q_container: str | None = None) -> tuple[Coded, Coded, Coded]:
    """The random operands of the relations: ``randn`` q (codes uniform over int8 in a container), K / V codes uniform over
    [-128, 127]; `trade`: every code within [-100, 100]."""
    gen = ax.generator("decode_cases_random", case.index, case.seed, trade, q_container)
    lo, hi = (-100, 101) if trade else (-128, 128)
    container = q_container or case.q_container
    if container == "plain":
        q = Coded(torch.randn(case.B, case.H, case.L, case.E, generator=gen).to(case.dtype))
    else:
        codes = torch.randint(lo, hi, (case.B, case.H, case.L, case.E), generator=gen)
        q = Coded(codes.to(case.dtype if container == "dtype" else torch.int8), 0.04, 5.0)
    k, v = (torch.randint(lo, hi, (case.B, case.HKV, case.S, case.E), generator=gen).to(torch.int8) for _ in range(2))
    return q, Coded(k, 0.031, 3.0), Coded(v, 0.027, -9.0)


def random_mask(case: Case, kind: str, form: str, salt: int = 0) -> torch.Tensor:
    """A random mask of `kind` ("bool", "float32", "float") at the leading dims of `form`, contiguous: keep probability 0.7 with row
    ``L // 3`` fully masked where L >= 3 (bool); ``2 randn`` with a run of -inf (float)."""
    gen = ax.generator("decode_cases_mask", case.index, kind, form, salt)
    shape = (*lead_shape(case, form), case.L, case.S)
    if kind == "bool":
        mask = torch.rand(shape, generator=gen) < ax.KEEP
        if case.L >= 3:
            mask[..., case.L // 3, :] = False
        return mask
    mask = (torch.randn(shape, generator=gen) * 2).to(torch.float32 if kind == "float32" else case.dtype)
    mask[..., 0, 5:9] = -float("inf")
    return mask


def tril(case: Case, kind: str = "bool") -> torch.Tensor:
    """The explicit top-left mask of ``is_causal``: row t sees keys <= t; bool, or 0 / -inf in fp32 or in the data dtype."""
    visible = torch.ones(case.L, case.S, dtype=torch.bool).tril()
    if kind == "bool":
        return visible
    zero = torch.zeros(case.L, case.S, dtype=torch.float32 if kind == "float32" else case.dtype)
    return zero.masked_fill(~visible, -float("inf"))


# ---- views, each checked to be what it claims -----------------------------------------------------------------------------------------------
def _aligned(t: torch.Tensor) -> torch.Tensor:
    assert t.data_ptr() % 16 == 0 and t.stride(-1) == 1, (t.data_ptr() % 16, t.stride())
    return t


def _bshe(t: torch.Tensor) -> torch.Tensor:
    B, N, R, E = t.shape
    view = t.transpose(1, 2).contiguous().transpose(1, 2)
    steps = [(st, want) for n, st, want in zip(view.shape, view.stride(), (R * N * E, E, N * E, 1)) if n > 1]  # (a dim of size 1 is never stepped)
    assert all(st == want for st, want in steps) and (view.is_contiguous() is (N == 1 or R == 1))
    return view


def _prefix(t: torch.Tensor) -> torch.Tensor:
    B, N, S, E = t.shape
    buffer = torch.full((B, N, S + CACHE_TAIL, E), 77, dtype=t.dtype, device=t.device)
    buffer[:, :, :S] = t
    view = buffer[:, :, :S]
    assert view.stride() == (N * (S + CACHE_TAIL) * E, (S + CACHE_TAIL) * E, E, 1) and bool((buffer[:, :, S:] == 77).all())
    assert view.is_contiguous() is (B * N == 1)
    return view


def _expanded(t: torch.Tensor) -> torch.Tensor:
    view = t[:1].clone().expand(t.shape)
    assert view.stride(0) == 0 and view.stride()[1:] == t.contiguous().stride()[1:] and (view.is_contiguous() is (t.shape[0] == 1))
    return view


def _shifted(t: torch.Tensor, nbytes: int) -> torch.Tensor:
    item = t.element_size()
    flat = torch.full((t.numel() + 64 // item,), 77, dtype=t.dtype, device=t.device)
    assert flat.data_ptr() % 64 == 0
    view = flat[nbytes // item: nbytes // item + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.storage_offset() * item == nbytes and view.data_ptr() % 16 == 0 and view.data_ptr() % 64 == nbytes
    return view


def lay_out(layout: str, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """q / k / v (any strides) in `layout`, every view aligned to 16 bytes. All views hold the values handed in but ``batch_expand``,
    whose K and V hold those of batch 0 in every batch: compare against ``view.clone()``."""
    q, k, v = q.contiguous().clone(), k.contiguous().clone(), v.contiguous().clone()
    B, HKV, S, E = k.shape
    if layout == "contiguous":
        assert q.is_contiguous() and k.is_contiguous() and v.is_contiguous()
    elif layout == "bshe":
        q, k, v = _bshe(q), _bshe(k), _bshe(v)
    elif layout == "fused_kv":
        kv = torch.cat([k, v], dim=-1)
        k, v = kv[..., :E], kv[..., E:]
        assert k.stride() == v.stride() == (HKV * S * 2 * E, S * 2 * E, 2 * E, 1) and v.data_ptr() - k.data_ptr() == E
        assert k.untyped_storage().data_ptr() == v.untyped_storage().data_ptr() and not k.is_contiguous() and not v.is_contiguous()
    elif layout == "cache_prefix":
        k, v = _prefix(k), _prefix(v)
    elif layout == "batch_expand":
        k, v = _expanded(k), _expanded(v)
    elif layout == "shifted":
        q, k, v = _shifted(q, 16), _shifted(k, 16), _shifted(v, 48)
    else:
        raise ValueError(layout)
    return _aligned(q), _aligned(k), _aligned(v)


def laid_out(layout: str, q: Coded, k: Coded, v: Coded) -> tuple[Coded, Coded, Coded]:
    raw = lay_out(layout, q.raw, k.raw, v.raw)
    return tuple(Coded(r, c.scale, c.offset) for r, c in zip(raw, (q, k, v)))  # type: ignore[return-value]


def layouts_of(case: Case) -> tuple[str, ...]:
    """The layouts whose claim means something at the case's shape (its own among them)."""
    return tuple(name for name in LAYOUTS if not (name == "batch_expand" and case.B == 1) and not (name == "bshe" and case.HKV == 1 and case.G == 1))


def lead_shape(case: Case, form: str) -> tuple[int, ...]:
    return {"LS": (), "transposed": (), "byte_offset": (), "B1LS": (case.B, 1), "1HLS": (1, case.H), "BHLS": (case.B, case.H)}[form]


def forms_of(case: Case, kind: str) -> tuple[str, ...]:
    return tuple(f for f in FORMS if not (f == "byte_offset" and kind != "bool") and not (f == "transposed" and case.L == 1))


def in_form(case: Case, form: str, mask: torch.Tensor) -> torch.Tensor:
    """`mask` (leading dims that broadcast to those of `form`) as the call gets it."""
    L, S = case.L, case.S
    lead = lead_shape(case, form)
    mask = mask.expand(*lead, L, S).contiguous() if lead else mask.reshape(L, S).contiguous()
    if form == "transposed":
        view = mask.t().contiguous().t()
        assert view.stride() == (1, L) and not view.is_contiguous()
    elif form == "byte_offset":
        assert mask.dtype == torch.bool
        buffer = torch.full((L * S + 16,), 1, dtype=torch.uint8, device=mask.device)
        view = buffer[1:1 + L * S].view(torch.bool).view(L, S)
        view.copy_(mask)
        assert view.storage_offset() == 1 and view.data_ptr() % 2 == 1 and view.is_contiguous()
    else:
        view = mask
        assert view.is_contiguous() and tuple(view.shape) == (*lead, L, S)
    assert torch.equal(view, mask)
    return view


def dense(case: Case, mask: torch.Tensor) -> torch.Tensor:
    """The materialised contiguous [B, H, L, S] mask."""
    return mask.expand(case.B, case.H, case.L, case.S).contiguous()


# ---- the relations ------------------------------------------------------------------------------------------------------------------------
Run = Callable[..., torch.Tensor]


def bits(x: torch.Tensor) -> torch.Tensor:
    return x.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[x.element_size()])


def same(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {tuple(got.shape)} {got.dtype} against {tuple(want.shape)} {want.dtype}"
    assert torch.equal(bits(got), bits(want)), f"{what}: {ax.first_mismatch(got, want)}"


@dataclasses.dataclass(frozen=True)
class Call:
    """One call as drawn: operands in their layout, the mask in its form (None without one) and materialised, the explicit split count."""
    case: Case
    q: Coded
    k: Coded
    v: Coded
    mask: torch.Tensor | None
    causal: bool
    splits: int  # as drawn: 0 is the rule

    def full(self, run: Run) -> torch.Tensor:
        return run(self.q, self.k, self.v, mask=self.mask, causal=self.causal, splits=self.splits)

    def dense_mask(self) -> torch.Tensor | None:
        """[B, H, L, S]; the bool tril for a causal call."""
        if self.causal:
            return dense(self.case, tril(self.case).to(self.q.raw.device))
        return None if self.mask is None else dense(self.case, self.mask)


def call_of(case: Case, device: str = "cpu", trade: bool = False, layout: str | None = None) -> Call:
    """The case's call on random operands."""
    q, k, v = (c.to(device) for c in random_operands(case, trade))
    mask = None
    if case.mask in EXPLICIT:
        mask = in_form(case, case.mask_form, random_mask(case, case.mask, case.mask_form).to(device))
    return Call(case, *laid_out(layout or case.layout, q, k, v), mask, case.mask == "causal", case.splits)


def row_alone(run: Run, call: Call, full: torch.Tensor, picks: tuple[tuple[int, int, int], ...] | None = None) -> int:
    """One query row with its kv head and its mask row alone, at the same split count, has the bits of that row in the full call."""
    case, mask = call.case, call.dense_mask()
    for b, head, l in picks or case.picks:
        kvh = head // case.G
        one = slice(b, b + 1), slice(head, head + 1), slice(l, l + 1)
        group = slice(b, b + 1), slice(kvh, kvh + 1)
        got = run(call.q.cut(*one), call.k.cut(*group), call.v.cut(*group), mask=None if mask is None else mask[one], splits=case.count)
        same(got[0, 0, 0], full[b, head, l], f"row alone (batch {b}, head {head}, row {l})")
    return len(picks or case.picks)


def kv_head_alone(run: Run, call: Call, full: torch.Tensor, kvh: int) -> None:
    case, mask = call.case, call.dense_mask()
    heads = slice(kvh * case.G, (kvh + 1) * case.G)
    every, one = slice(None), slice(kvh, kvh + 1)
    got = run(call.q.cut(every, heads), call.k.cut(every, one), call.v.cut(every, one), mask=None if mask is None else mask[:, heads], splits=case.count)
    same(got, full[:, heads], f"kv head {kvh} alone")


def batch_alone(run: Run, call: Call, full: torch.Tensor, b: int) -> None:
    case, mask = call.case, call.dense_mask()
    one = slice(b, b + 1)
    got = run(call.q.cut(one), call.k.cut(one), call.v.cut(one), mask=None if mask is None else mask[one], splits=case.count)
    same(got, full[one], f"batch {b} alone")


def causal_is_tril(run: Run, call: Call) -> int:
    """``is_causal`` against the explicit top-left tril: bool, and 0 / -inf in fp32 and in the data dtype."""
    device = call.q.raw.device
    want = run(call.q, call.k, call.v, causal=True, splits=call.splits)
    for kind in ("bool", "float32", "float"):
        same(run(call.q, call.k, call.v, mask=tril(call.case, kind).to(device), splits=call.splits), want, f"is_causal against the {kind} tril")
    return 4


def mask_forms(run: Run, call: Call, kind: str, forms: tuple[str, ...] | None = None) -> int:
    """Every form of a mask of `kind` against the materialised contiguous [B, H, L, S] mask."""
    case, device = call.case, call.q.raw.device
    forms = forms or forms_of(case, kind)
    for form in forms:
        mask = in_form(case, form, random_mask(case, kind, form, salt=1).to(device))
        got = run(call.q, call.k, call.v, mask=mask, splits=call.splits)
        same(got, run(call.q, call.k, call.v, mask=dense(case, mask), splits=call.splits), f"{kind} mask as {form}")
    return 2 * len(forms)


def containers(run: Run, call: Call) -> int:
    """q as int8 codes, as the same codes in the data dtype, and as their plain values."""
    case, device = call.case, call.q.raw.device
    codes = random_operands(case, q_container="int8")[0].to(device)
    held = Coded(codes.raw.to(case.dtype), codes.scale, codes.offset)
    plain = Coded(values(codes, case.dtype))
    k, v = Coded(call.k.raw.clone(), *call.k[1:]), Coded(call.v.raw.clone(), *call.v[1:])
    got = [run(*laid_out(case.layout, q, k, v), mask=call.mask, causal=call.causal, splits=call.splits) for q in (codes, held, plain)]
    same(got[1], got[0], "q codes in the data dtype against int8 q codes")
    same(got[2], got[0], "plain q against int8 q codes")
    return 3


def rne(offset: float) -> float:
    return float(torch.round(torch.tensor(offset, dtype=torch.float32)))


def code_offset_trade(run: Run, call: Call, d: int, offsets: tuple[float, float, float]) -> int:
    """``(c + d, rne(o) - d)`` has the result of ``(c, o)`` for K, V and int8 q (call: codes within [-100, 100], int8 q), and ``o`` that of
    ``rne(o)``. The shift is taken from ``rne(o)``: ``rne(o - d)`` is another integer for a half-integer ``o`` and an odd ``d`` (ties go
    to even: rne(2.5 - 1) = 2, rne(2.5) - 1 = 1), so that is where the kernel's own definition of the offset puts it."""
    assert call.q.raw.dtype == torch.int8 and abs(d) <= 27

    def go(q: Coded, k: Coded, v: Coded) -> torch.Tensor:
        return run(q, k, v, mask=call.mask, causal=call.causal, splits=call.splits)

    base = [Coded(c.raw, c.scale, o) for c, o in zip((call.q, call.k, call.v), offsets)]
    want = go(*base)
    same(go(*(Coded(c.raw, c.scale, rne(c.offset)) for c in base)), want, f"offsets {offsets} against their rne")
    for i, name in enumerate("qkv"):
        moved = list(base)
        moved[i] = Coded(base[i].raw + d, base[i].scale, rne(base[i].offset) - d)
        same(go(*moved), want, f"{name}: codes + {d} with offset {rne(base[i].offset)} - {d}")
        if base[i].offset == rne(base[i].offset):
            assert moved[i].offset == base[i].offset - d
    return 5


def layouts_agree(run: Run, call: Call, full: torch.Tensor) -> int:
    """Every layout against its cloned contiguous operands; the case's own layout is `full`."""
    case = call.case
    plain = tuple(Coded(c.raw.clone(memory_format=torch.contiguous_format), c.scale, c.offset) for c in (call.q, call.k, call.v))  # (the values `full` read, contiguous)
    assert all(c.raw.is_contiguous() for c in plain)
    want = run(*plain, mask=call.mask, causal=call.causal, splits=call.splits)
    same(full, want, f"layout {case.layout} against its clone")
    launches = 1
    for name in layouts_of(case):
        if name == case.layout:
            continue
        views = laid_out(name, *plain)
        got = run(*views, mask=call.mask, causal=call.causal, splits=call.splits)
        clones = tuple(Coded(c.raw.clone(memory_format=torch.contiguous_format), c.scale, c.offset) for c in views)
        assert all(c.raw.is_contiguous() for c in clones)
        same(got, run(*clones, mask=call.mask, causal=call.causal, splits=call.splits), f"layout {name} against its clone")
        launches += 2
    return launches


# ---- a model of the kernel's indexing -------------------------------------------------------------------------------------------------------
DEFECTS = (None, "g_l_swapped", "shift_and_mask", "mask_strides_swapped", "kv_head_modulo")


def model(defect: str | None = None, dtype: torch.dtype = torch.bfloat16) -> Run:
    """The decode kernels' index arithmetic in pure torch: for every output (batch, head, row) the combine kernel's slot
    ``r = (head % G) * L + row`` of kv head ``head / G``, the partial kernel's ``(g, l) = (r / L, r % L)`` of that slot, query head
    ``kvh * G + g``, and the mask read through its four strides; the row itself is ``attention_exact.reference64`` over the gathered
    q row, keys and mask row. Defects: ``g_l_swapped`` decodes the slot as ``(r % G, r / G)``; ``shift_and_mask`` divides by L rounded
    up to a power of two; ``mask_strides_swapped`` steps the mask with ``ms[3]`` over rows and ``ms[2]`` over keys; ``kv_head_modulo``
    reads the keys of kv head ``head % HKV``."""
    assert defect in DEFECTS

    def run(q: Coded, k: Coded, v: Coded, *, mask: torch.Tensor | None = None, causal: bool = False, splits: int = 0) -> torch.Tensor:
        qv, kv, vv = (values(c, dtype).double() for c in (q, k, v))
        B, H, L, E = qv.shape
        HKV, S = kv.shape[1:3]
        G = H // HKV
        flat = ms = None
        if mask is not None:
            m = mask.expand(B, H, L, S)
            ms = list(m.stride())
            flat = torch.as_strided(m, (m.untyped_storage().nbytes() // m.element_size() - m.storage_offset(),), (1,))
            if defect == "mask_strides_swapped":
                ms[2], ms[3] = ms[3], ms[2]
        out = torch.zeros(B, H, L, E, dtype=torch.float64)
        keys = torch.arange(S)
        for b in range(B):
            for head in range(H):
                kvh = head % HKV if defect == "kv_head_modulo" else head // G
                for row in range(L):
                    r = (head % G) * L + row
                    if defect == "g_l_swapped":
                        g, l = r % G, r // G
                    elif defect == "shift_and_mask":
                        shift = (L - 1).bit_length()
                        g, l = (r >> shift) % G, (r & ((1 << shift) - 1)) % L
                    else:
                        g, l = r // L, r % L
                    source = (head // G) * G + g
                    visible, add = torch.ones(1, S, dtype=torch.bool), None
                    if causal:
                        visible = (keys <= l).reshape(1, S)
                    if flat is not None:
                        line = flat[(b * ms[0] + source * ms[1] + l * ms[2] + keys * ms[3]) % flat.numel()].reshape(1, S)
                        if line.dtype == torch.bool:
                            visible = line
                        else:
                            add = line.double()
                    scores = qv[b, source, l].reshape(1, 1, 1, E)
                    p = ax.reference64(scores, kv[b:b + 1, kvh:kvh + 1], vv[b:b + 1, kvh:kvh + 1], mask=visible if add is None else add)
                    out[b, head, row] = p[0, 0, 0]
        return out

    return run
