"""Affine convolutions whose result does not depend on the order of the sums: the draws, the cases and the float64 reference that
tests/test_conv_exact_cpu.py and tests/test_conv_exact_gpu.py share (docs/parity.md, "Order-free convolutions").

Every scale is a power of two, every offset an integer, the bias an integer multiple of ``sx * sw[n]``, and the codes lie in
``[-A, A)`` with A halved from 128 until, with R the reduction length,

    R * (A^2 + |ox| * A + owmax * A + |ox| * owmax) + 128 < 2^24          (``Draw.bound``; the 128 is the bias)

so the epilogue ``acc + ox * rsw + ow * rsx + cnt * ox * ow``, its product with ``sx * sw[n]`` and the bias are integers below 2^24
times a power of two at every step: fp32 computes them exactly in any order, with or without FMA. The value is the float64 ATen
convolution of ``(xc + ox) * sx`` and ``(wc + ow) * sw`` with zero padding — padding is the REAL value 0, not code 0 —, which knows
nothing of taps, counts, row sums or phases.

A family is one row of ``FAMILIES``: its ``ops`` entry point, its ``ff.nn.functional`` operators by spatial rank, and how its
geometry is drawn. ``draws(family)`` gives the 64 draws of the committed seed ``"conv-exact-<family>"``; ``case(family, index)``
builds the draw's tensors and the expected output once (cached: the CPU and the GPU tests read the same objects, unchanged).
"""

from __future__ import annotations

import dataclasses
import functools
import math
import random

from typing import Any

import torch

import fastforward_amd as ff

from fastforward_amd.quantization.affine.function import AffineQuantizationFunction, StaticAffineQuantParams
from fastforward_amd.quantization.function import QuantizationContext

N_DRAWS = 64
BLOCK = 8  # draws per test id of the GPU file
LIMIT = 1 << 24
MAX_OUTPUTS = 100_000  # positions * OC
MAX_WORK = 50_000_000  # positions * OC * R: what the float64 reference costs
REAL = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
MODES = ("f32", "bf16", "f16", "int8")
X_OFFSETS = (200, -200, 131, -150, 57, -3, 255, -77)
CHANNELS = (1, 3, 15, 16, 17, 32, 48)
OUT_CHANNELS = (1, 7, 40, 127, 128, 129, 200)
DEPTHWISE = ((2, 1), (3, 2), (5, 3), (16, 1), (17, 2), (43, 3), (64, 2), (127, 1), (128, 1), (65, 2), (67, 3), (32, 1))  # (C, M)


@dataclasses.dataclass(frozen=True)
class Family:
    name: str
    kind: str  # "forward", "transposed" or "depthwise"
    entry: str  # the wrapper in fastforward_amd.ops: the 1-D draws reach it as H = KH = 1
    functional: dict[int, str]  # spatial rank -> operator of ff.nn.functional
    extent: dict[int, int]  # spatial rank -> the largest extent of an axis, input and output
    pads_channels: bool  # the layout pass pads C to Cp = 16 * ceil(C / 16)
    oc_axis: int = 0  # of the weight


FAMILIES = {f.name: f for f in (
    Family("conv", "forward", "conv2d_w8a8", {1: "conv1d", 2: "conv2d"}, {1: 61, 2: 23}, True),
    Family("conv3d", "forward", "conv3d_w8a8", {3: "conv3d"}, {3: 9}, True),
    Family("conv_transpose", "transposed", "conv_transpose2d_w8a8", {1: "conv_transpose1d", 2: "conv_transpose2d"}, {1: 61, 2: 23}, True, 1),
    Family("depthwise", "depthwise", "depthwise_conv2d_w8a8", {1: "conv1d", 2: "conv2d"}, {1: 61, 2: 23}, False),
)}


@dataclasses.dataclass(frozen=True)
class Draw:
    family: str
    index: int
    dims: int
    B: int
    C: int
    OC: int
    size: tuple[int, ...]
    kernel: tuple[int, ...]
    stride: tuple[int, ...]
    padding: tuple[int, ...]
    dilation: tuple[int, ...]
    output_padding: tuple[int, ...]  # zeros but for the transposed family
    out_size: tuple[int, ...]
    A: int  # codes in [-A, A)
    a: int  # sx = 2^-a
    b: tuple[int, ...]  # sw[n] = 2^-b[n]: one entry (per tensor) or OC
    x_form: str  # "none", "zero" or "real"
    ox: int
    w_form: str  # "none", "zero" or "real"
    owmax: int
    bias: str | None  # the bias's dtype on the ops route (the functional route takes the data dtype), None without one
    mode: str  # "f32", "bf16", "f16": the real output; "int8": the re-quantizing epilogue
    y_dt: str  # what the output quantizer rounds from
    bits: int
    out_offset: bool  # an integer output offset, else none
    route: str  # "ops" on raw codes or "functional" on QuantizedTensors
    channels_last: bool
    seed: int

    @property
    def groups(self) -> int:
        return self.C if FAMILIES[self.family].kind == "depthwise" else 1

    @property
    def taps(self) -> int:
        return math.prod(self.kernel)

    @property
    def reduction(self) -> int:
        return self.taps if FAMILIES[self.family].kind == "depthwise" else self.C * self.taps

    @property
    def positions(self) -> int:
        return self.B * math.prod(self.out_size)

    @property
    def bound(self) -> int:
        return bound(self.reduction, self.A, self.ox, self.owmax)

    def __str__(self) -> str:
        geometry = f"B={self.B} C={self.C} OC={self.OC} size={self.size} k={self.kernel} s={self.stride} p={self.padding} d={self.dilation}"
        if any(self.output_padding):
            geometry += f" op={self.output_padding}"
        forms = (f"A={self.A} sx=2^-{self.a} sw=2^-{self.b[0] if len(self.b) == 1 else sorted(set(self.b))}{'' if len(self.b) == 1 else ' per channel'} "
                 f"x_offset={self.x_form}:{self.ox} w_offset={self.w_form}:{self.owmax} bias={self.bias} mode={self.mode}")
        if self.mode == "int8":
            forms += f" from {self.y_dt}, {self.bits} bits, offset={self.out_offset}"
        return f"{self.family}[{self.index}] {self.dims}-D {geometry} -> {self.out_size}; {forms}; {self.route}{' channels-last' if self.channels_last else ''}"


def bound(reduction: int, A: int, ox: int, owmax: int) -> int:
    """The largest |integer| any step of the epilogue can hold, bias included."""
    return reduction * (A * A + abs(ox) * A + owmax * A + abs(ox) * owmax) + 128


def codes_amplitude(reduction: int, ox: int, owmax: int) -> int | None:
    """A: 128 halved until the bound holds; None where even 16 does not (the draw then takes fewer channels)."""
    A = 128
    while A >= 16:
        if bound(reduction, A, ox, owmax) < LIMIT:
            return A
        A //= 2
    return None


# ---- one axis ----------------------------------------------------------------------------------------------------------------------
def axis_taps(kind: str, n: int, k: int, s: int, p: int, d: int, out: int) -> list[int]:
    """How many taps of output index o read inside the image, for every o < out — by the definition of the operator, not by the
    kernels' ranges and phases."""
    if kind == "transposed":  # input i and tap t reach o = i * s - p + t * d
        return [sum(1 for t in range(k) if (o + p - t * d) % s == 0 and 0 <= (o + p - t * d) // s < n) for o in range(out)]
    return [sum(1 for t in range(k) if 0 <= o * s - p + t * d < n) for o in range(out)]


def _forward_axis(rng: random.Random, extent: int, wish: set[str]) -> tuple[int, int, int, int, int, int, int] | None:
    k, s, d = rng.randint(1, 5), rng.randint(1, 4), rng.randint(1, 3)
    if "long" in wish:
        s = min(s, rng.randint(1, 2))
    eff = d * (k - 1) + 1
    p = rng.randint(eff, eff + 1) if "notap" in wish else rng.randint(0, eff + 1)  # up to d * (k - 1) + 2
    lo = max(1, eff - 2 * p)
    if "one" in wish:
        hi = min(extent, eff - 2 * p + s - 1)  # (n + 2p - eff) // s == 0
    else:
        hi = extent
        if "long" in wish:
            lo = max(lo, extent * 2 // 3)
    if hi < lo:
        return None
    n = rng.randint(lo, hi)
    out = (n + 2 * p - eff) // s + 1
    return n, k, s, p, d, 0, out


def _transposed_axis(rng: random.Random, extent: int, wish: set[str]) -> tuple[int, int, int, int, int, int, int] | None:
    k, s, d = rng.randint(1, 5), rng.randint(1, 4), rng.randint(1, 3)
    if "gcd" in wish:
        s, d = rng.choice(((2, 2), (4, 2), (3, 3)))
    op = rng.randint(0, max(s, d) - 1)
    n = rng.randint(1, max(1, (extent if "long" in wish else extent // 2) // s))
    full = (n - 1) * s + d * (k - 1) + op + 1
    p_hi = min(d * (k - 1) + 2, (full - 1) // 2)
    p = rng.randint(0, p_hi)
    if "one" in wish:
        p = (full - 1) // 2
        if p > d * (k - 1) + 2:
            return None
    out = full - 2 * p
    return (n, k, s, p, d, op, out) if 1 <= out <= extent else None


# ---- the draws ---------------------------------------------------------------------------------------------------------------------
def _wishes(rng: random.Random, kind: str) -> set[str]:
    wish = set()
    for name, chance in (("notap", 0.3), ("one", 0.4), ("long", 0.45), ("longer", 0.15), ("gcd", 0.3 if kind == "transposed" else 0.0)):
        if rng.random() < chance:
            wish.add(name)
    return wish


def _geometry(rng: random.Random, family: Family, dims: int, wish: set[str]) -> tuple[int, list[tuple[int, ...]]]:
    """(B, one (n, k, s, p, d, op, out) per axis) with the wished properties, by rejection; every candidate is a valid call."""
    axis = _transposed_axis if family.kind == "transposed" else _forward_axis
    extent = family.extent[dims]
    for attempt in range(400):
        if attempt == 200:
            wish = set()  # (never reached with the committed seeds: the coverage test would say so)
        special = rng.sample(range(dims), dims)  # the axes the per-axis wishes land on
        per_axis = [set() for _ in range(dims)]
        for name, where in (("notap", special[0]), ("one", special[-1]), ("gcd", special[0])):
            if name in wish:
                per_axis[where].add(name)
        if wish & {"long", "longer"}:
            for i in range(dims):
                if "one" not in per_axis[i]:
                    per_axis[i].add("long")
        axes = [axis(rng, extent, per_axis[i]) for i in range(dims)]
        if any(a is None for a in axes):
            continue
        B = 3 if "longer" in wish else rng.randint(1, 3)
        positions = B * math.prod(a[6] for a in axes)
        if positions > MAX_OUTPUTS or ("long" in wish and positions <= 128) or ("longer" in wish and positions <= 256):
            continue
        counts = [axis_taps(family.kind, a[0], a[1], a[2], a[3], a[4], a[6]) for a in axes]
        if any(max(c) == 0 for c in counts):
            continue  # no position at all reads the image: the output is the bias
        if "notap" in wish and all(min(c) > 0 for c in counts):
            continue
        return B, axes
    raise AssertionError("no geometry")


@functools.lru_cache(maxsize=None)
def draws(name: str) -> tuple[Draw, ...]:
    family = FAMILIES[name]
    rng = random.Random(f"conv-exact-{name}")
    ranks = sorted(family.functional)
    out = []
    for index in range(N_DRAWS):
        dims = ranks[(index // 2) % len(ranks)]
        B, axes = _geometry(rng, family, dims, _wishes(rng, family.kind))
        size, kernel, stride, padding, dilation, output_padding, out_size = (tuple(a[i] for a in axes) for i in range(7))
        positions, taps = B * math.prod(out_size), math.prod(kernel)
        x_form, w_form = rng.choice(("none", "zero", "real")), rng.choice(("none", "zero", "real"))
        ox = rng.choice(X_OFFSETS) if x_form == "real" else 0
        owmax = rng.choice((5, 32)) if w_form == "real" else 0
        if family.kind == "depthwise":
            C, M = DEPTHWISE[index % len(DEPTHWISE)]
            if positions * C * M > MAX_OUTPUTS:
                fits = [(c, m) for c, m in DEPTHWISE if positions * c * m <= MAX_OUTPUTS]
                C, M = fits[index % len(fits)]
            OC, reduction = C * M, taps
        else:
            OC = OUT_CHANNELS[index % len(OUT_CHANNELS)]
            if positions * OC > MAX_OUTPUTS:
                OC = max(n for n in OUT_CHANNELS if positions * n <= MAX_OUTPUTS)
            fits = [c for c in CHANNELS if positions * OC * c * taps <= MAX_WORK and codes_amplitude(c * taps, ox, owmax) is not None]
            C = rng.choice(fits)
            reduction = C * taps
        per_channel = rng.random() < 0.5
        b0 = rng.randint(6, 8)
        mode = rng.choice(MODES)
        route = ("ops", "functional")[index % 2]
        out.append(Draw(
            family=name, index=index, dims=dims, B=B, C=C, OC=OC, size=size, kernel=kernel, stride=stride, padding=padding, dilation=dilation,
            output_padding=output_padding, out_size=out_size, A=codes_amplitude(reduction, ox, owmax), a=rng.randint(2, 6),
            b=tuple(b0 + rng.randrange(3) for _ in range(OC)) if per_channel else (b0,), x_form=x_form, ox=ox, w_form=w_form, owmax=owmax,
            bias=rng.choice((None, "f32", "bf16", "f16")), mode=mode, y_dt=rng.choice(("f32", "bf16", "f16")), bits=rng.choice((8, 4)),
            # (with both offsets real every value lies far to one side of zero: without an output offset every code would clamp)
            out_offset=rng.random() < 0.5 or (x_form == "real" and w_form == "real"), route=route, channels_last=route == "ops" and C % 16 == 0 and rng.random() < 0.75,
            seed=rng.getrandbits(31),
        ))
    return tuple(out)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    draw: Draw
    x_codes: torch.Tensor  # int8 [B, C, *size]
    w_codes: torch.Tensor  # int8, the operator's weight layout
    x_scale: torch.Tensor  # fp32 [1]
    x_offset: torch.Tensor | None  # fp32 [1]
    w_scale: torch.Tensor  # fp32 [1] or [OC]
    w_offset: torch.Tensor | None
    bias_m: torch.Tensor | None  # the integers m[n]: bias[n] = m[n] * sx * sw[n]
    bias: torch.Tensor | None  # fp32 (exact in bf16 and fp16 too)
    out_scale: torch.Tensor | None  # fp32 [1], a power of two
    out_offset: torch.Tensor | None  # fp32 [1], an integer
    y: torch.Tensor  # the float64 value
    expected: torch.Tensor  # in the output's dtype
    ties: int  # exact halves among the codes before rounding (the re-quantizing epilogue)


def weight_shape(d: Draw) -> tuple[int, ...]:
    kind = FAMILIES[d.family].kind
    if kind == "transposed":
        return (d.C, d.OC, *d.kernel)
    return (d.OC, 1 if kind == "depthwise" else d.C, *d.kernel)


def _per_output_channel(d: Draw, v: torch.Tensor) -> torch.Tensor:
    """[1] or [OC] against the weight."""
    shape = [1] * (d.dims + 2)
    if v.numel() > 1:
        shape[FAMILIES[d.family].oc_axis] = -1
    return v.reshape(shape)


def float64_convolution(d: Draw, x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None) -> torch.Tensor:
    """ATen's convolution of the family on float64 operands."""
    nnf = torch.nn.functional
    if FAMILIES[d.family].kind == "transposed":
        op = {1: nnf.conv_transpose1d, 2: nnf.conv_transpose2d}[d.dims]
        return op(x, w, bias, d.stride, d.padding, d.output_padding, 1, d.dilation)
    op = {1: nnf.conv1d, 2: nnf.conv2d, 3: nnf.conv3d}[d.dims]
    return op(x, w, bias, d.stride, d.padding, d.dilation, d.groups)


def code_range(bits: int) -> tuple[int, int]:
    return -(1 << (bits - 1)), (1 << (bits - 1)) - 1


def requantized(yr: torch.Tensor, scale: float, offset: float, bits: int) -> tuple[torch.Tensor, torch.Tensor]:
    """(clamp(rne(yr / s - o), lo, hi), yr / s - o) in float64: torch.round rounds halves to even."""
    lo, hi = code_range(bits)
    q = yr / scale - offset
    return torch.clamp(torch.round(q), lo, hi), q


def _output_quantizer(d: Draw, y: torch.Tensor, rng: random.Random) -> tuple[float, float | None, torch.Tensor, int]:
    """(scale, offset, expected codes, ties): ties counts the exact halves strictly inside the code range, where rne decides the
    code. The scale starts at the power of two at which the values (about the offset, an integer near their middle) fill one and a
    half code ranges, so a part of them clamps, and is halved until a tie occurs, down to twice the finest ``sx * sw[n]``; a scale
    at which the fp32 form of ``y / s - o`` would round before the rne (a value of many bits beside a far offset) is passed over:
    what remains is exact in fp32 as in float64. Where no scale gives a tie the first one stands."""
    yr = y.float().to(REAL[d.y_dt]).double()
    lo, hi = code_range(d.bits)
    if d.out_offset:
        spread = float(yr.max() - yr.min())
        middle = float(yr.max() + yr.min()) / 2
    else:
        spread, middle = 2 * float(yr.abs().max()), 0.0
    finest = -(d.a + max(d.b)) + 1
    first = max(math.ceil(math.log2(max(spread, 2.0 ** finest) / (1.5 * (hi - lo)))), finest)
    jitter = rng.randint(-2, 2)
    fallback = None
    for e in range(first, finest - 1, -1):
        scale = 2.0 ** e
        offset = float(round(middle / scale) + jitter) if d.out_offset else None
        codes, q = requantized(yr, scale, offset or 0.0, d.bits)
        q32 = yr.float() / torch.tensor(scale, dtype=torch.float32) - torch.tensor(offset or 0.0, dtype=torch.float32)
        if not torch.equal(torch.clamp(torch.round(q32), lo, hi).double(), codes) or abs(offset or 0.0) >= LIMIT:
            continue
        ties = int((((q - torch.floor(q)) == 0.5) & (q > lo) & (q < hi)).sum())
        if fallback is None:
            fallback = (scale, offset, codes.to(torch.int8), ties)
        if ties > 0:
            return scale, offset, codes.to(torch.int8), ties
    assert fallback is not None, str(d)
    return fallback  # (an output of a few elements: no scale puts a half inside the range)


@functools.lru_cache(maxsize=None)
def case(name: str, index: int) -> Case:
    d = draws(name)[index]
    rng = random.Random(d.seed)
    g = torch.Generator().manual_seed(d.seed)
    x_codes = torch.randint(-d.A, d.A, (d.B, d.C, *d.size), generator=g, dtype=torch.int8)
    w_codes = torch.randint(-d.A, d.A, weight_shape(d), generator=g, dtype=torch.int8)
    x_scale = torch.tensor([2.0 ** -d.a])
    w_scale = torch.tensor([2.0 ** -e for e in d.b])
    x_offset = None if d.x_form == "none" else torch.tensor([float(d.ox)])
    if d.w_form == "none":
        w_offset = None
    elif d.w_form == "zero":
        w_offset = torch.zeros(len(d.b))
    else:
        w_offset = torch.randint(-d.owmax, d.owmax + 1, (len(d.b),), generator=g).float()
        w_offset[rng.randrange(len(d.b))] = float(rng.choice((-d.owmax, d.owmax)))  # the largest one occurs
    bias_m = bias = None
    if d.bias is not None:
        bias_m = torch.randint(-128, 129, (d.OC,), generator=g).double()
        bias = (bias_m * x_scale.double() * w_scale.double()).float()  # exact: an 8-bit integer times a power of two
    x = (x_codes.double() + d.ox) * x_scale.double()
    ow = torch.zeros(1, dtype=torch.float64) if w_offset is None else w_offset.double()
    w = (w_codes.double() + _per_output_channel(d, ow)) * _per_output_channel(d, w_scale.double())
    y = float64_convolution(d, x, w, None if bias is None else bias.double())
    assert tuple(y.shape) == (d.B, d.OC, *d.out_size), (str(d), tuple(y.shape))
    out_scale = out_offset = None
    ties = 0
    if d.mode == "int8":
        scale, offset, expected, ties = _output_quantizer(d, y, rng)
        out_scale = torch.tensor([scale], dtype=torch.float32)
        out_offset = None if offset is None else torch.tensor([offset], dtype=torch.float32)
    else:
        expected = y.float().to(REAL[d.mode])  # fp32 holds y exactly (the CPU test asserts it): one rounding to bf16 / fp16
    return Case(d, x_codes, w_codes, x_scale, x_offset, w_scale, w_offset, bias_m, bias, out_scale, out_offset, y, expected, ties)


# ---- what a draw covers --------------------------------------------------------------------------------------------------------------
def tap_counts(d: Draw) -> list[list[int]]:
    kind = FAMILIES[d.family].kind
    return [axis_taps(kind, d.size[i], d.kernel[i], d.stride[i], d.padding[i], d.dilation[i], d.out_size[i]) for i in range(d.dims)]


def phase_without_tap(d: Draw) -> bool:
    """Transposed: a residue r < stride of some axis that no tap reaches — no t < k with stride dividing r + p - t * d."""
    return any(any(all((r + p - t * dil) % s for t in range(k)) for r in range(s))
               for k, s, p, dil in zip(d.kernel, d.stride, d.padding, d.dilation))


# ---- running a case ------------------------------------------------------------------------------------------------------------------
def _as_2d(d: Draw, t: torch.Tensor) -> torch.Tensor:
    return t.unsqueeze(2) if d.dims == 1 else t


def _pair(d: Draw, v: tuple[int, ...], fill: int) -> tuple[int, ...]:
    return (fill, *v) if d.dims == 1 else v


def run_ops(c: Case, device: str, ops: Any) -> torch.Tensor:
    """The family's ``ops`` entry on the raw codes (looked up on `ops` at the call, so a counting wrapper sees it)."""
    d = c.draw
    to = lambda t: None if t is None else t.to(device)  # noqa: E731
    x = _as_2d(d, c.x_codes).to(device)
    if d.channels_last:
        x = x.to(memory_format=torch.channels_last_3d if d.dims == 3 else torch.channels_last)
    w = _as_2d(d, c.w_codes).to(device)
    bias = None if c.bias is None else c.bias.to(device, REAL[d.bias])
    geometry = [_pair(d, d.stride, 1), _pair(d, d.padding, 0)]
    if FAMILIES[d.family].kind == "transposed":
        geometry.append(_pair(d, d.output_padding, 0))
    geometry.append(_pair(d, d.dilation, 1))
    if d.mode == "int8":
        out = dict(out_scale=to(c.out_scale), out_offset=to(c.out_offset), out_num_bits=float(d.bits), requant_from=REAL[d.y_dt])
    else:
        out = dict(out_dtype=REAL[d.mode])
    y = getattr(ops, FAMILIES[d.family].entry)(x, w, to(c.x_scale), to(c.x_offset), to(c.w_scale), to(c.w_offset), bias, *geometry, **out)
    return y.squeeze(2) if d.dims == 1 else y


def quantized(codes: torch.Tensor, scale: torch.Tensor, offset: torch.Tensor | None, granularity: Any, data_dtype: torch.dtype) -> ff.QuantizedTensor:
    """The QuantizedTensor a static 8-bit quantizer with these parameters returns for data of `data_dtype` — around the given codes."""
    params = StaticAffineQuantParams(scale=scale, offset=offset, num_bits=8, granularity=granularity, quantized_dtype=torch.int8,
                                     dequantize_dtype=data_dtype)
    return ff.QuantizedTensor(codes, QuantizationContext(AffineQuantizationFunction, params))


def output_quantizer(c: Case, device: str) -> ff.nn.LinearQuantizer:
    d = c.draw
    q = ff.nn.LinearQuantizer(d.bits, symmetric=c.out_offset is None, allow_one_sided=False, quantized_dtype=torch.int8, device=device)
    q.quantization_range = (torch.tensor([-1.0], device=device), torch.tensor([1.0], device=device))
    with torch.no_grad():
        q.scale.copy_(c.out_scale)
        if c.out_offset is not None:
            q.offset.copy_(c.out_offset)
    return q


def run_functional(c: Case, device: str, data_dtype: torch.dtype | None = None, fused_output: bool = True) -> Any:
    """The family's ``ff.nn.functional`` operator on QuantizedTensors of the draw's data dtype (or `data_dtype`), with the output
    quantizer where the draw has one and `fused_output`."""
    d = c.draw
    family = FAMILIES[d.family]
    dt = data_dtype or REAL[d.y_dt if d.mode == "int8" else d.mode]
    to = lambda t: None if t is None else t.to(device)  # noqa: E731
    xq = quantized(c.x_codes.to(device), to(c.x_scale), to(c.x_offset), ff.PerTensor(), dt)
    granularity = ff.PerChannel(family.oc_axis) if len(d.b) > 1 else ff.PerTensor()
    wq = quantized(c.w_codes.to(device), to(c.w_scale), to(c.w_offset), granularity, dt)
    bias = None if c.bias is None else c.bias.to(device, dt)
    kwargs: dict[str, Any] = dict(stride=d.stride, padding=d.padding, dilation=d.dilation, groups=d.groups, strict_quantization=False)
    if family.kind == "transposed":
        kwargs["output_padding"] = d.output_padding
    if d.mode == "int8" and fused_output:
        kwargs["output_quantizer"] = output_quantizer(c, device)
    return getattr(ff.nn.functional, family.functional[d.dims])(xq, wq, bias, **kwargs)


def first_difference(got: torch.Tensor, want: torch.Tensor) -> str:
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"{tuple(got.shape)} {got.dtype} against {tuple(want.shape)} {want.dtype}"
    differ = (got != want).nonzero()
    if differ.numel() == 0:
        return "no element differs (NaN?)"
    at = tuple(int(i) for i in differ[0])
    return f"{differ.shape[0]} of {want.numel()} differ, first at {at}: {got[at].item()!r} against {want[at].item()!r}"
