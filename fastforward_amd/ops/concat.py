"""The reference's quantized cat and pad as one-pass kernels with A1 fused in (csrc/ffq_concat.hip), each with its quantized
inputs dequantized in registers (A2) and up to three static per-tensor output quantizers (reference ff.nn.functional through
_gen/fallback.py: cat :1453, pad :1546).

An input given as codes comes with ``(scale, offset)``: int8 or value-dtype codes with fp32 parameters — one pair per input of a
``cat``, one pair for the tensor or one per channel (dim 1) for ``pad``. Each function returns
``(value or None, [codes per quantizer])``; the value has the data dtype and the shape and (contiguous) strides ATen gives."""

from __future__ import annotations

import ctypes
import math

from typing import Sequence

import torch

from fastforward_amd._cabi import FFQ_CAT_MAX_INPUTS, CatInputs
from fastforward_amd.ops import _base
from fastforward_amd.ops._base import _ptr, _tag
from fastforward_amd.ops.modules import Quantizers, _entry, _operand
from fastforward_amd.ops.producers import _fan

PAD_MODES = {"constant": 0, "reflect": 1, "replicate": 2}
Dequant = tuple[torch.Tensor, torch.Tensor | None]


def fill_bits(value: float | None, dtype: torch.dtype) -> int:
    """The 16 bits a constant ``F.pad`` writes into a `dtype` tensor for the Python number `value` (None: 0), found on the host by
    padding a one-element host tensor: ATen converts the number before any kernel runs, the same way for every device
    (double -> fp32 -> `dtype`, two roundings — ``1.00390625 + 2**-30`` is 1.0 in bf16, not 1.0078125; checked against ``F.pad`` on
    the MI355X). Raises ATen's error for a finite number beyond `dtype`'s range."""
    filled = torch.nn.functional.pad(torch.zeros(1, dtype=dtype), (1, 0), "constant", value)[:1]
    return int(filled.view(torch.int16).item()) & 0xFFFF


def cat_quantize(
    tensors: Sequence[torch.Tensor],
    dim: int = 0,
    quantizers: Quantizers = (),
    num_bits: float = 8.0,
    dtype: torch.dtype | None = None,
    dequant: Sequence[Dequant | None] | None = None,
    want_value: bool = True,
) -> tuple[torch.Tensor | None, list[torch.Tensor]]:
    """``torch.cat(tensors, dim)`` + A1, one pass per 8 inputs (more inputs are further launches into column ranges of the same
    result: no temporary). Every input is plain (`dtype`) or, with ``dequant[i] = (scale, offset)``, codes (int8 or `dtype`) with
    its own per-tensor parameters. Inputs of one rank whose sizes agree off `dim`, none of them empty."""
    tensors = list(tensors)
    if not tensors:
        raise RuntimeError("cat_quantize: expected a non-empty list of tensors")
    dequant = list(dequant) if dequant is not None else [None] * len(tensors)
    if len(dequant) != len(tensors):
        raise RuntimeError(f"cat_quantize: {len(tensors)} tensors but {len(dequant)} dequant entries")
    first = tensors[0]
    dtype = dtype or first.dtype
    ndim = first.dim()
    if isinstance(dim, bool) or not isinstance(dim, int) or not -ndim <= dim < ndim:
        raise RuntimeError(f"cat_quantize: dim {dim!r} is out of range for {ndim} dims")
    dim %= ndim
    off = tuple(first.shape[:dim]), tuple(first.shape[dim + 1:])
    outer, inner = math.prod(off[0]), math.prod(off[1])
    operands, extent = [], 0
    for t, d in zip(tensors, dequant):
        if t.dim() != ndim or (tuple(t.shape[:dim]), tuple(t.shape[dim + 1:])) != off or t.numel() == 0:
            raise RuntimeError(f"cat_quantize: inputs are non-empty and agree off dim {dim}: {tuple(first.shape)} and {tuple(t.shape)}")
        tc, s, o, _ = _operand(t, dtype, 1, d, "cat_quantize")
        operands.append((tc, s, o, t.shape[dim] * inner))
        extent += t.shape[dim]
    flat = [t for op in operands for t in op[:3]]
    lib, stream = _base._prepare(*flat, *[t for q in quantizers for t in q])
    shape = (*off[0], extent, *off[1])
    device = operands[0][0].device
    value = torch.empty(shape, dtype=dtype, device=device) if want_value else None
    fan, codes, keep = _fan(quantizers, num_bits, shape, device)
    entry = _entry(lib, "ffq_cat_quantize")
    col = 0
    for at in range(0, len(operands), FFQ_CAT_MAX_INPUTS):
        batch = operands[at:at + FFQ_CAT_MAX_INPUTS]
        inputs = CatInputs.make([(_ptr(tc), _tag(tc.dtype), _ptr(s), _ptr(o), run) for tc, s, o, run in batch])
        lib.check(entry(ctypes.byref(inputs), _tag(dtype), outer, extent * inner, col, _ptr(value), ctypes.byref(fan), stream))
        col += sum(run for *_, run in batch)
    del keep
    return value, codes


def padded_shape(shape: Sequence[int], pad: Sequence[int]) -> tuple[int, ...]:
    """The shape ``F.pad`` gives: `pad` holds (left, right) pairs from the last dimension backwards."""
    out = list(shape)
    for d in range(len(pad) // 2):
        out[-1 - d] += pad[2 * d] + pad[2 * d + 1]
    return tuple(out)


def pad_quantize(
    x: torch.Tensor,
    pad: Sequence[int],
    mode: str = "constant",
    value: float | None = None,
    quantizers: Quantizers = (),
    num_bits: float = 8.0,
    dtype: torch.dtype | None = None,
    dequant: Dequant | None = None,
    want_value: bool = True,
) -> tuple[torch.Tensor | None, list[torch.Tensor]]:
    """``F.pad(x, pad, mode, value)`` + A1, one pass, on the last one, two or three dimensions. mode "constant" (any `value`,
    negative pads crop), "reflect" or "replicate" (non-negative pads; reflect pads smaller than the extent). `x` plain or codes with
    per-tensor parameters, or one pair per channel (dim 1) when dim 1 is not padded. Geometry the kernel does not take raises before
    a launch."""
    if mode not in PAD_MODES:
        raise RuntimeError(f"pad_quantize: mode is one of {sorted(PAD_MODES)}, got {mode!r}")
    pad = tuple(pad)
    if len(pad) not in (2, 4, 6) or len(pad) // 2 > x.dim() or any(isinstance(p, bool) or not isinstance(p, int) for p in pad):
        raise RuntimeError(f"pad_quantize: pad holds one, two or three (left, right) pairs of ints for the last dimensions, got {pad!r}")
    if mode != "constant" and value not in (None, 0):
        raise RuntimeError(f'pad_quantize: padding mode "{mode}" takes no value')
    dtype = dtype or x.dtype
    k = len(pad) // 2
    lead = tuple(x.shape[:x.dim() - k])
    extents = [1, 1, 1]  # D0, D1, D2
    for d in range(k):
        extents[d] = x.shape[-1 - d]
    pads = list(pad) + [0] * (6 - len(pad))
    shape = padded_shape(x.shape, pad)
    if x.numel() == 0 or min(shape) < 1:
        raise RuntimeError(f"pad_quantize: the input {tuple(x.shape)} and the result {shape} are not empty")
    channels = x.shape[1] if x.dim() >= 2 else 1
    xc, s, o, per_channel = _operand(x, dtype, channels, dequant, "pad_quantize")
    if per_channel and x.dim() - k < 2:
        raise RuntimeError("pad_quantize: per-channel parameters need a channel dimension (dim 1) that is not padded")
    lib, stream = _base._prepare(xc, s, o, *[t for q in quantizers for t in q])
    out = torch.empty(shape, dtype=dtype, device=xc.device) if want_value else None
    fan, codes, keep = _fan(quantizers, num_bits, shape, xc.device)
    lib.check(
        _entry(lib, "ffq_pad_quantize")(
            PAD_MODES[mode], _ptr(xc), _tag(xc.dtype), _ptr(s), _ptr(o), channels if per_channel else 0,
            math.prod(lead[2:]) if per_channel else 0, _tag(dtype), math.prod(lead), extents[2], extents[1], extents[0],
            (ctypes.c_int64 * 6)(*pads), fill_bits(value, dtype), _ptr(out), ctypes.byref(fan), stream,
        )
    )
    del keep
    return out, codes
