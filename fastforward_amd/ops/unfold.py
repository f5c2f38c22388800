"""The reference's quantized unfold (im2col) as a one-pass kernel with A1 fused in (csrc/ffq_unfold.hip, include/ffq_unfold.h), with
its quantized input dequantized in registers (A2) and up to three static per-tensor output quantizers (reference ff.nn.functional
through _gen/fallback.py: unfold :1650).

An input given as codes comes with ``(scale, offset)``: int8 or value-dtype codes with fp32 parameters — one pair for the tensor, or
one per channel. A strided or misaligned view reaches the kernel as an aligned copy (``ops._base._dense``). The function returns
``(value or None, [codes per quantizer])``; the value has the data dtype and is contiguous in the shape ATen gives."""

from __future__ import annotations

import ctypes

from typing import Any

import torch

from fastforward_amd.ops import _base
from fastforward_amd.ops._base import _ptr, _tag
from fastforward_amd.ops.modules import Quantizers, _entry, _operand
from fastforward_amd.ops.producers import _fan

Dequant = tuple[torch.Tensor, torch.Tensor | None]
AXIS_LIMIT = 2**24  # the entry point's limit on every extent, window, stride, dilation and padding


def pair(value: Any) -> tuple[int, int] | None:
    """`value` as (along H, along W): an int for both, or a pair of ints; None for anything else."""
    items = tuple(value) if isinstance(value, (tuple, list, torch.Size)) else (value, value)
    if len(items) != 2 or any(isinstance(v, bool) or not isinstance(v, int) for v in items):
        return None
    return items


def output_extents(H: int, W: int, kernel: tuple[int, int], dilation: tuple[int, int], padding: tuple[int, int],
                   stride: tuple[int, int]) -> tuple[int, int] | None:
    """(OH, OW) as ATen's im2col computes them, or None for geometry the entry point refuses."""
    if min(kernel) < 1 or min(dilation) < 1 or min(stride) < 1 or min(padding) < 0:
        return None
    if max(H, W, *kernel, *dilation, *padding, *stride) > AXIS_LIMIT:
        return None
    spans = [d * (k - 1) + 1 for d, k in zip(dilation, kernel)]
    padded = [H + 2 * padding[0], W + 2 * padding[1]]
    if any(span > size for span, size in zip(spans, padded)):
        return None
    return tuple((size - span) // s + 1 for size, span, s in zip(padded, spans, stride))


def unfold_quantize(
    x: torch.Tensor,
    kernel_size: Any,
    dilation: Any = 1,
    padding: Any = 0,
    stride: Any = 1,
    quantizers: Quantizers = (),
    num_bits: float = 8.0,
    dtype: torch.dtype | None = None,
    dequant: Dequant | None = None,
    per_channel: bool = False,
    want_value: bool = True,
) -> tuple[torch.Tensor | None, list[torch.Tensor]]:
    """``F.unfold(x, kernel_size, dilation, padding, stride)`` + A1, one pass. `x` is ``[B, C, H, W]`` (or ``[C, H, W]``, which runs
    as ``B = 1`` and returns ``[C * taps, L]``), plain (`dtype`) or, with ``dequant = (scale, offset)``, codes (int8 or `dtype`)
    with one parameter pair, or with `per_channel` one pair per channel. A position in the padding holds +0.0 (and the codes of
    0.0). Geometry the kernel does not take raises before a launch."""
    dtype = dtype or x.dtype
    if x.dim() not in (3, 4):
        raise RuntimeError(f"unfold_quantize: the input is [B, C, H, W] or [C, H, W], got {tuple(x.shape)}")
    geometry = [pair(v) for v in (kernel_size, dilation, padding, stride)]
    if None in geometry:
        raise RuntimeError("unfold_quantize: kernel_size, dilation, padding and stride are ints or pairs of ints")
    kernel, dil, pad, step = geometry
    B = x.shape[0] if x.dim() == 4 else 1
    C, H, W = x.shape[-3:]
    extents = output_extents(H, W, kernel, dil, pad, step)
    if extents is None:
        raise RuntimeError(f"unfold_quantize: kernel_size {kernel}, dilation {dil}, padding {pad}, stride {step} do not fit an image of {H} x {W}")
    xc, s, o, many = _operand(x, dtype, C if per_channel else 1, dequant, "unfold_quantize")
    lib, stream = _base._prepare(xc, s, o, *[t for q in quantizers for t in q])
    rows, L = C * kernel[0] * kernel[1], extents[0] * extents[1]
    shape = (B, rows, L) if x.dim() == 4 else (rows, L)
    out = torch.empty(shape, dtype=dtype, device=xc.device) if want_value else None
    fan, codes, keep = _fan(quantizers, num_bits, shape, xc.device)
    lib.check(
        _entry(lib, "ffq_unfold_quantize")(
            _ptr(xc), _tag(xc.dtype), _ptr(s), _ptr(o), int(many), _tag(dtype), B, C, H, W, *kernel, *dil, *pad, *step,
            _ptr(out), ctypes.byref(fan), stream,
        )
    )
    del keep
    return out, codes
