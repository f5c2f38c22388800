"""The reference's quantized avg_pool1d / avg_pool2d / max_pool2d and nearest interpolate as one-pass kernels with A1 fused in
(csrc/ffq_pool.hip), each with its quantized input dequantized in registers (A2) and up to three static per-tensor output
quantizers (reference ff.nn.functional through _gen/fallback.py: avg_pool1d :505, avg_pool2d :542, max_pool2d :1574,
interpolate :1611).

The input is ``[B, C, H, W]`` (the 1-D forms come as ``[B, C, 1, L]``). Given as codes it comes with ``dequant=(scale, offset)``:
int8 or value-dtype codes with fp32 parameters, one pair for the tensor or one per channel. Each function returns
``(value or None, [codes per quantizer])``; the value has the data dtype and the shape the ATen op gives.

``avg_pool3d`` (reference _gen/fallback.py:579) is csrc/ffq_pool3d.hip's one pass over ``[B, C, D, H, W]`` (include/ffq_3d.h)."""

from __future__ import annotations

import ctypes

import torch

from fastforward_amd.exceptions import BackendError
from fastforward_amd.ops import _base
from fastforward_amd.ops._base import _ptr, _tag
from fastforward_amd.ops.modules import Quantizers, _entry, _operand
from fastforward_amd.ops.producers import _fan

POOL_MODES = {"avg": 0, "avg_exclude_pad": 1, "max": 2}
NEAREST_MODES = {"nearest": 0, "nearest-exact": 1}


def pooled_size(size: int, kernel: int, pad: int, stride: int, dilation: int = 1, ceil_mode: bool = False) -> int:
    """ATen's ``pooling_output_shape``: the last window starts inside the input or its left padding."""
    num = size + 2 * pad - dilation * (kernel - 1) - 1 + (stride - 1 if ceil_mode else 0)
    out = num // stride + 1
    if ceil_mode and (out - 1) * stride >= size + pad:
        out -= 1
    return out


def _planes(x: torch.Tensor, what: str) -> tuple[int, int, int, int]:
    if x.dim() != 4:
        raise RuntimeError(f"{what}: the input is [B, C, H, W], got {x.dim()} dims")
    return tuple(x.shape)


def _pair(v, what: str) -> tuple[int, int]:
    h, w = v
    if isinstance(h, bool) or isinstance(w, bool) or not isinstance(h, int) or not isinstance(w, int):
        raise RuntimeError(f"{what} is a pair of ints, got {v!r}")
    return h, w


def pool2d_quantize(
    mode: str,
    x: torch.Tensor,
    kernel_size: tuple[int, int],
    stride: tuple[int, int],
    padding: tuple[int, int] = (0, 0),
    dilation: tuple[int, int] = (1, 1),
    ceil_mode: bool = False,
    quantizers: Quantizers = (),
    num_bits: float = 8.0,
    dtype: torch.dtype | None = None,
    dequant: tuple[torch.Tensor, torch.Tensor | None] | None = None,
    want_value: bool = True,
) -> tuple[torch.Tensor | None, list[torch.Tensor]]:
    """``F.avg_pool2d`` (mode="avg": count_include_pad, "avg_exclude_pad": without) or ``F.max_pool2d`` (mode="max") of
    `x` [B, C, H, W] + A1, one pass; every geometry argument is an (h, w) pair. `x` plain or codes with per-tensor or per-channel
    parameters. Geometry ATen refuses raises ``RuntimeError`` before a launch."""
    if mode not in POOL_MODES:
        raise RuntimeError(f"pool2d_quantize: mode is one of {sorted(POOL_MODES)}, got {mode!r}")
    dtype = dtype or x.dtype
    B, C, H, W = _planes(x, "pool2d_quantize")
    (kh, kw), (sh, sw) = _pair(kernel_size, "kernel_size"), _pair(stride, "stride")
    (ph, pw), (dh, dw) = _pair(padding, "padding"), _pair(dilation, "dilation")
    if min(kh, kw, sh, sw, dh, dw) < 1 or min(ph, pw) < 0 or 0 in (H, W):
        raise RuntimeError("pool2d_quantize: kernel size, stride and dilation must be positive, padding non-negative, the map not empty")
    OH, OW = pooled_size(H, kh, ph, sh, dh, ceil_mode), pooled_size(W, kw, pw, sw, dw, ceil_mode)
    xc, s, o, per_channel = _operand(x, dtype, C, dequant, "pool2d_quantize")
    lib, stream = _base._prepare(xc, s, o, *[t for q in quantizers for t in q])
    shape = (B, C, max(OH, 0), max(OW, 0))
    value = torch.empty(shape, dtype=dtype, device=xc.device) if want_value else None
    fan, codes, keep = _fan(quantizers, num_bits, shape, xc.device)
    lib.check(
        _entry(lib, "ffq_pool2d_quantize")(
            POOL_MODES[mode], _ptr(xc), _tag(xc.dtype), _ptr(s), _ptr(o), C if per_channel else 0, _tag(dtype), B * C, H, W, kh, kw, sh, sw,
            ph, pw, dh, dw, int(bool(ceil_mode)), OH, OW, _ptr(value), ctypes.byref(fan), stream,
        )
    )
    del keep
    return value, codes


def _triple(v, what: str) -> tuple[int, int, int]:
    t = tuple(v)
    if len(t) != 3 or any(isinstance(e, bool) or not isinstance(e, int) for e in t):
        raise RuntimeError(f"{what} is a triple of ints, got {v!r}")
    return t  # type: ignore[return-value]


def pool3d_quantize(
    mode: str,
    x: torch.Tensor,
    kernel_size: tuple[int, int, int],
    stride: tuple[int, int, int],
    padding: tuple[int, int, int] = (0, 0, 0),
    ceil_mode: bool = False,
    quantizers: Quantizers = (),
    num_bits: float = 8.0,
    dtype: torch.dtype | None = None,
    dequant: tuple[torch.Tensor, torch.Tensor | None] | None = None,
    want_value: bool = True,
) -> tuple[torch.Tensor | None, list[torch.Tensor]]:
    """``F.avg_pool3d`` (mode="avg": count_include_pad, "avg_exclude_pad": without) of `x` [B, C, D, H, W] + A1, one pass; every
    geometry argument is a (d, h, w) triple. `x` plain or codes with per-tensor or per-channel parameters. Geometry ATen refuses
    raises before a launch; a library without the entry point raises ``BackendError`` ("not covered")."""
    if mode not in ("avg", "avg_exclude_pad"):
        raise RuntimeError(f"pool3d_quantize: mode is 'avg' or 'avg_exclude_pad', got {mode!r}")
    dtype = dtype or x.dtype
    if x.dim() != 5:
        raise RuntimeError(f"pool3d_quantize: the input is [B, C, D, H, W], got {x.dim()} dims")
    B, C, D, H, W = x.shape
    k, s_, p = _triple(kernel_size, "kernel_size"), _triple(stride, "stride"), _triple(padding, "padding")
    if min(*k, *s_) < 1 or min(p) < 0 or 0 in (D, H, W):
        raise RuntimeError("pool3d_quantize: kernel size and stride must be positive, padding non-negative, the map not empty")
    size = [pooled_size(n, ki, pi, si, 1, ceil_mode) for n, ki, pi, si in zip((D, H, W), k, p, s_)]
    xc, s, o, per_channel = _operand(x, dtype, C, dequant, "pool3d_quantize")
    lib, stream = _base._prepare(xc, s, o, *[t for q in quantizers for t in q])
    entry = getattr(lib, "ffq_pool3d_quantize", None)
    if entry is None:
        raise BackendError("not covered: the loaded library does not export ffq_pool3d_quantize (include/ffq_3d.h)")
    shape = (B, C, *(max(n, 0) for n in size))
    value = torch.empty(shape, dtype=dtype, device=xc.device) if want_value else None
    fan, codes, keep = _fan(quantizers, num_bits, shape, xc.device)
    lib.check(
        entry(
            POOL_MODES[mode], _ptr(xc), _tag(xc.dtype), _ptr(s), _ptr(o), C if per_channel else 0, _tag(dtype), B * C, D, H, W, *k, *s_, *p,
            int(bool(ceil_mode)), *size, _ptr(value), ctypes.byref(fan), stream,
        )
    )
    del keep
    return value, codes


def upsample_nearest_quantize(
    x: torch.Tensor,
    size: tuple[int, int],
    scale_factor: tuple[float, float] | None = None,
    mode: str = "nearest",
    quantizers: Quantizers = (),
    num_bits: float = 8.0,
    dtype: torch.dtype | None = None,
    dequant: tuple[torch.Tensor, torch.Tensor | None] | None = None,
    want_value: bool = True,
) -> tuple[torch.Tensor | None, list[torch.Tensor]]:
    """``F.interpolate(x, mode="nearest" / "nearest-exact")`` of `x` [B, C, H, W] to `size` (OH, OW) + A1, one pass.
    `scale_factor` is the pair the caller gave ``F.interpolate`` (ATen then maps indices by 1 / scale_factor), or None when it gave
    ``size`` (indices map by in / out). `x` plain or codes with per-tensor or per-channel parameters."""
    if mode not in NEAREST_MODES:
        raise RuntimeError(f"upsample_nearest_quantize: mode is one of {sorted(NEAREST_MODES)}, got {mode!r}")
    dtype = dtype or x.dtype
    B, C, H, W = _planes(x, "upsample_nearest_quantize")
    OH, OW = _pair(size, "size")
    fh, fw = (0.0, 0.0) if scale_factor is None else (float(scale_factor[0]), float(scale_factor[1]))
    if OH < 1 or OW < 1 or 0 in (H, W):
        raise RuntimeError(f"upsample_nearest_quantize: input [{H}, {W}] and output [{OH}, {OW}] sizes should be greater than 0")
    xc, s, o, per_channel = _operand(x, dtype, C, dequant, "upsample_nearest_quantize")
    lib, stream = _base._prepare(xc, s, o, *[t for q in quantizers for t in q])
    shape = (B, C, OH, OW)
    value = torch.empty(shape, dtype=dtype, device=xc.device) if want_value else None
    fan, codes, keep = _fan(quantizers, num_bits, shape, xc.device)
    lib.check(
        _entry(lib, "ffq_upsample_nearest_quantize")(
            _ptr(xc), _tag(xc.dtype), _ptr(s), _ptr(o), C if per_channel else 0, _tag(dtype), B * C, H, W, OH, OW, fh, fw,
            NEAREST_MODES[mode], _ptr(value), ctypes.byref(fan), stream,
        )
    )
    del keep
    return value, codes
