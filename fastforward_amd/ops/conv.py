"""The W8A8 convolution on int8 codes (csrc/ffq_conv.hip): what QuantizedConv2d / QuantizedConv1d run on the device instead of the
reference's fallback.conv2d / fallback.conv1d (_gen/fallback.py:116-214: A2 of input and weight, F.conv2d, the output quantizer),
its transposed twin (csrc/ffq_conv_transpose.hip; fallback.conv_transpose1d / conv_transpose2d, _gen/fallback.py:346-449), and the
3-D convolution (csrc/ffq_conv3d.hip; fallback.conv3d, _gen/fallback.py:218-265; include/ffq_3d.h), and the depthwise convolution
(groups == C: csrc/ffq_depthwise.hip, a direct stencil; include/ffq_depthwise.h)."""

from __future__ import annotations

import math

from typing import Any, Sequence

import torch

from fastforward_amd.exceptions import BackendError
from fastforward_amd.ops import _base
from fastforward_amd.ops._base import _dense, _ptr, _tag, _workspace

_REAL = (torch.float32, torch.bfloat16, torch.float16)
_TUPLE = {2: "pair", 3: "triple"}


def _ints(v: int | Sequence[int], n: int, what: str, op: str) -> tuple[int, ...]:
    """`v` as n ints: an int repeats."""
    if isinstance(v, int):
        return (v,) * n
    t = tuple(int(e) for e in v)
    if len(t) != n:
        raise RuntimeError(f"{op}: {what} is an int or a {_TUPLE[n]}, got {v!r}")
    return t


def _f32(t: torch.Tensor | None) -> torch.Tensor | None:
    return None if t is None else t.detach().reshape(-1).to(torch.float32).contiguous()


def _check_codes(op: str, layout: str, rank: int, x_codes: torch.Tensor, w_codes: torch.Tensor) -> None:
    """int8 codes of `rank` dimensions (`layout` names them in the message): what a wrapper needs before it unpacks the shapes."""
    if x_codes.dtype != torch.int8 or w_codes.dtype != torch.int8:
        raise TypeError(f"{op} expects int8 codes")
    if x_codes.dim() != rank or w_codes.dim() != rank:
        raise RuntimeError(f"{op}: {layout}, got {tuple(x_codes.shape)} and {tuple(w_codes.shape)}")


def _operands(op: str, OC: int, channels_last: torch.memory_format | None, x_codes: torch.Tensor, w_codes: torch.Tensor,
              x_scale: torch.Tensor, x_offset: torch.Tensor | None, w_scale: torch.Tensor, w_offset: torch.Tensor | None,
              bias: torch.Tensor | None, out_dtype: torch.dtype, out_scale: torch.Tensor | None, out_offset: torch.Tensor | None,
              requant_from: torch.dtype | None) -> tuple[Any, ...]:
    """The validation and normalisation the convolution wrappers share, after :func:`_check_codes`: dense codes — the input in
    `channels_last` where the caller names that format, the codes already are dense in it and C % 16 == 0 (the kernels' 16-channel
    runs), else contiguous —, fp32 flattened parameters with one pair for the input, 1 or `OC` pairs for the weight and a
    per-tensor output quantizer, a real output dtype without one, a bias [OC] of a real dtype. Touches no library. Returns
    (input codes, weight codes, x_scale, x_offset, w_scale, w_offset, bias, out_scale, out_offset, whether the input codes are in
    `channels_last`, the dtype of the tensor the launch writes — int8 with an output quantizer —, and `y_dt`: the tag of the real
    dtype that quantizer rounds from, 0 without one)."""
    cl = (channels_last is not None and not x_codes.is_contiguous() and x_codes.shape[1] % 16 == 0
          and x_codes.is_contiguous(memory_format=channels_last))
    xc = _dense(x_codes.detach(), channels_last if cl else torch.contiguous_format)
    wc = _dense(w_codes.detach())
    xs, xo, ws_, wo, os_, oo = _f32(x_scale), _f32(x_offset), _f32(w_scale), _f32(w_offset), _f32(out_scale), _f32(out_offset)
    if xs.numel() != 1 or (xo is not None and xo.numel() != 1):
        raise RuntimeError(f"{op}: the input has one parameter pair (per-tensor)")
    if ws_.numel() not in (1, OC) or (wo is not None and wo.numel() != ws_.numel()):
        raise RuntimeError(f"{op}: the weight has 1 or {OC} parameter pairs, got {ws_.numel()}")
    if os_ is not None and (os_.numel() != 1 or (oo is not None and oo.numel() != 1)):
        raise RuntimeError(f"{op}: the output quantizer is per tensor")
    if os_ is None and out_dtype not in _REAL:
        raise RuntimeError(f"{op}: a real-valued output is f32, bf16 or f16, got {out_dtype}")
    bias_c = None if bias is None else bias.detach().reshape(-1).contiguous()
    if bias_c is not None and (bias_c.numel() != OC or bias_c.dtype not in _REAL):
        raise RuntimeError(f"{op}: the bias is [{OC}] of f32, bf16 or f16")
    y_dt = _tag(requant_from or torch.bfloat16) if os_ is not None else 0
    return xc, wc, xs, xo, ws_, wo, bias_c, os_, oo, cl, torch.int8 if os_ is not None else out_dtype, y_dt


def _entry(symbol: str, header: str, *tensors: torch.Tensor | None) -> tuple[Any, Any, int | None]:
    """(library, its entry point `symbol`, stream) for the device of `tensors`; BackendError where the library lacks the symbol."""
    lib, stream = _base._prepare(*tensors)
    entry = getattr(lib, symbol, None)
    if entry is None:
        raise BackendError(f"not covered: the loaded library does not export {symbol} ({header}; a host library has no convolution kernel)")
    return lib, entry, stream


def conv2d_w8a8(
    x_codes: torch.Tensor,
    w_codes: torch.Tensor,
    x_scale: torch.Tensor,
    x_offset: torch.Tensor | None,
    w_scale: torch.Tensor,
    w_offset: torch.Tensor | None,
    bias: torch.Tensor | None = None,
    stride: int | Sequence[int] = 1,
    padding: int | Sequence[int] = 0,
    dilation: int | Sequence[int] = 1,
    out_dtype: torch.dtype = torch.bfloat16,
    out_scale: torch.Tensor | None = None,
    out_offset: torch.Tensor | None = None,
    out_num_bits: float = 8.0,
    requant_from: torch.dtype | None = None,
) -> torch.Tensor:
    """``F.conv2d`` (groups = 1) on int8 codes: `x_codes` [B, C, H, W] (contiguous, or channels-last with C % 16 == 0, which skips
    the layout pass's input half), `w_codes` [OC, C, KH, KW]; fp32 parameters, one pair for the input and one for the weight or one
    per output channel; integer `padding` (a pair, symmetric per side). Returns the contiguous NCHW [B, OC, OH, OW] result in
    `out_dtype`: the exact integer contraction with the affine terms over the taps inside the image (include/ffq.h,
    ffq_conv2d_w8a8). With `out_scale` (and optionally `out_offset`) the per-tensor output quantizer runs in the epilogue: the
    result is rounded to `requant_from` (default bf16) and A1 writes int8 codes — exactly ``quantize_by_tile(conv2d_w8a8(...,
    out_dtype=requant_from), out_scale, shape, bits, torch.int8, out_offset)``."""
    op = "conv2d_w8a8"
    _check_codes(op, "input [B, C, H, W] and weight [OC, C, KH, KW]", 4, x_codes, w_codes)
    B, C, H, W = x_codes.shape
    OC, Cw, KH, KW = w_codes.shape
    if Cw != C:
        raise RuntimeError(f"{op}: the weight has {Cw} input channels, the input {C} (groups > 1 is not built)")
    (sh, sw), (ph, pw), (dh, dw) = _ints(stride, 2, "stride", op), _ints(padding, 2, "padding", op), _ints(dilation, 2, "dilation", op)
    xc, wc, xs, xo, ws_, wo, bias_c, os_, oo, cl, out_dt, y_dt = _operands(
        op, OC, torch.channels_last, x_codes, w_codes, x_scale, x_offset, w_scale, w_offset, bias, out_dtype, out_scale, out_offset, requant_from
    )
    lib, entry, stream = _entry("ffq_conv2d_w8a8", "include/ffq.h", xc, wc, xs, xo, ws_, wo, bias_c, os_, oo)
    OH = (H + 2 * ph - dh * (KH - 1) - 1) // sh + 1
    OW = (W + 2 * pw - dw * (KW - 1) - 1) // sw + 1
    out = torch.empty((B, OC, max(OH, 0), max(OW, 0)), dtype=out_dt, device=xc.device)
    nbytes = lib.ffq_conv2d_w8a8_workspace_bytes(B, C, H, W, OC, KH, KW, int(cl))
    ws = _workspace(nbytes, xc.device)
    lib.check(
        entry(
            _ptr(xc), int(cl), _ptr(wc), _ptr(xs), _ptr(xo), _ptr(ws_), _ptr(wo), int(ws_.numel() != 1),
            _ptr(bias_c), _tag(bias_c.dtype) if bias_c is not None else 0, _ptr(out), _tag(out.dtype), _ptr(os_), _ptr(oo),
            float(out_num_bits), y_dt,
            B, C, H, W, OC, KH, KW, sh, sw, ph, pw, dh, dw, _ptr(ws), nbytes, stream,
        )
    )
    return out


def depthwise_conv2d_w8a8(
    x_codes: torch.Tensor,
    w_codes: torch.Tensor,
    x_scale: torch.Tensor,
    x_offset: torch.Tensor | None,
    w_scale: torch.Tensor,
    w_offset: torch.Tensor | None,
    bias: torch.Tensor | None = None,
    stride: int | Sequence[int] = 1,
    padding: int | Sequence[int] = 0,
    dilation: int | Sequence[int] = 1,
    out_dtype: torch.dtype = torch.bfloat16,
    out_scale: torch.Tensor | None = None,
    out_offset: torch.Tensor | None = None,
    out_num_bits: float = 8.0,
    requant_from: torch.dtype | None = None,
) -> torch.Tensor:
    """``F.conv2d(groups=C)`` on int8 codes: `x_codes` [B, C, H, W], `w_codes` [C * M, 1, KH, KW] (``torch.nn.Conv2d(groups=C)``'s
    layout, channel multiplier M >= 1, KH * KW <= 1024); parameters, bias, `padding` and the output quantizer as in
    :func:`conv2d_w8a8`. Returns the contiguous NCHW [B, C * M, OH, OW] result: channel n is bit for bit :func:`conv2d_w8a8` on
    the one-channel slice ``x_codes[:, n // M]``, ``w_codes[n]`` (include/ffq_depthwise.h, csrc/ffq_depthwise.hip: one launch, no
    workspace). The kernel reads NCHW: an input in another layout (``channels_last``, a view) is copied to it first, so it gives the
    bits of its contiguous copy. Raises ``BackendError`` ("not covered") on a library without the entry point."""
    op = "depthwise_conv2d_w8a8"
    _check_codes(op, "input [B, C, H, W] and weight [C * M, 1, KH, KW]", 4, x_codes, w_codes)
    B, C, H, W = x_codes.shape
    OC, Cw, KH, KW = w_codes.shape
    if Cw != 1 or (C == 0 and OC != 0) or (C != 0 and OC % C != 0):
        raise RuntimeError(f"{op}: the weight is [C * M, 1, KH, KW] for an input of {C} channels, got {tuple(w_codes.shape)}")
    M = OC // C if C else 1
    (sh, sw), (ph, pw), (dh, dw) = _ints(stride, 2, "stride", op), _ints(padding, 2, "padding", op), _ints(dilation, 2, "dilation", op)
    xc, wc, xs, xo, ws_, wo, bias_c, os_, oo, cl, out_dt, y_dt = _operands(
        op, OC, None, x_codes, w_codes, x_scale, x_offset, w_scale, w_offset, bias, out_dtype, out_scale, out_offset, requant_from
    )
    lib, entry, stream = _entry("ffq_depthwise_conv2d_w8a8", "include/ffq_depthwise.h", xc, wc, xs, xo, ws_, wo, bias_c, os_, oo)
    OH = (H + 2 * ph - dh * (KH - 1) - 1) // sh + 1
    OW = (W + 2 * pw - dw * (KW - 1) - 1) // sw + 1
    out = torch.empty((B, OC, max(OH, 0), max(OW, 0)), dtype=out_dt, device=xc.device)
    lib.check(
        entry(
            _ptr(xc), _ptr(wc), _ptr(xs), _ptr(xo), _ptr(ws_), _ptr(wo), int(ws_.numel() != 1),
            _ptr(bias_c), _tag(bias_c.dtype) if bias_c is not None else 0, _ptr(out), _tag(out.dtype), _ptr(os_), _ptr(oo),
            float(out_num_bits), y_dt,
            B, C, M, H, W, KH, KW, sh, sw, ph, pw, dh, dw, stream,
        )
    )
    return out


def conv_transpose2d_w8a8(
    x_codes: torch.Tensor,
    w_codes: torch.Tensor,
    x_scale: torch.Tensor,
    x_offset: torch.Tensor | None,
    w_scale: torch.Tensor,
    w_offset: torch.Tensor | None,
    bias: torch.Tensor | None = None,
    stride: int | Sequence[int] = 1,
    padding: int | Sequence[int] = 0,
    output_padding: int | Sequence[int] = 0,
    dilation: int | Sequence[int] = 1,
    out_dtype: torch.dtype = torch.bfloat16,
    out_scale: torch.Tensor | None = None,
    out_offset: torch.Tensor | None = None,
    out_num_bits: float = 8.0,
    requant_from: torch.dtype | None = None,
) -> torch.Tensor:
    """``F.conv_transpose2d`` (groups = 1) on int8 codes: `x_codes` [B, C, H, W] (contiguous, or channels-last with C % 16 == 0, which
    skips the reorder pass's input half), `w_codes` [C, OC, KH, KW] (torch's transposed-weight layout); fp32 parameters, one pair
    for the input and one for the weight or one per OUTPUT channel (dim 1 of the weight). Returns the contiguous NCHW
    [B, OC, OH, OW] result in `out_dtype`, OH = (H - 1) * stride - 2 * padding + dilation * (KH - 1) + output_padding + 1: the exact
    integer contraction over the taps that reach the input, with the affine terms over the same taps (include/ffq.h,
    ffq_conv_transpose2d_w8a8). With `out_scale` (and optionally `out_offset`) the per-tensor output quantizer runs in the epilogue
    as in :func:`conv2d_w8a8`: the result is rounded to `requant_from` (default bf16) and A1 writes int8 codes."""
    op = "conv_transpose2d_w8a8"
    _check_codes(op, "input [B, C, H, W] and weight [C, OC, KH, KW]", 4, x_codes, w_codes)
    B, C, H, W = x_codes.shape
    Cw, OC, KH, KW = w_codes.shape
    if Cw != C:
        raise RuntimeError(f"{op}: the weight has {Cw} input channels, the input {C} (groups > 1 is not built)")
    (sh, sw), (ph, pw), (dh, dw) = _ints(stride, 2, "stride", op), _ints(padding, 2, "padding", op), _ints(dilation, 2, "dilation", op)
    oph, opw = _ints(output_padding, 2, "output_padding", op)
    xc, wc, xs, xo, ws_, wo, bias_c, os_, oo, cl, out_dt, y_dt = _operands(
        op, OC, torch.channels_last, x_codes, w_codes, x_scale, x_offset, w_scale, w_offset, bias, out_dtype, out_scale, out_offset, requant_from
    )
    lib, entry, stream = _entry("ffq_conv_transpose2d_w8a8", "include/ffq.h", xc, wc, xs, xo, ws_, wo, bias_c, os_, oo)
    OH = (H - 1) * sh - 2 * ph + dh * (KH - 1) + oph + 1
    OW = (W - 1) * sw - 2 * pw + dw * (KW - 1) + opw + 1
    out = torch.empty((B, OC, max(OH, 0), max(OW, 0)), dtype=out_dt, device=xc.device)
    nbytes = lib.ffq_conv_transpose2d_w8a8_workspace_bytes(B, C, H, W, OC, KH, KW, int(cl))
    ws = _workspace(nbytes, xc.device)
    lib.check(
        entry(
            _ptr(xc), int(cl), _ptr(wc), _ptr(xs), _ptr(xo), _ptr(ws_), _ptr(wo), int(ws_.numel() != 1),
            _ptr(bias_c), _tag(bias_c.dtype) if bias_c is not None else 0, _ptr(out), _tag(out.dtype), _ptr(os_), _ptr(oo),
            float(out_num_bits), y_dt,
            B, C, H, W, OC, KH, KW, sh, sw, ph, pw, oph, opw, dh, dw, _ptr(ws), nbytes, stream,
        )
    )
    return out


def conv3d_w8a8(
    x_codes: torch.Tensor,
    w_codes: torch.Tensor,
    x_scale: torch.Tensor,
    x_offset: torch.Tensor | None,
    w_scale: torch.Tensor,
    w_offset: torch.Tensor | None,
    bias: torch.Tensor | None = None,
    stride: int | Sequence[int] = 1,
    padding: int | Sequence[int] = 0,
    dilation: int | Sequence[int] = 1,
    out_dtype: torch.dtype = torch.bfloat16,
    out_scale: torch.Tensor | None = None,
    out_offset: torch.Tensor | None = None,
    out_num_bits: float = 8.0,
    requant_from: torch.dtype | None = None,
) -> torch.Tensor:
    """``F.conv3d`` (groups = 1) on int8 codes: `x_codes` [B, C, D, H, W] (contiguous, or ``torch.channels_last_3d`` with
    C % 16 == 0, which skips the layout pass's input half), `w_codes` [OC, C, KD, KH, KW]; parameters, bias, `padding` (an int or a
    triple, symmetric per side) and the output quantizer as in :func:`conv2d_w8a8`. Returns the contiguous [B, OC, OD, OH, OW]
    result (include/ffq_3d.h, ffq_conv3d_w8a8). Raises ``BackendError`` ("not covered") on a library without the entry point."""
    op = "conv3d_w8a8"
    _check_codes(op, "input [B, C, D, H, W] and weight [OC, C, KD, KH, KW]", 5, x_codes, w_codes)
    B, C, D, H, W = x_codes.shape
    OC, Cw, KD, KH, KW = w_codes.shape
    if Cw != C:
        raise RuntimeError(f"{op}: the weight has {Cw} input channels, the input {C} (groups > 1 is not built)")
    s, p, d = _ints(stride, 3, "stride", op), _ints(padding, 3, "padding", op), _ints(dilation, 3, "dilation", op)
    xc, wc, xs, xo, ws_, wo, bias_c, os_, oo, cl, out_dt, y_dt = _operands(
        op, OC, torch.channels_last_3d, x_codes, w_codes, x_scale, x_offset, w_scale, w_offset, bias, out_dtype, out_scale, out_offset, requant_from
    )
    lib, entry, stream = _entry("ffq_conv3d_w8a8", "include/ffq_3d.h", xc, wc, xs, xo, ws_, wo, bias_c, os_, oo)
    size = [max((n + 2 * pi - di * (k - 1) - 1) // si + 1, 0) for n, k, si, pi, di in zip((D, H, W), (KD, KH, KW), s, p, d)]
    out = torch.empty((B, OC, *size), dtype=out_dt, device=xc.device)
    nbytes = lib.ffq_conv3d_w8a8_workspace_bytes(B, C, D, H, W, OC, KD, KH, KW, int(cl))
    ws = _workspace(nbytes, xc.device)
    lib.check(
        entry(
            _ptr(xc), int(cl), _ptr(wc), _ptr(xs), _ptr(xo), _ptr(ws_), _ptr(wo), int(ws_.numel() != 1),
            _ptr(bias_c), _tag(bias_c.dtype) if bias_c is not None else 0, _ptr(out), _tag(out.dtype), _ptr(os_), _ptr(oo),
            float(out_num_bits), y_dt,
            B, C, D, H, W, OC, KD, KH, KW, *s, *p, *d, _ptr(ws), nbytes, stream,
        )
    )
    return out


MAX_PHASES = 64  # stride_h * stride_w: the phase table of csrc/ffq_conv_transpose.hip


def axis_phases(kernel: int, stride: int, padding: int, dilation: int, out_size: int) -> tuple[list[tuple[int, int, int, int]], int, int]:
    """One axis of the transposed convolution's phase table, as the host code of csrc/ffq_conv_transpose.hip builds it: for every
    residue r < stride the tuple (k0, n, off0, extent) — the taps k0, k0 + kstep, ... (n of them) are those with stride dividing
    r + padding - k * dilation, tap a reads input index i + off0 + a * ostep for the output o = r + stride * i, and extent counts
    the outputs o = r (mod stride) below out_size — and the two steps (kstep, ostep)."""
    g = math.gcd(stride, dilation)
    kstep, ostep = stride // g, -(dilation // g)
    rows = []
    for r in range(stride):
        k0 = next((k for k in range(min(kernel, kstep)) if (r + padding - k * dilation) % stride == 0), None)
        extent = (out_size - r + stride - 1) // stride if r < out_size else 0
        if k0 is None:
            rows.append((0, 0, 0, extent))
        else:
            rows.append((k0, (kernel - k0 + kstep - 1) // kstep, (r + padding - k0 * dilation) // stride, extent))
    return rows, kstep, ostep


def phase_table(batch: int, kernel: Sequence[int], stride: Sequence[int], padding: Sequence[int], dilation: Sequence[int],
                out_size: Sequence[int], tile: int = 128) -> list[dict[str, object]]:
    """The phase table of a transposed convolution, phase p = rh * stride_w + rw: its output grid (`rows` x `cols` positions per
    image: oh = rh + stride_h * i, ow = rw + stride_w * j), its `taps` in the phase-major order the reordered weight holds them
    ((kh, kw, ih - i, iw - j) each, w fastest), `tap_begin` (the first of them) and `tile_end` (the prefix of 128-position tiles)."""
    (ah, ksh, osh), (aw, ksw, osw) = (axis_phases(kernel[i], stride[i], padding[i], dilation[i], out_size[i]) for i in range(2))
    table, tiles, tap = [], 0, 0
    for rh, (k0h, nh, offh, eh) in enumerate(ah):
        for rw, (k0w, nw, offw, ew) in enumerate(aw):
            tiles += (batch * eh * ew + tile - 1) // tile
            taps = [(k0h + a * ksh, k0w + b * ksw, offh + a * osh, offw + b * osw) for a in range(nh) for b in range(nw)]
            table.append(dict(rh=rh, rw=rw, rows=eh, cols=ew, taps=taps, tap_begin=tap, tile_end=tiles))
            tap += nh * nw
    return table
