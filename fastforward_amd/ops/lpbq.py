"""LPBQ weights on the kernels of csrc/ffq_lpbq.hip (include/lpbq/ffq_lpbq.h): a W4 block-quantized weight as int8 codes with one scale
per output channel (reference export/_lpbq.py), the operand of ``linear_w8a8``.

``lpbq_compress_scales`` turns block scales ``[N, J]`` into ``(int_scale uint8 [N, J], channel_scale fp32 [N])``; ``lpbq_quantize`` is the
weight quantizer in one launch (compression, A1 at `bits` bits, the product ``code4 * int_scale``); ``lpbq_expand`` multiplies 4-bit codes
at rest (int8, or the nibbles of ``pack_int4``) by their ``int_scale``. A matrix that is a column window of a wider one is read in place:
the entry points take a row stride. There is no host implementation: host tensors raise ``BackendError`` (the torch restatement of the
reference's arithmetic lives in ``fastforward_amd.quantization.lpbq``)."""

from __future__ import annotations

from typing import Sequence

import torch

from fastforward_amd.exceptions import BackendError
from fastforward_amd.ops import _base
from fastforward_amd.ops._base import _ptr, _tag

MAX_BLOCKS_PER_ROW = 1024  # J: the entry points' limit (a row's int_scale live in LDS)
BITS = (2, 3, 4)
_WEIGHT_DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def _entry(lib, name: str):
    fn = getattr(lib, name, None)
    if fn is None:
        raise BackendError(f"LPBQ is not covered by the loaded library: it does not export {name}")
    return fn


def _check_bits(name: str, bits: int) -> int:
    if isinstance(bits, bool) or bits not in BITS:
        raise RuntimeError(f"{name}: bits is 2, 3 or 4, got {bits}")
    return int(bits)


def _row_stride(name: str, t: torch.Tensor, what: str) -> int:
    """The row stride in elements of a 2-D tensor whose rows are contiguous and do not overlap, else RuntimeError."""
    rows, cols = t.shape
    if cols > 1 and t.stride(1) != 1:
        raise RuntimeError(f"{name}: the rows of {what} must be contiguous, got strides {tuple(t.stride())}")
    if rows <= 1:
        return max(cols, 1)
    if t.stride(0) < cols:
        raise RuntimeError(f"{name}: the rows of {what} overlap (stride {t.stride(0)} < {cols})")
    return t.stride(0)


def _check_scales(name: str, scales: torch.Tensor, rows: int | None = None, blocks: int | None = None) -> int:
    if scales.dim() != 2 or scales.dtype != torch.float32:
        raise RuntimeError(f"{name}: the block scales are fp32 [N, J], got {scales.dtype} {tuple(scales.shape)}")
    if (rows is not None and scales.shape[0] != rows) or (blocks is not None and scales.shape[1] != blocks):
        raise RuntimeError(f"{name}: expected block scales [{rows}, {blocks}], got {tuple(scales.shape)}")
    if scales.shape[1] > MAX_BLOCKS_PER_ROW:
        raise RuntimeError(f"{name}: at most {MAX_BLOCKS_PER_ROW} blocks per row, got {scales.shape[1]}")
    return _row_stride(name, scales, "the block scales")


def lpbq_compress_scales(scales: torch.Tensor, bits: int = 4) -> tuple[torch.Tensor, torch.Tensor]:
    """``(int_scale, channel_scale)`` of fp32 block scales ``[N, J]``: per row ``d = max / 2^bits``, ``q = clamp(rne(s / d), 1, 2^bits)``
    — ``LPBQProcessor.grouped_dynamic_quantize`` for ``PerBlock(1, G, 0)``, bit for bit for finite positive scales."""
    name = "lpbq_compress_scales"
    bits = _check_bits(name, bits)
    scales = scales.detach()
    stride = _check_scales(name, scales)
    lib, stream = _base._prepare(scales)
    entry = _entry(lib, "ffq_lpbq_compress_scales")
    N, J = scales.shape
    int_scale = torch.empty((N, J), dtype=torch.uint8, device=scales.device)
    channel_scale = torch.empty(N, dtype=torch.float32, device=scales.device)
    lib.check(entry(_ptr(scales), stride, N, J, bits, _ptr(int_scale), _ptr(channel_scale), stream))
    return int_scale, channel_scale


def lpbq_quantize(w: torch.Tensor, scales: torch.Tensor, group: int, bits: int = 4, requantize: bool = False,
                  want_int_scale: bool = True) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor | None]:
    """``(codes8 int8 [N, K], channel_scale fp32 [N], int_scale uint8 [N, K / group] or None)`` of a weight ``[N, K]`` (bf16, fp16 or
    fp32) and its fp32 block scales ``[N, K / group]`` in one launch: ``codes8 = quantize_by_tile(w, s, (1, group), bits, int8) *
    int_scale`` with ``s`` the block scales, or with `requantize` the compressed ones, ``channel_scale * int_scale``."""
    name = "lpbq_quantize"
    bits = _check_bits(name, bits)
    w, scales = w.detach(), scales.detach()
    if w.dim() != 2 or w.dtype not in _WEIGHT_DTYPES:
        raise RuntimeError(f"{name}: the weight is a bf16, fp16 or fp32 matrix, got {w.dtype} {tuple(w.shape)}")
    N, K = w.shape
    if isinstance(group, bool) or not isinstance(group, int) or group < 1 or K % group:
        raise RuntimeError(f"{name}: the group size must divide K = {K}, got {group}")
    w_stride = _row_stride(name, w, "the weight")
    s_stride = _check_scales(name, scales, N, K // group)
    lib, stream = _base._prepare(w, scales)
    entry = _entry(lib, "ffq_lpbq_quantize")
    codes8 = torch.empty((N, K), dtype=torch.int8, device=w.device)
    channel_scale = torch.empty(N, dtype=torch.float32, device=w.device)
    int_scale = torch.empty((N, K // group), dtype=torch.uint8, device=w.device) if want_int_scale else None
    lib.check(entry(_ptr(w), _tag(w.dtype), w_stride, _ptr(scales), s_stride, N, K, int(group), bits, int(bool(requantize)),
                    _ptr(codes8), _ptr(channel_scale), _ptr(int_scale), stream))
    return codes8, channel_scale, int_scale


def lpbq_expand(codes4: torch.Tensor, int_scale: torch.Tensor, group: int, shape: Sequence[int] | None = None, block: int = 32) -> torch.Tensor:
    """``codes4 * int_scale`` as int8 ``[N, K]``: `codes4` is the int8 matrix of 4-bit codes or, with `shape` ``(N, K)`` given, the uint8
    bytes of ``pack_int4(codes, block)``; `int_scale` is uint8 ``[N, K / group]``. Bit-equal to ``unpack_int4(...) * int_scale``."""
    name = "lpbq_expand"
    codes4, int_scale = codes4.detach(), int_scale.detach()
    packed = shape is not None
    if packed:
        if codes4.dtype != torch.uint8 or len(tuple(shape)) != 2:
            raise RuntimeError(f"{name}: packed codes are uint8 bytes with shape = (N, K), got {codes4.dtype} and shape {tuple(shape)}")
        N, K = (int(v) for v in shape)
        if isinstance(block, bool) or not isinstance(block, int) or block < 2 or block % 2 or (N * K) % block or codes4.numel() * 2 != N * K:
            raise RuntimeError(f"{name}: {codes4.numel()} bytes in blocks of {block} do not hold {N} x {K} codes")
    else:
        if codes4.dtype != torch.int8 or codes4.dim() != 2:
            raise RuntimeError(f"{name}: the codes are an int8 matrix (or uint8 nibbles with `shape`), got {codes4.dtype} {tuple(codes4.shape)}")
        N, K = codes4.shape
    if isinstance(group, bool) or not isinstance(group, int) or group < 1 or K % group:
        raise RuntimeError(f"{name}: the group size must divide K = {K}, got {group}")
    if int_scale.dtype != torch.uint8 or tuple(int_scale.shape) != (N, K // group) or K // group > MAX_BLOCKS_PER_ROW:
        raise RuntimeError(f"{name}: int_scale is uint8 [{N}, {K // group}] with at most {MAX_BLOCKS_PER_ROW} blocks per row, got {int_scale.dtype} {tuple(int_scale.shape)}")
    codes4, int_scale = codes4.contiguous(), int_scale.contiguous()  # (both are read as dense buffers)
    lib, stream = _base._prepare(codes4, int_scale)
    entry = _entry(lib, "ffq_lpbq_expand")
    codes8 = torch.empty((N, K), dtype=torch.int8, device=codes4.device)
    lib.check(entry(_ptr(codes4), int(packed), int(block) if packed else 0, _ptr(int_scale), N, K, int(group), _ptr(codes8), stream))
    return codes8
