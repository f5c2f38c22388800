"""OCP microscaling (MX) on the kernels of csrc/ffq_mx.hip (include_mx/ffq_mx.h): the MXFP8 / MXFP4 quantizer, its inverse, and the linear
on CDNA4's block-scaled matrix-core instruction.

``mx_quantize`` returns the element codes (one per byte and / or, for e2m1, packed two per byte) and one E8M0 scale byte per block of 32
elements of the last dimension, from one launch; ``mx_dequantize`` is the inverse from either container; ``linear_mx`` multiplies two
quantized matrices, ``out = A . W^T (+ bias)``, reading e4m3 codes as bytes and e2m1 codes packed. A matrix that is a column window of a
wider one is read in place. There is no host implementation here: host tensors raise ``BackendError`` (the torch restatement of the same
arithmetic is ``fastforward_amd._host.mx_quantize`` / ``mx_dequantize`` / ``mx_pack`` / ``mx_unpack``)."""

from __future__ import annotations

import torch

from fastforward_amd import _host
from fastforward_amd._cabi import MX_E2M1, MX_E4M3
from fastforward_amd.exceptions import BackendError
from fastforward_amd.ops import _base
from fastforward_amd.ops._base import _ptr, _tag

BLOCK = _host.MX_BLOCK
FORMATS = dict(zip(_host.MX_FORMATS, (MX_E4M3, MX_E2M1)))  # name -> the header's tag
PAIRS = (("e4m3", "e4m3"), ("e4m3", "e2m1"), ("e2m1", "e2m1"))  # (activation, weight) pairs ``linear_mx`` covers
_FLOATS = (torch.bfloat16, torch.float16, torch.float32)


def _entry(lib, name: str):
    fn = getattr(lib, name, None)
    if fn is None:
        raise BackendError(f"MX is not covered by the loaded library: it does not export {name}")
    return fn


def _format(name: str, element_format: str) -> int:
    if element_format not in FORMATS:
        raise ValueError(f"{name}: the element format is 'e4m3' or 'e2m1', got {element_format!r}")
    return FORMATS[element_format]


def _rows(t: torch.Tensor) -> tuple[torch.Tensor, int]:
    """`t` as a matrix whose rows are contiguous, and its row stride in elements: a 2-D column window is read in place, anything else
    that is not dense is copied."""
    if t.dim() == 2 and (t.shape[1] <= 1 or t.stride(1) == 1) and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1]):
        return t, (t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1))
    flat = t.contiguous().reshape(-1, t.shape[-1])
    return flat, max(t.shape[-1], 1)


def mx_quantize(data: torch.Tensor, element_format: str = "e2m1", *, codes: bool = True, packed: bool = False):
    """``(codes, packed, scales)`` of `data` (bf16, fp16 or fp32; blocks of 32 along the last dimension) in one launch: `codes` uint8 of
    data's shape, one code per byte; `packed` (e2m1 only) uint8 ``[..., K / 2]``; `scales` uint8 ``[..., K / 32]``. A container that was
    not asked for is None. Bit-equal to ``_host.mx_quantize`` (and ``_host.mx_pack`` of its codes)."""
    name = "mx_quantize"
    fmt = _format(name, element_format)
    data = data.detach()
    if data.dim() < 1 or data.dtype not in _FLOATS:
        raise RuntimeError(f"{name}: the input holds bf16, fp16 or fp32 values, got {data.dtype} {tuple(data.shape)}")
    K = data.shape[-1]
    if K % BLOCK:
        raise ValueError(f"{name}: the last dimension must be a multiple of {BLOCK}, got shape {tuple(data.shape)}")
    if packed and element_format != "e2m1":
        raise ValueError(f"{name}: only e2m1 codes have a packed form")
    if not codes and not packed:
        raise ValueError(f"{name}: ask for at least one container")
    view, stride = _rows(data)
    lib, stream = _base._prepare(view)
    entry = _entry(lib, "ffq_mx_quantize")
    rows = view.shape[0]
    lead = tuple(data.shape[:-1])
    out_codes = torch.empty((*lead, K), dtype=torch.uint8, device=data.device) if codes else None
    out_packed = torch.empty((*lead, K // 2), dtype=torch.uint8, device=data.device) if packed else None
    scales = torch.empty((*lead, K // BLOCK), dtype=torch.uint8, device=data.device)
    lib.check(entry(_ptr(view), _tag(view.dtype), stride, rows, K, fmt, _ptr(out_codes), _ptr(out_packed), _ptr(scales), stream))
    return out_codes, out_packed, scales


def mx_dequantize(codes: torch.Tensor, scales: torch.Tensor, element_format: str = "e2m1", dtype: torch.dtype = torch.float32, *,
                  packed: bool = False) -> torch.Tensor:
    """``value(code) * 2^(scale - 127)`` rounded once to `dtype`: `codes` uint8, one per byte or (``packed=True``, e2m1) two per byte;
    `scales` uint8 ``[..., K / 32]``. Bit-equal to ``_host.mx_dequantize``."""
    name = "mx_dequantize"
    fmt = _format(name, element_format)
    codes, scales = codes.detach(), scales.detach()
    if packed and element_format != "e2m1":
        raise ValueError(f"{name}: only e2m1 codes have a packed form")
    if codes.dtype != torch.uint8 or scales.dtype != torch.uint8 or codes.dim() < 1 or dtype not in _FLOATS:
        raise RuntimeError(f"{name}: uint8 codes and scales and a bf16, fp16 or fp32 result, got {codes.dtype}, {scales.dtype}, {dtype}")
    K = codes.shape[-1] * (2 if packed else 1)
    if K % BLOCK or tuple(scales.shape) != (*codes.shape[:-1], K // BLOCK):
        raise ValueError(f"{name}: codes {tuple(codes.shape)} and scales {tuple(scales.shape)} do not match")
    codes, scales = codes.contiguous(), scales.contiguous()  # (both are read as dense buffers)
    lib, stream = _base._prepare(codes, scales)
    entry = _entry(lib, "ffq_mx_dequantize")
    out = torch.empty((*codes.shape[:-1], K), dtype=dtype, device=codes.device)
    rows = out.numel() // K if K else 0
    lib.check(entry(_ptr(codes), int(packed), _ptr(scales), rows, K, fmt, _ptr(out), _tag(dtype), stream))
    return out


def linear_mx_supported(M: int, N: int, K: int, a_format: str, w_format: str) -> bool:
    """Whether ``linear_mx`` takes the shapes and the format pair: the library's own rule (``ffq_linear_mx_supported``)."""
    if a_format not in FORMATS or w_format not in FORMATS:
        return False
    from fastforward_amd import _native

    fn = getattr(_native.library(), "ffq_linear_mx_supported", None)
    return bool(fn is not None and fn(int(M), int(N), int(K), FORMATS[a_format], FORMATS[w_format]))


def _operand(name: str, what: str, codes: torch.Tensor, scales: torch.Tensor, element_format: str) -> tuple[int, int]:
    """(rows, K) of a GEMM operand: uint8 code matrix (e4m3 [rows, K], e2m1 packed [rows, K / 2]) and scale matrix [rows, K / 32], each
    with contiguous rows (any row stride)."""
    if codes.dtype != torch.uint8 or scales.dtype != torch.uint8 or codes.dim() != 2 or scales.dim() != 2:
        raise RuntimeError(f"{name}: {what} is a uint8 code matrix with a uint8 scale matrix, got {codes.dtype} {tuple(codes.shape)}, {scales.dtype} {tuple(scales.shape)}")
    rows = codes.shape[0]
    K = codes.shape[1] * (2 if element_format == "e2m1" else 1)
    if scales.shape[0] != rows or scales.shape[1] * BLOCK != K:
        raise RuntimeError(f"{name}: {what}: codes {tuple(codes.shape)} ({element_format}) and scales {tuple(scales.shape)} do not match")
    for t in (codes, scales):
        if (t.shape[1] > 1 and t.stride(1) != 1) or (rows > 1 and t.stride(0) < t.shape[1]):
            raise RuntimeError(f"{name}: the rows of {what} must be contiguous and must not overlap, got strides {tuple(t.stride())}")
    return rows, K


def _stride_bytes(t: torch.Tensor) -> int:
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)


def linear_mx(a_codes: torch.Tensor, a_scales: torch.Tensor, a_format: str, w_codes: torch.Tensor, w_scales: torch.Tensor, w_format: str,
              bias: torch.Tensor | None = None, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """``out[M, N] = A[M, K] . W[N, K]^T (+ bias)`` in one launch on the block-scaled MFMA: fp32 accumulation, one rounding to `out_dtype`.
    e4m3 codes are uint8 ``[rows, K]``, e2m1 codes PACKED uint8 ``[rows, K / 2]``; scales are uint8 ``[rows, K / 32]``. Every matrix may
    be a column window of a wider one (rows 16-byte aligned for codes, 4-byte aligned for scales: the library refuses others)."""
    name = "linear_mx"
    fa, fw = _format(name, a_format), _format(name, w_format)
    a_codes, a_scales, w_codes, w_scales = a_codes.detach(), a_scales.detach(), w_codes.detach(), w_scales.detach()
    M, K = _operand(name, "A", a_codes, a_scales, a_format)
    N, Kw = _operand(name, "W", w_codes, w_scales, w_format)
    if K != Kw:
        raise RuntimeError(f"{name}: A has K = {K}, W has K = {Kw}")
    if out_dtype not in _FLOATS:
        raise RuntimeError(f"{name}: the result is fp32, bf16 or fp16, got {out_dtype}")
    if bias is not None:
        bias = bias.detach()
        if bias.dim() != 1 or bias.shape[0] != N or bias.dtype not in (torch.float32, out_dtype):
            raise RuntimeError(f"{name}: the bias is [{N}] in fp32 or {out_dtype}, got {bias.dtype} {tuple(bias.shape)}")
        bias = bias.contiguous()
    lib, stream = _base._prepare(a_codes, a_scales, w_codes, w_scales, bias)
    entry = _entry(lib, "ffq_linear_mx")
    out = torch.empty((M, N), dtype=out_dtype, device=a_codes.device)
    lib.check(entry(_ptr(a_codes), _stride_bytes(a_codes), _ptr(a_scales), _stride_bytes(a_scales), fa, _ptr(w_codes), _stride_bytes(w_codes),
                    _ptr(w_scales), _stride_bytes(w_scales), fw, _ptr(bias), _tag(bias.dtype) if bias is not None else 0, _ptr(out),
                    _tag(out_dtype), M, N, K, stream))
    return out
