"""The reference's quantized ``scaled_dot_product_attention`` (nn/functional/custom/sdpa.py:116-285) as one launch
(csrc/ffq_sdpa.hip; with a scaled-key quantizer a first, small launch writes the K codes into scratch): q·kᵀ, bias, safe softmax and P·V with up to eight static per-tensor quantizers applied in registers.

``quantizers`` maps the reference's keyword names (``attn_scores_quantizer`` ...) to ``(scale, offset, num_bits)``; a missing name
is an inactive slot. q / k / v are plain bf16 / fp16 tensors or, with ``dequant``, their codes in that dtype with per-tensor
parameters. Returns ``(value, codes)``: the value [B, H_q, L, E] in the operands' dtype (A2 of the output codes when the output
quantizer is active) and the int8 output codes (None without an output quantizer or when not asked for)."""

from __future__ import annotations

import ctypes
import math

from typing import Mapping, Sequence

import torch

from fastforward_amd import _cabi
from fastforward_amd.ops import _base
from fastforward_amd.ops._base import _ptr, _tag
from fastforward_amd.ops.modules import _entry

# the reference's quantizer keywords, in the order of include/ffq.h's FFQ_SDPA_* slots (tests/test_sdpa_cpu.py checks the header)
QUANTIZER_SLOTS = (
    "attn_scores_quantizer",
    "attn_mask_quantizer",
    "masked_scores_quantizer",
    "attn_weights_quantizer",
    "scaled_query_quantizer",
    "scaled_key_quantizer",
    "dropout_quantizer",
    "output_quantizer",
)
MASK_KINDS = {"none": 0, "causal": 1, "bool": 2, "float": 3}

SdpaParams = tuple[torch.Tensor, torch.Tensor | None, float]


def _scalar(t: torch.Tensor | None, what: str) -> torch.Tensor | None:
    if t is None:
        return None
    t = t.detach().reshape(-1)
    if t.numel() != 1 or t.dtype != torch.float32:
        raise RuntimeError(f"sdpa_quantize: {what} must be one fp32 element, got {t.numel()} x {t.dtype}")
    return t.contiguous()


def _strides(t: torch.Tensor) -> tuple[int, ...]:
    """Element strides of (batch, head, row); a dimension of size 1 is never stepped, whatever its stride says."""
    return tuple(st if n > 1 else 0 for n, st in zip(t.shape[:3], t.stride()[:3]))


def sdpa_quantize(
    query: torch.Tensor,
    key: torch.Tensor,
    value: torch.Tensor,
    attn_mask: torch.Tensor | None = None,
    is_causal: bool = False,
    scale: float | None = None,
    neg_inf: float = float("-inf"),
    quantizers: Mapping[str, SdpaParams] | None = None,
    dequant: Sequence[tuple[torch.Tensor, torch.Tensor | None] | None] = (None, None, None),
    want_codes: bool = False,
    skip_above_diagonal: bool = False,
) -> tuple[torch.Tensor, torch.Tensor | None]:
    """One launch of ``ffq_sdpa_quantize``. query [B, H_q, L, E], key / value [B, H, S, E] (H_q a multiple of H: query head h reads
    kv head h // (H_q // H)), E in {64, 128}, last dimension contiguous, rows 16-byte aligned; any other strides. `attn_mask` (bool or
    float, last two dims [L, S]) broadcasts over the leading dims; it excludes `is_causal`. `skip_above_diagonal` (causal only): the
    caller knows that the masked score above the diagonal is -inf, so those tiles are never visited."""
    quantizers = dict(quantizers or {})
    unknown = set(quantizers) - set(QUANTIZER_SLOTS)
    if unknown:
        raise RuntimeError(f"sdpa_quantize: unknown quantizer slots {sorted(unknown)}")
    dt = query.dtype
    if dt not in (torch.bfloat16, torch.float16) or key.dtype != dt or value.dtype != dt:
        raise RuntimeError(f"sdpa_quantize: q / k / v are all bf16 or all fp16, got {query.dtype}, {key.dtype}, {value.dtype}")
    if query.dim() != 4 or key.dim() != 4 or value.dim() != 4:
        raise RuntimeError("sdpa_quantize: q / k / v are 4-D [B, H, L|S, E]")
    B, H, L, E = query.shape
    _, HKV, S, _ = key.shape
    if key.shape[0] != B or key.shape[3] != E or tuple(value.shape) != (B, HKV, S, E):
        raise RuntimeError(f"sdpa_quantize: shapes {tuple(query.shape)}, {tuple(key.shape)}, {tuple(value.shape)} do not fit")
    if E not in (64, 128):
        raise RuntimeError(f"sdpa_quantize: E must be 64 or 128, got {E}")
    if H % HKV:
        raise RuntimeError(f"sdpa_quantize: {H} query heads are not a multiple of {HKV} kv heads")
    for t in (query, key, value):
        if t.stride(-1) != 1 or any(st % 8 for st in _strides(t)) or t.data_ptr() % 16:
            raise RuntimeError("sdpa_quantize: the last dimension must be contiguous with 16-byte aligned rows")
    if attn_mask is not None and is_causal:
        raise ValueError("Explicit attn_mask should not be set when is_causal=True")
    mask, mask_kind, mask_dt, mask_strides = None, MASK_KINDS["causal" if is_causal else "none"], _tag(torch.float32), None
    if attn_mask is not None:
        if attn_mask.dim() < 2 or tuple(attn_mask.shape[-2:]) != (L, S) or attn_mask.dim() > 4:
            raise RuntimeError(f"sdpa_quantize: the mask's last two dims must be [{L}, {S}], got {tuple(attn_mask.shape)}")
        mask = attn_mask.detach().expand(B, H, L, S)
        if mask.dtype == torch.bool:
            mask_kind = MASK_KINDS["bool"]
        elif mask.dtype in (torch.float32, torch.bfloat16, torch.float16):
            mask_kind, mask_dt = MASK_KINDS["float"], _tag(mask.dtype)
        else:
            raise RuntimeError(f"sdpa_quantize: a mask is bool or float, got {mask.dtype}")
        mask_strides = (ctypes.c_int64 * 4)(*mask.stride())
    slots = (_cabi.SdpaQuantizer * _cabi.SDPA_QUANTIZERS)()
    keep: list[torch.Tensor] = []
    for i, name in enumerate(QUANTIZER_SLOTS):
        if name not in quantizers:
            continue
        s, o, bits = quantizers[name]
        s, o = _scalar(s, f"{name} scale"), _scalar(o, f"{name} offset")
        keep += [t for t in (s, o) if t is not None]
        slots[i] = _cabi.SdpaQuantizer(_ptr(s), _ptr(o), float(bits))
    deq_s, deq_o = (ctypes.c_void_p * 3)(), (ctypes.c_void_p * 3)()
    for i, d in enumerate(dequant):
        if d is not None:
            s, o = _scalar(d[0], "dequant scale"), _scalar(d[1], "dequant offset")
            keep += [t for t in (s, o) if t is not None]
            deq_s[i], deq_o[i] = _ptr(s), _ptr(o)
    if want_codes and "output_quantizer" not in quantizers:
        raise RuntimeError("sdpa_quantize: codes need the output quantizer")
    lib, stream = _base._prepare(query, key, value, mask, *keep)
    out = torch.empty((B, H, L, E), dtype=dt, device=query.device)
    codes = torch.empty((B, H, L, E), dtype=torch.int8, device=query.device) if want_codes else None
    # the scaled-K codes are written once per call into this scratch (include/ffq.h)
    key_codes = torch.empty((B, HKV, S, E), dtype=dt, device=query.device) if "scaled_key_quantizer" in quantizers else None
    strides = (ctypes.c_int64 * 9)(*_strides(query), *_strides(key), *_strides(value))
    sqrt_scale = math.sqrt(1.0 / math.sqrt(E) if scale is None else scale)  # the math path's scale_factor_sqrt
    lib.check(
        _entry(lib, "ffq_sdpa_quantize")(
            _ptr(query), _ptr(key), _ptr(value), _tag(dt), deq_s, deq_o, B, H, HKV, L, S, E, strides, _ptr(mask), mask_kind, mask_dt,
            mask_strides, sqrt_scale, float(neg_inf), slots, int(bool(skip_above_diagonal)), _ptr(out), _ptr(codes), _ptr(key_codes), stream,
        )
    )
    del keep
    return out, codes
