"""A preallocated, quantized KV cache for a decode loop (no counterpart in the reference, which never decodes).

``QuantizedKVCache`` owns two int8 buffers ``[B, H, S_max, E]`` and the lengths of its sequences as an int32 tensor ON THE DEVICE.
``append`` advances the lengths with an ordinary ``add_`` and quantizes the new K / V rows into place in one launch
(``ops.kv_append``); ``attend`` is one ``ops.kv_decode`` call that reads the lengths on the device. Nothing reads a length on the host
and no shape moves from step to step, so ``append`` + ``attend`` can be captured once in a ``torch.cuda.graph`` and replayed while the
sequences grow, each at its own length. ``is_causal`` is bottom-right: the L new queries sit at the END of the cache.

``composed_append`` / ``composed_attend`` run the same semantics from existing pieces (torch ops for the rotation, the quantizer
modules, an indexed copy per batch, ``scaled_dot_product_attention`` per batch on the slices with a bottom-right bool mask). They read
the lengths on the host: they are the chain the kernels are tested against and what the class runs on host tensors or with a library
that lacks the entry points, not a fast path.
"""

from __future__ import annotations

from typing import Any, Sequence

import torch

from fastforward_amd import _native, ops
from fastforward_amd.nn.linear_quantizer import LinearQuantizer
from fastforward_amd.quantized_tensor import QuantizedTensor

LAYOUTS = ("bhse", "bshe")
_VALUES = (torch.bfloat16, torch.float16)
Rope = tuple[torch.Tensor, torch.Tensor]


def _kernels():
    from fastforward_amd import fused_sdpa_decode  # (imports this package's modules: resolved at call time)

    return fused_sdpa_decode.KERNELS


def _quantizer_params(quantizer: Any, what: str) -> tuple[torch.Tensor, torch.Tensor | None, float]:
    """(scale, offset, bits) of a quantizer the append kernel reproduces, else ValueError: the ``_fused`` rule of the attention
    kernels (a plain, initialised, per-tensor, static ``LinearQuantizer`` with fp32 parameters) with an int8 container and 2..8 bits."""
    if not isinstance(quantizer, LinearQuantizer):
        raise ValueError(f"QuantizedKVCache: the {what} quantizer must be a LinearQuantizer, got {type(quantizer).__name__}")
    with torch.no_grad():  # (a cache serves inference: parameters that could take a gradient are no reason to decline)
        fused = _kernels()._fused(quantizer)
    if not fused or quantizer.quantized_dtype != torch.int8 or not 2 <= fused[2] <= 8:
        raise ValueError(
            f"QuantizedKVCache: the {what} quantizer must be an initialised per-tensor static LinearQuantizer with fp32 parameters, "
            "quantized_dtype=torch.int8 and an integral bit-width in 2..8"
        )
    return fused[0].detach(), None if fused[1] is None else fused[1].detach(), float(fused[2])


def _rotate(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """``x * cos + rotate_half(x) * sin`` in x's dtype, every step rounded (x [..., L, E], cos / sin [L, E])."""
    half = x.shape[-1] // 2
    rotated = torch.cat((-x[..., half:], x[..., :half]), dim=-1)
    return x * cos + rotated * sin


def _bottom_right(L: int, S: int, device: torch.device) -> torch.Tensor:
    """bool [L, S]: row l sees key <= l + (S - L)."""
    rows = torch.arange(L, device=device).unsqueeze(1)
    return torch.arange(S, device=device).unsqueeze(0) <= rows + (S - L)


def composed_append(k_cache: torch.Tensor, v_cache: torch.Tensor, lengths: torch.Tensor, key: torch.Tensor, value: torch.Tensor,
                    key_quantizer: LinearQuantizer, value_quantizer: LinearQuantizer, rope: Rope | None = None) -> None:
    """``ops.kv_append`` from existing pieces. `lengths` already counts the L new rows; it is read on the host."""
    L, S_max = key.shape[2], k_cache.shape[2]
    with torch.no_grad():
        for b, n in enumerate(lengths.tolist()):
            rows = [l for l in range(L) if 0 <= n - L + l < S_max]
            if not rows:
                continue
            at = torch.tensor([n - L + l for l in rows], device=key.device)
            take = torch.tensor(rows, device=key.device)
            k_rows, v_rows = key[b].index_select(1, take), value[b].index_select(1, take)
            if rope is not None:
                k_rows = _rotate(k_rows, rope[0].index_select(0, at), rope[1].index_select(0, at))
            k_cache[b].index_copy_(1, at, key_quantizer(k_rows.contiguous()).raw_data)
            v_cache[b].index_copy_(1, at, value_quantizer(v_rows.contiguous()).raw_data)


def composed_attend(query: Any, k_cache: torch.Tensor, v_cache: torch.Tensor, lengths: torch.Tensor, key_quantizer: LinearQuantizer,
                    value_quantizer: LinearQuantizer, dtype: torch.dtype, is_causal: bool = True, scale: float | None = None,
                    output_quantizer: Any = None) -> torch.Tensor:
    """``ops.kv_decode`` from existing pieces: per batch, ``scaled_dot_product_attention`` over the ``[:, :, :S_b]`` slices with a
    bottom-right bool mask; exact zeros for a sequence without keys. `lengths` is read on the host."""
    from fastforward_amd.nn import functional as F

    B, H, L, E = query.shape
    HKV, S_max = k_cache.shape[1], k_cache.shape[2]
    out = torch.zeros((B, H, L, E), dtype=dtype, device=k_cache.device)
    extra = {} if output_quantizer is None else dict(output_quantizer=output_quantizer)
    with torch.no_grad():
        for b, n in enumerate(lengths.tolist()):
            S = min(max(n, 0), S_max)
            if S == 0:
                continue
            keys = key_quantizer.wrap_codes(k_cache[b:b + 1, :, :S], dtype)
            values = value_quantizer.wrap_codes(v_cache[b:b + 1, :, :S], dtype)
            mask = _bottom_right(L, S, k_cache.device) if is_causal else None
            got = F.scaled_dot_product_attention(query[b:b + 1], keys, values, attn_mask=mask, scale=scale, enable_gqa=H != HKV,
                                                 strict_quantization=False, **extra)
            out[b] = (got.dequantize() if isinstance(got, QuantizedTensor) else got)[0].to(dtype)
    return out


class QuantizedKVCache:
    """int8 K / V codes for `batch` sequences of up to `max_len` positions, quantized by two per-tensor static quantizers.

    ``layout="bhse"`` allocates ``[B, H, S_max, E]``; ``"bshe"`` allocates ``[B, S_max, H, E]`` (a position's heads side by side, the
    projection's own order) and works on its ``transpose(1, 2)`` view. ``k_cache`` / ``v_cache`` are always ``[B, H, S_max, E]`` views,
    ``lengths`` is int32 ``[B]``."""

    def __init__(self, batch: int, kv_heads: int, max_len: int, head_dim: int, key_quantizer: LinearQuantizer, value_quantizer: LinearQuantizer,
                 dtype: torch.dtype = torch.bfloat16, device: torch.device | str = "cuda", layout: str = "bhse") -> None:
        if layout not in LAYOUTS:
            raise ValueError(f"QuantizedKVCache: layout is one of {LAYOUTS}, got {layout!r}")
        if dtype not in _VALUES:
            raise ValueError(f"QuantizedKVCache: the data dtype is bf16 or fp16, got {dtype}")
        if head_dim not in (64, 128):
            raise ValueError(f"QuantizedKVCache: head_dim must be 64 or 128, got {head_dim}")
        if min(batch, kv_heads, max_len) < 1:
            raise ValueError(f"QuantizedKVCache: batch, kv_heads and max_len are positive, got {batch}, {kv_heads}, {max_len}")
        _quantizer_params(key_quantizer, "key")
        _quantizer_params(value_quantizer, "value")
        self.key_quantizer, self.value_quantizer = key_quantizer, value_quantizer
        self.dtype, self.layout, self.max_len = dtype, layout, max_len
        shape = (batch, kv_heads, max_len, head_dim) if layout == "bhse" else (batch, max_len, kv_heads, head_dim)
        buffers = [torch.zeros(shape, dtype=torch.int8, device=device) for _ in range(2)]
        self.k_cache, self.v_cache = (t if layout == "bhse" else t.transpose(1, 2) for t in buffers)
        self.lengths = torch.zeros(batch, dtype=torch.int32, device=device)

    def _native(self, *tensors: torch.Tensor) -> bool:
        lib = _native.library()
        return all(t.is_cuda for t in (*tensors, self.k_cache)) and all(getattr(lib, name, None) is not None for name in ("ffq_kv_append", "ffq_kv_decode"))

    def reset(self, lengths: torch.Tensor | Sequence[int] | None = None) -> None:
        """Every sequence back to length 0, or to `lengths` (the codes stay where they are: positions below a length are the cache)."""
        if lengths is None:
            self.lengths.zero_()
        else:
            self.lengths.copy_(torch.as_tensor(lengths, dtype=torch.int32).reshape(self.lengths.shape))

    def append(self, key: torch.Tensor, value: torch.Tensor, rope: Rope | None = None) -> None:
        """Quantize key / value ``[B, H, L, E]`` (plain values in the cache's dtype) to the end of every sequence: ``lengths += L``, then
        row l of batch b goes to position ``lengths[b] - L + l``; rows outside ``[0, max_len)`` are dropped. ``rope=(cos, sin)``,
        ``[P >= max_len, E]`` tables in the data dtype: K is rotated with the row of its position first."""
        if key.dim() != 4 or tuple(key.shape) != tuple(value.shape) or (key.shape[0], key.shape[1], key.shape[3]) != (self.k_cache.shape[0], self.k_cache.shape[1], self.k_cache.shape[3]):
            raise ValueError(f"QuantizedKVCache.append: key / value are [B, H, L, E] rows of a {tuple(self.k_cache.shape)} cache, got {tuple(key.shape)}, {tuple(value.shape)}")
        if key.dtype != self.dtype or value.dtype != self.dtype:
            raise ValueError(f"QuantizedKVCache.append: the new rows are plain {self.dtype} values, got {key.dtype}, {value.dtype}")
        k_params, v_params = _quantizer_params(self.key_quantizer, "key"), _quantizer_params(self.value_quantizer, "value")
        self.lengths.add_(key.shape[2])
        if self._native(key, value):
            ops.kv_append(key.detach(), value.detach(), self.k_cache, self.v_cache, self.lengths, k_params, v_params, rope=rope)
        else:
            composed_append(self.k_cache, self.v_cache, self.lengths, key.detach(), value.detach(), self.key_quantizer, self.value_quantizer, rope)

    def attend(self, query: Any, is_causal: bool = True, scale: float | None = None, output_quantizer: Any = None, splits: int = 0,
               plan_len: int | None = None) -> torch.Tensor:
        """Attention of query ``[B, H_q, L, E]`` (plain, or per-tensor codes in an int8 or value-dtype container) over every sequence's
        own keys; ``H_q`` is a multiple of the cache's heads (GQA). ``is_causal`` is bottom-right. `output_quantizer`: None, a stub, or
        one the decode kernels fuse (then the result is A2 of its codes in the data dtype). ``splits`` / ``plan_len``: ``ops.kv_decode``."""
        kernels = _kernels()
        if isinstance(query, QuantizedTensor):
            if kernels._codes_dtype(query, ("int8", "value")) != self.dtype:
                raise ValueError("QuantizedKVCache.attend: a quantized query holds per-tensor codes of the cache's dtype in an int8 or value-dtype container")
        elif type(query) is not torch.Tensor or query.dtype != self.dtype:
            raise ValueError(f"QuantizedKVCache.attend: the query is plain {self.dtype} or per-tensor codes of it")
        with torch.no_grad():
            fused = kernels._fused(output_quantizer)
        if fused is False:
            raise ValueError("QuantizedKVCache.attend: the output quantizer is not one the decode kernels fuse")
        raw, q_dequant = kernels._dequant(query)
        if not self._native(raw):
            return composed_attend(query, self.k_cache, self.v_cache, self.lengths, self.key_quantizer, self.value_quantizer, self.dtype,
                                   is_causal=is_causal, scale=scale, output_quantizer=output_quantizer if fused else None)
        k_params, v_params = _quantizer_params(self.key_quantizer, "key"), _quantizer_params(self.value_quantizer, "value")
        return ops.kv_decode(raw, self.k_cache, self.v_cache, self.lengths, is_causal=is_causal, scale=scale, output_quantizer=fused or None,
                             dequant=(q_dequant, k_params[:2], v_params[:2]), dtype=self.dtype, splits=splits, plan_len=plan_len)

    def keys(self, length: int) -> QuantizedTensor:
        """The first `length` positions of every sequence's keys as the QuantizedTensor the key quantizer would have returned."""
        return self.key_quantizer.wrap_codes(self.k_cache[:, :, :length], self.dtype)

    def values(self, length: int) -> QuantizedTensor:
        return self.value_quantizer.wrap_codes(self.v_cache[:, :, :length], self.dtype)
