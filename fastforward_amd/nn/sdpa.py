"""Quantized ``scaled_dot_product_attention``, its ``sdpa_upcast`` switch and the ATen-math implementation it dispatches to.

Reference: src/fastforward/nn/functional/custom/sdpa.py. :func:`scaled_dot_product_attention` is ``dispatch(...)`` first; the
``@register``-ed :func:`scaled_dot_product_attention_math` follows the reference step by step through this package's
``functional.mul / matmul / add / softmax / dropout`` (each of which still takes its own fused kernel where that kernel's predicate
accepts the step). On the device, ``fastforward_amd.fused_sdpa`` registers the one-launch kernel of csrc/ffq_sdpa.hip in front of it.
"""

from __future__ import annotations

import math

from typing import Any

import torch

from fastforward_amd import flags
from fastforward_amd.dispatcher import dispatch, register
from fastforward_amd.exceptions import QuantizationError
from fastforward_amd.flags import strict_quantization as strict_quantization_ctx
from fastforward_amd.nn import functional
from fastforward_amd.nn.quantizer import Quantizer, QuantizerStub
from fastforward_amd.ops.sdpa import QUANTIZER_SLOTS as QUANTIZER_NAMES  # the reference's keyword order = the kernel's slots


def scaled_dot_product_attention(
    query: torch.Tensor,
    key: torch.Tensor,
    value: torch.Tensor,
    attn_mask: torch.Tensor | None = None,
    dropout_p: float = 0.0,
    is_causal: bool = False,
    scale: float | None = None,
    enable_gqa: bool = False,
    *,
    neg_inf: float = float("-inf"),
    attn_scores_quantizer: Quantizer | None = None,
    attn_mask_quantizer: Quantizer | None = None,
    masked_scores_quantizer: Quantizer | None = None,
    attn_weights_quantizer: Quantizer | None = None,
    scaled_query_quantizer: Quantizer | None = None,
    scaled_key_quantizer: Quantizer | None = None,
    dropout_quantizer: Quantizer | None = None,
    output_quantizer: Quantizer | None = None,
    strict_quantization: bool | None = None,
    sdpa_torch_fallback: bool | None = None,
    **kwargs: Quantizer | None,
) -> torch.Tensor:
    """Quantized version of torch.nn.functional.scaled_dot_product_attention (reference sdpa.py:21-113).

    `sdpa_torch_fallback` (default: ``get_sdpa_torch_fallback_allowed()``) is accepted as the reference accepts it. The
    reference then calls torch's own SDPA when no quantizer is active, but throws that result away and returns the math path's
    value (sdpa.py:66-76); this function returns the same value and skips the discarded call.
    """
    if strict_quantization is None:
        strict_quantization = flags.get_strict_quantization()
    if sdpa_torch_fallback is None:
        sdpa_torch_fallback = flags.get_sdpa_torch_fallback_allowed()
    arguments: dict[str, Any] = dict(
        query=query,
        key=key,
        value=value,
        attn_mask=attn_mask,
        dropout_p=dropout_p,
        is_causal=is_causal,
        scale=scale,
        enable_gqa=enable_gqa,
        neg_inf=neg_inf,
        attn_scores_quantizer=attn_scores_quantizer,
        attn_mask_quantizer=attn_mask_quantizer,
        masked_scores_quantizer=masked_scores_quantizer,
        attn_weights_quantizer=attn_weights_quantizer,
        scaled_query_quantizer=scaled_query_quantizer,
        scaled_key_quantizer=scaled_key_quantizer,
        dropout_quantizer=dropout_quantizer,
        output_quantizer=output_quantizer,
        strict_quantization=strict_quantization,
        **kwargs,
    )
    selected_op = dispatch("scaled_dot_product_attention", **arguments)
    assert selected_op is not None
    return selected_op(**arguments)


@register("scaled_dot_product_attention")
def scaled_dot_product_attention_math(
    query: torch.Tensor,
    key: torch.Tensor,
    value: torch.Tensor,
    attn_mask: torch.Tensor | None = None,
    dropout_p: float = 0.0,
    is_causal: bool = False,
    scale: float | None = None,
    enable_gqa: bool = False,
    *,
    neg_inf: float = float("-inf"),
    attn_scores_quantizer: Quantizer | None = None,
    attn_mask_quantizer: Quantizer | None = None,
    masked_scores_quantizer: Quantizer | None = None,
    attn_weights_quantizer: Quantizer | None = None,
    scaled_query_quantizer: Quantizer | None = None,
    scaled_key_quantizer: Quantizer | None = None,
    dropout_quantizer: Quantizer | None = None,
    output_quantizer: Quantizer | None = None,
    strict_quantization: bool | None = None,
) -> torch.Tensor:
    """ATen's math SDPA with a quantizer after every step (reference sdpa.py:116-285).

    ``query`` [N, ..., H_q, L, E], ``key`` [N, ..., H, S, E], ``value`` [N, ..., H, S, E_v]; the result is [N, ..., H_q, L, E_v]
    in ``query``'s dtype. bf16 / fp16 operands are upcast to ``sdpa_upcast.dtype`` (fp32 by default) first; ``sqrt(scale)``
    multiplies both q and kᵀ; the bias comes from a bool mask (False -> `neg_inf`), a float mask, ``is_causal`` (top-left
    ``tril``) or is zero; the safe softmax gives 0 on rows whose (quantized) masked scores are all ``<= neg_inf``.

    Raises:
        ValueError: `attn_mask` together with `is_causal`.
        QuantizationError: `enable_gqa` under strict quantization, or a step the strict fallbacks reject.
    """
    L, S = query.size(-2), key.size(-2)
    if strict_quantization is None:
        strict_quantization = flags.get_strict_quantization()

    orig_dtype = query.dtype
    if sdpa_upcast.dtype is not None:
        if query.dtype == torch.float16 or query.dtype == torch.bfloat16:
            query = query.to(sdpa_upcast.dtype)
            key = key.to(sdpa_upcast.dtype)
            value = value.to(sdpa_upcast.dtype)

    if enable_gqa:
        if strict_quantization:
            raise QuantizationError("Strict quantization currently not supported when enable_gqa=True")
        with strict_quantization_ctx(False):
            key = key.repeat_interleave(query.size(-3) // key.size(-3), -3)
            value = value.repeat_interleave(query.size(-3) // value.size(-3), -3)

    scale_factor = 1.0 / math.sqrt(query.size(-1)) if scale is None else scale
    scale_factor_sqrt = math.sqrt(scale_factor)
    query = functional.mul(query, scale_factor_sqrt, output_quantizer=scaled_query_quantizer, strict_quantization=strict_quantization)
    key = functional.mul(key.transpose(-2, -1), scale_factor_sqrt, output_quantizer=scaled_key_quantizer, strict_quantization=strict_quantization)
    attn_scores = functional.matmul(query, key, output_quantizer=attn_scores_quantizer, strict_quantization=strict_quantization)
    attn_mask_bias = _get_quantized_attn_bias(attn_mask, is_causal, L, S, query.device, query.dtype, neg_inf=neg_inf, output_quantizer=attn_mask_quantizer)
    masked_attn_scores = functional.add(attn_scores, attn_mask_bias, output_quantizer=masked_scores_quantizer, strict_quantization=strict_quantization)
    attn_weight = _quantized_safe_softmax(masked_attn_scores, dim=-1, output_quantizer=attn_weights_quantizer, neg_inf=neg_inf)
    attn_weight = functional.dropout(attn_weight, dropout_p, training=True, output_quantizer=dropout_quantizer, strict_quantization=strict_quantization)
    attn_out = functional.matmul(attn_weight, value, output_quantizer=output_quantizer, strict_quantization=strict_quantization)
    return attn_out.to(orig_dtype)


def _get_quantized_attn_bias(
    attn_mask: torch.Tensor | None,
    is_causal: bool,
    L: int,
    S: int,
    device: torch.device | str,
    dtype: torch.dtype,
    *,
    neg_inf: float = float("-inf"),
    output_quantizer: Quantizer | None = None,
) -> torch.Tensor:
    """The additive bias of the scores (reference sdpa.py:288-324), through `output_quantizer` when one is given."""
    if attn_mask is not None and is_causal:
        raise ValueError("Explicit attn_mask should not be set when is_causal=True")  # torch's own message
    if attn_mask is not None:
        if attn_mask.dtype == torch.bool:
            attn_bias = torch.zeros_like(attn_mask, dtype=dtype, device=device)
            attn_bias.masked_fill_(attn_mask.logical_not(), neg_inf)
        else:
            attn_bias = attn_mask
    elif is_causal:
        temp_mask = torch.ones(L, S, dtype=torch.bool, device=device).tril(diagonal=0)
        attn_bias = torch.zeros(L, S, dtype=dtype, device=device)
        attn_bias.masked_fill_(temp_mask.logical_not(), neg_inf)
    else:
        attn_bias = torch.zeros(L, S, dtype=dtype, device=device)
    if output_quantizer is not None:
        attn_bias = output_quantizer(attn_bias)
    return attn_bias


def _quantized_safe_softmax(
    t: torch.Tensor,
    dim: int,
    dtype: torch.dtype | None = None,
    output_quantizer: Quantizer | None = None,
    neg_inf: float = float("-inf"),
) -> torch.Tensor:
    """ATen's safe softmax (a row that is masked everywhere gives 0), judged on `t` as given (reference sdpa.py:327-351)."""
    with strict_quantization_ctx(False):
        out = functional.softmax(t, dim, dtype)
        masked = t.isneginf() if neg_inf == float("-inf") else t <= neg_inf
        masked_rows = torch.all(masked, dim=dim, keepdim=True)
        zero = out.new_tensor(0.0)
        torch.where(condition=masked_rows, input=zero, other=out, out=out)
        if output_quantizer:
            out = output_quantizer(out)
    return out


def _is_quantizer_active(quantizer: Quantizer | None) -> bool:
    """True only for a quantizer that is neither None nor a stub (reference sdpa.py:354-356)."""
    return quantizer is not None and not isinstance(quantizer, QuantizerStub)


class _classproperty:
    def __init__(self, fget: Any) -> None:
        self.fget = fget

    def __get__(self, _obj: Any, owner: type) -> Any:
        return self.fget(owner)


class _SDPAUpcast:
    """Context manager selecting the dtype the math path upcasts bf16 / fp16 operands to (reference sdpa.py:405-456).

    ``sdpa_upcast(torch.float64)`` sets a dtype, ``sdpa_upcast(True)`` the default fp32, ``sdpa_upcast(False / None)`` turns
    upcasting off; leaving the ``with`` block restores the previous setting. ``sdpa_upcast.dtype`` reads it.
    """

    __DEFAULT_UPCAST_DTYPE: torch.dtype = torch.float32
    _DTYPE: torch.dtype | None = __DEFAULT_UPCAST_DTYPE

    def __init__(self, dtype: torch.dtype | bool | None):
        self._orig_dtype = _SDPAUpcast._DTYPE
        self._dtype: torch.dtype | None
        if isinstance(dtype, torch.dtype):
            self._dtype = dtype
        elif dtype:
            self._dtype = _SDPAUpcast.__DEFAULT_UPCAST_DTYPE
        else:
            self._dtype = None

    def __enter__(self) -> None:
        _SDPAUpcast._DTYPE = self._dtype

    def __exit__(self, *exc: object) -> None:
        _SDPAUpcast._DTYPE = self._orig_dtype

    @_classproperty
    def dtype(cls) -> torch.dtype | None:
        return cls._DTYPE

    @classmethod
    def upcast(cls, t: torch.Tensor) -> torch.Tensor:
        if cls.dtype:
            return t.to(cls.dtype)
        return t


sdpa_upcast = _SDPAUpcast
