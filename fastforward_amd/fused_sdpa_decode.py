"""``scaled_dot_product_attention`` for a short query over an int8 KV cache on the split-key kernels of csrc/ffq_sdpa_decode.hip,
registered in this package's dispatcher in front of the math implementation (nn/sdpa.py) and beside ``fused_sdpa``.

K / V kept as int8 codes (what ``LinearQuantizer(..., quantized_dtype=torch.int8)`` returns and the code-level ``cat`` of
quantization/_linear_quantized_ops.py appends to without dequantizing) decline in ``fused_sdpa``, whose kernel reads value-dtype
containers, so the call ran the math path: the whole cache dequantized, upcast to fp32 and repeated over the GQA group on every
step. The predicate below accepts exactly such calls, and only when everything else is what the kernels reproduce; every call
``fused_sdpa`` serves keeps its route (plain and value-dtype-container K / V are declined here), and everything else runs what it
ran before:

* non-strict calls, no extra keywords, ``dropout_p == 0``, ``sdpa_upcast.dtype`` fp32, nothing that needs a gradient;
* K and V both per-tensor static-affine codes in an int8 container: <= 8 bits, fp32 parameters, a dequantize dtype of bf16 or
  fp16 (the same for both); they carry separate parameter pairs, and offsets beyond int8 are fine;
* Q plain in that dtype, or per-tensor codes of it in an int8 or value-dtype container;
* 4-D tensors, ``E = E_v`` in {64, 128}, the last dimension contiguous and rows 16-byte aligned, other strides free (the
  ``[B, S, H, E].transpose(1, 2)`` view and a ``[:, :, :S]`` slice of a longer buffer are taken as they are);
* ``H_q == H``, or ``enable_gqa`` with ``H_q % H == 0``; ``L * (H_q / H) <= 32`` (longer queries over an int8 cache stay on the
  math path);
* ``neg_inf == -inf``;
* no mask, ``is_causal`` (the math path's top-left ``tril``), or a bool / fp32 / data-dtype mask ``[..., L, S]`` whose leading
  dims broadcast;
* every quantizer slot but ``output_quantizer`` None or a ``QuantizerStub``; ``output_quantizer`` None, a stub, or one the int8
  GEMM's ``_requant`` rule fuses, with 1..8 integral bits (it then runs in the combine kernel, and the call returns A2 of its codes in
  the data dtype, as ``fused_sdpa`` does);
* a device library that exports ``ffq_sdpa_decode``.
"""

from __future__ import annotations

import math

from typing import Any

import torch

from fastforward_amd import _native, ops
from fastforward_amd.dispatcher import Predicate, register
from fastforward_amd.fused_linear import KERNELS as _LINEAR
from fastforward_amd.fused_modules import _needs_grad, _on_device
from fastforward_amd.fused_sdpa import _VALUES, SdpaKernels, _number
from fastforward_amd.nn.quantizer import QuantizerStub
from fastforward_amd.nn.sdpa import QUANTIZER_NAMES, sdpa_upcast
from fastforward_amd.ops.decode import MAX_ROWS


class SdpaDecodeKernels(SdpaKernels):
    """Predicate and kernel of ``scaled_dot_product_attention`` over int8 K / V codes."""

    def _codes_dtype(self, x: Any, containers: tuple[str, ...]) -> torch.dtype | None:
        """The data dtype of per-tensor codes held in one of `containers` ("int8", "value"), else None."""
        if not isinstance(x, self._k.surface.quantized_tensor) or not self._codes_ok(x) or self._k.row_mode(x) != "tensor":
            return None
        dt = self._k._deq_dtype(x)
        held = "int8" if x.raw_data.dtype == torch.int8 else "value" if x.raw_data.dtype == dt else None
        return dt if dt in _VALUES and held in containers else None

    def _aligned_rows(self, x: Any) -> bool:
        if isinstance(x, self._k.surface.quantized_tensor):
            x = x.raw_data
        unit = 16 // x.element_size()
        return x.stride(-1) == 1 and x.data_ptr() % 16 == 0 and all(st % unit == 0 for n, st in zip(x.shape[:3], x.stride()[:3]) if n > 1)

    def supported(self, query: Any = None, key: Any = None, value: Any = None, attn_mask: Any = None, dropout_p: Any = 0.0, is_causal: Any = False,
                  scale: Any = None, enable_gqa: Any = False, *_args: Any, neg_inf: Any = float("-inf"), strict_quantization: Any = None, **kwargs: Any) -> bool:
        if _args or strict_quantization is not False or set(kwargs) - set(QUANTIZER_NAMES):
            return False
        if not (isinstance(dropout_p, (int, float)) and dropout_p == 0) or sdpa_upcast.dtype != torch.float32:
            return False
        if not _number(neg_inf) or not (neg_inf < 0 and math.isinf(neg_inf)):
            return False
        if not (scale is None or _number(scale)) or not isinstance(is_causal, bool) or not isinstance(enable_gqa, bool):
            return False
        dt = self._codes_dtype(key, ("int8",))
        if dt is None or self._codes_dtype(value, ("int8",)) != dt:
            return False
        if isinstance(query, self._k.surface.quantized_tensor):
            if self._codes_dtype(query, ("int8", "value")) != dt:
                return False
        elif type(query) is not torch.Tensor or query.dtype != dt:
            return False
        if query.dim() != 4 or key.dim() != 4 or value.dim() != 4 or not _on_device(query, key, value):
            return False
        if getattr(_native.library(), "ffq_sdpa_decode", None) is None:
            return False
        B, H, L, E = query.shape
        _, HKV, S, _ = key.shape
        if E not in (64, 128) or tuple(key.shape) != (B, HKV, S, E) or tuple(value.shape) != (B, HKV, S, E) or min(B, L, S) < 1:
            return False
        if HKV != H and not (enable_gqa and HKV >= 1 and H % HKV == 0):
            return False
        if L * (H // HKV) > MAX_ROWS:
            return False
        if not all(self._aligned_rows(t) for t in (query, key, value)):
            return False
        for name in QUANTIZER_NAMES:
            slot = kwargs.get(name)
            if name == "output_quantizer":
                if self._fused(slot) is False:
                    return False
            elif slot is not None and not isinstance(slot, QuantizerStub):
                return False
        if attn_mask is not None:
            if is_causal or type(attn_mask) is not torch.Tensor or not _on_device(attn_mask) or not 2 <= attn_mask.dim() <= 4:
                return False
            if attn_mask.dtype not in (torch.bool, torch.float32, dt):
                return False
            lead = tuple(attn_mask.shape[:-2])
            if tuple(attn_mask.shape[-2:]) != (L, S) or any(n not in (1, full) for n, full in zip(reversed(lead), (H, B))):
                return False
        return not _needs_grad(query, key, value, *([] if attn_mask is None else [attn_mask]))

    def sdpa(self, query: Any, key: Any, value: Any, attn_mask: Any = None, dropout_p: float = 0.0, is_causal: bool = False, scale: Any = None,
             enable_gqa: bool = False, *, neg_inf: float = float("-inf"), strict_quantization: Any = None, **kwargs: Any) -> torch.Tensor:
        dt = self._k._deq_dtype(key)
        operands, dequant = zip(*(self._dequant(t) for t in (query, key, value)))
        fused = self._fused(kwargs.get("output_quantizer"))
        return ops.sdpa_decode(*operands, attn_mask=attn_mask, is_causal=is_causal, scale=scale, output_quantizer=fused or None,
                               dequant=dequant, dtype=dt)


KERNELS = SdpaDecodeKernels(_LINEAR)
sdpa_decode_predicate = Predicate(KERNELS.supported)
_registration = register("scaled_dot_product_attention", sdpa_decode_predicate, KERNELS.sdpa)
