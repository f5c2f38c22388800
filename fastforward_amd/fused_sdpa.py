"""``scaled_dot_product_attention`` on the one-launch kernel of csrc/ffq_sdpa.hip, registered in this package's dispatcher in front
of the math implementation (nn/sdpa.py, the reference's custom/sdpa.py:116-285).

The math path materialises the [B, H, L, S] fp32 scores five to seven times (scores, bias, masked scores, softmax, dropout and the
A1 / A2 pairs in between). The predicate below accepts what the kernel reproduces and returns False for everything else, so the math
path runs unchanged there:

* non-strict calls (after the fp32 upcast a strict call either raises in the math path, or holds int8 codes the upcast does not
  touch), no extra keyword quantizers, ``dropout_p == 0`` (the kernel cannot reproduce torch's RNG), ``sdpa_upcast.dtype`` fp32;
* q / k / v on the HIP device with the library loaded, 4-D [B, H, L|S, E], all bf16 or all fp16: plain tensors or per-tensor
  static-affine codes in that dtype (dequantized in registers); E = E_v in {64, 128}; the last dimension contiguous with 16-byte
  aligned rows (other strides are free: the ``[B, S, H, D].transpose(1, 2)`` view of a projection is not copied);
  H_q == H, or H_q a multiple of H with ``enable_gqa``;
* no mask, ``is_causal``, or a bool / float mask whose last two dims are [L, S] and whose leading dims broadcast (a float mask under
  an active mask quantizer must be fp32: its quantizer then sees what the chain's sees);
* each of the eight quantizers None, a ``QuantizerStub``, or one the int8 GEMM's ``_requant`` rule fuses (plain, initialised,
  per-tensor LinearQuantizer, fp32 parameters, no override — so not under ``estimate_ranges`` —, no hook, not export mode, no
  gradient), with 1..8 integral bits: if any active quantizer fails, the whole call declines, and calibration always runs the math
  path where the observers see every intermediate;
* no operand that needs a gradient while grad mode is on.
"""

from __future__ import annotations

import numbers

from typing import Any

import torch

from fastforward_amd import ops
from fastforward_amd.dispatcher import Predicate, register
from fastforward_amd.fused_linear import KERNELS as _LINEAR
from fastforward_amd.fused_modules import ModuleKernels, _needs_grad, _on_device, _settle
from fastforward_amd.nn.quantizer import QuantizerStub
from fastforward_amd.nn.sdpa import QUANTIZER_NAMES, sdpa_upcast

_VALUES = (torch.bfloat16, torch.float16)


def _number(x: Any) -> bool:
    return isinstance(x, numbers.Real) and not isinstance(x, bool)


class SdpaKernels(ModuleKernels):
    """Predicate and kernel of ``scaled_dot_product_attention``."""

    def _operand_dtype(self, x: Any) -> torch.dtype | None:
        """bf16 / fp16 of a plain operand or of per-tensor codes held in that dtype, else None."""
        if isinstance(x, self._k.surface.quantized_tensor):
            if not self._codes_ok(x) or self._k.row_mode(x) != "tensor":
                return None
            dt = self._k._deq_dtype(x)
            return dt if dt in _VALUES and x.raw_data.dtype == dt else None
        if type(x) is torch.Tensor and x.dtype in _VALUES:
            return x.dtype
        return None

    def _rows_ok(self, x: Any) -> bool:
        if isinstance(x, self._k.surface.quantized_tensor):
            x = x.raw_data
        return x.stride(-1) == 1 and x.data_ptr() % 16 == 0 and all(st % 8 == 0 for n, st in zip(x.shape[:3], x.stride()[:3]) if n > 1)

    def _fused(self, quantizer: Any) -> tuple[torch.Tensor, torch.Tensor | None, float] | None | bool:
        """(scale, offset, bits) of an active quantizer the kernel runs, None for an inactive slot, False when it declines."""
        if quantizer is None or isinstance(quantizer, QuantizerStub):
            return None
        fused = self._k._requant(quantizer, torch.float32)
        if fused is None or not 1 <= fused["out_num_bits"] <= 8:
            return False
        return fused["out_scale"], fused["out_offset"], fused["out_num_bits"]

    def supported(self, query: Any = None, key: Any = None, value: Any = None, attn_mask: Any = None, dropout_p: Any = 0.0, is_causal: Any = False,
                  scale: Any = None, enable_gqa: Any = False, *_args: Any, neg_inf: Any = float("-inf"), strict_quantization: Any = None, **kwargs: Any) -> bool:
        if _args or strict_quantization is not False or set(kwargs) - set(QUANTIZER_NAMES):
            return False
        if not (isinstance(dropout_p, (int, float)) and dropout_p == 0) or sdpa_upcast.dtype != torch.float32:
            return False
        if not _number(neg_inf) or not (scale is None or _number(scale)) or not isinstance(is_causal, bool) or not isinstance(enable_gqa, bool):
            return False
        dt = self._operand_dtype(query)
        if dt is None or self._operand_dtype(key) != dt or self._operand_dtype(value) != dt:
            return False
        if query.dim() != 4 or key.dim() != 4 or value.dim() != 4 or not _on_device(query, key, value):
            return False
        B, H, L, E = query.shape
        _, HKV, S, _ = key.shape
        if E not in (64, 128) or tuple(key.shape) != (B, HKV, S, E) or tuple(value.shape) != (B, HKV, S, E) or min(B, L, S) < 1:
            return False
        if HKV != H and not (enable_gqa and HKV >= 1 and H % HKV == 0):
            return False
        if not all(self._rows_ok(t) for t in (query, key, value)):
            return False
        active = {name: self._fused(kwargs.get(name)) for name in QUANTIZER_NAMES}
        if any(v is False for v in active.values()):
            return False
        if attn_mask is not None:
            if is_causal or type(attn_mask) is not torch.Tensor or not _on_device(attn_mask) or not 2 <= attn_mask.dim() <= 4:
                return False
            if attn_mask.dtype != torch.bool and attn_mask.dtype not in (torch.float32, *_VALUES):
                return False
            if attn_mask.dtype != torch.bool and active["attn_mask_quantizer"] is not None and attn_mask.dtype != torch.float32:
                return False
            lead = tuple(attn_mask.shape[:-2])
            if tuple(attn_mask.shape[-2:]) != (L, S) or any(n not in (1, full) for n, full in zip(reversed(lead), (H, B))):
                return False
        return not _needs_grad(query, key, value, *([] if attn_mask is None else [attn_mask]))

    def sdpa(self, query: Any, key: Any, value: Any, attn_mask: Any = None, dropout_p: float = 0.0, is_causal: bool = False, scale: Any = None,
             enable_gqa: bool = False, *, neg_inf: float = float("-inf"), strict_quantization: Any = None, **kwargs: Any) -> torch.Tensor:
        dequant = []
        operands = []
        for t in (query, key, value):
            if isinstance(t, self._k.surface.quantized_tensor):
                _settle(t)
                x, d = self._dequant(t)
                operands.append(x)
                dequant.append(d)
            else:
                operands.append(t)
                dequant.append(None)
        quantizers = {}
        for name in QUANTIZER_NAMES:
            fused = self._fused(kwargs.get(name))
            if fused:
                quantizers[name] = fused
        skip = is_causal and neg_inf == float("-inf") and "attn_mask_quantizer" not in quantizers and "masked_scores_quantizer" not in quantizers
        out, _ = ops.sdpa_quantize(*operands, attn_mask=attn_mask, is_causal=is_causal, scale=scale, neg_inf=neg_inf, quantizers=quantizers,
                                   dequant=dequant, skip_above_diagonal=skip)
        return out


KERNELS = SdpaKernels(_LINEAR)
sdpa_predicate = Predicate(KERNELS.supported)
_registration = register("scaled_dot_product_attention", sdpa_predicate, KERNELS.sdpa)
