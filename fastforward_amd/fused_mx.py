"""``linear`` on two MX tensors (``fastforward_amd.quantization.mx``): one registration in the quantized-operator dispatcher.

The predicate accepts only an input and a weight that are both ``QuantizedTensor``s with an ``MXQuantizationFunction`` context, on the HIP
device, on a format pair and shapes ``ffq_linear_mx_supported`` takes, when no gradient is needed; the kernel is one ``ffq_linear_mx``
launch on the codes (e4m3 bytes, e2m1 packed) and scale bytes, and an output quantizer runs on the result as its own call. Everything else
is declined and takes the float chain (dequantize both, ``F.linear``) — the value this kernel approximates within fp32 accumulation."""

from __future__ import annotations

from typing import Any

import torch

from fastforward_amd import _host, _native, ops
from fastforward_amd.dispatcher import Predicate, register
from fastforward_amd.exceptions import QuantizationError
from fastforward_amd.quantization.mx import MXQuantizationFunction
from fastforward_amd.quantized_tensor import QuantizedTensor

_FLOATS = (torch.bfloat16, torch.float16, torch.float32)


def is_mx(t: Any) -> bool:
    return isinstance(t, QuantizedTensor) and issubclass(t.quantization_context.quantization_fn, MXQuantizationFunction)


def _params(t: Any) -> Any:
    return t.quantization_context.quantization_params


def _gemm_codes(t: Any) -> torch.Tensor:
    """The code matrix ``ffq_linear_mx`` reads: e4m3 bytes, e2m1 the packed image the quantizing launch left."""
    p = _params(t)
    codes = t.raw_data if p.element_format == "e4m3" else p.packed
    return codes.reshape(-1, codes.shape[-1])


def _has_gemm_codes(t: Any) -> bool:
    """An e2m1 tensor without the packed image of its launch (quantized on the host and moved, or built by hand) is declined: packing
    it here would be an extra pass the caller did not ask for."""
    p = _params(t)
    if p.element_format == "e4m3":
        return True
    return p.packed is not None and p.packed.device == t.device and p.packed.dtype == torch.uint8 and p.packed.is_contiguous() \
        and tuple(p.packed.shape) == (*t.shape[:-1], t.shape[-1] // 2)


def supported_linear_mx(input: Any = None, weight: Any = None, bias: Any = None, **_: Any) -> bool:
    if not (is_mx(input) and is_mx(weight)):
        return False
    pi, pw = _params(input), _params(weight)
    if pi.scale is None or pw.scale is None or not (input.is_cuda and weight.is_cuda and input.device == weight.device):
        return False
    if pi.scale.device != input.device or pw.scale.device != weight.device or not _native.library().is_device:
        return False
    if weight.dim() != 2 or input.dim() < 1 or input.numel() == 0 or input.shape[-1] != weight.shape[1]:
        return False
    if input.raw_data.dtype != torch.uint8 or weight.raw_data.dtype != torch.uint8 or not input.raw_data.is_contiguous() or not weight.raw_data.is_contiguous():
        return False
    if not (_has_gemm_codes(input) and _has_gemm_codes(weight)):
        return False
    deq = pi.dequantize_dtype or torch.get_default_dtype()
    if deq not in _FLOATS or (pw.dequantize_dtype or deq) != deq:
        return False  # the float chain would raise on mixed dtypes; let it
    if bias is not None and (isinstance(bias, QuantizedTensor) or not isinstance(bias, torch.Tensor) or bias.dtype not in (torch.float32, deq)
                             or bias.device != input.device or bias.shape != (weight.shape[0],)):
        return False
    if torch.is_grad_enabled() and ((bias is not None and bias.requires_grad) or input.requires_grad or weight.requires_grad):
        return False
    K = weight.shape[1]
    return ops.linear_mx_supported(input.numel() // K, weight.shape[0], K, pi.element_format, pw.element_format)


def fused_linear_mx(input: Any, weight: Any, bias: Any = None, *, output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
    if strict_quantization and output_quantizer is None:
        raise QuantizationError("'output_quantizer' must be provided if strict_quantization=True")
    pi, pw = _params(input), _params(weight)
    deq = pi.dequantize_dtype or torch.get_default_dtype()
    K = weight.shape[1]
    out = ops.linear_mx(_gemm_codes(input), pi.scale.reshape(-1, K // _host.MX_BLOCK), pi.element_format, _gemm_codes(weight),
                        pw.scale.reshape(-1, K // _host.MX_BLOCK), pw.element_format, bias=bias, out_dtype=deq)
    out = out.reshape(*input.shape[:-1], weight.shape[0])
    return output_quantizer(out) if output_quantizer is not None else out


fused_linear_mx_predicate = Predicate(supported_linear_mx)
_registration = register("linear", fused_linear_mx_predicate, fused_linear_mx)
