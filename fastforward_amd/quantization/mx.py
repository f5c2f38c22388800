"""OCP microscaling (MX) as a quantization function: blocks of 32 consecutive elements of the last dimension share one power-of-two scale
(an E8M0 byte), elements are e4m3 (MXFP8) or e2m1 (MXFP4). The rule is stated in docs/numerics.md and include_mx/ffq_mx.h; the torch
restatement is ``fastforward_amd._host.mx_*`` and the kernels are ``fastforward_amd.ops.mx_*``. The reference project has no
float-element quantizer; this follows the OCP MX specification.

A quantized tensor's raw data is the one-code-per-byte uint8 container of the input's shape; ``MXParameters`` carries the scale bytes and,
for e2m1 tensors quantized on the device, the packed image (two codes per byte) that the same launch wrote — the GEMM's operand."""

from __future__ import annotations

import dataclasses

import torch

from fastforward_amd import _host, ops  # (both still importing when this module is: their names are looked up at call time)
from fastforward_amd.quantization.function import QuantizationContext, QuantizationFunction, QuantizationParameters
from fastforward_amd.quantized_tensor import QuantizedTensor

_KERNEL_DTYPES = (torch.bfloat16, torch.float16, torch.float32)


@dataclasses.dataclass
class MXParameters(QuantizationParameters):
    """`scale`: uint8 E8M0 codes ``[..., K / 32]`` (None before quantization); `element_format`: 'e4m3' | 'e2m1'; `packed`: the e2m1 codes two
    per byte ``[..., K / 2]`` when the quantizing launch wrote them, else None; `dequantize_dtype`: the dtype ``dequantize`` returns."""

    scale: torch.Tensor | None
    element_format: str
    packed: torch.Tensor | None = None
    dequantize_dtype: torch.dtype | None = None


def _on_kernel(data: torch.Tensor) -> bool:
    return data.is_cuda and data.dtype in _KERNEL_DTYPES and data.numel() > 0


class MXQuantizationFunction(QuantizationFunction[MXParameters]):
    @classmethod
    def quantize(cls, data: torch.Tensor, params: MXParameters) -> QuantizedTensor:
        fmt = _host.mx_check_format(params.element_format)
        if data.dim() < 1 or data.shape[-1] % _host.MX_BLOCK:
            raise ValueError(f"MX quantization: the last dimension must be a multiple of {_host.MX_BLOCK}, got shape {tuple(data.shape)}")
        if not data.is_floating_point():
            raise TypeError(f"MX quantization: floating-point data expected, got {data.dtype}")
        packed = None
        if _on_kernel(data):
            codes, packed, scale = ops.mx_quantize(data, fmt, codes=True, packed=fmt == "e2m1")
        else:
            codes, scale = _host.mx_quantize(data, fmt)
        new = params.with_changes(scale=scale, packed=packed, dequantize_dtype=params.dequantize_dtype or data.dtype)
        return QuantizationContext(cls, new).attach(codes)

    @classmethod
    def dequantize(cls, data: torch.Tensor, params: MXParameters) -> torch.Tensor:
        if params.scale is None:
            raise ValueError("MX dequantization: the parameters carry no scales")
        dtype = params.dequantize_dtype or torch.get_default_dtype()
        if data.is_cuda and data.numel() > 0 and data.dtype == torch.uint8 and dtype in _KERNEL_DTYPES and params.scale.device == data.device:
            return ops.mx_dequantize(data, params.scale, params.element_format, dtype)
        return _host.mx_dequantize(data, params.scale, params.element_format, dtype)
