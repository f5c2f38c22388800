"""A quantizer for the OCP microscaling formats (``fastforward_amd.quantization.mx``): MXFP8 (e4m3) and MXFP4 (e2m1) with one power-of-two
scale per block of 32 elements of the last dimension.

``MXQuantizer`` has nothing to estimate: the scale of a block is a function of the block. It is dynamic, never uninitialised, and a range
estimator has nothing to set on it (it is not ``RangeSettable``: ``estimate_ranges(..., skip_unsupported_quantizers=True)`` passes it by).
Its output is a ``QuantizedTensor`` whose raw data is the one-code-per-byte uint8 container of the input's shape, so ``dequantize()`` and
every float fallback of ``nn.functional`` simulate the format anywhere; on the HIP device one ``ffq_mx_quantize`` launch writes the codes
and, for e2m1, the packed image ``functional.linear`` hands to the block-scaled GEMM (``fastforward_amd.fused_mx``)."""

from __future__ import annotations

from typing import Any

import torch

from fastforward_amd import _host
from fastforward_amd.exceptions import QuantizationError
from fastforward_amd.nn.quantizer import Quantizer
from fastforward_amd.quantization.function import QuantizationFunction
from fastforward_amd.quantization.mx import MXParameters, MXQuantizationFunction

NO_BACKWARD = ("MXQuantizer has no backward: the element codes have no gradient formula. Quantize under torch.no_grad() or detach the "
               "tensor.")


class MXQuantizer(Quantizer):
    """``element_format`` 'e2m1' (MXFP4) or 'e4m3' (MXFP8). `device` is the argument every quantizer's constructor takes (factories pass
    it along); it is checked to name a device, and that is all: there are no parameters to place, and the codes follow the data."""

    def __init__(self, element_format: str = "e2m1", *, device: torch.device | str | None = None) -> None:
        super().__init__()
        self.element_format = _host.mx_check_format(element_format)
        if device is not None:
            torch.device(device)  # (raises on a name that is no device)

    @property
    def has_uninitialized_params(self) -> bool:
        return False

    @property
    def block_size(self) -> int:
        return _host.MX_BLOCK

    def extra_repr(self) -> str:
        return f"element_format={self.element_format}, block_size={self.block_size}" + super().extra_repr()

    def quantization_parameters(self) -> MXParameters:
        return MXParameters(scale=None, element_format=self.element_format)

    @property
    def quantization_function(self) -> type[QuantizationFunction[Any]]:
        return MXQuantizationFunction

    def quantize(self, data: torch.Tensor) -> torch.Tensor:
        if torch.is_grad_enabled() and data.requires_grad:
            raise QuantizationError(NO_BACKWARD)
        return MXQuantizationFunction.quantize(data, self.quantization_parameters())

    def reset_parameters(self) -> None:
        pass
