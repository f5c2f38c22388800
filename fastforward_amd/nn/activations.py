"""Quantized activations (reference: src/fastforward/nn/activations.py): ``QuantizedRelu`` and ``QuantizedSilu``.

Both carry ``input_quantizer`` (activation/input) and ``output_quantizer`` (activation/output), never run in place, and call the
functional ``relu`` / ``silu`` with the output quantizer (one HIP launch where ``fastforward_amd.fused_modules`` takes it).
"""

from __future__ import annotations

import torch

from fastforward_amd.nn.functional import relu, silu
from fastforward_amd.nn.quantized_module import QuantizedModule
from fastforward_amd.nn.quantizer import QuantizerStub


class QuantizedActivation(QuantizedModule, include_in_module_map=False):
    """Base class for quantized activations."""

    def __init_quantization__(self) -> None:
        super().__init_quantization__()
        self.input_quantizer = QuantizerStub(input_quantizer=True)
        self.output_quantizer = QuantizerStub(output_quantizer=True)


class QuantizedRelu(QuantizedActivation, torch.nn.ReLU):
    def __init_quantization__(self) -> None:
        super().__init_quantization__()
        self.inplace = False

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        return relu(self.input_quantizer(input), output_quantizer=self.output_quantizer)


class QuantizedSilu(QuantizedActivation, torch.nn.SiLU):
    def __init_quantization__(self) -> None:
        super().__init_quantization__()
        self.inplace = False

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        return silu(self.input_quantizer(input), output_quantizer=self.output_quantizer)
