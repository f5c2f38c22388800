"""Quantized ``torch.nn.LayerNorm`` (reference: src/fastforward/nn/normalization.py).

Slots ``input_quantizer`` (activation/input), ``weight_quantizer`` (parameter/weight) and ``bias_quantizer`` (parameter/bias) —
both ``None`` without ``elementwise_affine`` — and ``output_quantizer`` (activation/output); the reference's forward: quantize the
input, quantize weight and bias, functional ``layer_norm`` with the output quantizer (one HIP launch where
``fastforward_amd.fused_modules`` takes it).
"""

from __future__ import annotations

import torch

from fastforward_amd.nn.functional import layer_norm
from fastforward_amd.nn.quantized_module import QuantizedModule
from fastforward_amd.nn.quantizer import QuantizerStub


class QuantizedLayerNorm(QuantizedModule, torch.nn.LayerNorm):
    weight: torch.Tensor | None  # type: ignore[assignment]
    bias: torch.Tensor | None  # type: ignore[assignment]

    def __init_quantization__(self) -> None:
        super().__init_quantization__()
        self.input_quantizer = QuantizerStub(input_quantizer=True)
        if self.elementwise_affine:
            self.weight_quantizer = QuantizerStub(weight_quantizer=True)
            self.bias_quantizer = QuantizerStub(bias_quantizer=True)
        else:
            self.register_quantizer("weight_quantizer", None)
            self.register_quantizer("bias_quantizer", None)
        self.output_quantizer = QuantizerStub(output_quantizer=True)

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        input = self.input_quantizer(input)
        weight, bias = self.weight, self.bias
        if weight is not None and self.weight_quantizer is not None:
            weight = self.weight_quantizer(self.weight)
        if bias is not None and self.bias_quantizer is not None:
            bias = self.bias_quantizer(self.bias)
        return layer_norm(input, self.normalized_shape, weight=weight, bias=bias, eps=self.eps, output_quantizer=self.output_quantizer)
