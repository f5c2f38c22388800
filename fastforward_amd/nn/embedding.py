"""Quantized ``torch.nn.Embedding`` (reference: src/fastforward/nn/embedding.py).

Slots ``weight_quantizer`` (parameter/weight) and ``output_quantizer`` (activation/output); the reference's forward: quantize the
table, functional ``embedding`` with the output quantizer (one HIP launch — gather, A2, A1 — where
``fastforward_amd.fused_modules`` takes it).
"""

from __future__ import annotations

import torch

from fastforward_amd.nn.functional import embedding
from fastforward_amd.nn.quantized_module import QuantizedModule
from fastforward_amd.nn.quantizer import QuantizerStub


class QuantizedEmbedding(QuantizedModule, torch.nn.Embedding):
    def __init_quantization__(self) -> None:
        super().__init_quantization__()
        self.weight_quantizer = QuantizerStub(weight_quantizer=True)
        self.output_quantizer = QuantizerStub(output_quantizer=True)

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        return embedding(
            input, self.weight_quantizer(self.weight), self.padding_idx, self.max_norm, self.norm_type, self.scale_grad_by_freq, self.sparse,
            output_quantizer=self.output_quantizer,
        )
