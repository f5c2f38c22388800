"""Quantized ``torch.nn.Conv2d`` / ``torch.nn.Conv1d`` (reference: src/fastforward/nn/conv.py).

Slots ``input_quantizer`` (activation/input), ``weight_quantizer`` (parameter/weight, shape = the weight's), ``bias_quantizer``
(parameter/bias; ``None`` without a bias) and ``output_quantizer`` (activation/output); the reference's forward: quantize the
input and the weight, the bias if there is one, then functional ``conv2d`` / ``conv1d`` with stride, padding, dilation and groups
— ``padding_mode`` is not consulted, as in the reference (one HIP implicit GEMM where ``fastforward_amd.fused_conv`` takes it).

Neither class is in the global module map: ``ff.quantize_model`` keeps raising on a model with a convolution unless it is asked to
convert them, as the Llama harness asks for its embedding class::

    ff.quantize_model(model, extra_conversion=ff.nn.quantized_conv_modules())

``QuantizedConvTranspose1d`` / ``QuantizedConvTranspose2d`` have no counterpart in the reference (it has the functional operators
only): they follow ``_QuantizedConv`` — the same four slots — and ``torch.nn.ConvTranspose2d.forward`` for ``output_size``. They are
offered through ``ff.nn.quantized_conv_transpose_modules()``; ``quantized_conv_modules()`` stays Conv1d / Conv2d.

``QuantizedConv3d`` has no counterpart in the reference either (functional ``conv3d`` only): it is ``_QuantizedConv`` on
``torch.nn.Conv3d``, offered through ``ff.nn.quantized_conv3d_modules()``.
"""

from __future__ import annotations

from typing import Callable

import torch

from fastforward_amd.nn.functional import conv1d, conv2d, conv3d, conv_transpose1d, conv_transpose2d
from fastforward_amd.nn.quantized_module import QuantizedModule
from fastforward_amd.nn.quantizer import Quantizer, QuantizerStub


class _QuantizedConv(QuantizedModule, include_in_module_map=False):
    weight_quantizer: Quantizer
    bias_quantizer: Quantizer | None
    input_quantizer: Quantizer
    output_quantizer: Quantizer
    _functional: Callable[..., torch.Tensor]

    def __init_quantization__(self) -> None:
        super().__init_quantization__()
        self.input_quantizer = QuantizerStub(input_quantizer=True)
        self.weight_quantizer = QuantizerStub(weight_quantizer=True, shape=self.weight.shape)
        if self.bias is not None:
            self.bias_quantizer = QuantizerStub(bias_quantizer=True, shape=self.bias.shape)
        else:
            self.register_quantizer("bias_quantizer", None)
        self.output_quantizer = QuantizerStub(output_quantizer=True)

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        input = self.input_quantizer(input)
        weight = self.weight_quantizer(self.weight)
        bias = self.bias
        if bias is not None and self.bias_quantizer is not None:
            bias = self.bias_quantizer(bias)
        return type(self)._functional(input, weight, bias, self.stride, self.padding, self.dilation, self.groups, output_quantizer=self.output_quantizer)


class QuantizedConv2d(_QuantizedConv, torch.nn.Conv2d, include_in_module_map=False):
    _functional = staticmethod(conv2d)


class QuantizedConv1d(_QuantizedConv, torch.nn.Conv1d, include_in_module_map=False):
    _functional = staticmethod(conv1d)


class QuantizedConv3d(_QuantizedConv, torch.nn.Conv3d, include_in_module_map=False):
    _functional = staticmethod(conv3d)


class _QuantizedConvTranspose(_QuantizedConv, include_in_module_map=False):
    _dims: int

    def forward(self, input: torch.Tensor, output_size: list[int] | None = None) -> torch.Tensor:  # type: ignore[override]
        # output_padding from the plain input's shape, as torch.nn.ConvTranspose2d.forward computes it
        output_padding = self._output_padding(input, output_size, self.stride, self.padding, self.kernel_size, self._dims, self.dilation)
        input = self.input_quantizer(input)
        weight = self.weight_quantizer(self.weight)
        bias = self.bias
        if bias is not None and self.bias_quantizer is not None:
            bias = self.bias_quantizer(bias)
        return type(self)._functional(input, weight, bias, self.stride, self.padding, output_padding, self.groups, self.dilation,
                                      output_quantizer=self.output_quantizer)


class QuantizedConvTranspose2d(_QuantizedConvTranspose, torch.nn.ConvTranspose2d, include_in_module_map=False):
    _functional = staticmethod(conv_transpose2d)
    _dims = 2


class QuantizedConvTranspose1d(_QuantizedConvTranspose, torch.nn.ConvTranspose1d, include_in_module_map=False):
    _functional = staticmethod(conv_transpose1d)
    _dims = 1


def quantized_conv_modules() -> dict[type[torch.nn.Module], type[QuantizedModule]]:
    """The ``extra_conversion`` entries of ``quantize_model`` (and ``surrogate_quantized_modules``) that convert Conv1d / Conv2d."""
    return {torch.nn.Conv1d: QuantizedConv1d, torch.nn.Conv2d: QuantizedConv2d}


def quantized_conv_transpose_modules() -> dict[type[torch.nn.Module], type[QuantizedModule]]:
    """The ``extra_conversion`` entries of ``quantize_model`` that convert ConvTranspose1d / ConvTranspose2d."""
    return {torch.nn.ConvTranspose1d: QuantizedConvTranspose1d, torch.nn.ConvTranspose2d: QuantizedConvTranspose2d}


def quantized_conv3d_modules() -> dict[type[torch.nn.Module], type[QuantizedModule]]:
    """The ``extra_conversion`` entry of ``quantize_model`` that converts Conv3d."""
    return {torch.nn.Conv3d: QuantizedConv3d}
