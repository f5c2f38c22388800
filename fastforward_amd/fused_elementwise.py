"""The elementwise operators — ``add``, ``sub``, ``mul``, ``div``, ``softmax``, ``sigmoid``, ``gelu`` — registered in this package's
dispatcher.

The reference registers no kernel for them (but ``mul`` by a number: quantization/_linear_quantized_ops.py): ff.nn.functional runs
the generated fallbacks (src/fastforward/_gen/fallback.py: softmax :269, sigmoid :321, add :801, sub :840, mul :879, div :917,
gelu :1373) — A2 of each quantized operand, the ATen op, the output quantizer: up to four launches with a temporary between each.
The predicates below accept what the one-pass kernels of csrc/ffq_elementwise.hip cover and return False for everything else, so
the reference chain (the fallbacks in :mod:`fastforward_amd.nn.functional`) runs unchanged there:

* calls of ``ff.nn.functional`` only: a call without the ``strict_quantization`` keyword is declined. ``qa + qb``,
  ``torch.softmax(qa, -1)`` ... reach these registrations through ``QuantizedTensor.__torch_function__`` with positional
  arguments and keep the dequantization fallback (which raises under strict quantization);
* operands on the HIP device and the device library loaded (the C oracle declines);
* bf16 / fp16 values: a plain tensor, or static-affine codes (int8 or value-dtype container, <= 8 bits, fp32 parameters) with
  per-tensor or per-row parameters; both tensor operands of one value dtype (ATen would promote mixed ones);
* ``other`` of ``input``'s shape, of a suffix of it (a bias [D] against [B, S, D]), or a Python number — never a 0-dim tensor or a
  broadcast of ``input`` itself; ``mul`` by a number of a per-tensor affine tensor without an output quantizer is the reference's
  rescale (``scalar_multiply``) and is left to it;
* softmax over the last dimension, ``dtype`` None or the value dtype, 8 | cols <= 16384; ``gelu`` with approximate "none" / "tanh";
* sizes: 8 | numel (and 8 | the row of per-row parameters);
* any layout: a strided view, or a contiguous one at a misaligned address (``x[1:]``, a split of a flat buffer), reaches the
  kernel as an aligned copy (``ops._base._dense``; the kernels read 16-byte aligned buffers only), a dense aligned operand as it is;
* no operand or parameter that needs a gradient while grad mode is on (the launches have no autograd formula);
* under strict quantization, only calls the fallback would accept (an output quantizer, quantized tensor operands).

The output quantizer runs inside the launch under the int8 GEMM's ``_requant`` rules (fused_modules.py); otherwise the launch
writes the value and the quantizer is called on it, so range estimation still sees the value.
"""

from __future__ import annotations

from typing import Any

import torch

from fastforward_amd import ops
from fastforward_amd.dispatcher import Predicate, register
from fastforward_amd.fused_linear import KERNELS as _LINEAR
from fastforward_amd.fused_modules import ModuleKernels, _needs_grad, _on_device
from fastforward_amd.quantization._linear_quantized_ops import scalar_multiply_predicate


def _number(x: Any) -> bool:
    """A Python number ATen takes as an fp32 scalar (a bool is not one; an int beyond any float is not either)."""
    if isinstance(x, bool) or not isinstance(x, (int, float)):
        return False
    return isinstance(x, float) or abs(x) < 2**64


class ElementwiseKernels(ModuleKernels):
    """Predicates and kernels of ``add`` / ``sub`` / ``mul`` / ``div`` / ``softmax`` / ``sigmoid`` / ``gelu``."""

    # ---- what an operand is ------------------------------------------------------------------------------------------
    def _streamed(self, x: Any) -> torch.dtype | None:
        """The value dtype of a non-empty operand on the device in a form the kernels take (8 | the per-row run), else None."""
        dt = self._value_dtype(x)
        if dt is None or x.dim() == 0 or x.numel() == 0 or x.numel() % 8 or not _on_device(x):
            return None
        if isinstance(x, self._k.surface.quantized_tensor):
            mode = self._k.row_mode(x)
            if mode is None or (mode == "row" and x.shape[-1] % 8):
                return None
        return dt

    def _broadcast_ok(self, other: torch.Tensor, input: Any) -> bool:
        shape = list(other.shape)
        while shape and shape[0] == 1:
            shape.pop(0)
        return other.dim() <= input.dim() and tuple(input.shape[input.dim() - len(shape):]) == tuple(shape)

    # ---- add / sub / mul / div ----------------------------------------------------------------------------------------
    def _supported_binary(self, input: Any, other: Any, alpha: Any, output_quantizer: Any, kwargs: dict[str, Any]) -> bool:
        if "strict_quantization" not in kwargs or "out" in kwargs:
            return False
        operands = [input] + ([other] if isinstance(other, torch.Tensor) else [])
        if not self._strict_ok(kwargs["strict_quantization"], output_quantizer, *operands):
            return False
        if not _number(alpha):
            return False
        dt = self._streamed(input)
        if dt is None:
            return False
        if isinstance(other, torch.Tensor):
            if self._streamed(other) != dt or not self._broadcast_ok(other, input):
                return False
        elif not _number(other):
            return False
        return not _needs_grad(*operands)

    def supported_add(self, input: Any = None, other: Any = None, *_args: Any, alpha: Any = 1, output_quantizer: Any = None, **kwargs: Any) -> bool:
        return not _args and self._supported_binary(input, other, alpha, output_quantizer, kwargs)

    def supported_div(self, input: Any = None, other: Any = None, *_args: Any, output_quantizer: Any = None, **kwargs: Any) -> bool:
        return not _args and "alpha" not in kwargs and self._supported_binary(input, other, 1, output_quantizer, kwargs)

    def supported_mul(self, input: Any = None, other: Any = None, *_args: Any, output_quantizer: Any = None, **kwargs: Any) -> bool:
        # a per-tensor affine input times a number without an output quantizer is the reference's rescale of the scale
        if scalar_multiply_predicate(input, other, output_quantizer=output_quantizer, **kwargs):
            return False
        return self.supported_div(input, other, *_args, output_quantizer=output_quantizer, **kwargs)

    def _binary(self, op: str, input: Any, other: Any, alpha: Any, output_quantizer: Any) -> Any:
        dt = self._value_dtype(input)
        a, a_deq = self._dequant(input)
        b, b_deq = self._dequant(other) if isinstance(other, torch.Tensor) else (other, None)
        fused = self._output(output_quantizer, dt)
        value, codes = ops.binary_quantize(op, a, b, dtype=dt, a_dequant=a_deq, b_dequant=b_deq, alpha=alpha, **self._launch_args(fused))
        return self._finish(value, codes, fused, output_quantizer, dt)

    def add(self, input: Any, other: Any, alpha: Any = 1, *, output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        return self._binary("add", input, other, alpha, output_quantizer)

    def sub(self, input: Any, other: Any, alpha: Any = 1, *, output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        return self._binary("sub", input, other, alpha, output_quantizer)

    def mul(self, input: Any, other: Any, *, output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        return self._binary("mul", input, other, 1, output_quantizer)

    def div(self, input: Any, other: Any, *, output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        return self._binary("div", input, other, 1, output_quantizer)

    # ---- softmax ------------------------------------------------------------------------------------------------------
    def supported_softmax(self, input: Any = None, dim: Any = None, *_args: Any, dtype: Any = None, output_quantizer: Any = None, **kwargs: Any) -> bool:
        if _args or "strict_quantization" not in kwargs or "out" in kwargs:
            return False
        if not self._strict_ok(kwargs["strict_quantization"], output_quantizer, input):
            return False
        dt = self._streamed(input)
        if dt is None or not isinstance(dim, int) or isinstance(dim, bool) or dim not in (-1, input.dim() - 1):
            return False
        if dtype is not None and dtype != dt:
            return False
        if input.shape[-1] % 8 or input.shape[-1] > 16384:
            return False
        return not _needs_grad(input)

    def softmax(self, input: Any, dim: int, dtype: Any = None, *, output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        dt = self._value_dtype(input)
        x, dequant = self._dequant(input)
        fused = self._output(output_quantizer, dt)
        value, codes = ops.softmax_quantize(x, dtype=dt, dequant=dequant, **self._launch_args(fused))
        return self._finish(value, codes, fused, output_quantizer, dt)

    # ---- sigmoid / gelu -----------------------------------------------------------------------------------------------
    def supported_activation(self, input: Any = None, *_args: Any, approximate: Any = "none", output_quantizer: Any = None, **kwargs: Any) -> bool:
        if _args or "strict_quantization" not in kwargs or "out" in kwargs or approximate not in ("none", "tanh"):
            return False
        if not self._strict_ok(kwargs["strict_quantization"], output_quantizer, input):
            return False
        return self._streamed(input) is not None and not _needs_grad(input)

    def _activation(self, op: str, input: Any, output_quantizer: Any) -> Any:
        dt = self._value_dtype(input)
        x, dequant = self._dequant(input)
        fused = self._output(output_quantizer, dt)
        value, codes = ops.activation_quantize(op, x, dtype=dt, dequant=dequant, **self._launch_args(fused))
        return self._finish(value, codes, fused, output_quantizer, dt)

    def sigmoid(self, input: Any, *, output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        return self._activation("sigmoid", input, output_quantizer)

    def gelu(self, input: Any, approximate: str = "none", *, output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        return self._activation("gelu_tanh" if approximate == "tanh" else "gelu", input, output_quantizer)


KERNELS = ElementwiseKernels(_LINEAR)
add_predicate = Predicate(KERNELS.supported_add)
mul_predicate = Predicate(KERNELS.supported_mul)
div_predicate = Predicate(KERNELS.supported_div)
softmax_predicate = Predicate(KERNELS.supported_softmax)
activation_predicate = Predicate(KERNELS.supported_activation)
_registrations = {
    "add": register("add", add_predicate, KERNELS.add),
    "sub": register("sub", add_predicate, KERNELS.sub),
    "mul": register("mul", mul_predicate, KERNELS.mul),
    "div": register("div", div_predicate, KERNELS.div),
    "softmax": register("softmax", softmax_predicate, KERNELS.softmax),
    "sigmoid": register("sigmoid", activation_predicate, KERNELS.sigmoid),
    "gelu": register("gelu", activation_predicate, KERNELS.gelu),
}
