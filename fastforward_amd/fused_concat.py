"""The joining operators — ``cat``, ``pad`` — registered in this package's dispatcher.

The reference registers one kernel for them, the concatenation of the codes of tensors that share their parameters
(quantization/_linear_quantized_ops.py; it wins over the kernels here whenever it applies). Everything else runs the generated
fallbacks (src/fastforward/_gen/fallback.py: cat :1453, pad :1546) — A2 of every quantized input, ``torch.cat`` / ``F.pad``, the
output quantizer: N + 2 launches for a cat of N inputs, with a temporary between each. The predicates below accept what the one-pass
kernels of csrc/ffq_concat.hip cover and return False for everything else, so the reference chain (the fallbacks in
:mod:`fastforward_amd.nn.functional`) runs unchanged there. They follow the rules of ``MathKernels`` (fused_math.py):

* calls of ``ff.nn.functional`` only: a call without the ``strict_quantization`` keyword (``torch.cat`` / ``F.pad`` through
  ``QuantizedTensor.__torch_function__``) is declined;
* the inputs on one HIP device and the device library loaded (the C oracle declines);
* bf16 / fp16 values: a plain tensor, or static-affine codes (int8 or value-dtype container, <= 8 bits, fp32 parameters);
* ``cat``: a non-empty list or tuple; every element plain or per-tensor codes, each with its own parameters; one value dtype
  throughout (ATen would promote mixed ones); equal rank and equal sizes off ``dim``; no element without elements (ATen skips
  ``[0]``-shaped ones); ``dim`` an int in range; fewer than 2^31 output elements. Any width: nothing asks for a multiple of 8;
* ``pad``: one, two or three (left, right) pairs of ints; ``mode="constant"`` with any ``value`` ATen's fill takes (None is 0),
  negative pads included as long as one pad is positive (ATen answers a pure crop with a clone of a view, whose strides follow the
  input's); ``"reflect"`` / ``"replicate"`` for the ranks ATen takes (n pairs on an n + 1 or n + 2 dimensional input) with
  non-negative pads (reflect: smaller than the extent) and ``value`` None or 0; per-tensor codes, or per-channel (``PerChannel(1)``)
  ones when dim 1 is not padded; no empty input or result; fewer than 2^31 input and output elements. ``"circular"`` is declined;
* any layout but one: a strided or misaligned view reaches the kernel as an aligned copy (``ops._base._dense``); inputs whose
  strides are channels-last (``cat``: every one of them) are declined, because ATen answers them in channels-last;
* geometry ATen refuses is declined, so the fallback raises ATen's own error;
* no operand that needs a gradient while grad mode is on (the launches have no autograd formula);
* under strict quantization, only calls the fallback would accept (an output quantizer, quantized inputs).

The output quantizer runs inside the launch under the int8 GEMM's ``_requant`` rules (fused_modules.py); otherwise the launch
writes the value and the quantizer is called on it, so range estimation still sees the value. Nothing reads device memory on the
host: the fill of a constant pad reaches the kernel as bits computed on the host (``ops.concat.fill_bits``).
"""

from __future__ import annotations

import math

from typing import Any

import torch

from fastforward_amd import ops
from fastforward_amd.dispatcher import Predicate, register
from fastforward_amd.fused_elementwise import _number
from fastforward_amd.fused_linear import KERNELS as _LINEAR
from fastforward_amd.fused_math import MathKernels, _dim
from fastforward_amd.fused_modules import _needs_grad, _on_device
from fastforward_amd.fused_pool import _channels_last_strides
from fastforward_amd.ops.concat import PAD_MODES, fill_bits, padded_shape
from fastforward_amd.quantization._linear_quantized_ops import cat_predicate as code_level_cat_predicate

_LIMIT = 2**31


def _answers_channels_last(data: torch.Tensor) -> bool:
    """ATen's ``suggest_memory_format`` of `data` is channels-last (4-D) or channels-last-3d (5-D)."""
    if data.dim() == 4:
        return _channels_last_strides(data)
    return data.dim() == 5 and not data.is_contiguous() and data.is_contiguous(memory_format=torch.channels_last_3d)


class ConcatKernels(MathKernels):
    """Predicates and kernels of ``cat`` / ``pad`` (an ``ElementwiseKernels`` through ``MathKernels``, whose ``_call_ok`` holds the
    rule for the ``strict_quantization`` keyword)."""

    def _data(self, x: Any) -> torch.Tensor:
        return x.raw_data if isinstance(x, self._k.surface.quantized_tensor) else x

    # ---- cat ------------------------------------------------------------------------------------------------------------
    def supported_cat(self, tensors: Any = None, dim: Any = 0, *_args: Any, output_quantizer: Any = None, **kwargs: Any) -> bool:
        if _args or not isinstance(tensors, (list, tuple)) or not tensors:
            return False
        if not self._call_ok(kwargs, output_quantizer, *tensors):
            return False
        # tensors that share their parameters, without an output quantizer, are concatenated as codes (the reference's kernel)
        if code_level_cat_predicate(tensors, dim, output_quantizer=output_quantizer, **kwargs):
            return False
        dt = self._value_dtype(tensors[0])
        if dt is None:
            return False
        first = tensors[0]
        d = _dim(dim, first.dim())
        if d is None:
            return False
        total = 0
        for t in tensors:
            if self._value_dtype(t) != dt or t.dim() != first.dim() or t.numel() == 0 or t.device != first.device:
                return False
            if tuple(t.shape[:d]) != tuple(first.shape[:d]) or tuple(t.shape[d + 1:]) != tuple(first.shape[d + 1:]):
                return False
            if isinstance(t, self._k.surface.quantized_tensor) and self._k._tile(t) != tuple(t.shape):
                return False
            total += t.numel()
        if total >= _LIMIT or not _on_device(*tensors):
            return False
        if all(_answers_channels_last(self._data(t)) for t in tensors):
            return False
        return not _needs_grad(*tensors)

    def cat(self, tensors: Any, dim: int = 0, *, output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        dt = self._value_dtype(tensors[0])
        pairs = [self._dequant(t) for t in tensors]
        fused = self._output(output_quantizer, dt)
        value, codes = ops.cat_quantize([x for x, _ in pairs], dim, dtype=dt, dequant=[d for _, d in pairs], **self._launch_args(fused))
        return self._finish(value, codes, fused, output_quantizer, dt)

    # ---- pad ------------------------------------------------------------------------------------------------------------
    def supported_pad(self, input: Any = None, pad: Any = None, mode: Any = "...", value: Any = None, *_args: Any, output_quantizer: Any = None,
                      **kwargs: Any) -> bool:
        if _args or not self._call_ok(kwargs, output_quantizer, input):
            return False
        dt = self._value_dtype(input)
        if dt is None or input.numel() == 0 or input.numel() >= _LIMIT or not _on_device(input):
            return False
        if not isinstance(mode, str) or mode not in PAD_MODES or not isinstance(pad, (tuple, list, torch.Size)):
            return False
        pad = tuple(pad)
        k = len(pad) // 2
        if len(pad) not in (2, 4, 6) or k > input.dim() or any(isinstance(p, bool) or not isinstance(p, int) for p in pad):
            return False
        if mode == "constant":
            if max(pad) <= 0 or not (value is None or _number(value)):  # (nothing padded: ATen narrows and clones)
                return False
            try:
                fill_bits(value, dt)
            except (RuntimeError, OverflowError):  # a number ATen's fill refuses: its error is the fallback's to raise
                return False
        else:
            if input.dim() - k not in (1, 2) or min(pad) < 0 or not (value is None or (_number(value) and value == 0)):
                return False
            if mode == "reflect" and any(max(pad[2 * i], pad[2 * i + 1]) >= input.shape[-1 - i] for i in range(k)):
                return False
        shape = padded_shape(input.shape, pad)
        if min(shape) < 1 or math.prod(shape) >= _LIMIT:
            return False
        if isinstance(input, self._k.surface.quantized_tensor):
            tile, full = self._k._tile(input), tuple(input.shape)
            per_channel = input.dim() - k >= 2 and tile == (full[0], 1, *full[2:])
            if tile != full and not per_channel:
                return False
        if _answers_channels_last(self._data(input)):
            return False
        return not _needs_grad(input)

    def pad(self, input: Any, pad: Any, mode: str = "...", value: Any = None, *, output_quantizer: Any = None,
            strict_quantization: bool | None = None) -> Any:
        dt = self._value_dtype(input)
        x, dequant = self._dequant(input)
        fused = self._output(output_quantizer, dt)
        out, codes = ops.pad_quantize(x, tuple(pad), mode, value, dtype=dt, dequant=dequant, **self._launch_args(fused))
        return self._finish(out, codes, fused, output_quantizer, dt)


KERNELS = ConcatKernels(_LINEAR)
cat_predicate = Predicate(KERNELS.supported_cat)
pad_predicate = Predicate(KERNELS.supported_pad)
_registrations = {
    "cat": register("cat", cat_predicate, KERNELS.cat),
    "pad": register("pad", pad_predicate, KERNELS.pad),
}
