"""The gather / scatter operators — ``index_add``, ``permute`` — registered in this package's dispatcher.

The reference registers no kernel for them: ff.nn.functional runs the generated fallbacks (src/fastforward/_gen/fallback.py:
permute :1427, index_add :1483) — A2 of every quantized input, ``torch.index_add`` / ``torch.permute``, the output quantizer: four
launches for an ``index_add`` of two quantized tensors (ATen's with bf16 atomics: the order of repeated indices, and with it the
result, changes from run to run), and A2, a strided view and a densifying A1 for a ``permute``. The predicates below accept what the
one-pass kernels of csrc/ffq_index.hip cover and return False for everything else, so the reference chain (the fallbacks in
:mod:`fastforward_amd.nn.functional`) runs unchanged there. They follow the rules of ``ConcatKernels`` (fused_concat.py):

* calls of ``ff.nn.functional`` only: a call without the ``strict_quantization`` keyword (``torch.index_add`` / ``x.permute``
  through ``QuantizedTensor.__torch_function__``) is declined;
* the operands on one HIP device and the device library loaded (the C oracle declines);
* bf16 / fp16 values, one dtype throughout: a plain tensor, or static-affine codes (int8 or value-dtype container, <= 8 bits, fp32
  parameters); fewer than 2^31 elements, none of the tensors empty (but ``index``);
* ``index_add``: ``input`` and ``source`` per tensor; ``input.dim() >= 1``; ``dim`` an int in range; ``index`` a plain 1-D int32 /
  int64 tensor on the device (``index.numel() == 0`` is a requantization of ``input``); ``source.shape`` equal to ``input.shape``
  but ``source.shape[dim] == index.numel()``; ``alpha`` a Python int / float (not a bool) that is finite in the value dtype. An
  index value out of range is skipped by the kernel; ATen asserts on the device and leaves the result undefined;
* ``permute``: an output quantizer (without one the result is a free view: the fallback's); ``dims`` a permutation of 1 to 6 axes
  (negative axes as ATen counts them); ``input`` per tensor or ``PerChannel`` on one axis;
* any layout: a strided or misaligned view reaches the kernel as an aligned copy (``ops._base._dense``);
* no operand that needs a gradient while grad mode is on (the launches have no autograd formula);
* under strict quantization, only calls the fallback would accept (an output quantizer, quantized inputs).

The output quantizer runs inside the launch under the int8 GEMM's ``_requant`` rules (fused_modules.py); otherwise the launch
writes the value and the quantizer is called on it, so range estimation still sees the value. Nothing reads device memory on the
host, so both calls can be captured in a ``torch.cuda.graph``.
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
from fastforward_amd.ops.index import MAX_RANK

_LIMIT = 2**31


def _finite_in(alpha: Any, dt: torch.dtype) -> bool:
    """`alpha` is a Python number whose value in `dt` (double -> fp32 -> `dt`, as ATen converts it) is finite."""
    if not _number(alpha):
        return False
    try:
        return math.isfinite(float(torch.tensor(float(alpha), dtype=torch.float32).to(dt)))
    except OverflowError:
        return False


class IndexKernels(MathKernels):
    """Predicates and kernels of ``index_add`` / ``permute`` (an ``ElementwiseKernels`` through ``MathKernels``, whose ``_call_ok``
    holds the rule for the ``strict_quantization`` keyword)."""

    def _per_tensor(self, x: Any) -> bool:
        return not isinstance(x, self._k.surface.quantized_tensor) or self._k._tile(x) == tuple(x.shape)

    # ---- index_add ------------------------------------------------------------------------------------------------------
    def supported_index_add(self, input: Any = None, dim: Any = None, index: Any = None, source: Any = None, alpha: Any = 1, *_args: Any,
                            output_quantizer: Any = None, **kwargs: Any) -> bool:
        if _args or not self._call_ok(kwargs, output_quantizer, input, source):
            return False
        dt = self._value_dtype(input)
        if dt is None or self._value_dtype(source) != dt or input.dim() < 1:
            return False
        d = _dim(dim, input.dim())
        if d is None or not self._per_tensor(input) or not self._per_tensor(source):
            return False
        if type(index) is not torch.Tensor or index.dim() != 1 or index.dtype not in (torch.int32, torch.int64):
            return False
        if tuple(source.shape) != (*input.shape[:d], index.numel(), *input.shape[d + 1:]):
            return False
        if input.numel() == 0 or input.numel() >= _LIMIT or source.numel() >= _LIMIT or not _finite_in(alpha, dt):
            return False
        if input.device != source.device or input.device != index.device or not _on_device(input, source, index):
            return False
        return not _needs_grad(input, source)

    def index_add(self, input: Any, dim: int, index: torch.Tensor, source: Any, alpha: Any = 1, *, output_quantizer: Any = None,
                  strict_quantization: bool | None = None) -> Any:
        dt = self._value_dtype(input)
        x, dequant = self._dequant(input)
        src, source_dequant = self._dequant(source)
        fused = self._output(output_quantizer, dt)
        value, codes = ops.index_add_quantize(x, dim, index, src, alpha, dtype=dt, dequant=dequant, source_dequant=source_dequant,
                                              **self._launch_args(fused))
        return self._finish(value, codes, fused, output_quantizer, dt)

    # ---- permute --------------------------------------------------------------------------------------------------------
    def _param_axis(self, x: Any) -> int | None | bool:
        """None for per-tensor parameters (or a plain tensor), the axis of ``PerChannel(axis)``, False for any other tiling."""
        if self._per_tensor(x):
            return None
        tile, full = self._k._tile(x), tuple(x.shape)
        axes = [i for i, (t, n) in enumerate(zip(tile, full)) if t != n]
        return axes[0] if len(axes) == 1 and tile[axes[0]] == 1 else False

    def supported_permute(self, input: Any = None, dims: Any = None, *_args: Any, output_quantizer: Any = None, **kwargs: Any) -> bool:
        if _args or output_quantizer is None or not self._call_ok(kwargs, output_quantizer, input):
            return False
        dt = self._value_dtype(input)
        if dt is None or not isinstance(dims, (tuple, list, torch.Size)) or not 1 <= input.dim() <= MAX_RANK or len(dims) != input.dim():
            return False
        axes = [_dim(d, input.dim()) for d in dims]
        if None in axes or sorted(axes) != list(range(input.dim())):
            return False
        if self._param_axis(input) is False:
            return False
        if input.numel() == 0 or input.numel() >= _LIMIT or not _on_device(input):
            return False
        return not _needs_grad(input)

    def permute(self, input: Any, dims: Any, *, output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        dt = self._value_dtype(input)
        x, dequant = self._dequant(input)
        fused = self._output(output_quantizer, dt)
        value, codes = ops.permute_quantize(x, tuple(dims), dtype=dt, dequant=dequant, param_axis=self._param_axis(input),
                                            **self._launch_args(fused))
        return self._finish(value, codes, fused, output_quantizer, dt)


KERNELS = IndexKernels(_LINEAR)
index_add_predicate = Predicate(KERNELS.supported_index_add)
permute_predicate = Predicate(KERNELS.supported_permute)
_registrations = {
    "index_add": register("index_add", index_add_predicate, KERNELS.index_add),
    "permute": register("permute", permute_predicate, KERNELS.permute),
}
