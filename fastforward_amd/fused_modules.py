"""The generic modules' operators — ``layer_norm``, ``embedding``, ``relu``, ``silu`` — registered in this package's dispatcher.

The reference registers no kernel for them: QuantizedLayerNorm / QuantizedEmbedding / QuantizedRelu / QuantizedSilu run the
generated fallbacks (src/fastforward/_gen/fallback.py: relu :296, embedding :616, layer_norm :655, silu :1348) — A2 of the
quantized operand, the ATen op, the output quantizer: three launches with a temporary between each. The predicates below accept
what the one-pass kernels of csrc/ffq_modules.hip cover and return False for everything else, so the reference chain (the
fallbacks in :mod:`fastforward_amd.nn.functional`) runs unchanged there:

* operands on the HIP device and the device library loaded (the C oracle declines);
* bf16 / fp16 values: a plain tensor, or static-affine codes (int8 or value-dtype container, <= 8 bits, fp32 parameters) with
  per-tensor or per-row parameters; an embedding table per tensor, per row, per column or in groups of G % 8 == 0 along D;
* sizes: 8 | the row (LayerNorm: 8 | cols <= 16384; Embedding: 8 | D; ReLU / SiLU: 8 | numel); ``max_norm is None``;
* any layout: a strided view, or a contiguous one at a misaligned address (``x[1:]``, a split of a flat buffer), reaches the
  kernel as an aligned copy (``ops._base._dense``; the kernels read 16-byte aligned buffers only), a dense aligned operand as it is;
* no operand or parameter that needs a gradient while grad mode is on (the launches have no autograd formula).

The output quantizer runs inside the launch under the rules that decide it for the int8 GEMM (``DispatcherKernels._requant``:
a plain initialised per-tensor ``LinearQuantizer`` with an int8 container, no override — so range estimation is excluded — no
hook, not export mode, no gradient); otherwise the launch writes the value and the quantizer is called on it.
An embedding id outside [0, V) gives a row of zeros here (ATen's device kernel asserts); ``ops.embedding_quantize`` reports the
position in a device word, which this route does not read (reading it synchronises).
"""

from __future__ import annotations

import math

from typing import Any

import torch

from fastforward_amd import _native, ops
from fastforward_amd.dispatcher import Predicate, register
from fastforward_amd.fused_linear import KERNELS as _LINEAR

_VALUES = (torch.bfloat16, torch.float16)


def _on_device(*tensors: Any) -> bool:
    return all(t.is_cuda for t in tensors) and _native.is_available() and _native.library().is_device


def _fp32_param(p: Any) -> bool:
    return p is None or isinstance(p, (int, float)) or (isinstance(p, torch.Tensor) and p.dtype == torch.float32)


def _needs_grad(*objs: Any) -> bool:
    if not torch.is_grad_enabled():
        return False
    for t in objs:
        if isinstance(t, _LINEAR.surface.quantized_tensor):
            p = t.quantization_context.quantization_params
            if t.requires_grad or t.raw_data.requires_grad or any(isinstance(v, torch.Tensor) and v.requires_grad for v in (p.scale, p.offset)):
                return True
        elif isinstance(t, torch.Tensor) and t.requires_grad:
            return True
    return False


def _settle(t: Any) -> None:
    # codes a sibling quantizer left to the device to write (quantization/affine/_memo.py): written before they are read here
    if getattr(t, "_ffq_earlier", None) is not None:
        from fastforward_amd.quantization.affine._memo import RECENT

        RECENT.settle(t)


class ModuleKernels:
    """Predicates and kernels of ``layer_norm`` / ``embedding`` / ``relu`` / ``silu`` (on the int8 GEMM's Surface)."""

    def __init__(self, linear: Any) -> None:
        self._k = linear

    # ---- what an operand is ------------------------------------------------------------------------------------------
    def _codes_ok(self, t: Any) -> bool:
        """Static-affine codes the kernels dequantize in registers: int8 / value-dtype container, <= 8 bits, fp32 parameters."""
        k = self._k
        if not k.static_affine(t) or not k._bits_ok(t):
            return False
        p = k._params(t)
        deq = k._deq_dtype(t)
        return deq in _VALUES and t.raw_data.dtype in (torch.int8, deq) and _fp32_param(p.scale) and _fp32_param(p.offset)

    def _value_dtype(self, x: Any) -> torch.dtype | None:
        """The data dtype of a plain or quantized operand the kernels take, else None."""
        if isinstance(x, self._k.surface.quantized_tensor):
            return self._k._deq_dtype(x) if self._codes_ok(x) else None
        if type(x) is torch.Tensor and x.dtype in _VALUES:
            return x.dtype
        return None

    def _dequant(self, x: Any) -> tuple[torch.Tensor, tuple[torch.Tensor, torch.Tensor | None] | None]:
        if not isinstance(x, self._k.surface.quantized_tensor):
            return x, None
        _settle(x)
        p = self._k._params(x)
        scale = torch.as_tensor(p.scale, dtype=torch.float32, device=x.device)
        offset = None if p.offset is None else torch.as_tensor(p.offset, dtype=torch.float32, device=x.device)
        return x.raw_data, (scale, offset)

    def _output(self, output_quantizer: Any, deq: torch.dtype) -> dict[str, Any] | None:
        fused = self._k._requant(output_quantizer, deq)
        return fused if fused is not None and fused["out_dtype"] == torch.int8 else None

    def _finish(self, value: torch.Tensor | None, codes: list[torch.Tensor], fused: dict[str, Any] | None, output_quantizer: Any, deq: torch.dtype) -> Any:
        if fused is not None:
            return self._k._wrap(None, codes[0], output_quantizer, deq)
        return output_quantizer(value) if output_quantizer is not None else value

    def _launch_args(self, fused: dict[str, Any] | None) -> dict[str, Any]:
        if fused is None:
            return dict(quantizers=(), want_value=True)
        return dict(quantizers=[(fused["out_scale"], fused["out_offset"])], num_bits=fused["out_num_bits"], want_value=False)

    def _strict_ok(self, strict: bool | None, output_quantizer: Any, *required: Any) -> bool:
        """Under strict quantization the fallback raises the reference's errors: leave those calls to it."""
        if not strict:
            return True
        return output_quantizer is not None and all(isinstance(t, self._k.surface.quantized_tensor) for t in required)

    # ---- layer_norm ---------------------------------------------------------------------------------------------------
    def supported_layer_norm(self, input: Any = None, normalized_shape: Any = None, weight: Any = None, bias: Any = None, eps: float = 1e-5,
                             output_quantizer: Any = None, strict_quantization: bool | None = None, **_: Any) -> bool:
        if not self._strict_ok(strict_quantization, output_quantizer, input, *([] if weight is None else [weight])):
            return False
        dt = self._value_dtype(input)
        if dt is None or not _on_device(input) or input.numel() == 0:
            return False
        shape = tuple(normalized_shape) if isinstance(normalized_shape, (tuple, list, torch.Size)) else (int(normalized_shape),)
        if not shape or tuple(input.shape[input.dim() - len(shape):]) != shape or input.dim() < len(shape):
            return False
        cols = math.prod(shape)
        if cols % 8 or cols > 16384:
            return False
        if isinstance(input, self._k.surface.quantized_tensor):
            mode = self._k.row_mode(input)
            if mode is None or (mode == "row" and len(shape) != 1):
                return False
        for t in (weight, bias):
            if t is None:
                continue
            if isinstance(t, self._k.surface.quantized_tensor):
                if not self.static_or_dequantizable(t, dt):
                    return False
            elif not isinstance(t, torch.Tensor) or t.dtype != dt:  # (module parameters: nn.Parameter)
                return False
            if t.numel() != cols or not _on_device(t):
                return False
        return not _needs_grad(input, weight, bias)

    def static_or_dequantizable(self, t: Any, dt: torch.dtype) -> bool:
        """A quantized LayerNorm weight / bias: dequantized on its own (A2 of [cols]) into the value dtype."""
        return self._k.static_affine(t) and self._k._deq_dtype(t) == dt

    def layer_norm(self, input: Any, normalized_shape: Any, weight: Any = None, bias: Any = None, eps: float = 1e-5, *, output_quantizer: Any = None,
                   strict_quantization: bool | None = None) -> Any:
        dt = self._value_dtype(input)
        shape = tuple(normalized_shape) if isinstance(normalized_shape, (tuple, list, torch.Size)) else (int(normalized_shape),)
        qt = self._k.surface.quantized_tensor
        weight = weight.dequantize() if isinstance(weight, qt) else weight
        bias = bias.dequantize() if isinstance(bias, qt) else bias
        x, dequant = self._dequant(input)
        fused = self._output(output_quantizer, dt)
        value, codes = ops.layer_norm_quantize(x, math.prod(shape), weight, bias, eps, dtype=dt, dequant=dequant, **self._launch_args(fused))
        return self._finish(value, codes, fused, output_quantizer, dt)

    # ---- embedding ----------------------------------------------------------------------------------------------------
    def _table_grid(self, weight: Any) -> tuple[bool, int] | None:
        """(per_row, group) of the table's parameter grid, or None for a tiling the kernel does not take."""
        V, D = weight.shape
        tile = self._k._tile(weight)
        if tile == (V, D):
            return False, D
        if tile == (V, 1):
            return False, 1
        if tile[0] == 1 and D % tile[1] == 0 and (tile[1] == D or tile[1] % 8 == 0):
            return True, int(tile[1])
        return None

    def supported_embedding(self, input: Any = None, weight: Any = None, padding_idx: Any = None, max_norm: Any = None, norm_type: float = 2.0,
                            scale_grad_by_freq: bool = False, sparse: bool = False, output_quantizer: Any = None, strict_quantization: bool | None = None,
                            **_: Any) -> bool:
        if not self._strict_ok(strict_quantization, output_quantizer, weight) or max_norm is not None:
            return False
        if not isinstance(weight, self._k.surface.quantized_tensor) or not self._codes_ok(weight) or weight.dim() != 2:
            return False
        if type(input) is not torch.Tensor or input.dtype not in (torch.int64, torch.int32) or input.numel() == 0:
            return False
        if not _on_device(input, weight) or weight.shape[0] == 0 or weight.shape[1] % 8 or self._table_grid(weight) is None:
            return False
        return not _needs_grad(weight)

    def embedding(self, input: torch.Tensor, weight: Any, padding_idx: Any = None, max_norm: Any = None, norm_type: float = 2.0,
                  scale_grad_by_freq: bool = False, sparse: bool = False, *, output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        # padding_idx / norm_type / scale_grad_by_freq / sparse change gradients only (max_norm, which rewrites the table, declines)
        dt = self._k._deq_dtype(weight)
        per_row, group = self._table_grid(weight)
        table, (scale, offset) = self._dequant(weight)
        fused = self._output(output_quantizer, dt)
        args = self._launch_args(fused)
        value, codes, _bad = ops.embedding_quantize(input, table, scale, offset, per_row, group, dt, args["quantizers"], args.get("num_bits", 8.0), args["want_value"])
        return self._finish(value, codes, fused, output_quantizer, dt)

    # ---- relu / silu --------------------------------------------------------------------------------------------------
    def supported_pointwise(self, input: Any = None, output_quantizer: Any = None, strict_quantization: bool | None = None, **_: Any) -> bool:
        if not self._strict_ok(strict_quantization, output_quantizer, input):
            return False
        if self._value_dtype(input) is None or not _on_device(input) or input.numel() == 0 or input.numel() % 8:
            return False
        if isinstance(input, self._k.surface.quantized_tensor):
            mode = self._k.row_mode(input)
            if mode is None or (mode == "row" and input.shape[-1] % 8):
                return False
        return not _needs_grad(input)

    def _pointwise(self, op: str, input: Any, output_quantizer: Any) -> Any:
        dt = self._value_dtype(input)
        x, dequant = self._dequant(input)
        fused = self._output(output_quantizer, dt)
        value, codes = ops.pointwise_quantize(op, x, dtype=dt, dequant=dequant, **self._launch_args(fused))
        return self._finish(value, codes, fused, output_quantizer, dt)

    def relu(self, input: Any, *, output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        return self._pointwise("relu", input, output_quantizer)

    def silu(self, input: Any, *, output_quantizer: Any = None, strict_quantization: bool | None = None) -> Any:
        return self._pointwise("silu", input, output_quantizer)


KERNELS = ModuleKernels(_LINEAR)
layer_norm_predicate = Predicate(KERNELS.supported_layer_norm)
embedding_predicate = Predicate(KERNELS.supported_embedding)
pointwise_predicate = Predicate(KERNELS.supported_pointwise)
_registrations = {
    "layer_norm": register("layer_norm", layer_norm_predicate, KERNELS.layer_norm),
    "embedding": register("embedding", embedding_predicate, KERNELS.embedding),
    "relu": register("relu", pointwise_predicate, KERNELS.relu),
    "silu": register("silu", pointwise_predicate, KERNELS.silu),
}
