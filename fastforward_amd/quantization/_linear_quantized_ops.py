"""View-like operators on affine-quantized tensors that act on the raw codes.

Subset of src/fastforward/quantization/_linear_quantized_ops.py needed on the Llama linear path
(SURVEY §2): ``contiguous`` (:94-96) for any quantized tensor and ``view`` / ``view_as`` /
``reshape`` / ``transpose`` for per-tensor affine tensors (:99-123). They only move metadata.
So does ``mul`` by a Python number (:126-171): the same codes with ``scale * other``. ``cat`` of per-tensor affine tensors that
share one scale and one offset, without an output quantizer, concatenates the codes (:174-224). ``expand``, ``unsqueeze``,
``take_along_dim`` and ``topk`` of per-tensor affine tensors act on the codes too (:232-280): the order of the codes is the order of
the values (a positive scale), so the top-k codes are the top-k values and their indices. Per-channel and per-tile tensors keep the
dequantizing route for them, and ``__getitem__`` stays unimplemented.
"""

from __future__ import annotations

from typing import Any, Sequence

import torch

from fastforward_amd.dispatcher import Predicate, register
from fastforward_amd.quantization import granularity as granularities
from fastforward_amd.quantized_tensor import QuantizedTensor, apply_and_reattach


def _static_affine(tensor: Any) -> bool:
    from fastforward_amd.quantization.affine import AffineQuantizationFunction, StaticAffineQuantParams

    if not isinstance(tensor, QuantizedTensor):
        return False
    context = tensor.quantization_context
    return issubclass(context.quantization_fn, AffineQuantizationFunction) and isinstance(
        context.quantization_params, StaticAffineQuantParams
    )


def _granularity_of(tensor: QuantizedTensor) -> Any:
    return getattr(tensor.quantization_context.quantization_params, "granularity", None)


affine_predicate = Predicate(lambda input, *a, **k: _static_affine(input))
affine_per_tensor_predicate = Predicate(
    lambda input, *a, **k: _static_affine(input) and isinstance(_granularity_of(input), granularities.PerTensor)
)
affine_per_channel_predicate = Predicate(
    lambda input, *a, **k: _static_affine(input) and isinstance(_granularity_of(input), granularities.PerChannel)
)


@register("contiguous")
def contiguous(input: QuantizedTensor) -> QuantizedTensor:
    return apply_and_reattach(lambda x: x.contiguous(), input)


def _no_dtype_view(name: str, args: tuple[Any, ...]) -> None:
    if args and isinstance(args[0], torch.dtype):
        raise TypeError(f"QuantizedTensor.{name}(dtype) is not supported")


@register("view", affine_per_tensor_predicate)
def view(input: QuantizedTensor, *args: Any) -> QuantizedTensor:
    _no_dtype_view("view", args)
    return apply_and_reattach(lambda x: x.view(*args), input)


@register("view_as", affine_per_tensor_predicate)
def view_as(input: QuantizedTensor, *args: Any) -> QuantizedTensor:
    _no_dtype_view("view_as", args)
    return apply_and_reattach(lambda x: x.view_as(*args), input)


@register("reshape", affine_per_tensor_predicate)
def reshape(input: QuantizedTensor, *args: Any) -> QuantizedTensor:
    return apply_and_reattach(lambda x: x.reshape(*args), input)


@register("transpose", affine_per_tensor_predicate)
def transpose(input: QuantizedTensor, *args: Any) -> QuantizedTensor:
    return apply_and_reattach(lambda x: x.transpose(*args), input)


# ---- mul by a Python number: a rescale of the parameters (reference :126-171) ------------------------------------------------------
class _ScaleGradient(torch.autograd.Function):
    """The identity on the raw codes, with the gradient scaled by `scalar` on the way back."""

    @staticmethod
    def forward(ctx: Any, input: torch.Tensor, scalar: float) -> torch.Tensor:
        ctx.scalar = scalar
        return input

    @staticmethod
    def backward(ctx: Any, grad: torch.Tensor) -> tuple[torch.Tensor, None]:
        return grad * ctx.scalar, None


def _is_scalar_multiply(input: Any = None, other: Any = None, *_args: Any, output_quantizer: Any = None, **kwargs: Any) -> bool:
    """A per-tensor affine `input` times a Python number, without an output quantizer (or with a stub), as the reference's
    predicate — but only for calls of ``ff.nn.functional.mul``, which pass ``strict_quantization``: ``qt * 2`` reaches the dispatcher
    through ``QuantizedTensor.__torch_function__`` and keeps its dequantizing route."""
    from fastforward_amd.nn.quantizer import QuantizerStub

    if "strict_quantization" not in kwargs:
        return False
    if not isinstance(other, (int, float)) or isinstance(other, bool):
        return False
    if not _static_affine(input) or not isinstance(_granularity_of(input), granularities.PerTensor):
        return False
    return output_quantizer is None or isinstance(output_quantizer, QuantizerStub)


scalar_multiply_predicate = Predicate(_is_scalar_multiply)


@register("mul", scalar_multiply_predicate)
def scalar_multiply(input: QuantizedTensor, other: float, *_args: Any, **_kwargs: Any) -> QuantizedTensor:
    """``input * other`` of an affine quantized tensor: only the scale moves."""
    params = input.quant_args()
    scaled = _ScaleGradient.apply(input.raw_data, other)
    return input.quantization_context.with_changes(scale=params.scale * other).attach(scaled)


# ---- cat of tensors that share their parameters: a concatenation of the codes (reference :174-224) ---------------------------------
def _values_equal(a: Any, b: Any) -> bool:
    """The reference's ``a == b`` on two parameters. On device tensors it reads the result on the host: it synchronises."""
    return bool(torch.as_tensor(a == b).all())


def _same_tensor(a: torch.Tensor, b: torch.Tensor) -> bool:
    """One view of one storage: equal without looking at the values."""
    return (a.device == b.device and a.dtype == b.dtype and a.shape == b.shape and a.stride() == b.stride()
            and a.storage_offset() == b.storage_offset() and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr())


def _same_parameter(a: Any, b: Any) -> bool:
    if a is b:
        return True
    if a is None or b is None:
        return False
    if isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and _same_tensor(a, b):
        return True
    return _values_equal(a, b)


def _is_code_level_cat(tensors: Any = None, dim: Any = 0, *_args: Any, output_quantizer: Any = None, **kwargs: Any) -> bool:
    """Every element a per-tensor static-affine ``QuantizedTensor``, all scales equal and all offsets equal, no output quantizer:
    the reference's predicate. Parameters that are one tensor object, or one view of one storage, are equal without a look at
    their values; only otherwise are the values compared as the reference compares them, which reads device memory on the host —
    such a call synchronises and cannot be captured in a graph."""
    if output_quantizer is not None or "out" in kwargs or not isinstance(tensors, (list, tuple)) or not tensors:
        return False
    first = None
    for tensor in tensors:
        if not _static_affine(tensor) or not isinstance(_granularity_of(tensor), granularities.PerTensor):
            return False
        params = tensor.quant_args()
        if first is not None and not (_same_parameter(params.scale, first.scale) and _same_parameter(params.offset, first.offset)):
            return False
        first = params if first is None else first
    return True


cat_predicate = Predicate(_is_code_level_cat)


@register("cat", cat_predicate)
def cat(tensors: Sequence[QuantizedTensor], dim: int = 0, *_args: Any, **_kwargs: Any) -> QuantizedTensor:
    """``torch.cat`` of the codes, under the first element's context. Serves ``ff.nn.functional.cat`` and ``torch.cat``."""
    output = torch.cat([t.raw_data for t in tensors], dim=dim)
    return tensors[0].quantization_context.attach(output)


# ---- expand / unsqueeze / take_along_dim / topk of per-tensor affine tensors: the torch op on the codes (reference :232-280) --------
@register("expand", affine_per_tensor_predicate)
def expand(input: QuantizedTensor, *args: Any) -> QuantizedTensor:
    return apply_and_reattach(lambda x: x.expand(*args), input)


@register("unsqueeze", affine_per_tensor_predicate)
def unsqueeze(input: QuantizedTensor, dim: int) -> QuantizedTensor:
    # (per tensor only: the reference's per-channel arm computes the new axes as ``ax + ax >= dim``, a bool per axis)
    return apply_and_reattach(lambda x: x.unsqueeze(dim), input)


@register("take_along_dim", affine_per_tensor_predicate)
def take_along_dim(input: QuantizedTensor, indices: torch.Tensor, dim: int | None = None) -> QuantizedTensor:
    return apply_and_reattach(lambda x: torch.take_along_dim(x, indices, dim=dim), input)


@register("topk", affine_per_tensor_predicate)
def topk(input: QuantizedTensor, k: int, dim: int = -1, largest: bool = True, sorted: bool = True) -> Any:
    values, indices = torch.topk(input.raw_data, k, dim=dim, largest=largest, sorted=sorted)
    return torch.return_types.topk((apply_and_reattach(lambda _: values, input), indices))
