"""Quantized functional operators: the linear path (``linear``, ``matmul``, ``mm``, ``bmm``), the convolutions (``conv1d``,
``conv2d``, ``conv3d``, ``conv_transpose1d``, ``conv_transpose2d``), the generic modules' operators (``layer_norm``, ``embedding``, ``relu``, ``silu``) and the elementwise operators of a
transformer block outside its linears (``add``, ``sub``, ``mul``, ``div``, ``softmax``, ``sigmoid``, ``gelu``).

Reference: the generated ``ff.nn.functional.*`` (src/fastforward/_gen/operators.py:79-106 for
``linear``; matmul/mm/bmm follow the same template) and their fallbacks
(src/fastforward/_gen/fallback.py:77-112, 699-798). Each operator is
``dispatch(name, **kwargs) or fallback`` — the dispatcher lookup is plug-in seam #2, where
``fastforward_amd.fused_linear`` registers the int8-MFMA kernel and ``fastforward_amd.fused_modules`` the one-pass LayerNorm /
Embedding / ReLU / SiLU kernels (fallbacks: _gen/fallback.py:296-317, 616-652, 655-696, 1348-1369), and ``fastforward_amd.fused_conv``
the int8 implicit-GEMM convolution (fallbacks: _gen/fallback.py:116-214), and ``fastforward_amd.fused_elementwise`` the one-pass
add / sub / mul / div, softmax, sigmoid and GELU kernels (fallbacks: _gen/fallback.py:269-293, 321-342, 801-955, 1373-1395).
``mul`` of a per-tensor affine tensor by a Python number without an output quantizer is the reference's rescale of the scale
(quantization/_linear_quantized_ops.py:126-171). ``dropout`` follows fallback.py:1399-1423 with no kernel of its own, and
``scaled_dot_product_attention`` is the reference's custom operator (nn/sdpa.py; ``fastforward_amd.fused_sdpa`` registers its
kernel, and ``fastforward_amd.fused_sdpa_decode`` the split-key ``sdpa_decode`` kernels for a query of at most 32 rows per kv head
over K / V kept as int8 codes, a quantized KV cache; ``nn.QuantizedKVCache`` keeps one in place as a dense slab per tensor,
``nn.PagedQuantizedKVCache`` as fixed-size pages of a shared pool behind a per-sequence block table). ``rms_norm``, ``pow``, ``exp``, ``sin``, ``cos``, ``sum`` and ``cumsum`` follow their fallbacks (_gen/fallback.py:955-1014,
1520-1541, 1831-1941), and ``fastforward_amd.fused_math`` registers their one-pass kernels. ``avg_pool1d``, ``avg_pool2d``,
``max_pool2d`` and ``interpolate`` follow theirs (_gen/fallback.py:505-575, 1574-1646) with the reference's signatures, and
``fastforward_amd.fused_pool`` registers the one-pass kernels of the pools and of nearest interpolation. ``cat`` and ``pad`` follow
theirs (_gen/fallback.py:1453-1479, 1546-1570) with the reference's signatures (``pad``'s default ``mode="..."`` included);
``fastforward_amd.fused_concat`` registers their one-pass kernels, and a ``cat`` of per-tensor affine tensors that share their
parameters, without an output quantizer, is the reference's concatenation of the codes
(quantization/_linear_quantized_ops.py:174-224). ``conv_transpose1d`` and ``conv_transpose2d`` follow theirs
(_gen/fallback.py:346-449) with the reference's signatures, and ``fastforward_amd.fused_conv_transpose`` registers the phase-split
int8 implicit GEMM. ``conv3d`` and ``avg_pool3d`` follow theirs (_gen/fallback.py:218-265, 579-612) with the reference's signatures;
``fastforward_amd.fused_conv3d`` registers the 3-D int8 implicit GEMM and ``fastforward_amd.fused_pool`` the one-pass 3-D average
pool (entry points of include/ffq_3d.h). ``conv1d`` / ``conv2d`` with ``groups == C`` (depthwise, any channel multiplier, at most 1024
taps) have a second kernel, the direct int8 stencil ``fastforward_amd.fused_depthwise`` registers (include/ffq_depthwise.h); every other
``groups != 1`` runs the fallback. ``index_add`` and ``permute`` follow theirs (_gen/fallback.py:1427-1449, 1483-1516) with the
reference's signatures, and ``fastforward_amd.fused_index`` registers their one-pass kernels (include/ffq_index.h): an
``index_add`` that sums the addends of a row in fp32 in index order, and a ``permute`` under an output quantizer that writes the
permuted codes directly. ``unfold`` follows its fallback (_gen/fallback.py:1650-1677) with the reference's signature, and
``fastforward_amd.fused_unfold`` registers the one-pass im2col (include/ffq_unfold.h), which writes the codes of the columns
directly. The other generated operators of the reference (``conv_transpose3d`` among them) are pure float fallbacks and are out of
scope.
"""

from __future__ import annotations

from typing import TYPE_CHECKING, Any, Callable, Optional, Sequence

import torch

from fastforward_amd import flags
from fastforward_amd.dispatcher import dispatch
from fastforward_amd.exceptions import QuantizationError
from fastforward_amd.quantized_tensor import QuantizedTensor

if TYPE_CHECKING:
    from fastforward_amd.nn.quantizer import Quantizer

__all__ = ["linear", "matmul", "mm", "bmm", "conv1d", "conv2d", "conv3d", "conv_transpose1d", "conv_transpose2d", "layer_norm", "embedding", "relu", "silu", "add", "sub", "mul", "div",
           "softmax", "sigmoid", "gelu", "dropout", "scaled_dot_product_attention", "rms_norm", "pow", "exp", "sin", "cos", "sum",
           "cumsum", "avg_pool1d", "avg_pool2d", "avg_pool3d", "max_pool2d", "interpolate", "cat", "pad", "index_add", "permute", "unfold"]


def _dequantized(name: str, value: Any, strict: bool, required: bool = True) -> Any:
    if strict and required and not isinstance(value, QuantizedTensor):
        raise QuantizationError(
            f"Expected '{name}' to be an instance of 'QuantizedTensor' because strict_quantization=True."
        )
    return value.dequantize() if isinstance(value, QuantizedTensor) else value


def _check_output_quantizer(output_quantizer: Any, strict: bool) -> None:
    if strict and output_quantizer is None:
        raise QuantizationError("'output_quantizer' must be provided if strict_quantization=True")


def _fallback_linear(input: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None = None, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool = True) -> torch.Tensor:
    """Dequantize operands, float linear, optional output quantizer (reference fallback.py:77-112)."""
    _check_output_quantizer(output_quantizer, strict_quantization)
    input = _dequantized("input", input, strict_quantization)
    weight = _dequantized("weight", weight, strict_quantization)
    bias = _dequantized("bias", bias, strict_quantization, required=False)
    output = torch.nn.functional.linear(input=input, weight=weight, bias=bias)
    return output_quantizer(output) if output_quantizer is not None else output


def _binary_fallback(torch_op: Callable[..., torch.Tensor], second: str) -> Callable[..., torch.Tensor]:
    def fallback(input: torch.Tensor, other: torch.Tensor, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool = True) -> torch.Tensor:
        _check_output_quantizer(output_quantizer, strict_quantization)
        input = _dequantized("input", input, strict_quantization)
        other = _dequantized(second, other, strict_quantization)
        output = torch_op(input, other)
        return output_quantizer(output) if output_quantizer is not None else output

    return fallback


_fallback_matmul = _binary_fallback(torch.matmul, "other")
_fallback_mm = _binary_fallback(torch.mm, "mat2")
_fallback_bmm = _binary_fallback(torch.bmm, "mat2")


def _strict(value: bool | None) -> bool:
    return flags.get_strict_quantization() if value is None else value


def linear(input: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None = None, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, weight=weight, bias=bias, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    kernel = dispatch("linear", **kwargs) or _fallback_linear
    # codes of a sibling quantizer whose A1 launch the device may have skipped (quantization/affine/_memo.py): a kernel that has
    # not declared that it reads the codes in force gets them written first
    if getattr(input, "_ffq_earlier", None) is not None and not getattr(kernel, "reads_undecided_codes", False):
        from fastforward_amd.quantization.affine._memo import RECENT

        RECENT.settle(input)
    return kernel(**kwargs)


def matmul(input: torch.Tensor, other: torch.Tensor, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, other=other, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    kernel = dispatch("matmul", **kwargs)
    if kernel:
        return kernel(**kwargs)
    return _fallback_matmul(input, other, output_quantizer=output_quantizer, strict_quantization=kwargs["strict_quantization"])


def mm(input: torch.Tensor, mat2: torch.Tensor, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, mat2=mat2, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    kernel = dispatch("mm", **kwargs)
    if kernel:
        return kernel(**kwargs)
    return _fallback_mm(input, mat2, output_quantizer=output_quantizer, strict_quantization=kwargs["strict_quantization"])


def bmm(input: torch.Tensor, mat2: torch.Tensor, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, mat2=mat2, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    kernel = dispatch("bmm", **kwargs)
    if kernel:
        return kernel(**kwargs)
    return _fallback_bmm(input, mat2, output_quantizer=output_quantizer, strict_quantization=kwargs["strict_quantization"])


# ---- the generic modules' operators (reference _gen/operators.py: dispatch(op, **kwargs) or the generated fallback) -------------
def _fallback_layer_norm(input: torch.Tensor, normalized_shape: tuple[int, ...], weight: torch.Tensor | None = None, bias: torch.Tensor | None = None, eps: float = 1e-5, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool = True) -> torch.Tensor:
    """Dequantize, F.layer_norm, optional output quantizer (reference fallback.py:655-696)."""
    _check_output_quantizer(output_quantizer, strict_quantization)
    input = _dequantized("input", input, strict_quantization)
    if weight is not None:
        weight = _dequantized("weight", weight, strict_quantization)
    if bias is not None:
        bias = _dequantized("bias", bias, strict_quantization, required=False)
    output = torch.nn.functional.layer_norm(input=input, normalized_shape=normalized_shape, weight=weight, bias=bias, eps=eps)
    return output_quantizer(output) if output_quantizer is not None else output


def _fallback_embedding(input: torch.Tensor, weight: torch.Tensor, padding_idx: int | None = None, max_norm: float | None = None, norm_type: float = 2.0, scale_grad_by_freq: bool = False, sparse: bool = False, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool = True) -> torch.Tensor:
    """Dequantize the table, F.embedding, optional output quantizer (reference fallback.py:616-652)."""
    _check_output_quantizer(output_quantizer, strict_quantization)
    weight = _dequantized("weight", weight, strict_quantization)
    output = torch.nn.functional.embedding(input=input, weight=weight, padding_idx=padding_idx, max_norm=max_norm, norm_type=norm_type, scale_grad_by_freq=scale_grad_by_freq, sparse=sparse)
    return output_quantizer(output) if output_quantizer is not None else output


def _unary_fallback(torch_op: Callable[..., torch.Tensor]) -> Callable[..., torch.Tensor]:
    def fallback(input: torch.Tensor, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool = True) -> torch.Tensor:
        _check_output_quantizer(output_quantizer, strict_quantization)
        input = _dequantized("input", input, strict_quantization)
        output = torch_op(input=input)
        return output_quantizer(output) if output_quantizer is not None else output

    return fallback


_fallback_relu = _unary_fallback(torch.nn.functional.relu)  # fallback.py:296-317
_fallback_silu = _unary_fallback(torch.nn.functional.silu)  # fallback.py:1348-1369


def layer_norm(input: torch.Tensor, normalized_shape: tuple[int, ...], weight: torch.Tensor | None = None, bias: torch.Tensor | None = None, eps: float = 1e-5, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, normalized_shape=normalized_shape, weight=weight, bias=bias, eps=eps, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("layer_norm", **kwargs) or _fallback_layer_norm)(**kwargs)


def embedding(input: torch.Tensor, weight: torch.Tensor, padding_idx: int | None = None, max_norm: float | None = None, norm_type: float = 2.0, scale_grad_by_freq: bool = False, sparse: bool = False, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, weight=weight, padding_idx=padding_idx, max_norm=max_norm, norm_type=norm_type, scale_grad_by_freq=scale_grad_by_freq, sparse=sparse, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("embedding", **kwargs) or _fallback_embedding)(**kwargs)


def relu(input: torch.Tensor, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("relu", **kwargs) or _fallback_relu)(**kwargs)


def silu(input: torch.Tensor, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("silu", **kwargs) or _fallback_silu)(**kwargs)


# ---- the convolutions (reference _gen/operators.py:110-193: dispatch(op, **kwargs) or the generated fallback) ------------------
def _conv_fallback(torch_op: Callable[..., torch.Tensor]) -> Callable[..., torch.Tensor]:
    def fallback(input: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None = None, stride: Any = 1, padding: Any = 0, dilation: Any = 1, groups: int = 1, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool = True) -> torch.Tensor:
        """Dequantize input / weight / bias, the float convolution, optional output quantizer (reference fallback.py:116-214)."""
        _check_output_quantizer(output_quantizer, strict_quantization)
        input = _dequantized("input", input, strict_quantization)
        weight = _dequantized("weight", weight, strict_quantization)
        if bias is not None:
            bias = _dequantized("bias", bias, strict_quantization, required=False)
        output = torch_op(input=input, weight=weight, bias=bias, stride=stride, padding=padding, dilation=dilation, groups=groups)
        return output_quantizer(output) if output_quantizer is not None else output

    return fallback


_fallback_conv1d = _conv_fallback(torch.nn.functional.conv1d)  # fallback.py:116-164
_fallback_conv2d = _conv_fallback(torch.nn.functional.conv2d)  # fallback.py:167-214
_fallback_conv3d = _conv_fallback(torch.nn.functional.conv3d)  # fallback.py:218-265


def conv1d(input: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None = None, stride: Any = 1, padding: Any = 0, dilation: Any = 1, groups: int = 1, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, weight=weight, bias=bias, stride=stride, padding=padding, dilation=dilation, groups=groups, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("conv1d", **kwargs) or _fallback_conv1d)(**kwargs)


def conv2d(input: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None = None, stride: Any = 1, padding: Any = 0, dilation: Any = 1, groups: int = 1, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, weight=weight, bias=bias, stride=stride, padding=padding, dilation=dilation, groups=groups, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("conv2d", **kwargs) or _fallback_conv2d)(**kwargs)


def conv3d(input: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None = None, stride: Any = 1, padding: Any = 0, dilation: Any = 1, groups: int = 1, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, weight=weight, bias=bias, stride=stride, padding=padding, dilation=dilation, groups=groups, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("conv3d", **kwargs) or _fallback_conv3d)(**kwargs)


# ---- the transposed convolutions (reference _gen/operators.py:362-392: dispatch(op, **kwargs) or the generated fallback) --------
def _conv_transpose_fallback(torch_op: Callable[..., torch.Tensor]) -> Callable[..., torch.Tensor]:
    def fallback(input: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None = None, stride: Any = 1, padding: Any = 0, output_padding: Any = 0, groups: int = 1, dilation: Any = 1, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool = True) -> torch.Tensor:
        """Dequantize input / weight / bias, the float transposed convolution, optional output quantizer (reference fallback.py:346-449)."""
        _check_output_quantizer(output_quantizer, strict_quantization)
        input = _dequantized("input", input, strict_quantization)
        weight = _dequantized("weight", weight, strict_quantization)
        if bias is not None:
            bias = _dequantized("bias", bias, strict_quantization, required=False)
        output = torch_op(input=input, weight=weight, bias=bias, stride=stride, padding=padding, output_padding=output_padding, groups=groups, dilation=dilation)
        return output_quantizer(output) if output_quantizer is not None else output

    return fallback


_fallback_conv_transpose1d = _conv_transpose_fallback(torch.nn.functional.conv_transpose1d)  # fallback.py:346-395
_fallback_conv_transpose2d = _conv_transpose_fallback(torch.nn.functional.conv_transpose2d)  # fallback.py:399-448


def conv_transpose1d(input: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None = None, stride: Any = 1, padding: Any = 0, output_padding: Any = 0, groups: int = 1, dilation: Any = 1, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, weight=weight, bias=bias, stride=stride, padding=padding, output_padding=output_padding, groups=groups, dilation=dilation, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("conv_transpose1d", **kwargs) or _fallback_conv_transpose1d)(**kwargs)


def conv_transpose2d(input: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None = None, stride: Any = 1, padding: Any = 0, output_padding: Any = 0, groups: int = 1, dilation: Any = 1, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, weight=weight, bias=bias, stride=stride, padding=padding, output_padding=output_padding, groups=groups, dilation=dilation, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("conv_transpose2d", **kwargs) or _fallback_conv_transpose2d)(**kwargs)


# ---- the elementwise operators (reference _gen/operators.py: dispatch(op, **kwargs) or the generated fallback) ---------------------
def _arith_fallback(torch_op: Callable[..., torch.Tensor], with_alpha: bool) -> Callable[..., torch.Tensor]:
    def fallback(input: torch.Tensor, other: torch.Tensor | float, alpha: float = 1, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool = True) -> torch.Tensor:
        """Dequantize input / other, the torch op, optional output quantizer; a number `other` is no strict-mode error."""
        _check_output_quantizer(output_quantizer, strict_quantization)
        input = _dequantized("input", input, strict_quantization)
        other = _dequantized("other", other, strict_quantization, required=isinstance(other, torch.Tensor))
        output = torch_op(input=input, other=other, alpha=alpha) if with_alpha else torch_op(input=input, other=other)
        return output_quantizer(output) if output_quantizer is not None else output

    return fallback


_fallback_add = _arith_fallback(torch.add, True)  # fallback.py:801-837
_fallback_sub = _arith_fallback(torch.sub, True)  # fallback.py:840-876
_fallback_mul = _arith_fallback(torch.mul, False)  # fallback.py:879-914
_fallback_div = _arith_fallback(torch.div, False)  # fallback.py:917-952
_fallback_sigmoid = _unary_fallback(torch.nn.functional.sigmoid)  # fallback.py:321-342


def _fallback_softmax(input: torch.Tensor, dim: int, dtype: torch.dtype | None = None, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool = True) -> torch.Tensor:
    """Dequantize, F.softmax, optional output quantizer (reference fallback.py:269-293)."""
    _check_output_quantizer(output_quantizer, strict_quantization)
    input = _dequantized("input", input, strict_quantization)
    output = torch.nn.functional.softmax(input=input, dim=dim, dtype=dtype)
    return output_quantizer(output) if output_quantizer is not None else output


def _fallback_gelu(input: torch.Tensor, approximate: str = "none", *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool = True) -> torch.Tensor:
    """Dequantize, F.gelu, optional output quantizer (reference fallback.py:1373-1395)."""
    _check_output_quantizer(output_quantizer, strict_quantization)
    input = _dequantized("input", input, strict_quantization)
    output = torch.nn.functional.gelu(input=input, approximate=approximate)
    return output_quantizer(output) if output_quantizer is not None else output


def add(input: torch.Tensor, other: torch.Tensor | float, alpha: float = 1, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, other=other, alpha=alpha, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("add", **kwargs) or _fallback_add)(**kwargs)


def sub(input: torch.Tensor, other: torch.Tensor | float, alpha: float = 1, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, other=other, alpha=alpha, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("sub", **kwargs) or _fallback_sub)(**kwargs)


def mul(input: torch.Tensor, other: torch.Tensor | float, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, other=other, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("mul", **kwargs) or _fallback_mul)(**kwargs)


def div(input: torch.Tensor, other: torch.Tensor | float, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, other=other, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("div", **kwargs) or _fallback_div)(**kwargs)


def softmax(input: torch.Tensor, dim: int, dtype: torch.dtype | None = None, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, dim=dim, dtype=dtype, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("softmax", **kwargs) or _fallback_softmax)(**kwargs)


def sigmoid(input: torch.Tensor, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("sigmoid", **kwargs) or _fallback_sigmoid)(**kwargs)


def gelu(input: torch.Tensor, approximate: str = "none", *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, approximate=approximate, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("gelu", **kwargs) or _fallback_gelu)(**kwargs)


def _fallback_dropout(input: torch.Tensor, p: float = 0.5, training: bool = True, inplace: bool = False, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool = True) -> torch.Tensor:
    """Dequantize, F.dropout, optional output quantizer (reference fallback.py:1399-1423)."""
    _check_output_quantizer(output_quantizer, strict_quantization)
    input = _dequantized("input", input, strict_quantization)
    output = torch.nn.functional.dropout(input=input, p=p, training=training, inplace=inplace)
    return output_quantizer(output) if output_quantizer is not None else output


def dropout(input: torch.Tensor, p: float = 0.5, training: bool = True, inplace: bool = False, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, p=p, training=training, inplace=inplace, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("dropout", **kwargs) or _fallback_dropout)(**kwargs)


# ---- rms_norm, pow, exp / sin / cos, sum, cumsum (reference _gen/operators.py: dispatch(op, **kwargs) or the generated fallback) --
def _fallback_rms_norm(input: torch.Tensor, normalized_shape: tuple[int, ...], weight: torch.Tensor | None = None, eps: float | None = None, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool = True) -> torch.Tensor:
    """Dequantize input / weight, F.rms_norm, optional output quantizer (reference fallback.py:1906-1941)."""
    _check_output_quantizer(output_quantizer, strict_quantization)
    input = _dequantized("input", input, strict_quantization)
    if weight is not None:
        weight = _dequantized("weight", weight, strict_quantization)
    output = torch.nn.functional.rms_norm(input=input, normalized_shape=normalized_shape, weight=weight, eps=eps)
    return output_quantizer(output) if output_quantizer is not None else output


def _fallback_pow(input: torch.Tensor, exponent: torch.Tensor | float, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool = True) -> torch.Tensor:
    """Dequantize input / a tensor exponent, torch.pow, optional output quantizer (reference fallback.py:955-990); a number
    exponent is no strict-mode error."""
    _check_output_quantizer(output_quantizer, strict_quantization)
    input = _dequantized("input", input, strict_quantization)
    exponent = _dequantized("exponent", exponent, strict_quantization, required=isinstance(exponent, torch.Tensor))
    output = torch.pow(input=input, exponent=exponent)
    return output_quantizer(output) if output_quantizer is not None else output


def _reduction_fallback(torch_op: Callable[..., torch.Tensor]) -> Callable[..., torch.Tensor]:
    def fallback(input: torch.Tensor, dim: int | None = None, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool = True) -> torch.Tensor:
        """Dequantize, the torch reduction / scan over `dim`, optional output quantizer."""
        _check_output_quantizer(output_quantizer, strict_quantization)
        input = _dequantized("input", input, strict_quantization)
        output = torch_op(input=input, dim=dim)
        return output_quantizer(output) if output_quantizer is not None else output

    return fallback


_fallback_exp = _unary_fallback(torch.exp)  # fallback.py:1831-1853
_fallback_sin = _unary_fallback(torch.sin)  # fallback.py:1856-1878
_fallback_cos = _unary_fallback(torch.cos)  # fallback.py:1881-1903
_fallback_sum = _reduction_fallback(torch.sum)  # fallback.py:993-1014
_fallback_cumsum = _reduction_fallback(torch.cumsum)  # fallback.py:1520-1541


def rms_norm(input: torch.Tensor, normalized_shape: tuple[int, ...], weight: torch.Tensor | None = None, eps: float | None = None, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, normalized_shape=normalized_shape, weight=weight, eps=eps, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("rms_norm", **kwargs) or _fallback_rms_norm)(**kwargs)


def pow(input: torch.Tensor, exponent: torch.Tensor | float, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, exponent=exponent, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("pow", **kwargs) or _fallback_pow)(**kwargs)


def exp(input: torch.Tensor, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("exp", **kwargs) or _fallback_exp)(**kwargs)


def sin(input: torch.Tensor, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("sin", **kwargs) or _fallback_sin)(**kwargs)


def cos(input: torch.Tensor, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("cos", **kwargs) or _fallback_cos)(**kwargs)


def sum(input: torch.Tensor, dim: int | None = None, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, dim=dim, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("sum", **kwargs) or _fallback_sum)(**kwargs)


def cumsum(input: torch.Tensor, dim: int, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, dim=dim, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("cumsum", **kwargs) or _fallback_cumsum)(**kwargs)


# ---- avg_pool1d / avg_pool2d, max_pool2d, interpolate (reference _gen/operators.py: dispatch(op, **kwargs) or the generated fallback) --
def _avg_pool_fallback(torch_op: Callable[..., torch.Tensor]) -> Callable[..., torch.Tensor]:
    def fallback(input: torch.Tensor, kernel_size: Any, stride: Any, padding: Any = 0, ceil_mode: bool = False, count_include_pad: bool = True, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool = True) -> torch.Tensor:
        """Dequantize, the torch average pool, optional output quantizer."""
        _check_output_quantizer(output_quantizer, strict_quantization)
        input = _dequantized("input", input, strict_quantization)
        output = torch_op(input=input, kernel_size=kernel_size, stride=stride, padding=padding, ceil_mode=ceil_mode, count_include_pad=count_include_pad)
        return output_quantizer(output) if output_quantizer is not None else output

    return fallback


_fallback_avg_pool1d = _avg_pool_fallback(torch.nn.functional.avg_pool1d)  # fallback.py:505-538
_fallback_avg_pool2d = _avg_pool_fallback(torch.nn.functional.avg_pool2d)  # fallback.py:542-575
_fallback_avg_pool3d = _avg_pool_fallback(torch.nn.functional.avg_pool3d)  # fallback.py:579-612


def _fallback_max_pool2d(input: torch.Tensor, kernel_size: Any, stride: Any = None, padding: Any = 0, dilation: Any = 1, ceil_mode: bool = False, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool = True) -> torch.Tensor:
    """Dequantize, F.max_pool2d, optional output quantizer (reference fallback.py:1574-1607)."""
    _check_output_quantizer(output_quantizer, strict_quantization)
    input = _dequantized("input", input, strict_quantization)
    output = torch.nn.functional.max_pool2d(input=input, kernel_size=kernel_size, stride=stride, padding=padding, dilation=dilation, ceil_mode=ceil_mode)
    return output_quantizer(output) if output_quantizer is not None else output


def _fallback_interpolate(input: torch.Tensor, size: Any = None, scale_factor: Any = None, mode: str = "nearest", align_corners: bool | None = None, recompute_scale_factor: bool | None = None, antialias: bool = False, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool = True) -> torch.Tensor:
    """Dequantize, F.interpolate, optional output quantizer (reference fallback.py:1611-1646)."""
    _check_output_quantizer(output_quantizer, strict_quantization)
    input = _dequantized("input", input, strict_quantization)
    output = torch.nn.functional.interpolate(input=input, size=size, scale_factor=scale_factor, mode=mode, align_corners=align_corners, recompute_scale_factor=recompute_scale_factor, antialias=antialias)
    return output_quantizer(output) if output_quantizer is not None else output


def avg_pool1d(input: torch.Tensor, kernel_size: Any, stride: Any, padding: Any = 0, ceil_mode: bool = False, count_include_pad: bool = True, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, kernel_size=kernel_size, stride=stride, padding=padding, ceil_mode=ceil_mode, count_include_pad=count_include_pad, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("avg_pool1d", **kwargs) or _fallback_avg_pool1d)(**kwargs)


def avg_pool2d(input: torch.Tensor, kernel_size: Any, stride: Any, padding: Any = 0, ceil_mode: bool = False, count_include_pad: bool = True, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, kernel_size=kernel_size, stride=stride, padding=padding, ceil_mode=ceil_mode, count_include_pad=count_include_pad, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("avg_pool2d", **kwargs) or _fallback_avg_pool2d)(**kwargs)


def avg_pool3d(input: torch.Tensor, kernel_size: Any, stride: Any, padding: Any = 0, ceil_mode: bool = False, count_include_pad: bool = True, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, kernel_size=kernel_size, stride=stride, padding=padding, ceil_mode=ceil_mode, count_include_pad=count_include_pad, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("avg_pool3d", **kwargs) or _fallback_avg_pool3d)(**kwargs)


def max_pool2d(input: torch.Tensor, kernel_size: Any, stride: Any = None, padding: Any = 0, dilation: Any = 1, ceil_mode: bool = False, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, kernel_size=kernel_size, stride=stride, padding=padding, dilation=dilation, ceil_mode=ceil_mode, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("max_pool2d", **kwargs) or _fallback_max_pool2d)(**kwargs)


def interpolate(input: torch.Tensor, size: Any = None, scale_factor: Any = None, mode: str = "nearest", align_corners: bool | None = None, recompute_scale_factor: bool | None = None, antialias: bool = False, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, size=size, scale_factor=scale_factor, mode=mode, align_corners=align_corners, recompute_scale_factor=recompute_scale_factor, antialias=antialias, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("interpolate", **kwargs) or _fallback_interpolate)(**kwargs)


# ---- cat, pad (reference _gen/operators.py:1290, 1383: dispatch(op, **kwargs) or the generated fallback) ---------------------------
def _fallback_cat(tensors: Sequence[torch.Tensor], dim: int = 0, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool = True) -> torch.Tensor:
    """Dequantize every element, torch.cat, optional output quantizer (reference fallback.py:1453-1479)."""
    _check_output_quantizer(output_quantizer, strict_quantization)
    tensors = [_dequantized("elem__", elem__, strict_quantization) for elem__ in tensors]
    output = torch.cat(tensors=tensors, dim=dim)
    return output_quantizer(output) if output_quantizer is not None else output


def _fallback_pad(input: torch.Tensor, pad: Sequence[int], mode: str = "...", value: float | None = None, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool = True) -> torch.Tensor:
    """Dequantize, F.pad, optional output quantizer (reference fallback.py:1546-1570)."""
    _check_output_quantizer(output_quantizer, strict_quantization)
    input = _dequantized("input", input, strict_quantization)
    output = torch.nn.functional.pad(input=input, pad=pad, mode=mode, value=value)
    return output_quantizer(output) if output_quantizer is not None else output


def cat(tensors: Sequence[torch.Tensor], dim: int = 0, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(tensors=tensors, dim=dim, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("cat", **kwargs) or _fallback_cat)(**kwargs)


def pad(input: torch.Tensor, pad: Sequence[int], mode: str = "...", value: float | None = None, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    # (the default mode is the reference's, an artefact of its generator: F.pad refuses it)
    kwargs = dict(input=input, pad=pad, mode=mode, value=value, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("pad", **kwargs) or _fallback_pad)(**kwargs)


# ---- index_add, permute (reference _gen/operators.py: dispatch(op, **kwargs) or the generated fallback) ------------------------------
def _fallback_index_add(input: torch.Tensor, dim: int, index: torch.Tensor, source: torch.Tensor, alpha: float = 1, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool = True) -> torch.Tensor:
    """Dequantize input / source, torch.index_add, optional output quantizer (reference fallback.py:1483-1516)."""
    _check_output_quantizer(output_quantizer, strict_quantization)
    input = _dequantized("input", input, strict_quantization)
    source = _dequantized("source", source, strict_quantization)
    output = torch.index_add(input=input, dim=dim, index=index, source=source, alpha=alpha)
    return output_quantizer(output) if output_quantizer is not None else output


def _fallback_permute(input: torch.Tensor, dims: tuple[int, ...], *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool = True) -> torch.Tensor:
    """Dequantize, torch.permute, optional output quantizer (reference fallback.py:1427-1449)."""
    _check_output_quantizer(output_quantizer, strict_quantization)
    input = _dequantized("input", input, strict_quantization)
    output = torch.permute(input=input, dims=dims)
    return output_quantizer(output) if output_quantizer is not None else output


def index_add(input: torch.Tensor, dim: int, index: torch.Tensor, source: torch.Tensor, alpha: float = 1, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, dim=dim, index=index, source=source, alpha=alpha, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("index_add", **kwargs) or _fallback_index_add)(**kwargs)


def permute(input: torch.Tensor, dims: tuple[int, ...], *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, dims=dims, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("permute", **kwargs) or _fallback_permute)(**kwargs)


# ---- unfold (reference _gen/operators.py:1500: dispatch(op, **kwargs) or the generated fallback) --------------------------------------
def _fallback_unfold(input: torch.Tensor, kernel_size: Any, dilation: Any = 1, padding: Any = 0, stride: Any = 1, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool = True) -> torch.Tensor:
    """Dequantize, F.unfold, optional output quantizer (reference fallback.py:1650-1677)."""
    _check_output_quantizer(output_quantizer, strict_quantization)
    input = _dequantized("input", input, strict_quantization)
    output = torch.nn.functional.unfold(input=input, kernel_size=kernel_size, dilation=dilation, padding=padding, stride=stride)
    return output_quantizer(output) if output_quantizer is not None else output


def unfold(input: torch.Tensor, kernel_size: Any, dilation: Any = 1, padding: Any = 0, stride: Any = 1, *, output_quantizer: Optional["Quantizer"] = None, strict_quantization: bool | None = None) -> torch.Tensor:
    kwargs = dict(input=input, kernel_size=kernel_size, dilation=dilation, padding=padding, stride=stride, output_quantizer=output_quantizer, strict_quantization=_strict(strict_quantization))
    return (dispatch("unfold", **kwargs) or _fallback_unfold)(**kwargs)


from fastforward_amd.nn.sdpa import scaled_dot_product_attention  # noqa: E402  (nn/sdpa.py calls back into this module)
