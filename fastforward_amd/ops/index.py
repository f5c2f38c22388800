"""The reference's quantized index_add and permute as one-pass kernels with A1 fused in (csrc/ffq_index.hip, include/ffq_index.h),
each with its quantized inputs dequantized in registers (A2) and up to three static per-tensor output quantizers (reference
ff.nn.functional through _gen/fallback.py: permute :1427, index_add :1483).

An input given as codes comes with ``(scale, offset)``: int8 or value-dtype codes with fp32 parameters — one pair per tensor for
``index_add``, one pair for the tensor or one per index of one axis for ``permute``. A strided or misaligned view reaches the
kernel as an aligned copy (``ops._base._dense``). Each function returns ``(value or None, [codes per quantizer])``; the value has
the data dtype and is contiguous in the shape ATen gives."""

from __future__ import annotations

import ctypes
import math

from typing import Sequence

import torch

from fastforward_amd.ops import _base
from fastforward_amd.ops._base import _ptr, _tag
from fastforward_amd.ops.modules import Quantizers, _entry, _operand
from fastforward_amd.ops.producers import _fan

Dequant = tuple[torch.Tensor, torch.Tensor | None]
MAX_RANK = 6


def _axis(dim: int, ndim: int, what: str) -> int:
    if isinstance(dim, bool) or not isinstance(dim, int) or not -ndim <= dim < ndim:
        raise RuntimeError(f"{what}: dim {dim!r} is out of range for {ndim} dims")
    return dim % ndim


def index_add_quantize(
    x: torch.Tensor,
    dim: int,
    index: torch.Tensor,
    source: torch.Tensor,
    alpha: float = 1,
    quantizers: Quantizers = (),
    num_bits: float = 8.0,
    dtype: torch.dtype | None = None,
    dequant: Dequant | None = None,
    source_dequant: Dequant | None = None,
    want_value: bool = True,
) -> tuple[torch.Tensor | None, list[torch.Tensor]]:
    """``torch.index_add(x, dim, index, source, alpha=alpha)`` + A1, one pass. `x` and `source` are plain (`dtype`) or, with
    ``dequant`` / ``source_dequant`` ``= (scale, offset)``, codes (int8 or `dtype`) with per-tensor parameters; `index` is a 1-D
    int32 / int64 tensor of ``source.shape[dim]`` row numbers. Addends of one row are summed in fp32 in ascending order of their
    position in `index` and the sum is rounded once (include/ffq_index.h); an index value outside ``[0, x.shape[dim])`` is skipped."""
    dtype = dtype or x.dtype
    if x.dim() < 1:
        raise RuntimeError("index_add_quantize: the input has at least one dimension")
    d = _axis(dim, x.dim(), "index_add_quantize")
    if index.dim() != 1 or index.dtype not in (torch.int32, torch.int64):
        raise RuntimeError(f"index_add_quantize: index is a 1-D int32 or int64 tensor, got {tuple(index.shape)} of {index.dtype}")
    n = index.numel()
    if tuple(source.shape) != (*x.shape[:d], n, *x.shape[d + 1:]):
        raise RuntimeError(f"index_add_quantize: source {tuple(source.shape)} is input {tuple(x.shape)} with {n} rows along dim {d}")
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)):
        raise RuntimeError(f"index_add_quantize: alpha is a Python number, got {alpha!r}")
    xc, xs, xo, _ = _operand(x, dtype, 1, dequant, "index_add_quantize")
    sc, ss, so, _ = _operand(source, dtype, 1, source_dequant, "index_add_quantize")
    ic = index.detach().contiguous()
    lib, stream = _base._prepare(xc, xs, xo, ic, sc, ss, so, *[t for q in quantizers for t in q])
    shape = tuple(x.shape)
    out = torch.empty(shape, dtype=dtype, device=xc.device) if want_value else None
    fan, codes, keep = _fan(quantizers, num_bits, shape, xc.device)
    lib.check(
        _entry(lib, "ffq_index_add_quantize")(
            _ptr(xc), _tag(xc.dtype), _ptr(xs), _ptr(xo), _ptr(ic), _tag(ic.dtype), n, _ptr(sc), _tag(sc.dtype), _ptr(ss), _ptr(so),
            float(alpha), _tag(dtype), math.prod(shape[:d]), shape[d], math.prod(shape[d + 1:]), _ptr(out), ctypes.byref(fan), stream,
        )
    )
    del keep
    return out, codes


def permute_quantize(
    x: torch.Tensor,
    dims: Sequence[int],
    quantizers: Quantizers = (),
    num_bits: float = 8.0,
    dtype: torch.dtype | None = None,
    dequant: Dequant | None = None,
    param_axis: int | None = None,
    want_value: bool = True,
) -> tuple[torch.Tensor | None, list[torch.Tensor]]:
    """``torch.permute(x, dims).contiguous()`` + A1, one pass, for 1 to 6 dimensions. `x` plain or codes with one parameter pair, or
    with ``x.shape[param_axis]`` pairs indexed along axis `param_axis` of `x` (``PerChannel(param_axis)``)."""
    dtype = dtype or x.dtype
    rank = x.dim()
    if not 1 <= rank <= MAX_RANK:
        raise RuntimeError(f"permute_quantize: 1 to {MAX_RANK} dimensions, got {rank}")
    dims = [_axis(d, rank, "permute_quantize") for d in dims]
    if sorted(dims) != list(range(rank)):
        raise RuntimeError(f"permute_quantize: dims {dims} is not a permutation of {rank} axes")
    channels = 1 if param_axis is None else x.shape[_axis(param_axis, rank, "permute_quantize")]
    xc, s, o, per_channel = _operand(x, dtype, channels, dequant, "permute_quantize")
    lib, stream = _base._prepare(xc, s, o, *[t for q in quantizers for t in q])
    shape = tuple(x.shape[d] for d in dims)
    out = torch.empty(shape, dtype=dtype, device=xc.device) if want_value else None
    fan, codes, keep = _fan(quantizers, num_bits, shape, xc.device)
    lib.check(
        _entry(lib, "ffq_permute_quantize")(
            _ptr(xc), _tag(xc.dtype), _ptr(s), _ptr(o), param_axis % rank if per_channel else -1, _tag(dtype), rank,
            (ctypes.c_int64 * rank)(*x.shape), (ctypes.c_int64 * rank)(*dims), _ptr(out), ctypes.byref(fan), stream,
        )
    )
    del keep
    return out, codes
