"""Tensor-level entry points of the hot path: torch tensors in, C-ABI calls out.

These functions are the bodies of the torch custom ops ``fastforward_amd::quantize_by_tile``,
``dequantize_by_tile``, ``quantize_dynamic_by_tile`` and ``quantize_by_tile_backward`` — the same
four schemas the reference registers under ``fastforward::`` (reference:
src/fastforward/quantization/_quantizer_impl.py:144-285) — plus the reduction / parameter / packing /
linear kernels the reference expresses as ATen chains. Every call is one enqueue on torch's current
HIP stream through the C ABI of ``include/ffq.h``: no host synchronisation, no hidden allocation in
the library (outputs and scratch are torch allocations), legal under hipGraph capture.


The package is split by family (round 6; one 1,700-line module before): ``static`` (the four registry operators and the row-batched
forms of A1), ``reductions`` (A4 / A5), ``packing`` (A7, GGUF, GPTQ, the grid estimator), ``gemm`` (A6 on int8 codes), ``wq`` (A6 with a
quantized weight and a plain input), ``producers`` (RMSNorm / SiLU*up / rotary / attention with A1 fused), ``modules``
(LayerNorm / Embedding / ReLU / SiLU with A2 and A1 fused), ``conv`` (the W8A8 convolutions, 2-D, transposed and 3-D), ``elementwise`` (add / sub / mul / div,
softmax, sigmoid, GELU with A2 and A1 fused), ``math`` (rms_norm, pow by a number, exp / sin / cos, sum and cumsum with A2 and A1
fused), ``pool`` (avg_pool1d / avg_pool2d / avg_pool3d / max_pool2d and nearest interpolate with A2 and A1 fused), ``concat`` (cat and pad with A2 and A1 fused), ``index`` (index_add and permute with A2 and A1 fused), ``unfold`` (im2col with A2 and A1 fused), ``sdpa`` (the quantized scaled_dot_product_attention in one launch), ``decode`` (the same for a short query over int8 K / V codes, split over the keys), ``kv_cache`` (the in-place append of a preallocated int8 KV cache and that attention with device-side lengths, dense, in pages behind a block table, or with one dynamic (scale, offset) per position), ``lpbq`` (W4 block-quantized weights as int8 per-channel codes: scale compression, the fused weight quantizer, the expansion of codes at rest), ``mx`` (OCP microscaling: the MXFP8 / MXFP4 quantizer, its inverse and the linear on the block-scaled matrix cores), ``registry`` (the torch operator
library and the C++ extension), ``_base`` (device check, tags, scratch). Every public name is re-exported here: ``ops.linear_wq`` etc.
"""

from __future__ import annotations

from fastforward_amd import _native  # noqa: F401  (tests and tools reach the loaded library through ops._native)
from fastforward_amd._cabi import FLAG_INF, FLAG_NAN  # noqa: F401
from fastforward_amd.ops import _base
from fastforward_amd.ops._base import (  # noqa: F401
    _DTYPES, _EXTREMA_WORDS, _PRODUCT_PREPARE, _TAGS, _TICKETS, _extrema_words, _flat, _host_route, _native_route, _ptr, _tag, _tickets, _tile_of,
    _workspace,
)
from fastforward_amd.ops.static import (  # noqa: F401
    _quantize_by_tile_backward_composite, dequantize_by_tile, quantize_by_tile, quantize_by_tile_backward, quantize_by_tile_unless_same, quantize_dynamic_by_tile, quantize_rows_batch, quantize_rows_rowsum,
)
from fastforward_amd.ops.packing import (  # noqa: F401
    _pack_gguf, gptq_block, gptq_block_grid, grid_sqerror_by_tile, pack_int4, pack_q4_0_blocks, pack_q8_0_blocks, quantize_pack_int4, unpack_dequantize_int4, unpack_int4,
)
from fastforward_amd.ops.reductions import (  # noqa: F401
    _running_minmax_step, minmax_by_tile, parameters_for_range, running_minmax_quantize, running_minmax_step,
)
from fastforward_amd.ops.gemm import (  # noqa: F401
    _bmm_w8a8, _linear_w8a8, bmm_w8a8, linear_w8a8, linear_w8a8_earlier, linear_w8a8_gated, linear_w8a8_multi, linear_w8a8_takes_earlier, mlp_gate_up_w8a8, mlp_gate_up_w8a8_estimating,
)
from fastforward_amd.ops.wq import (  # noqa: F401
    _linear_wq, _wq_scratch, linear_wq, linear_wq_multi, mlp_gate_up_wq,
)
from fastforward_amd.ops.producers import (  # noqa: F401
    _fan, add_rmsnorm_quantize, attention, rope_, silu_mul_quantize,
)
from fastforward_amd.ops.modules import (  # noqa: F401
    embedding_quantize, layer_norm_quantize, pointwise_quantize,
)
from fastforward_amd.ops.conv import conv2d_w8a8, conv3d_w8a8, conv_transpose2d_w8a8, depthwise_conv2d_w8a8  # noqa: F401
from fastforward_amd.ops.elementwise import activation_quantize, binary_quantize, softmax_quantize  # noqa: F401
from fastforward_amd.ops.math import cumsum_quantize, rms_norm_quantize, sum_quantize, unary_quantize  # noqa: F401
from fastforward_amd.ops.pool import pool2d_quantize, pool3d_quantize, upsample_nearest_quantize  # noqa: F401
from fastforward_amd.ops.concat import cat_quantize, pad_quantize  # noqa: F401
from fastforward_amd.ops.index import index_add_quantize, permute_quantize  # noqa: F401
from fastforward_amd.ops.unfold import unfold_quantize  # noqa: F401
from fastforward_amd.ops.sdpa import sdpa_quantize  # noqa: F401
from fastforward_amd.ops.decode import sdpa_decode, sdpa_decode_plan, sdpa_decode_workspace_bytes  # noqa: F401
from fastforward_amd.ops.kv_cache import kv_append, kv_decode, kv_paged_append, kv_paged_decode, kv_token_append, kv_token_decode  # noqa: F401
from fastforward_amd.ops.kv_cache import kv_paged_token_append, kv_paged_token_decode  # noqa: F401
from fastforward_amd.ops.lpbq import lpbq_compress_scales, lpbq_expand, lpbq_quantize  # noqa: F401
from fastforward_amd.ops.mx import linear_mx, linear_mx_supported, mx_dequantize, mx_quantize  # noqa: F401
from fastforward_amd.ops.registry import NATIVE_DISPATCH, TORCH_EXTENSION_PATH, _LIBRARY  # noqa: F401,E402

__all__ = [
    "quantize_by_tile",
    "dequantize_by_tile",
    "quantize_dynamic_by_tile",
    "quantize_by_tile_backward",
    "minmax_by_tile",
    "running_minmax_step",
    "parameters_for_range",
    "pack_int4",
    "unpack_int4",
    "pack_q4_0_blocks",
    "pack_q8_0_blocks",
    "quantize_pack_int4",
    "unpack_dequantize_int4",
    "gptq_block",
    "gptq_block_grid",
    "grid_sqerror_by_tile",
    "linear_w8a8",
    "linear_w8a8_multi",
    "bmm_w8a8",
    "linear_wq",
    "linear_wq_multi",
    "mlp_gate_up_w8a8",
    "add_rmsnorm_quantize",
    "silu_mul_quantize",
    "rope_",
    "quantize_rows_rowsum",
    "quantize_rows_batch",
    "attention",
    "layer_norm_quantize",
    "embedding_quantize",
    "pointwise_quantize",
    "conv2d_w8a8",
    "conv_transpose2d_w8a8",
    "conv3d_w8a8",
    "depthwise_conv2d_w8a8",
    "binary_quantize",
    "softmax_quantize",
    "activation_quantize",
    "rms_norm_quantize",
    "unary_quantize",
    "sum_quantize",
    "cumsum_quantize",
    "pool2d_quantize",
    "upsample_nearest_quantize",
    "pool3d_quantize",
    "cat_quantize",
    "pad_quantize",
    "index_add_quantize",
    "permute_quantize",
    "unfold_quantize",
    "sdpa_quantize",
    "sdpa_decode",
    "sdpa_decode_plan",
    "kv_append",
    "kv_decode",
    "kv_paged_append",
    "kv_paged_decode",
    "kv_paged_token_append",
    "kv_paged_token_decode",
    "kv_token_append",
    "kv_token_decode",
    "lpbq_compress_scales",
    "lpbq_quantize",
    "lpbq_expand",
    "mx_quantize",
    "mx_dequantize",
    "linear_mx",
    "linear_mx_supported",
    "FLAG_INF",
    "FLAG_NAN",
]


def __getattr__(name: str):
    # `_prepare` is looked up at call time by every module of the package (``_base._prepare``): the one seam oracle/inject.py substitutes
    if name == "_prepare":
        return _base._prepare
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
