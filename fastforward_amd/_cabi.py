"""ctypes view of the C ABI declared in ``include/ffq.h``.

Any shared library that exports that ABI can be wrapped by :class:`FFQLibrary`. The product wraps
``fastforward_amd/csrc/libffq_hip.so`` (see :mod:`fastforward_amd._native`); the test-suite wraps
the CPU oracle with the same class so both sides are driven through identical call sites.

Nothing in this module touches torch: arguments are raw addresses and integers.
"""

from __future__ import annotations

import ctypes
import enum
import os

from typing import Sequence

from fastforward_amd.exceptions import QuantizationError

FFQ_MAX_DIMS = 8
FFQ_MAX_FANOUT = 3
FFQ_ABI_VERSION = 9


class Status(enum.IntEnum):
    OK = 0
    ERR_TILE_RANK = 1
    ERR_TILE_DIVIDE = 2
    ERR_PARAM_NUMEL = 3
    ERR_PRECISION = 4
    ERR_EMPTY = 5
    ERR_DTYPE = 6
    ERR_ARG = 7
    ERR_WORKSPACE = 8
    ERR_LAUNCH = 9
    ERR_PARAM_ROWS = 10


class DType(enum.IntEnum):
    F32 = 0
    BF16 = 1
    F16 = 2
    F64 = 3
    I8 = 4
    I16 = 5
    I32 = 6
    I64 = 7
    U8 = 8


FLAG_INF = 1
FLAG_NAN = 2

# Exception type the reference raises for each failure (see the comments in include/ffq.h).
_EXCEPTIONS: dict[int, type[Exception]] = {
    Status.ERR_TILE_RANK: ValueError,
    Status.ERR_TILE_DIVIDE: ValueError,
    Status.ERR_PARAM_NUMEL: RuntimeError,
    Status.ERR_PRECISION: RuntimeError,
    Status.ERR_EMPTY: QuantizationError,
    Status.ERR_DTYPE: NotImplementedError,
    Status.ERR_ARG: ValueError,
    Status.ERR_WORKSPACE: RuntimeError,
    Status.ERR_LAUNCH: RuntimeError,
    Status.ERR_PARAM_ROWS: ValueError,
}


class Tiling(ctypes.Structure):
    """``ffq_tiling``: data shape and parameter-sharing tile."""

    _fields_ = [
        ("ndim", ctypes.c_int32),
        ("shape", ctypes.c_int64 * FFQ_MAX_DIMS),
        ("tile", ctypes.c_int64 * FFQ_MAX_DIMS),
    ]

    @classmethod
    def make(cls, shape: Sequence[int], tile: Sequence[int]) -> "Tiling":
        if len(shape) != len(tile):
            # check_tile_compatibility, quantization/tiled_tensor.py:24-29
            msg = (
                "Input dimensionality must match tile_size dimensionality got "
                f"{len(shape)} and {len(tile)}"
            )
            raise ValueError(msg)
        if len(shape) > FFQ_MAX_DIMS:
            raise NotImplementedError(f"tensors of rank > {FFQ_MAX_DIMS} are not supported")
        t = cls()
        t.ndim = len(shape)
        for i, (s, b) in enumerate(zip(shape, tile)):
            t.shape[i] = int(s)
            t.tile[i] = int(b)
        return t


class FanOut(ctypes.Structure):
    """``ffq_fanout``: the static per-tensor int8 quantizers fed by one fused producer."""

    _fields_ = [
        ("count", ctypes.c_int32),
        ("num_bits", ctypes.c_double),
        ("scale", ctypes.c_void_p * FFQ_MAX_FANOUT),
        ("offset", ctypes.c_void_p * FFQ_MAX_FANOUT),
        ("codes", ctypes.c_void_p * FFQ_MAX_FANOUT),
    ]

    @classmethod
    def make(cls, num_bits: float, scales: Sequence[int], offsets: Sequence[int | None], codes: Sequence[int]) -> "FanOut":
        if not (len(scales) == len(offsets) == len(codes)) or len(scales) > FFQ_MAX_FANOUT:
            raise ValueError(f"a fused producer feeds at most {FFQ_MAX_FANOUT} quantizers")
        f = cls()
        f.count = len(scales)
        f.num_bits = float(num_bits)
        for j, (s, o, c) in enumerate(zip(scales, offsets, codes)):
            f.scale[j], f.offset[j], f.codes[j] = s, o, c
        return f


FFQ_MAX_BATCH = 8


class RowsBatch(ctypes.Structure):
    """``ffq_rows_batch``: several row-quantized bf16 weights for one A1 launch."""

    _fields_ = [
        ("count", ctypes.c_int32),
        ("num_bits", ctypes.c_double),
        ("data", ctypes.c_void_p * FFQ_MAX_BATCH),
        ("scale", ctypes.c_void_p * FFQ_MAX_BATCH),
        ("offset", ctypes.c_void_p * FFQ_MAX_BATCH),
        ("codes", ctypes.c_void_p * FFQ_MAX_BATCH),
        ("rows", ctypes.c_int64 * FFQ_MAX_BATCH),
        ("cols", ctypes.c_int64 * FFQ_MAX_BATCH),
        ("rowsum", ctypes.c_void_p * FFQ_MAX_BATCH),
    ]


class SdpaQuantizer(ctypes.Structure):
    """``ffq_sdpa_quantizer``: one of the eight quantizer slots of ``ffq_sdpa_quantize`` (scale NULL: inactive)."""

    _fields_ = [("scale", ctypes.c_void_p), ("offset", ctypes.c_void_p), ("num_bits", ctypes.c_double)]


SDPA_QUANTIZERS = 8  # FFQ_SDPA_QUANTIZERS

FFQ_CAT_MAX_INPUTS = 8


class CatInputs(ctypes.Structure):
    """``ffq_cat_inputs``: the inputs of one ``ffq_cat_quantize`` launch (scale NULL: a plain input)."""

    _fields_ = [
        ("count", ctypes.c_int32),
        ("data", ctypes.c_void_p * FFQ_CAT_MAX_INPUTS),
        ("dt", ctypes.c_int32 * FFQ_CAT_MAX_INPUTS),
        ("scale", ctypes.c_void_p * FFQ_CAT_MAX_INPUTS),
        ("offset", ctypes.c_void_p * FFQ_CAT_MAX_INPUTS),
        ("run", ctypes.c_int64 * FFQ_CAT_MAX_INPUTS),
    ]

    @classmethod
    def make(cls, inputs: Sequence[tuple[int | None, int, int | None, int | None, int]]) -> "CatInputs":
        """`inputs`: (data, container tag, scale, offset, run) per input; the count is checked by the entry point."""
        c = cls()
        c.count = len(inputs)
        for i, (data, tag, scale, offset, run) in enumerate(inputs[:FFQ_CAT_MAX_INPUTS]):
            c.data[i], c.dt[i], c.scale[i], c.offset[i], c.run[i] = data, int(tag), scale, offset, int(run)
        return c

_vp = ctypes.c_void_p
_i = ctypes.c_int
_i64 = ctypes.c_int64
_d = ctypes.c_double
_sz = ctypes.c_size_t
_tp = ctypes.POINTER(Tiling)
_fp = ctypes.POINTER(FanOut)

# name -> (restype, argtypes); mirrors include/ffq.h one to one.
SIGNATURES: dict[str, tuple[object, list[object]]] = {
    "ffq_abi_version": (_i, []),
    "ffq_last_error": (ctypes.c_char_p, []),
    "ffq_backend_name": (ctypes.c_char_p, []),
    "ffq_num_tiles": (_i64, [_tp]),
    "ffq_can_support_bitwidth": (_i, [_i, _d]),
    "ffq_promote_types": (_i, [_i, _i]),
    "ffq_quantize_by_tile": (_i, [_vp, _i, _vp, _i, _i64, _vp, _i, _i64, _tp, _d, _vp, _i, _vp]),
    "ffq_dequantize_by_tile": (_i, [_vp, _i, _vp, _i, _i64, _vp, _i, _i64, _tp, _vp, _i, _vp]),
    "ffq_dequantize_result_dtype": (_i, [_i, _i, _i, _i]),
    "ffq_minmax_workspace_bytes": (_sz, [_tp, _i]),
    "ffq_minmax_by_tile": (_i, [_vp, _i, _tp, _vp, _vp, _i, _vp, _vp, _sz, _vp, _vp]),
    "ffq_running_minmax_step": (_i, [_vp, _i, _tp, _vp, _vp, _vp, _d, _i, _i, _vp, _i, _vp, _i, _vp, _sz, _vp, _vp]),
    "ffq_running_minmax_quantize": (_i, [_vp, _i, _tp, _vp, _vp, _vp, _d, _i, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "ffq_parameters_for_range_workspace_bytes": (_sz, [_i64, _i, _i]),
    "ffq_parameters_for_range": (_i, [_vp, _vp, _i, _i64, _d, _i, _i, _vp, _i, _vp, _i, _vp, _sz, _vp]),
    "ffq_quantize_dynamic_workspace_bytes": (_sz, [_tp, _i]),
    "ffq_quantize_dynamic_by_tile": (_i, [_vp, _i, _tp, _d, _i, _i, _vp, _i, _vp, _vp, _vp, _sz, _vp, _vp]),
    "ffq_pack_int4": (_i, [_vp, _i, _i64, _i64, _vp, _vp]),
    "ffq_unpack_int4": (_i, [_vp, _i64, _i64, _vp, _i, _vp]),
    "ffq_linear_w8a8_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "ffq_bmm_w8a8_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64]),
    "ffq_bmm_w8a8": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _d, _i, _i64, _i64, _i64, _i64, _vp, _sz, _vp]),
    "ffq_linear_w8a8": (
        _i,
        [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _d, _i, _i64, _i64, _i64, _vp, _sz, _vp],
    ),
    "ffq_linear_w8a8_multi": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _i, _i64, _vp, _i64, _vp, _sz, _vp]),
    "ffq_quantize_by_tile_unless_same": (_i, [_vp, _i, _vp, _vp, _i64, _d, _vp, _vp, _vp, _vp]),
    "ffq_linear_w8a8_takes_earlier": (_i, [_i64, _i64, _i64]),
    "ffq_linear_w8a8_earlier": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _i64, _i64, _i64, _vp, _sz, _vp]),
    "ffq_linear_w8a8_gated": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i64, _i64, _i64, _vp, _sz, _vp, _vp, _vp]),
    "ffq_gptq_block": (_i, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _d, _vp]),
    "ffq_gptq_block_grid": (_i, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _i64, _i64, _vp, _i, _i, _i, _d, _vp]),
    "ffq_pack_gguf_blocks": (_i, [_vp, _vp, _i64, _i, _vp, _vp]),
    "ffq_quantize_pack_int4": (_i, [_vp, _i, _vp, _i64, _vp, _i64, _tp, _i64, _vp, _vp]),
    "ffq_unpack_dequantize_int4": (_i, [_vp, _vp, _i64, _vp, _i64, _tp, _i64, _vp, _i, _vp]),
    "ffq_grid_sqerror_workspace_bytes": (_sz, [_tp, _i64]),
    "ffq_grid_sqerror_by_tile": (_i, [_vp, _i, _vp, _vp, _i64, _tp, _d, _vp, _i, _vp, _sz, _vp]),
    "ffq_quantize_backward_workspace_bytes": (_sz, [_tp]),
    "ffq_quantize_by_tile_backward": (_i, [_vp, _vp, _i, _vp, _i64, _vp, _i64, _tp, _d, _vp, _vp, _vp, _vp, _sz, _vp]),
    "ffq_mlp_gate_up_wq_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "ffq_mlp_gate_up_wq": (_i, [_vp, _i, _vp, _vp, _i, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _sz, _vp, _i64, _vp]),
    "ffq_mlp_gate_up_w8a8_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "ffq_mlp_gate_up_w8a8": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _d, _i64, _i64, _i64, _vp, _sz, _vp]),
    "ffq_mlp_gate_up_w8a8_estimating_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "ffq_mlp_gate_up_w8a8_estimating": (_i, [_vp] * 14 + [_i64, _i64, _i64, _vp, _sz, _vp, _vp, _vp]),
    "ffq_add_rmsnorm_quantize": (_i, [_vp, _vp, _vp, _vp, _i, _i64, _i64, _d, _vp, _fp, _vp]),
    "ffq_silu_mul_quantize": (_i, [_vp, _vp, _i, _i64, _vp, _fp, _vp]),
    "ffq_rope_inplace": (_i, [_vp, _i64, _vp, _i64, _i, _i64, _i64, _i64, _vp, _vp, _vp]),
    "ffq_layer_norm_quantize": (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _i, _i64, _i64, _d, _vp, _fp, _vp]),
    "ffq_embedding_quantize": (_i, [_vp, _i, _i64, _vp, _i, _i64, _i64, _vp, _vp, _i, _i64, _i, _vp, _fp, _vp, _vp]),
    "ffq_pointwise_quantize": (_i, [_i, _vp, _i, _vp, _vp, _i64, _i, _i64, _vp, _fp, _vp]),
    "ffq_binary_quantize": (_i, [_i, _vp, _i, _vp, _vp, _i64, _vp, _i, _vp, _vp, _i64, _i64, _d, _d, _i, _i64, _vp, _fp, _vp]),
    "ffq_softmax_quantize": (_i, [_vp, _i, _vp, _vp, _i, _i, _i64, _i64, _vp, _fp, _vp]),
    "ffq_activation_quantize": (_i, [_i, _vp, _i, _vp, _vp, _i64, _i, _i64, _vp, _fp, _vp]),
    "ffq_rms_norm_quantize": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _i64, _i64, _d, _vp, _fp, _vp]),
    "ffq_unary_quantize": (_i, [_i, _vp, _i, _vp, _vp, _i64, _d, _i, _i64, _vp, _fp, _vp]),
    "ffq_sum_quantize_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "ffq_sum_quantize": (_i, [_vp, _i, _vp, _vp, _i64, _i, _i64, _i64, _i64, _vp, _fp, _vp, _sz, _vp]),
    "ffq_cumsum_quantize": (_i, [_vp, _i, _vp, _vp, _i64, _i, _i64, _i64, _i64, _vp, _fp, _vp]),
    "ffq_pool2d_quantize": (_i, [_i, _vp, _i, _vp, _vp, _i64, _i] + [_i64] * 11 + [_i, _i64, _i64, _vp, _fp, _vp]),
    "ffq_upsample_nearest_quantize": (_i, [_vp, _i, _vp, _vp, _i64, _i, _i64, _i64, _i64, _i64, _i64, _d, _d, _i, _vp, _fp, _vp]),
    "ffq_cat_quantize": (_i, [ctypes.POINTER(CatInputs), _i, _i64, _i64, _i64, _vp, _fp, _vp]),
    "ffq_pad_quantize": (_i, [_i, _vp, _i, _vp, _vp, _i64, _i64, _i, _i64, _i64, _i64, _i64, ctypes.POINTER(_i64), _i, _vp, _fp, _vp]),
    "ffq_sdpa_quantize": (
        _i,
        [_vp, _vp, _vp, _i, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _i64, _i64, _i64, _i64, _i64, _i64, ctypes.POINTER(_i64), _vp, _i, _i,
         ctypes.POINTER(_i64), _d, _d, ctypes.POINTER(SdpaQuantizer), _i, _vp, _vp, _vp, _vp],
    ),
    "ffq_conv2d_w8a8_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64, _i64, _i64, _i64, _i]),
    "ffq_conv2d_w8a8": (
        _i,
        [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _d, _i,
         _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _sz, _vp],
    ),
    "ffq_conv_transpose2d_w8a8_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64, _i64, _i64, _i64, _i]),
    "ffq_conv_transpose2d_w8a8": (
        _i,
        [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _d, _i,
         _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _sz, _vp],
    ),
    "ffq_quantize_rows_rowsum": (_i, [_vp, _i, _vp, _vp, _i64, _i64, _d, _vp, _vp, _vp]),
    "ffq_linear_wq_supported": (_i, [_i, _i, _i, _i64, _i64, _i64, _i64, _i64]),
    "ffq_linear_wq_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "ffq_linear_wq_multi": (_i, [_vp, _i, _i, _vp, _i, _i64, _vp, _vp, _i, _i64, _vp, _i, _i64, _vp, _i64, _vp, _sz, _vp, _i64, _vp]),
    "ffq_linear_wq_split": (_i64, [_i64, _i64, _i64, _i]),
    "ffq_linear_wq_tickets": (_i64, [_i64, _i64, _i64, _i]),
    "ffq_linear_wq_slab_bytes": (_sz, [_i64, _i64, _i64, _i, _i64]),
    "ffq_linear_wq": (_i, [_vp, _i, _vp, _i, _i64, _vp, _vp, _i64, _i64, _vp, _i, _vp, _i, _i64, _i64, _i64, _vp, _sz, _vp, _i64, _vp]),
    "ffq_force_generic_kernels": (_i, [_i]),
    "ffq_quantize_rows_batch": (_i, [ctypes.POINTER(RowsBatch), _i, _vp]),
    "ffq_attention": (_i, [_vp, _vp, _vp, _i, _i64, _i64, _i64, _i64, _i64, _d, _i, _vp, _vp, _vp, _vp, _d, _vp, _vp, _vp]),
}

# Entry points only the HIP library must export: a host library (the CPU oracle) without one gets the attribute bound to None and
# callers treat that as "not covered". Whether the symbol is there is the capability check (FFQ_ABI_VERSION does not move for them).
DEVICE_ONLY: frozenset[str] = frozenset({"ffq_gptq_block_grid", "ffq_layer_norm_quantize", "ffq_embedding_quantize", "ffq_pointwise_quantize",
                                         "ffq_conv2d_w8a8", "ffq_conv2d_w8a8_workspace_bytes", "ffq_conv_transpose2d_w8a8",
                                         "ffq_conv_transpose2d_w8a8_workspace_bytes", "ffq_binary_quantize", "ffq_softmax_quantize",
                                         "ffq_activation_quantize", "ffq_sdpa_quantize", "ffq_rms_norm_quantize", "ffq_unary_quantize",
                                         "ffq_sum_quantize_workspace_bytes", "ffq_sum_quantize", "ffq_cumsum_quantize",
                                         "ffq_pool2d_quantize", "ffq_upsample_nearest_quantize", "ffq_cat_quantize", "ffq_pad_quantize"})


# name -> (restype, argtypes); mirrors include/ffq_3d.h one to one. A second table for a second header: SIGNATURES is the ABI both
# libraries export at FFQ_ABI_VERSION 9, and it stays as it is; these entry points exist in the HIP library only. A library that lacks
# one gets the attribute bound to None (DEVICE_ONLY's rule), whichever library it is.
SIGNATURES_3D: dict[str, tuple[object, list[object]]] = {
    "ffq_conv3d_w8a8_workspace_bytes": (_sz, [_i64] * 9 + [_i]),
    "ffq_conv3d_w8a8": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _d, _i] + [_i64] * 18 + [_vp, _sz, _vp]),
    "ffq_pool3d_quantize": (_i, [_i, _vp, _i, _vp, _vp, _i64, _i] + [_i64] * 13 + [_i, _i64, _i64, _i64, _vp, _fp, _vp]),
}

# name -> (restype, argtypes); mirrors include/ffq_depthwise.h one to one: the third header's table, bound as SIGNATURES_3D is (None on
# a library without the symbol).
SIGNATURES_DEPTHWISE: dict[str, tuple[object, list[object]]] = {
    "ffq_depthwise_conv2d_w8a8": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _d, _i] + [_i64] * 13 + [_vp]),
}

# name -> (restype, argtypes); mirrors include/ffq_index.h one to one: the fourth header's table (the quantized index_add and permute),
# bound as SIGNATURES_3D is (None on a library without the symbol).
SIGNATURES_INDEX: dict[str, tuple[object, list[object]]] = {
    "ffq_index_add_quantize": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i64, _vp, _i, _vp, _vp, _d, _i, _i64, _i64, _i64, _vp, _fp, _vp]),
    "ffq_permute_quantize": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, ctypes.POINTER(_i64), ctypes.POINTER(_i64), _vp, _fp, _vp]),
}

# name -> (restype, argtypes); mirrors include/ffq_unfold.h one to one: the fifth header's table (the quantized unfold), bound as
# SIGNATURES_3D is (None on a library without the symbol).
SIGNATURES_UNFOLD: dict[str, tuple[object, list[object]]] = {
    "ffq_unfold_quantize": (_i, [_vp, _i, _vp, _vp, _i, _i] + [_i64] * 12 + [_vp, _fp, _vp]),
}

# name -> (restype, argtypes); mirrors include/ffq_sdpa_decode.h one to one: the sixth header's table (attention for a short query over
# int8 K / V codes, split over the keys), bound as SIGNATURES_3D is (None on a library without the symbol).
SIGNATURES_DECODE: dict[str, tuple[object, list[object]]] = {
    "ffq_sdpa_decode_splits": (_i64, [_i64] * 5),
    "ffq_sdpa_decode_workspace_bytes": (_sz, [_i64] * 5),
    "ffq_sdpa_decode": (
        _i,
        [_vp, _i, _vp, _vp, _i, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _i64, _i64, _i64, _i64, _i64, _i64, ctypes.POINTER(_i64), _vp, _i, _i,
         ctypes.POINTER(_i64), _d, _vp, _vp, _d, _i64, _vp, _vp, _sz, _vp],
    ),
}

# name -> (restype, argtypes); mirrors include/ffq_kv_cache.h one to one: the seventh header's table (the in-place append of a
# preallocated int8 KV cache and the decode attention with device-side lengths), bound as SIGNATURES_3D is (None on a library without
# the symbol).
SIGNATURES_KV: dict[str, tuple[object, list[object]]] = {
    "ffq_kv_append": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, ctypes.POINTER(_i64), _vp, _vp, _d, _vp, _vp, _d, _vp, _vp, _i64, _vp]),
    "ffq_kv_decode": (
        _i,
        [_vp, _i, _vp, _vp, _i, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, _i64, _i64, _i64, _i64, _i64, _i64, ctypes.POINTER(_i64), _i, _d, _vp,
         _vp, _d, _i64, _i64, _vp, _vp, _sz, _vp],
    ),
}

# name -> (restype, argtypes); mirrors include/ffq_kv_paged.h one to one: the eighth header's table (the append and the decode
# attention of ffq_kv_cache.h over K / V held in fixed-size pages behind a per-sequence block table), bound as SIGNATURES_3D is (None
# on a library without the symbol).
SIGNATURES_PAGED: dict[str, tuple[object, list[object]]] = {
    "ffq_kv_paged_append": (
        _i,
        [_vp, _vp, _i, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, ctypes.POINTER(_i64), _vp, _vp, _d, _vp, _vp, _d, _vp, _vp,
         _i64, _vp],
    ),
    "ffq_kv_paged_decode": (
        _i,
        [_vp, _i, _vp, _vp, _i, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64,
         ctypes.POINTER(_i64), _i, _d, _vp, _vp, _d, _i64, _i64, _vp, _vp, _sz, _vp],
    ),
}

# name -> (restype, argtypes); mirrors include/ffq_kv_token.h one to one: the ninth header's table (the KV cache of ffq_kv_cache.h with one
# dynamic (scale, offset) per position: the append that computes them and the decode attention that reads them), bound as
# SIGNATURES_3D is (None on a library without the symbol).
SIGNATURES_KV_TOKEN: dict[str, tuple[object, list[object]]] = {
    "ffq_kv_token_append": (
        _i,
        [_vp, _vp, _i, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, ctypes.POINTER(_i64), _d, _i, _d, _i, _vp, _vp, _i64, _vp],
    ),
    "ffq_kv_token_decode": (
        _i,
        [_vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, ctypes.POINTER(_i64), _i, _d, _vp, _vp, _d, _i64, _i64,
         _vp, _vp, _sz, _vp],
    ),
}

# name -> (restype, argtypes); mirrors include/ffq_kv_paged_token.h one to one: the tenth header's table (the paged cache of
# ffq_kv_paged.h with the per-position parameters of ffq_kv_token.h in a third pool), bound as SIGNATURES_3D is (None on a library
# without the symbol).
SIGNATURES_PAGED_TOKEN: dict[str, tuple[object, list[object]]] = {
    "ffq_kv_paged_token_append": (
        _i,
        [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, ctypes.POINTER(_i64), _d, _i, _d, _i, _vp, _vp, _i64,
         _vp],
    ),
    "ffq_kv_paged_token_decode": (
        _i,
        [_vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, ctypes.POINTER(_i64), _i, _d, _vp,
         _vp, _d, _i64, _i64, _vp, _vp, _sz, _vp],
    ),
}

# name -> (restype, argtypes); mirrors include/lpbq/ffq_lpbq.h one to one: the eleventh header's table (LPBQ weights: scale compression,
# the fused weight quantizer into int8 per-channel codes, and the expansion of 4-bit codes at rest), bound as SIGNATURES_3D is (None
# on a library without the symbol).
SIGNATURES_LPBQ: dict[str, tuple[object, list[object]]] = {
    "ffq_lpbq_compress_scales": (_i, [_vp, _i64, _i64, _i64, _i, _vp, _vp, _vp]),
    "ffq_lpbq_quantize": (_i, [_vp, _i, _i64, _vp, _i64, _i64, _i64, _i64, _i, _i, _vp, _vp, _vp, _vp]),
    "ffq_lpbq_expand": (_i, [_vp, _i, _i64, _vp, _i64, _i64, _i64, _vp, _vp]),
}

# name -> (restype, argtypes); mirrors include_mx/ffq_mx.h one to one: the twelfth header's table (OCP microscaling: the MXFP8 / MXFP4
# quantizer, its inverse, and the linear on the block-scaled matrix cores), bound as SIGNATURES_3D is (None on a library without the symbol).
SIGNATURES_MX: dict[str, tuple[object, list[object]]] = {
    "ffq_mx_quantize": (_i, [_vp, _i, _i64, _i64, _i64, _i, _vp, _vp, _vp, _vp]),
    "ffq_mx_dequantize": (_i, [_vp, _i, _vp, _i64, _i64, _i, _vp, _i, _vp]),
    "ffq_linear_mx_supported": (_i, [_i64, _i64, _i64, _i, _i]),
    "ffq_linear_mx": (_i, [_vp, _i64, _vp, _i64, _i, _vp, _i64, _vp, _i64, _i, _vp, _i, _vp, _i, _i64, _i64, _i64, _vp]),
}

MX_E4M3 = 0  # FFQ_MX_E4M3
MX_E2M1 = 1  # FFQ_MX_E2M1

SDPA_DECODE_MAX_ROWS = 32  # FFQ_SDPA_DECODE_MAX_ROWS
SDPA_DECODE_KEY_TILE = 128  # FFQ_SDPA_DECODE_KEY_TILE
SDPA_DECODE_MAX_SPLITS = 64  # FFQ_SDPA_DECODE_MAX_SPLITS


class FFQLibrary:
    """A loaded implementation of the ``ffq_*`` ABI."""

    def __init__(self, path: str | os.PathLike[str]):
        self.path = os.fspath(path)
        self._dll = ctypes.CDLL(self.path)
        missing = []
        for name, (restype, argtypes) in SIGNATURES.items():
            try:
                fn = getattr(self._dll, name)
            except AttributeError as e:
                if name not in DEVICE_ONLY:
                    raise ImportError(f"{self.path} does not export {name}") from e
                missing.append(name)
                continue
            fn.restype = restype
            fn.argtypes = argtypes
            setattr(self, name, fn)
        version = self.ffq_abi_version()  # type: ignore[attr-defined]
        if version != FFQ_ABI_VERSION:
            raise ImportError(f"{self.path}: ABI version {version}, expected {FFQ_ABI_VERSION}")
        self.backend_name: str = self.ffq_backend_name().decode()  # type: ignore[attr-defined]
        if missing and self.is_device:
            raise ImportError(f"{self.path} does not export {missing[0]}")
        for name in missing:
            setattr(self, name, None)
        for name, (restype, argtypes) in (*SIGNATURES_3D.items(), *SIGNATURES_DEPTHWISE.items(), *SIGNATURES_INDEX.items(),
                                          *SIGNATURES_UNFOLD.items(), *SIGNATURES_DECODE.items(), *SIGNATURES_KV.items(), *SIGNATURES_PAGED.items(),
                                          *SIGNATURES_KV_TOKEN.items(), *SIGNATURES_PAGED_TOKEN.items(), *SIGNATURES_LPBQ.items(),
                                          *SIGNATURES_MX.items()):
            fn = getattr(self._dll, name, None)
            if fn is not None:
                fn.restype = restype
                fn.argtypes = argtypes
            setattr(self, name, fn)

    @property
    def is_device(self) -> bool:
        """True when the library expects device pointers."""
        return self.backend_name.startswith("hip")

    def check(self, status: int) -> None:
        """Raise the exception the reference raises for `status`."""
        if status == Status.OK:
            return
        message = self.ffq_last_error().decode(errors="replace")  # type: ignore[attr-defined]
        exc = _EXCEPTIONS.get(status, RuntimeError)
        raise exc(message or f"ffq status {status}")
