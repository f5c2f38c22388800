"""Host-tensor route of the four operators, the min/max reduction and the range -> parameter rule.

BASELINE configs[0] is "single nn.Linear 1024 x 1024, 8-bit per-tensor weight LinearQuantizer on CPU eager (plumbing, no GPU)",
and the reference's quantizers default to ``device="cpu"`` (nn/linear_quantizer.py:147-173): its operators are device-agnostic
ATen chains (quantization/_quantizer_impl.py:144-285). The HIP kernels of this package take device pointers only, so a tensor that
lives in HOST memory takes the same chain here — tiles_to_rows, div, sub, round, clamp, rows_to_tiles, cast — written once more
in terms of this package's own ``tiled_tensor`` helpers. This is not a fallback of the device path:

* a HIP tensor never reaches this module (``ops._host_route`` looks at the tensor's device, nothing else), and without
  ``libffq_hip.so`` every operator on a HIP tensor still raises ``BackendError``;
* nothing here is timed, fused or tuned — host tensors are the plumbing case (conversion, calibration and a forward of a small
  module before it is moved to the GPU), checked against the golden fixtures G1-G5 in ``tests/test_host_route.py``;
* the quantized-operator dispatcher claims HIP operands only, so a quantized linear on host tensors runs the generated
  fallback — dequantize, ``F.linear``, output quantizer — exactly as in the reference (_gen/fallback.py:77-112).
"""

from __future__ import annotations

from typing import Sequence

import torch

from fastforward_amd.exceptions import QuantizationError
from fastforward_amd.quantization.tiled_tensor import rows_to_tiles, tiles_to_rows


# explicit mantissa bits by torch.finfo(...).dtype name; complex dtypes report their component's name
_MANTISSA_BITS = {"bfloat16": 7, "float16": 10, "float32": 23, "float64": 52,
                  "float8_e4m3fn": 3, "float8_e4m3fnuz": 3, "float8_e5m2": 2, "float8_e5m2fnuz": 2}


def can_support_bitwidth(dtype: torch.dtype, num_bits: float) -> bool:
    """reference _quantizer_impl.py:44-75: the container's precision bits + 2 (the first unrepresentable integer lies beyond
    2^(mantissa + 1), and the sign is a bit of its own) must cover `num_bits`; precision bits = explicit mantissa of a float
    (fp8 variants included, complex dtypes by their component), the width of an integer type, and — a float type the table does
    not know — `num_bits` itself, with a warning, as the reference decides."""
    if dtype.is_complex or dtype.is_floating_point:
        name = torch.finfo(dtype).dtype
        if name in _MANTISSA_BITS:
            precision = _MANTISSA_BITS[name]
        else:
            import logging

            logging.getLogger(__name__).warning(f"Unknown mantissa size for {dtype}; precision loss possible.")
            precision = num_bits
    else:
        precision = torch.iinfo(dtype).bits
    return precision + 2 >= num_bits


def _params(scale: torch.Tensor, offset: torch.Tensor | None, rows: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    s = scale.reshape(-1)
    o = torch.round(offset.reshape(-1)) if offset is not None else torch.zeros_like(s)  # _infer_offset (:140-141)
    if rows.numel() and s.numel() not in (1, rows.shape[0]):
        if rows.shape[0] == 1:
            raise ValueError(f"tiled_data is expected to be of size (1, L) but scale has {s.numel()} entries")
        raise RuntimeError(f"The size of tensor a ({rows.shape[0]}) must match the size of tensor b ({s.numel()}) at non-singleton dimension 0")
    return s, o


def quantize_by_tile(data: torch.Tensor, scale: torch.Tensor, tile_size: Sequence[int], num_bits: float, output_dtype: torch.dtype | None,
                     offset: torch.Tensor | None = None) -> torch.Tensor:
    """A1 (:144-169)."""
    lo = -(2 ** (num_bits - 1))
    hi = -lo - 1
    rows = tiles_to_rows(data, tile_size)
    s, o = _params(scale, offset, rows)
    q = torch.clamp(torch.round(rows / s[:, None] - o[:, None]), lo, hi)
    out = rows_to_tiles(q, data.shape, tile_size)
    output_dtype = output_dtype or out.dtype
    if not can_support_bitwidth(output_dtype, num_bits):
        raise RuntimeError(f"Provided dtype ({output_dtype}) is not enough to store {num_bits} bits quantized values.")
    return out.to(output_dtype)


def dequantize_by_tile(data: torch.Tensor, scale: torch.Tensor, tile_size: Sequence[int], offset: torch.Tensor | None = None,
                       output_dtype: torch.dtype | None = None) -> torch.Tensor:
    """A2 (:172-190)."""
    rows = tiles_to_rows(data, tile_size)
    s, o = _params(scale, offset, rows)
    out = rows_to_tiles((rows + o[:, None]) * s[:, None], data.shape, tile_size)
    return out.to(output_dtype) if output_dtype is not None else out


def minmax_by_tile(data: torch.Tensor, tile_size: Sequence[int]) -> tuple[torch.Tensor, torch.Tensor]:
    """A4's reduction (range_setting/minmax.py:227-228): per-tile extrema in the data dtype."""
    if data.numel() == 0:
        raise QuantizationError(f"Cannot dynamically quantize an empty tensor of shape {tuple(data.shape)}")
    rows = tiles_to_rows(data, tile_size)
    return torch.min(rows, dim=1).values, torch.max(rows, dim=1).values


def parameters_for_range(min_range: torch.Tensor, max_range: torch.Tensor, num_bits: float, symmetric: bool, allow_one_sided: bool,
                         round_offset: bool = False) -> tuple[torch.Tensor, torch.Tensor | None]:
    """A5 (affine/range.py:54-122)."""
    lo, hi = min_range.reshape(-1).to(torch.float32), max_range.reshape(-1).to(torch.float32)
    one_sided = bool(lo.min() >= 0) and allow_one_sided
    int_min = -(2 ** (num_bits - 1))
    if symmetric and one_sided:
        lo = torch.zeros_like(lo)
    if symmetric and not one_sided:
        return torch.max(torch.abs(lo) / abs(int_min), torch.abs(hi) / abs(-int_min - 1)), None
    scale = ((hi - lo) / (2**num_bits - 1)).clamp(torch.finfo(torch.float32).eps)
    offset = lo / scale - int_min
    return scale, torch.round(offset) if round_offset else offset


def quantize_dynamic_by_tile(data: torch.Tensor, tile_size: Sequence[int], num_bits: float, symmetric: bool, allow_one_sided: bool,
                             output_dtype: torch.dtype | None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """A3 (:243-285)."""
    lo, hi = minmax_by_tile(data, tile_size)
    scale, offset = parameters_for_range(lo, hi, num_bits, symmetric, allow_one_sided)
    offset = torch.round(offset) if offset is not None else torch.zeros_like(scale)
    rows = tiles_to_rows(data, tile_size)
    bound = -(2 ** (num_bits - 1))
    q = torch.clamp(torch.round(rows / scale[:, None] - offset[:, None]), bound, -bound - 1)
    out = rows_to_tiles(q, data.shape, tile_size)
    output_dtype = output_dtype or out.dtype
    if not can_support_bitwidth(output_dtype, num_bits):
        raise RuntimeError(f"Provided dtype ({output_dtype}) is not enough to store {num_bits} bits quantized values.")
    return out.to(output_dtype), scale, offset


# ---- OCP microscaling (MX): the torch restatement of include_mx/ffq_mx.h and docs/numerics.md, on any device ------------------------------
MX_BLOCK = 32
MX_FORMATS = ("e4m3", "e2m1")
_MX_EMAX = {"e4m3": 8, "e2m1": 2}
_MX_MAX = {"e4m3": 448.0, "e2m1": 6.0}
_E2M1_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def mx_check_format(element_format: str) -> str:
    if element_format not in MX_FORMATS:
        raise ValueError(f"the MX element format is 'e4m3' or 'e2m1', got {element_format!r}")
    return element_format


def mx_quantize(data: torch.Tensor, element_format: str) -> tuple[torch.Tensor, torch.Tensor]:
    """``(codes uint8 of data's shape, scales uint8 [..., K / 32])``: one code per byte (e2m1: in the low nibble), one E8M0 byte per block
    of 32 consecutive elements of the last dimension."""
    fmt = mx_check_format(element_format)
    if data.dim() < 1 or data.shape[-1] % MX_BLOCK:
        raise ValueError(f"mx_quantize: the last dimension must be a multiple of {MX_BLOCK}, got shape {tuple(data.shape)}")
    x = data.detach().to(torch.float32).contiguous()
    blocks = x.reshape(*x.shape[:-1], x.shape[-1] // MX_BLOCK, MX_BLOCK)
    magnitude = blocks.view(torch.int32) & 0x7FFFFFFF  # NaN and Inf sort above every finite value
    e = magnitude.amax(dim=-1) >> 23
    poisoned = e == 255
    scale = torch.where(poisoned, torch.full_like(e, 255), (e - _MX_EMAX[fmt]).clamp(min=0))
    mult = ((254 - torch.where(poisoned, torch.full_like(e, 127), scale)) << 23).to(torch.int32).view(torch.float32)  # 2^(127 - scale)
    y = (blocks * mult[..., None]).clamp(-_MX_MAX[fmt], _MX_MAX[fmt])
    y = torch.where(poisoned[..., None], torch.zeros_like(y), y)
    if fmt == "e4m3":
        codes = y.to(torch.float8_e4m3fn).view(torch.uint8)
    else:
        ay = y.abs()
        mag = ((ay > 0.25).to(torch.uint8) + (ay >= 0.75) + (ay > 1.25) + (ay >= 1.75) + (ay > 2.5) + (ay >= 3.5) + (ay > 5.0)).to(torch.uint8)
        codes = mag | (torch.signbit(y).to(torch.uint8) << 3)
    codes = torch.where(poisoned[..., None], torch.zeros_like(codes), codes)
    return codes.reshape(x.shape), scale.to(torch.uint8)


def mx_scale_values(scales: torch.Tensor) -> torch.Tensor:
    """2^(code - 127) in fp32: subnormal for code 0, NaN for code 255."""
    s = scales.to(torch.int32)
    bits = torch.where(s == 0, torch.full_like(s, 0x00400000), torch.where(s == 255, torch.full_like(s, 0x7FC00000), s << 23))
    return bits.view(torch.float32)


def mx_element_values(codes: torch.Tensor, element_format: str) -> torch.Tensor:
    """The fp32 value of each element code (one per byte)."""
    if mx_check_format(element_format) == "e4m3":
        return codes.view(torch.float8_e4m3fn).to(torch.float32)
    grid = torch.tensor(_E2M1_GRID, dtype=torch.float32, device=codes.device)
    value = grid[(codes & 7).long()]
    return torch.where((codes & 8) != 0, -value, value)


def mx_dequantize(codes: torch.Tensor, scales: torch.Tensor, element_format: str, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """``value(code) * 2^(scale - 127)`` as one fp32 product, rounded once to `dtype`. `codes` holds one code per byte."""
    if codes.shape[-1] % MX_BLOCK or tuple(scales.shape) != (*codes.shape[:-1], codes.shape[-1] // MX_BLOCK):
        raise ValueError(f"mx_dequantize: codes {tuple(codes.shape)} and scales {tuple(scales.shape)} do not match")
    value = mx_element_values(codes, element_format)
    blocks = value.reshape(*scales.shape, MX_BLOCK) * mx_scale_values(scales)[..., None]
    return blocks.reshape(codes.shape).to(dtype)


def mx_pack(codes: torch.Tensor) -> torch.Tensor:
    """e2m1 codes one per byte -> two per byte along the last dimension: element 2i in the low nibble, 2i + 1 in the high one."""
    if codes.dtype != torch.uint8 or codes.shape[-1] % 2:
        raise ValueError(f"mx_pack: uint8 codes with an even last dimension, got {codes.dtype} {tuple(codes.shape)}")
    pairs = codes.reshape(*codes.shape[:-1], codes.shape[-1] // 2, 2)
    return (pairs[..., 0] & 15) | (pairs[..., 1] << 4)


def mx_unpack(packed: torch.Tensor) -> torch.Tensor:
    """The inverse of ``mx_pack``."""
    if packed.dtype != torch.uint8:
        raise ValueError(f"mx_unpack: uint8 bytes, got {packed.dtype}")
    return torch.stack((packed & 15, packed >> 4), dim=-1).reshape(*packed.shape[:-1], packed.shape[-1] * 2)
