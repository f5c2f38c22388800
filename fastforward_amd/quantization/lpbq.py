"""LPBQ — low-precision block quantization of weights (reference: src/fastforward/export/_lpbq.py, the encoding its QNN export writes
for 4-bit block-quantized weights).

A symmetric `compressed_bw`-bit weight with one scale per block of input channels has every block scale re-expressed as
``int_scale[n, j] * channel_scale[n]``: ``int_scale`` an integer in ``[1, 2^compressed_bw]``, ``channel_scale`` one float per output
channel. ``code * int_scale`` is then an integer of ``2 * compressed_bw`` bits — for 4-bit weights an int8 code in ``[-128, 112]`` — and the
weight is an ordinary per-channel symmetric tensor, which the int8 GEMM takes (``ops.linear_w8a8``, per-row weight scales).

    encode(weight_or_params)     the reference's ``generate_lpbq_encoding``: suitability checks, compression, ``LPBQEncoding.as_dict``
    decompress(qweight)          4-bit ``PerBlock(1, G, 0)`` QuantizedTensor -> int8 ``PerChannel(0)`` QuantizedTensor
    convert_model(model)         swap every matching weight quantizer for an ``nn.LPBQLinearQuantizer`` that shares its ``scale``

The device kernels (csrc/ffq_lpbq.hip through ``ops.lpbq_*``) take ``PerBlock(block_dims=(1,), per_channel_dims=(0,))`` with fp32
scales on the HIP device; the other orientation, other scale dtypes and host tensors take ``compress_scales_host``, the reference's
arithmetic in torch, op for op."""

from __future__ import annotations

import dataclasses

from typing import Any, Sequence

import torch

from fastforward_amd import ops
from fastforward_amd.quantization import granularity as granularities
from fastforward_amd.quantization.affine.function import AffineQuantizationFunction, StaticAffineQuantParams
from fastforward_amd.quantization.function import QuantizationContext

ROWS = ((1,), (0,))     # (block_dims, per_channel_dims): blocks along the input channels of an [out, in] weight — the kernels' case
COLUMNS = ((0,), (1,))  # blocks along dim 0 of an [in, out] weight


def check_bitwidths(compressed_bw: int, decompressed_bw: int) -> None:
    """The refusals of the reference's ``LPBQProcessor.__new__`` (_lpbq.py:22-46), in its order and words."""
    if compressed_bw <= 0 or decompressed_bw <= 0:
        raise ValueError(f"Bitwidths cannot be 0 or negative (compressed_bitwidth={compressed_bw}, decompressed_bitwdith={decompressed_bw})")
    if compressed_bw >= decompressed_bw:
        raise ValueError(
            "Compressed bitwidth cannot be larger than decompressed bitwidth "
            f"(compressed_bitwidth={compressed_bw}, decompressed_bitwdith={decompressed_bw})"
        )
    if compressed_bw > 8:
        raise ValueError(f"Compressed bitwidth can be max 8, got compressed_bitwidth={compressed_bw}")
    if decompressed_bw > 32:
        raise ValueError(f"Decompressed bitwidth can be max 32, got decompressed_bitwidth={decompressed_bw}")


def _int_scale_dtype(bits: int) -> torch.dtype:
    return torch.uint8 if 2**bits <= 255 else torch.int32


def compress_scales_host(scale_2d: torch.Tensor, block_axis: int, bits: int) -> tuple[torch.Tensor, torch.Tensor]:
    """``grouped_dynamic_quantize`` (_lpbq.py:138-175) in torch: the maximum over `block_axis` of the 2-D scales, ``d = max / 2^bits`` in
    the scales' dtype, ``q = clamp(round(s / d), 1, 2^bits)``. Returns ``(q in scale_2d's shape, d flat, one per channel)``."""
    top = 2**bits
    peak = torch.amax(scale_2d, dim=block_axis, keepdim=True)
    d = peak / peak.new_tensor(top)
    q = torch.clamp(torch.round(scale_2d / d), 1, top).to(_int_scale_dtype(bits))
    return q, d.reshape(-1)


def compress_scales(scale_2d: torch.Tensor, block_axis: int = 1, bits: int = 4) -> tuple[torch.Tensor, torch.Tensor]:
    """``(int_scale, channel_scale)`` of 2-D block scales: the kernel for fp32 ``[N, J]`` on the HIP device with blocks along dim 1 (up
    to 1024 per row, 2 to 4 bits), the host path for everything else."""
    on_kernel = (scale_2d.is_cuda and scale_2d.dtype == torch.float32 and block_axis in (1, -1) and bits in ops.lpbq.BITS
                 and scale_2d.shape[1] <= ops.lpbq.MAX_BLOCKS_PER_ROW and scale_2d.numel() > 0)
    if on_kernel:
        view = scale_2d.detach()
        return ops.lpbq_compress_scales(view if view.stride(1) == 1 or view.shape[1] == 1 else view.contiguous(), bits)
    # the host path runs on the host whatever the device (the scales are small): the reference's CPU arithmetic, bit for bit
    int_scale, channel_scale = compress_scales_host(scale_2d.detach().cpu(), block_axis, bits)
    return int_scale.to(scale_2d.device), channel_scale.to(scale_2d.device)


@dataclasses.dataclass
class LPBQEncoding:
    """One weight's LPBQ parameters: ``int_scale`` in the shape of the 2-D block scales (``[N, J]``, or ``[J, N]`` for blocks along
    dim 0), ``channel_scale`` flat, one per channel."""

    int_scale: torch.Tensor
    channel_scale: torch.Tensor
    block_size: int
    compressed_bw: int = 4
    decompressed_bw: int = 8

    def as_dict(self, name: str) -> dict[str, Any]:
        """The dict of the reference's ``generate_lpbq_encoding``, key for key (_lpbq.py:86-136)."""
        scales = self.channel_scale.flatten().tolist()
        return {
            "name": name,
            "dtype": "INT",
            "enc_type": "LPBQ",
            "is_sym": True,
            "compressed_bw": self.compressed_bw,
            "bw": self.decompressed_bw,
            "block_size": self.block_size,
            "per_block_int_scale": [int(v) for v in self.int_scale.flatten().tolist()],
            "scale": scales,
            "offset": [float(-(2 ** (self.decompressed_bw - 1)))] * len(scales),
        }


def _static_params(weight_or_params: Any, data_shape: Sequence[int] | None) -> tuple[StaticAffineQuantParams, torch.Size]:
    from fastforward_amd.quantized_tensor import QuantizedTensor

    if isinstance(weight_or_params, QuantizedTensor):
        params = weight_or_params.quantization_context.quantization_params
        data_shape = weight_or_params.shape
    else:
        params = weight_or_params
    if not isinstance(params, StaticAffineQuantParams):
        raise TypeError(f"LPBQ takes a statically quantized weight or its StaticAffineQuantParams, got {type(weight_or_params).__name__}")
    if data_shape is None:
        raise TypeError("LPBQ needs the weight's shape: pass the QuantizedTensor, or data_shape with the parameters")
    return params, torch.Size(data_shape)


def _symmetric(offset: Any) -> bool:
    """No offset, or one that rounds to zero everywhere (read on the host)."""
    if offset is None:
        return True
    return not bool(torch.round(torch.as_tensor(offset).detach().float()).any())


def _suitable(name: str, params: StaticAffineQuantParams, data_shape: torch.Size, compressed_bw: int) -> tuple[granularities.PerBlock, int]:
    """``_lpbq_granularity_and_block_size`` (_lpbq.py:48-74): the PerBlock granularity the tile amounts to and its block size, or the
    reference's ValueError."""
    refusal = ValueError(f"Parameters for {name} not suitable for LPBQ")
    try:
        tile = params.granularity.tile_size(data_shape)
    except ValueError:
        raise refusal from None
    granularity = granularities.granularity_from_sizes(data_shape, data_shape if isinstance(tile, str) else tile)
    suitable = (
        isinstance(granularity, granularities.PerBlock)
        and len(granularity.block_dims) == 1
        and len(granularity.per_channel_dims) == 1
        and (granularity.block_dims, granularity.per_channel_dims) in (ROWS, COLUMNS)
        and len(data_shape) == 2
        and params.num_bits == compressed_bw
        and _symmetric(params.offset)
    )
    if not suitable:
        raise refusal
    return granularity, int(granularity.block_sizes[0])


def encode(weight_or_params: Any, compressed_bw: int = 4, decompressed_bw: int = 8, *, name: str = "weight",
           data_shape: Sequence[int] | None = None) -> LPBQEncoding:
    """The LPBQ encoding of a block-quantized weight (a QuantizedTensor, or its StaticAffineQuantParams with `data_shape`): the
    reference's bit-width rules and suitability checks with its ValueError texts (`name` appears in them), then the compression."""
    check_bitwidths(compressed_bw, decompressed_bw)
    params, shape = _static_params(weight_or_params, data_shape)
    granularity, block_size = _suitable(name, params, shape, compressed_bw)
    scale = torch.as_tensor(params.scale).detach()
    if (granularity.block_dims, granularity.per_channel_dims) == ROWS:
        int_scale, channel_scale = compress_scales(scale.reshape(shape[0], shape[1] // block_size), 1, compressed_bw)
    else:
        int_scale, channel_scale = compress_scales(scale.reshape(shape[0] // block_size, shape[1]), 0, compressed_bw)
    return LPBQEncoding(int_scale, channel_scale, block_size, compressed_bw, decompressed_bw)


def int8_weight(codes8: torch.Tensor, channel_scale: torch.Tensor, dequantize_dtype: torch.dtype | None, decompressed_bw: int = 8) -> Any:
    """The QuantizedTensor around decompressed codes: int8, ``PerChannel(0)``, `decompressed_bw` bits, no offset."""
    from fastforward_amd.quantized_tensor import QuantizedTensor

    params = StaticAffineQuantParams(scale=channel_scale, offset=None, num_bits=decompressed_bw, granularity=granularities.PerChannel(0),
                                     quantized_dtype=torch.int8, dequantize_dtype=dequantize_dtype)
    return QuantizedTensor(codes8, QuantizationContext(AffineQuantizationFunction, params))


def expand_host(codes: torch.Tensor, int_scale: torch.Tensor, block_size: int) -> torch.Tensor:
    """``codes * int_scale`` as int8 in torch (any device): the composition the expand kernel equals."""
    return (codes.to(torch.int32) * int_scale.to(torch.int32).repeat_interleave(block_size, dim=1)).to(torch.int8)


def _int8_codes(raw: torch.Tensor) -> torch.Tensor:
    """Codes as int8: float and wider containers hold the same integers."""
    return raw if raw.dtype == torch.int8 else raw.to(torch.int8)


def decompress(qweight: Any, decompressed_bw: int = 8) -> Any:
    """A symmetric ``PerBlock(1, G, 0)`` weight QuantizedTensor of at most 4 bits as the int8 ``PerChannel(0)`` tensor whose codes are
    ``code * int_scale`` and whose scale is ``channel_scale``; the dequantize dtype is the input's. On the HIP device the compression
    and ``ops.lpbq_expand`` (two launches), elsewhere their torch composition."""
    params, shape = _static_params(qweight, None)
    bits = params.num_bits
    if bits != int(bits) or not 1 <= bits <= 4 or 2 * bits > decompressed_bw or decompressed_bw != 8:
        raise ValueError(f"LPBQ decompresses weights of at most 4 bits into 8, got {bits} into {decompressed_bw}")
    bits = int(bits)
    granularity, block_size = _suitable("weight", params, shape, bits)
    if (granularity.block_dims, granularity.per_channel_dims) != ROWS:
        raise ValueError("LPBQ decompresses weights with blocks along the input channels: PerBlock(1, G, 0)")
    raw = qweight.raw_data
    scale_2d = torch.as_tensor(params.scale, device=raw.device).detach().reshape(shape[0], shape[1] // block_size)
    int_scale, channel_scale = compress_scales(scale_2d, 1, bits)
    codes = _int8_codes(raw)
    on_kernel = raw.is_cuda and int_scale.dtype == torch.uint8 and int_scale.shape[1] <= ops.lpbq.MAX_BLOCKS_PER_ROW and raw.numel() > 0
    codes8 = ops.lpbq_expand(codes, int_scale, block_size) if on_kernel else expand_host(codes, int_scale, block_size)
    return int8_weight(codes8, channel_scale, params.dequantize_dtype, decompressed_bw)


def _convertible(quantizer: Any, weight_shape: Any) -> int | None:
    """The block size when `quantizer` is one ``convert_model`` replaces, else None."""
    from fastforward_amd.nn.linear_quantizer import LinearQuantizer

    if type(quantizer) is not LinearQuantizer or quantizer.has_uninitialized_params or not quantizer.symmetric:
        return None
    bits, granularity = quantizer.num_bits, quantizer.granularity
    if bits != int(bits) or not 1 <= bits <= 4:
        return None
    if not isinstance(granularity, granularities.PerBlock) or (granularity.block_dims, granularity.per_channel_dims) != ROWS:
        return None
    block_size = int(granularity.block_sizes[0])
    if weight_shape is None or len(weight_shape) != 2 or weight_shape[1] % block_size:
        return None
    if quantizer.scale.numel() != weight_shape[0] * (weight_shape[1] // block_size):
        return None
    if not _symmetric(quantizer.offset):  # (a one-sided quantizer holds -int_min here)
        return None
    return block_size


def convert_model(model: torch.nn.Module) -> list[str]:
    """Replace every initialised weight quantizer of `model` that is a plain symmetric ``LinearQuantizer`` of at most 4 bits with
    ``PerBlock((1,), (G,), (0,))`` on a 2-D weight and an absent or all-zero offset (read once, on the host, here) by an
    ``LPBQLinearQuantizer`` that shares the same ``scale`` parameter object. Returns the names it replaced; everything else stays."""
    from fastforward_amd.nn.lpbq_quantizer import LPBQLinearQuantizer

    replaced: list[str] = []
    for prefix, parent in list(model.named_modules()):
        for child_name, child in list(parent.named_children()):
            metadata = getattr(child, "quant_metadata", None)
            weight = getattr(parent, "weight", None)
            shape = getattr(metadata, "shape", None) if metadata is not None else None
            if shape is None and isinstance(weight, torch.Tensor) and child_name == "weight_quantizer":
                shape = weight.shape
            block_size = _convertible(child, shape)
            if block_size is None:
                continue
            new = LPBQLinearQuantizer(int(child.num_bits), block_size, param_dtype=child.scale.dtype, device=child.scale.device)
            new.scale = child.scale  # the same Parameter object: range setting through either name moves both
            new.quantized_dtype = child.quantized_dtype
            new.quant_metadata = metadata
            new.train(child.training)
            setattr(parent, child_name, new)
            replaced.append(f"{prefix}.{child_name}" if prefix else child_name)
    return replaced
