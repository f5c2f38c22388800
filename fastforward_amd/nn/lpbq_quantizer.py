"""A weight quantizer that hands the int8 GEMM a W4 block-quantized weight (reference format: src/fastforward/export/_lpbq.py; see
``fastforward_amd.quantization.lpbq``).

``LPBQLinearQuantizer`` is a symmetric ``LinearQuantizer`` with ``PerBlock(1, block_size, 0)`` block scales as its parameters — range
setting and ``estimate_ranges`` work through the inherited setter — whose ``quantize`` returns the DECOMPRESSED tensor: int8 codes
``code4 * int_scale`` with one scale per output channel. On the HIP device that is one ``ffq_lpbq_quantize`` launch; ``functional.linear``
then takes the int8 GEMM instead of the weight-only bf16 one."""

from __future__ import annotations

from typing import Sequence

import torch

from fastforward_amd import flags, ops
from fastforward_amd.exceptions import QuantizationError
from fastforward_amd.nn.linear_quantizer import LinearQuantizer
from fastforward_amd.quantization import granularity as granularities
from fastforward_amd.quantization import lpbq
from fastforward_amd.quantized_tensor import QuantizedTensor

NO_BACKWARD = ("LPBQLinearQuantizer has no backward: the decompressed int8 codes have no gradient formula. Quantize under "
               "torch.no_grad() or detach the weight; train with the LinearQuantizer it was converted from.")


class LPBQLinearQuantizer(LinearQuantizer):
    """``num_bits``-bit symmetric block quantizer (blocks of `block_size` input channels of a 2-D weight, no offset) whose output is
    the LPBQ-decompressed int8 per-channel tensor. With `requantize` the codes round against the compressed scale ``channel_scale *
    int_scale`` that is applied, otherwise against the block scale itself (the export's semantics). ``2 * num_bits <=
    decompressed_bits == 8``."""

    def __init__(self, num_bits: int = 4, block_size: int | None = None, *, decompressed_bits: int = 8, requantize: bool = False,
                 param_dtype: torch.dtype | None = None, device: torch.device | str = "cpu") -> None:
        if isinstance(num_bits, bool) or not isinstance(num_bits, int) or num_bits < 1:
            raise ValueError(f"LPBQLinearQuantizer: num_bits is a positive integer, got {num_bits}")
        if decompressed_bits != 8 or 2 * num_bits > decompressed_bits:
            raise ValueError(f"LPBQLinearQuantizer: 2 * num_bits <= decompressed_bits == 8 is required, got num_bits={num_bits}, decompressed_bits={decompressed_bits}")
        if isinstance(block_size, bool) or not isinstance(block_size, int) or block_size < 1:
            raise ValueError(f"LPBQLinearQuantizer: block_size is a positive integer, got {block_size}")
        super().__init__(num_bits, symmetric=True, allow_one_sided=False, granularity=granularities.PerBlock(1, block_size, 0),
                         param_dtype=param_dtype, device=device)
        self.block_size = block_size
        self.decompressed_bits = decompressed_bits
        self.requantize = bool(requantize)
        self._data_shape: torch.Size | None = None

    def extra_repr(self) -> str:
        return f"{super().extra_repr()}, decompressed_bits={self.decompressed_bits}, requantize={self.requantize}"

    def compressed(self, data: torch.Tensor) -> QuantizedTensor:
        """The ``num_bits``-bit PerBlock tensor a LinearQuantizer with these parameters returns."""
        return LinearQuantizer.quantize(self, data)  # type: ignore[return-value]

    def _block_scales(self, data: torch.Tensor) -> torch.Tensor:
        rows, cols = data.shape
        return self.scale.detach().reshape(rows, cols // self.block_size)

    def quantize(self, data: torch.Tensor) -> torch.Tensor:
        if torch.is_grad_enabled() and data.requires_grad:
            raise QuantizationError(NO_BACKWARD)
        blocks = data.shape[1] // self.block_size if data.dim() == 2 and self.block_size <= data.shape[1] else 0
        if (self.has_uninitialized_params or flags.get_export_mode() or data.dim() != 2 or data.shape[1] % self.block_size
                or self.scale.numel() != data.shape[0] * blocks):
            # the parent's answer: its error for an uninitialised quantizer or a shape the blocks do not fit, its quantize-dequantize
            # under export mode (the codes of the calibrated scale)
            return self.compressed(data)
        self._data_shape = data.shape
        bits, G = self.num_bits, self.block_size
        scales = self._block_scales(data)
        on_kernel = (data.is_cuda and data.dtype in (torch.bfloat16, torch.float16, torch.float32) and scales.dtype == torch.float32
                     and scales.device == data.device and bits in ops.lpbq.BITS and blocks <= ops.lpbq.MAX_BLOCKS_PER_ROW and data.numel() > 0)
        if on_kernel:
            view = data.detach()
            if view.shape[1] > 1 and view.stride(1) != 1 or (view.shape[0] > 1 and view.stride(0) < view.shape[1]):
                view = view.contiguous()
            codes8, channel_scale, _ = ops.lpbq_quantize(view, scales, G, bits, self.requantize, want_int_scale=False)
        else:
            int_scale, channel_scale = lpbq.compress_scales(scales, 1, bits)
            applied = channel_scale[:, None] * int_scale.to(channel_scale.dtype) if self.requantize else scales
            codes4 = ops.quantize_by_tile(data.detach(), applied, (1, G), bits, torch.int8)
            codes8 = lpbq.expand_host(codes4, int_scale, G)
        return lpbq.int8_weight(codes8, channel_scale, data.dtype, self.decompressed_bits)

    def encoding(self, data_shape: Sequence[int] | None = None) -> lpbq.LPBQEncoding:
        """The LPBQ encoding of the current block scales for a weight of `data_shape` (default: the shape in the quantizer's metadata,
        else that of the last tensor quantized)."""
        shape = data_shape
        if shape is None and self.quant_metadata is not None:
            shape = self.quant_metadata.shape
        if shape is None:
            shape = self._data_shape
        if shape is None:
            raise ValueError("LPBQLinearQuantizer.encoding: the weight's shape is unknown: pass data_shape")
        if self.has_uninitialized_params:
            raise ValueError("LPBQLinearQuantizer.encoding: the quantizer is uninitialised: set its quantization_range first")
        return lpbq.encode(self.quantization_parameters(), self.num_bits, self.decompressed_bits, data_shape=shape)
