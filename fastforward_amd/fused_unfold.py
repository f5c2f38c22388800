"""The sliding-window operator — ``unfold`` — registered in this package's dispatcher.

The reference registers no kernel for it: ff.nn.functional runs the generated fallback (src/fastforward/_gen/fallback.py: unfold
:1650) — A2 of the quantized input, ATen's ``im2col`` into a tensor ``KH * KW`` times larger, the output quantizer over that
tensor. The predicate below accepts what the one-pass kernel of csrc/ffq_unfold.hip covers and returns False for everything else,
so the reference chain (the fallback in :mod:`fastforward_amd.nn.functional`) runs unchanged there. It follows the rules of
``IndexKernels`` (fused_index.py):

* calls of ``ff.nn.functional`` only: a call without the ``strict_quantization`` keyword (``torch.nn.functional.unfold`` through
  ``QuantizedTensor.__torch_function__``) is declined;
* a 4-D ``[B, C, H, W]`` or unbatched 3-D ``[C, H, W]`` input on the HIP device, and a device library that exports
  ``ffq_unfold_quantize`` (a library without the symbol — the C oracle — declines);
* bf16 / fp16 values: a plain tensor WITH an output quantizer (without one the chain is ATen's im2col alone), or static-affine codes
  (int8 or value-dtype container, <= 8 bits, fp32 parameters) per tensor or per channel (``PerChannel(1)``; ``PerChannel(0)`` on an
  unbatched input), with or without an output quantizer;
* ``kernel_size`` / ``dilation`` / ``padding`` / ``stride`` each an int or a pair of ints (no bool, float or string) inside the entry
  point's limits (at most 2^24 per axis), with a dilated window that fits the padded image: geometry ATen refuses is declined, so
  the fallback raises ATen's own error;
* a non-empty input, and fewer than 2^31 elements in both the input and the result;
* any layout: a strided, channels-last or misaligned view reaches the kernel as an aligned copy (``ops._base._dense``); the result
  is contiguous, as ATen's;
* no operand that needs a gradient while grad mode is on (the launch has no autograd formula);
* under strict quantization, only calls the fallback would accept (an output quantizer, a quantized input).

The output quantizer runs inside the launch under the int8 GEMM's ``_requant`` rules (fused_modules.py); otherwise the launch
writes the value and the quantizer is called on it, so range estimation still sees the value. Nothing reads device memory on the
host, so the call can be captured in a ``torch.cuda.graph``.
"""

from __future__ import annotations

from typing import Any

from fastforward_amd import _native, ops
from fastforward_amd.dispatcher import Predicate, register
from fastforward_amd.fused_linear import KERNELS as _LINEAR
from fastforward_amd.fused_math import MathKernels
from fastforward_amd.fused_modules import _needs_grad, _on_device
from fastforward_amd.ops.unfold import output_extents, pair

_LIMIT = 2**31


class UnfoldKernels(MathKernels):
    """Predicate and kernel of ``unfold`` (an ``ElementwiseKernels`` through ``MathKernels``, whose ``_call_ok`` holds the rule for
    the ``strict_quantization`` keyword)."""

    def _per_channel(self, x: Any) -> bool | None:
        """False for per-tensor parameters (or a plain tensor), True for one pair per channel, None for any other tiling."""
        if not isinstance(x, self._k.surface.quantized_tensor):
            return False
        tile, full = self._k._tile(x), tuple(x.shape)
        if tile == full:
            return False
        channel = x.dim() - 3
        return True if tile == (*full[:channel], 1, *full[channel + 1:]) else None

    def supported_unfold(self, input: Any = None, kernel_size: Any = None, dilation: Any = 1, padding: Any = 0, stride: Any = 1, *_args: Any,
                         output_quantizer: Any = None, **kwargs: Any) -> bool:
        if _args or not self._call_ok(kwargs, output_quantizer, input):
            return False
        dt = self._value_dtype(input)
        if dt is None or input.dim() not in (3, 4) or input.numel() == 0 or input.numel() >= _LIMIT:
            return False
        quantized = isinstance(input, self._k.surface.quantized_tensor)
        if not quantized and output_quantizer is None:
            return False
        if self._per_channel(input) is None:
            return False
        geometry = [pair(v) for v in (kernel_size, dilation, padding, stride)]
        if None in geometry:
            return False
        kernel = geometry[0]
        C, H, W = input.shape[-3:]
        extents = output_extents(H, W, *geometry)
        if extents is None or (input.numel() // (H * W)) * kernel[0] * kernel[1] * extents[0] * extents[1] >= _LIMIT:
            return False
        if not _on_device(input) or getattr(_native.library(), "ffq_unfold_quantize", None) is None:
            return False
        return not _needs_grad(input)

    def unfold(self, input: Any, kernel_size: Any, dilation: Any = 1, padding: Any = 0, stride: Any = 1, *, output_quantizer: Any = None,
               strict_quantization: bool | None = None) -> Any:
        dt = self._value_dtype(input)
        x, dequant = self._dequant(input)
        fused = self._output(output_quantizer, dt)
        value, codes = ops.unfold_quantize(x, kernel_size, dilation, padding, stride, dtype=dt, dequant=dequant,
                                           per_channel=bool(self._per_channel(input)), **self._launch_args(fused))
        return self._finish(value, codes, fused, output_quantizer, dt)


KERNELS = UnfoldKernels(_LINEAR)
unfold_predicate = Predicate(KERNELS.supported_unfold)
_registrations = {"unfold": register("unfold", unfold_predicate, KERNELS.unfold)}
