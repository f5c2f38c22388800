"""The depthwise convolutions — ``conv1d`` / ``conv2d`` with ``groups == C`` — registered in this package's dispatcher as a second
kernel next to the implicit GEMM of fused_conv.py (whose predicate declines every ``groups != 1``).

The reference registers no kernel for them: the generated fallbacks (src/fastforward/_gen/fallback.py:116-214) run A2 of input and
weight, the float grouped convolution and the output quantizer. The predicate below accepts exactly what the direct int8 stencil of
csrc/ffq_depthwise.hip covers (include/ffq_depthwise.h) and returns False for everything else, so the reference chain runs unchanged
there — general grouped convolutions (``1 < groups < C``) included:

* ``groups == input.shape[1] > 1``, ``weight.shape[1] == 1``, ``weight.shape[0] % groups == 0`` (a channel multiplier M >= 1);
* ``prod(kernel) <= 1024`` (31 x 31 fits): one channel's taps stay on chip;
* every other rule of ``ConvKernels.supported`` (fused_conv.py): static-affine codes of <= 8 bits in an int8 or float container with
  fp32 parameters, the input per tensor and the weight per tensor or per output channel, one data dtype (bf16 / fp16 / fp32) for both,
  a batched input, ``geometry()`` (integer stride / dilation / padding, ``'valid'``, ``'same'`` where it is symmetric), the bias
  forms, everything on the HIP device, no gradient needed, and under strict quantization an output quantizer with quantized operands;
* the device library exports ``ffq_depthwise_conv2d_w8a8`` (a library without the symbol — the C oracle — declines).

Conv1d runs as H = KH = 1. The output quantizer runs inside the launch (``DispatcherKernels._requant``'s rules). Nothing here reads
device memory on the host: the route is capturable in a ``torch.cuda.graph``. ``QuantizedConv1d`` / ``QuantizedConv2d`` pass
``groups`` through, so a converted model's depthwise layers take this route with no class of their own.
"""

from __future__ import annotations

from typing import Any

from fastforward_amd.dispatcher import Predicate, register
from fastforward_amd.fused_conv import ConvKernels, ConvSet, geometry
from fastforward_amd.fused_modules import KERNELS as _MODULES

MAX_TAPS = 1024  # KH * KW (include/ffq_depthwise.h)


def many_groups(groups: Any) -> bool:
    """The groups rule of the stencil: a plain int above 1 (``groups == 1`` is the implicit GEMM's, C = 1 included)."""
    return isinstance(groups, int) and not isinstance(groups, bool) and groups > 1


def one_channel_per_group(groups: Any, x_shape: Any, w_shape: Any, weight: Any) -> bool:
    """... and of the operands: as many groups as input channels, whole channel multipliers, no PerChannel(1) weight."""
    if groups != x_shape[1] or w_shape[0] % groups != 0:
        return False
    # PerChannel(1): one "input channel" per group, so its tile IS the tensor; still not a per-tensor quantizer
    return getattr(_MODULES._k._params(weight).granularity, "channel_dims", (0,)) == (0,)


# the predicates and kernels of the depthwise ``conv1d`` / ``conv2d`` are ``ConvKernels``' own, on this set
KERNELS = ConvKernels(_MODULES, ConvSet(in_axis=1, oc_axis=0, groups_rule=many_groups, grouping_rule=one_channel_per_group, bound=MAX_TAPS, geometry=geometry,
                                        geometry_operands=("stride", "padding", "dilation"), op="depthwise_conv2d_w8a8",
                                        symbol="ffq_depthwise_conv2d_w8a8"))
conv1d_predicate = Predicate(KERNELS.supported_conv1d)
conv2d_predicate = Predicate(KERNELS.supported_conv2d)
_registrations = {
    "conv1d": register("conv1d", conv1d_predicate, KERNELS.conv1d),
    "conv2d": register("conv2d", conv2d_predicate, KERNELS.conv2d),
}
