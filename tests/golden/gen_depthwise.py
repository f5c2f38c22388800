"""Generate g28_depthwise.pt: the REFERENCE's functional conv2d / conv1d with ``groups == C`` on the CPU.

Run where the reference is importable, with the same two-line `optree` shim as gen_golden.py:

    PYTHONPATH=<reference>/src:<shim> python tests/golden/gen_depthwise.py

The file holds ``{"conv": [...]}``. A case calls ``ff.nn.functional.conv2d`` (or ``conv1d``: ``dims == 1``) on operands the
reference's own LinearQuantizers produced and holds the operator's arguments, the input, weight and bias, every quantizer's
(num_bits, symmetric, granularity, min, max) with the resulting scale / offset, the value the operator returns without an output
quantizer, and the codes + dequantized value it returns with one (its range: that value's min / max). Eleven geometries in fp32 and
bf16: 3x3 s1 p1 (MobileNet), 3x3 s2 p1 on an odd image, 5x5 p2, 7x7 p3 (ConvNeXt), 3x3 under dilation 2 with ``'same'``, 1x1, channel
multipliers 2 and 3, the 1-D k31 p15 (Conformer) and k4 p3 (Mamba), and a (1, 5) kernel; C in {3, 5, 8}. Per-tensor asymmetric
activations; weights per tensor or PerChannel(0), symmetric or asymmetric; the bias absent, plain or quantized. Nothing of the
reference travels: inputs, parameters and its outputs only.
"""

from __future__ import annotations

import pathlib

import torch

HERE = pathlib.Path(__file__).resolve().parent

try:
    import fastforward as ff
except ImportError as e:  # pragma: no cover
    raise SystemExit(f"the reference is not importable ({e}); see the module docstring")


def quantizer(spec):
    bits, symmetric, gran, lo, hi = spec
    granularity = ff.PerTensor() if gran == "tensor" else ff.PerChannel(gran[1])
    q = ff.nn.LinearQuantizer(bits, symmetric=symmetric, granularity=granularity, quantized_dtype=torch.int8)
    q.quantization_range = (torch.as_tensor(lo, dtype=torch.float32), torch.as_tensor(hi, dtype=torch.float32))
    return q


def params(q):
    return dict(scale=q.scale.detach().clone(), offset=None if q.offset is None else q.offset.detach().clone())


# (dims, C, M, spatial, kernel, stride, padding, dilation, bias: None / "plain" / "quantized",
#  weight quantizer: "tensor" / "tensor-asym" / "channel" / "channel-asym")
CASES = [
    (2, 8, 1, (14, 14), (3, 3), 1, 1, 1, "plain", "channel"),                     # MobileNet 3x3
    (2, 5, 1, (15, 13), (3, 3), 2, 1, 1, "quantized", "channel-asym"),            # stride 2 on an odd image
    (2, 3, 1, (12, 12), (5, 5), (1, 1), (2, 2), (1, 1), None, "tensor"),          # EfficientNet 5x5
    (2, 8, 1, (14, 14), (7, 7), 1, 3, 1, "plain", "channel-asym"),                # ConvNeXt 7x7
    (2, 5, 1, (11, 12), (3, 3), 1, "same", 2, None, "channel"),                   # 'same' under dilation 2
    (2, 8, 1, (9, 10), (1, 1), 1, 0, 1, "quantized", "tensor-asym"),              # 1x1
    (2, 3, 2, (10, 11), (3, 3), 1, 1, 1, "plain", "channel"),                     # channel multiplier 2
    (2, 5, 3, (9, 9), (3, 3), (2, 1), (1, 0), 1, "quantized", "channel-asym"),    # channel multiplier 3
    (1, 8, 1, (70,), (31,), 1, 15, 1, "plain", "channel"),                        # Conformer k31
    (1, 5, 1, (40,), (4,), 1, 3, 1, "plain", "tensor"),                           # Mamba's causal conv1d (the caller drops the tail)
    (2, 3, 1, (8, 17), (1, 5), (1, 2), (0, 2), 1, None, "tensor-asym"),           # a (1, 5) kernel
]


def cases(gen):
    out = []
    for dtype in (torch.float32, torch.bfloat16):
        for dims, C, M, spatial, k, stride, padding, dilation, bias_kind, w_kind in CASES:
            OC = C * M
            x = (torch.rand(2, C, *spatial, generator=gen) * 3 + 0.25).to(dtype) if bias_kind == "plain" else \
                (torch.randn(2, C, *spatial, generator=gen) * 1.5 + 0.3).to(dtype)
            weight = (torch.randn(OC, 1, *k, generator=gen) * 0.3).to(dtype)
            bias = None if bias_kind is None else (torch.randn(OC, generator=gen) * 0.2).to(dtype)
            w_flat = weight.float().reshape(OC, -1)
            if w_kind == "tensor":
                w_spec = (8, True, "tensor", float(weight.float().min()), float(weight.float().max()))
            elif w_kind == "tensor-asym":
                w_spec = (8, False, "tensor", float(weight.float().min()) * 1.3, float(weight.float().max()) * 0.7)
            elif w_kind == "channel":
                w_spec = (8, True, ("channel", 0), w_flat.amin(1).clamp(max=-0.01), w_flat.amax(1).clamp(min=0.01))
            else:
                w_spec = (8, False, ("channel", 0), w_flat.amin(1).clamp(max=-0.01) * 1.3, w_flat.amax(1).clamp(min=0.01) * 0.7)
            slots = {"input_quantizer": (8, False, "tensor", float(x.float().min()), float(x.float().max())), "weight_quantizer": w_spec}
            if bias_kind == "quantized":
                slots["bias_quantizer"] = (8, True, "tensor", -0.5, 0.5)
            quantizers = {name: quantizer(spec) for name, spec in slots.items()}
            op = ff.nn.functional.conv1d if dims == 1 else ff.nn.functional.conv2d
            with torch.no_grad(), ff.strict_quantization(False):
                xq = quantizers["input_quantizer"](x)
                wq = quantizers["weight_quantizer"](weight)
                bq = quantizers["bias_quantizer"](bias) if bias_kind == "quantized" else bias
                value = op(xq, wq, bq, stride, padding, dilation, C)
                slots["output_quantizer"] = (8, False, "tensor", float(value.float().min()), float(value.float().max()))
                quantizers["output_quantizer"] = quantizer(slots["output_quantizer"])
                quantized = op(xq, wq, bq, stride, padding, dilation, C, output_quantizer=quantizers["output_quantizer"])
            got = {name: params(q) for name, q in quantizers.items()}
            out.append(dict(dims=dims, groups=C, multiplier=M, dtype=str(dtype), stride=stride, padding=padding, dilation=dilation, x=x,
                            weight=weight, bias=bias, bias_kind=bias_kind, w_kind=w_kind, slots=slots, params=got,
                            value=value.detach().clone(), codes=quantized.raw_data.detach().clone(),
                            dequantized=quantized.dequantize().detach().clone()))
    return out


def main() -> None:
    gen = torch.Generator().manual_seed(28)
    data = dict(conv=cases(gen))
    torch.save(data, HERE / "g28_depthwise.pt")
    print(f"wrote {len(data['conv'])} cases to {HERE / 'g28_depthwise.pt'}")


if __name__ == "__main__":
    main()
