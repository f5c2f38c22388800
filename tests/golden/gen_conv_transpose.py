"""Generate g26_conv_transpose.pt: the REFERENCE's functional conv_transpose1d / conv_transpose2d on the CPU.

Run where the reference is importable, with the same two-line `optree` shim as gen_golden.py:

    PYTHONPATH=/root/reference/src:/tmp/ffshim python tests/golden/gen_conv_transpose.py

The reference has no module for these operators, so each case calls ``ff.nn.functional.conv_transpose{1,2}d`` on operands its own
LinearQuantizers produced. A case holds the operator's arguments, the input, weight and bias, every quantizer's (num_bits,
symmetric, granularity, min, max) with the resulting scale / offset, the value the operator returns without an output quantizer,
and the codes + dequantized value it returns with one (its range: that value's min / max). Per-tensor asymmetric activations;
weights per tensor or PerChannel(1) (per output channel of the [C, OC, *kernel] layout), symmetric or asymmetric; the bias absent,
plain or quantized; fp32 and bf16. Nothing of the reference travels: inputs, parameters and its outputs only.
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


# (kind, C, OC, spatial input shape, kernel, stride, padding, output_padding, dilation, bias: None / "plain" / "quantized",
#  weight quantizer: "tensor" / "channel" / "channel-asym")
CASES = [
    ("conv_transpose2d", 5, 6, (5, 6), (2, 2), (2, 2), (0, 0), (0, 0), (1, 1), "quantized", "channel"),       # U-Net up-convolution
    ("conv_transpose2d", 4, 5, (6, 5), (4, 4), (2, 2), (1, 1), (0, 0), (1, 1), "plain", "channel-asym"),      # DCGAN k4 s2 p1
    ("conv_transpose2d", 3, 4, (5, 4), (3, 3), (2, 2), (1, 1), (1, 1), (1, 1), None, "channel"),              # output_padding
    ("conv_transpose2d", 4, 3, (4, 5), (3, 2), (1, 1), (0, 1), (0, 0), (2, 3), "plain", "tensor"),            # dilation > 1, stride 1
    ("conv_transpose2d", 3, 5, (4, 4), (3, 3), (2, 4), (1, 0), (1, 2), (2, 2), "quantized", "channel-asym"),  # gcd(stride, dilation) > 1
    ("conv_transpose2d", 6, 4, (4, 3), (2, 2), (3, 3), (0, 0), (0, 0), (1, 1), "plain", "channel"),           # stride > kernel extent
    ("conv_transpose2d", 4, 4, (3, 4), (2, 3), (2, 3), (1, 2), (1, 2), (2, 3), None, "tensor"),               # stride (2,3) dilation (2,3)
    ("conv_transpose1d", 6, 5, (9,), (16,), (8,), (4,), (0,), (1,), "plain", "channel"),                      # vocoder k16 s8 p4
    ("conv_transpose1d", 5, 4, (11,), (4,), (4,), (0,), (0,), (1,), "quantized", "channel-asym"),             # k4 s4
    ("conv_transpose1d", 4, 6, (10,), (3,), (2,), (1,), (1,), (2,), None, "channel"),                         # empty phases, 1-D
]


def main() -> None:
    gen = torch.Generator().manual_seed(26)
    cases = []
    for dtype in (torch.float32, torch.bfloat16):
        for kind, C, OC, spatial, k, stride, padding, output_padding, dilation, bias_kind, w_kind in CASES:
            fn = getattr(ff.nn.functional, kind)
            x = (torch.rand(2, C, *spatial, generator=gen) * 3 + 0.25).to(dtype)
            weight = (torch.randn(C, OC, *k, generator=gen) * 0.3).to(dtype)
            bias = None if bias_kind is None else (torch.randn(OC, generator=gen) * 0.2).to(dtype)
            w_flat = weight.float().transpose(0, 1).reshape(OC, -1)
            if w_kind == "tensor":
                w_spec = (8, True, "tensor", float(weight.float().min()), float(weight.float().max()))
            elif w_kind == "channel":
                w_spec = (8, True, ("channel", 1), w_flat.amin(1), w_flat.amax(1))
            else:
                w_spec = (8, False, ("channel", 1), w_flat.amin(1) * 1.3, w_flat.amax(1) * 0.7)
            slots = {"input_quantizer": (8, False, "tensor", float(x.float().min()), float(x.float().max())), "weight_quantizer": w_spec}
            if bias_kind == "quantized":
                slots["bias_quantizer"] = (8, True, "tensor", -0.5, 0.5)
            quantizers = {name: quantizer(spec) for name, spec in slots.items()}
            with torch.no_grad(), ff.strict_quantization(False):
                xq = quantizers["input_quantizer"](x)
                wq = quantizers["weight_quantizer"](weight)
                bq = quantizers["bias_quantizer"](bias) if bias_kind == "quantized" else bias
                value = fn(xq, wq, bq, stride, padding, output_padding, 1, dilation)
                slots["output_quantizer"] = (8, False, "tensor", float(value.float().min()), float(value.float().max()))
                quantizers["output_quantizer"] = quantizer(slots["output_quantizer"])
                quantized = fn(xq, wq, bq, stride, padding, output_padding, 1, dilation, output_quantizer=quantizers["output_quantizer"])
            got = {name: params(q) for name, q in quantizers.items()}
            cases.append(dict(kind=kind, dtype=str(dtype), stride=stride, padding=padding, output_padding=output_padding, dilation=dilation,
                              x=x, weight=weight, bias=bias, bias_kind=bias_kind, slots=slots, params=got, value=value.detach().clone(),
                              codes=quantized.raw_data.detach().clone(), dequantized=quantized.dequantize().detach().clone()))
    torch.save(cases, HERE / "g26_conv_transpose.pt")
    print(f"wrote {len(cases)} cases to {HERE / 'g26_conv_transpose.pt'}")


if __name__ == "__main__":
    main()
