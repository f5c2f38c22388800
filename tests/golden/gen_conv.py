"""Generate g20_conv.pt: the REFERENCE's QuantizedConv2d / QuantizedConv1d on the CPU.

Run where the reference is importable, with the same two-line `optree` shim as gen_golden.py:

    PYTHONPATH=/root/reference/src:/tmp/ffshim python tests/golden/gen_conv.py

Each case holds the module's constructor arguments, its input, weight and bias, every quantizer's (num_bits, symmetric,
granularity, min, max) with the resulting scale / offset, the value the module returns with its output quantizer left a stub,
and the codes + dequantized value it returns with the output quantizer installed (its range: the stub value's min / max).
Per-channel symmetric weights, per-tensor asymmetric activations; fp32 and bf16. One module has padding_mode='reflect', which
the reference's forward does not consult. Nothing of the reference travels: inputs, parameters and its outputs only.
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


# (kind, C, OC, spatial input shape, kernel_size, stride, padding, dilation, bias: None / "plain" / "quantized", padding_mode)
CASES = [
    ("conv2d", 5, 6, (7, 9), 3, 1, 1, 1, "quantized", "zeros"),
    ("conv2d", 4, 5, (11, 10), 3, 2, 0, 2, None, "zeros"),
    ("conv2d", 8, 7, (5, 6), 1, 1, 0, 1, "plain", "zeros"),
    ("conv2d", 4, 3, (6, 7), 3, 1, "same", 1, "plain", "zeros"),
    ("conv2d", 3, 4, (6, 5), 3, 1, 1, 1, "plain", "reflect"),
    ("conv1d", 6, 5, (13,), 3, 1, 1, 1, "quantized", "zeros"),
    ("conv1d", 6, 4, (13,), 3, 2, 0, 1, "plain", "zeros"),
]


def main() -> None:
    gen = torch.Generator().manual_seed(20)
    cases = []
    for dtype in (torch.float32, torch.bfloat16):
        for kind, C, OC, spatial, k, stride, padding, dilation, bias_kind, padding_mode in CASES:
            cls = torch.nn.Conv2d if kind == "conv2d" else torch.nn.Conv1d
            module = cls(C, OC, k, stride=stride, padding=padding, dilation=dilation, bias=bias_kind is not None, padding_mode=padding_mode)
            module = module.to(dtype)
            x = (torch.randn(2, C, *spatial, generator=gen) * 1.5 + 0.4).to(dtype)
            with torch.no_grad():
                module.weight.copy_(torch.randn(module.weight.shape, generator=gen) * 0.3)
                if module.bias is not None:
                    module.bias.copy_(torch.randn(OC, generator=gen) * 0.2)
            weight = module.weight.detach().clone()
            bias = None if module.bias is None else module.bias.detach().clone()
            w_flat = weight.float().reshape(OC, -1)
            slots = {"input_quantizer": (8, False, "tensor", float(x.float().min()), float(x.float().max())),
                     "weight_quantizer": (8, True, ("channel", 0), w_flat.amin(1), w_flat.amax(1))}
            if bias_kind == "quantized":
                slots["bias_quantizer"] = (8, True, "tensor", -0.5, 0.5)
            ff.quantize_model(module)
            for name, spec in slots.items():
                setattr(module, name, quantizer(spec))
            with torch.no_grad(), ff.strict_quantization(False):
                value = module(x)
                slots["output_quantizer"] = (8, False, "tensor", float(value.float().min()), float(value.float().max()))
                module.output_quantizer = quantizer(slots["output_quantizer"])
                quantized = module(x)
            got = {name: params(getattr(module, name)) for name in slots}
            cases.append(dict(kind=kind, dtype=str(dtype), in_channels=C, out_channels=OC, kernel_size=k, stride=stride, padding=padding,
                              dilation=dilation, padding_mode=padding_mode, x=x, weight=weight, bias=bias, slots=slots, params=got,
                              value=value.detach().clone(), codes=quantized.raw_data.detach().clone(),
                              dequantized=quantized.dequantize().detach().clone()))
    torch.save(cases, HERE / "g20_conv.pt")
    print(f"wrote {len(cases)} cases to {HERE / 'g20_conv.pt'}")


if __name__ == "__main__":
    main()
