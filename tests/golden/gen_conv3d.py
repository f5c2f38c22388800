"""Generate g27_conv3d.pt: the REFERENCE's functional conv3d and avg_pool3d on the CPU.

Run where the reference is importable, with the same two-line `optree` shim as gen_golden.py:

    PYTHONPATH=/root/reference/src:/tmp/ffshim python tests/golden/gen_conv3d.py

The file holds ``{"conv": [...], "pool": [...]}``.

A conv case calls ``ff.nn.functional.conv3d`` on operands the reference's own LinearQuantizers produced and holds the operator's
arguments, the input, weight and bias, every quantizer's (num_bits, symmetric, granularity, min, max) with the resulting scale /
offset, the value the operator returns without an output quantizer, and the codes + dequantized value it returns with one (its
range: that value's min / max). The geometries are those of tests/test_conv3d_gpu.py's exact list (kernel, stride, padding,
dilation; the patch embedding with fewer channels so that the file stays small) and four more: k3 p1, ``padding='same'`` under
dilation 2, windows clipped down to a single tap (k3 p2 s2) and a (1, 3, 3) kernel. Per-tensor asymmetric activations; weights per tensor or
PerChannel(0), symmetric or asymmetric; the bias absent, plain or quantized; fp32 and bf16.

A pool case calls ``ff.nn.functional.avg_pool3d`` on a plain, per-tensor or per-channel quantized input and holds the same: six
geometries (k2 s2, k3 s2 p1 with count_include_pad both ways, ceil_mode with a last window that starts in the padding, a
(1, 3, 2) kernel, a mixed kernel with padding on two axes), in fp32 only: ATen's CPU avg_pool3d is not built for bf16 / fp16, so the
reference cannot run them here. Nothing of the reference travels: inputs, parameters and its outputs only.
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


# (C, OC, (D, H, W), kernel, stride, padding, dilation, bias: None / "plain" / "quantized",
#  weight quantizer: "tensor" / "tensor-asym" / "channel" / "channel-asym")
CONV_CASES = [
    (3, 40, (5, 9, 11), (3, 3, 3), (1, 2, 3), (1, 0, 2), (1, 1, 1), "plain", "channel"),
    (20, 130, (4, 6, 7), (2, 1, 3), (1, 1, 1), (0, 0, 0), (2, 1, 2), "quantized", "channel-asym"),
    (16, 32, (4, 5, 6), (3, 3, 3), (1, 1, 1), (0, 0, 0), (1, 1, 1), None, "tensor"),
    (2, 6, (4, 28, 28), (2, 14, 14), (2, 14, 14), (0, 0, 0), (1, 1, 1), "plain", "channel"),          # patch embedding
    (4, 6, (4, 5, 6), (3, 3, 3), 1, 1, 1, "quantized", "tensor-asym"),                                # U-Net k3 p1, int arguments
    (3, 4, (5, 6, 5), (3, 3, 3), 1, "same", 2, None, "channel"),                                      # 'same' under dilation 2
    (3, 5, (3, 4, 4), (3, 3, 3), (2, 2, 2), (2, 2, 2), (1, 1, 1), "plain", "channel-asym"),           # windows clipped to one tap
    (5, 7, (3, 7, 8), (1, 3, 3), (1, 2, 2), (0, 1, 1), (1, 1, 1), "quantized", "channel"),            # (2 + 1)-D
]

# (spatial input shape, keyword arguments)
POOL_CASES = [
    ((6, 8, 6), dict(kernel_size=2, stride=2)),
    ((6, 7, 8), dict(kernel_size=3, stride=2, padding=1)),
    ((6, 7, 8), dict(kernel_size=3, stride=2, padding=1, count_include_pad=False)),
    ((5, 7, 9), dict(kernel_size=2, stride=2, padding=1, ceil_mode=True)),    # the last window would start in the padding
    ((5, 7, 9), dict(kernel_size=(1, 3, 2), stride=(1, 2, 1))),
    ((5, 7, 9), dict(kernel_size=(2, 3, 3), stride=(2, 1, 2), padding=(0, 1, 1), ceil_mode=True, count_include_pad=False)),
]


def channel_spec(x):
    t = x.float().transpose(0, 1).reshape(x.shape[1], -1)
    return (8, False, ("channel", 1), t.amin(1).clamp(max=-0.25), t.amax(1).clamp(min=0.25))


def conv_cases(gen):
    cases = []
    for dtype in (torch.float32, torch.bfloat16):
        for C, OC, spatial, k, stride, padding, dilation, bias_kind, w_kind in CONV_CASES:
            x = (torch.rand(2, C, *spatial, generator=gen) * 3 + 0.25).to(dtype) if bias_kind == "plain" else \
                (torch.randn(2, C, *spatial, generator=gen) * 1.5 + 0.3).to(dtype)
            weight = (torch.randn(OC, C, *k, generator=gen) * 0.3).to(dtype)
            bias = None if bias_kind is None else (torch.randn(OC, generator=gen) * 0.2).to(dtype)
            w_flat = weight.float().reshape(OC, -1)
            if w_kind == "tensor":
                w_spec = (8, True, "tensor", float(weight.float().min()), float(weight.float().max()))
            elif w_kind == "tensor-asym":
                w_spec = (8, False, "tensor", float(weight.float().min()) * 1.3, float(weight.float().max()) * 0.7)
            elif w_kind == "channel":
                w_spec = (8, True, ("channel", 0), w_flat.amin(1), w_flat.amax(1))
            else:
                w_spec = (8, False, ("channel", 0), w_flat.amin(1) * 1.3, w_flat.amax(1) * 0.7)
            slots = {"input_quantizer": (8, False, "tensor", float(x.float().min()), float(x.float().max())), "weight_quantizer": w_spec}
            if bias_kind == "quantized":
                slots["bias_quantizer"] = (8, True, "tensor", -0.5, 0.5)
            quantizers = {name: quantizer(spec) for name, spec in slots.items()}
            with torch.no_grad(), ff.strict_quantization(False):
                xq = quantizers["input_quantizer"](x)
                wq = quantizers["weight_quantizer"](weight)
                bq = quantizers["bias_quantizer"](bias) if bias_kind == "quantized" else bias
                value = ff.nn.functional.conv3d(xq, wq, bq, stride, padding, dilation, 1)
                slots["output_quantizer"] = (8, False, "tensor", float(value.float().min()), float(value.float().max()))
                quantizers["output_quantizer"] = quantizer(slots["output_quantizer"])
                quantized = ff.nn.functional.conv3d(xq, wq, bq, stride, padding, dilation, 1, output_quantizer=quantizers["output_quantizer"])
            got = {name: params(q) for name, q in quantizers.items()}
            cases.append(dict(dtype=str(dtype), stride=stride, padding=padding, dilation=dilation, x=x, weight=weight, bias=bias,
                              bias_kind=bias_kind, w_kind=w_kind, slots=slots, params=got, value=value.detach().clone(),
                              codes=quantized.raw_data.detach().clone(), dequantized=quantized.dequantize().detach().clone()))
    return cases


def pool_cases(gen):
    cases = []
    per_tensor = (8, False, "tensor", -4.0, 5.0)
    out = (8, False, "tensor", -3.0, 3.5)
    forms = (("plain", lambda x: None), ("q", lambda x: per_tensor), ("per-channel q", channel_spec))
    for dtype in (torch.float32,):
        for spatial, kwargs in POOL_CASES:
            x = (torch.randn(2, 3, *spatial, generator=gen) * 2).to(dtype)
            for form, slot_of in forms:
                slot = slot_of(x)
                slots = {} if slot is None else dict(input=slot)
                quantizers = {k: quantizer(v) for k, v in slots.items()}
                with torch.no_grad(), ff.strict_quantization(False):
                    arg = quantizers["input"](x) if quantizers else x
                    value = ff.nn.functional.avg_pool3d(arg, **kwargs)
                    oq = quantizer(out)
                    quantized = ff.nn.functional.avg_pool3d(arg, **kwargs, output_quantizer=oq)
                cases.append(dict(form=form, dtype=str(dtype), x=x, slots=slots, out_slot=out, params={k: params(q) for k, q in quantizers.items()},
                                  out_params=params(oq), kwargs=kwargs, value=value.detach().clone(), codes=quantized.raw_data.detach().clone(),
                                  dequantized=quantized.dequantize().detach().clone()))
    return cases


def main() -> None:
    gen = torch.Generator().manual_seed(27)
    data = dict(conv=conv_cases(gen), pool=pool_cases(gen))
    torch.save(data, HERE / "g27_conv3d.pt")
    print(f"wrote {len(data['conv'])} conv and {len(data['pool'])} pool cases to {HERE / 'g27_conv3d.pt'}")


if __name__ == "__main__":
    main()
