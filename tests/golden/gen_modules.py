"""Generate g19_modules.pt: the REFERENCE's QuantizedLayerNorm / QuantizedEmbedding / QuantizedRelu / QuantizedSilu on the CPU.

Run where the reference is importable, with the same two-line `optree` shim as gen_golden.py:

    PYTHONPATH=/root/reference/src:/tmp/ffshim python tests/golden/gen_modules.py

Each case holds the module's inputs, every quantizer's (num_bits, symmetric, granularity, scale, offset), the value the module
returns with its output quantizer left a stub, and the codes + dequantized value it returns with the output quantizer installed.
fp32 and bf16 activations. Nothing of the reference travels: inputs, parameters and the reference's outputs only.
"""

from __future__ import annotations

import pathlib

import torch

HERE = pathlib.Path(__file__).resolve().parent

try:
    import fastforward as ff
except ImportError as e:  # pragma: no cover
    raise SystemExit(f"the reference is not importable ({e}); see the module docstring")


def quantizer(spec, device="cpu"):
    bits, symmetric, gran, lo, hi = spec
    granularity = ff.PerTensor() if gran == "tensor" else ff.PerChannel(gran[1])
    q = ff.nn.LinearQuantizer(bits, symmetric=symmetric, granularity=granularity, quantized_dtype=torch.int8, device=device)
    q.quantization_range = (torch.as_tensor(lo, dtype=torch.float32), torch.as_tensor(hi, dtype=torch.float32))
    return q


def params(q):
    return dict(scale=q.scale.detach().clone(), offset=None if q.offset is None else q.offset.detach().clone())


def run(module, slots, x):
    """(value with the output quantizer a stub, output codes, output dequantized) of the converted `module`."""
    ff.quantize_model(module)
    for name, spec in slots.items():
        setattr(module, name, quantizer(spec))
    out_q = module.output_quantizer
    module.output_quantizer = ff.nn.QuantizerStub(output_quantizer=True)
    with torch.no_grad(), ff.strict_quantization(False):
        value = module(x)
        module.output_quantizer = out_q
        quantized = module(x)
    got = {name: params(getattr(module, name)) for name in slots}
    return value.detach().clone(), quantized.raw_data.detach().clone(), quantized.dequantize().detach().clone(), got


def main() -> None:
    gen = torch.Generator().manual_seed(19)
    cases = []
    out_spec = (8, False, "tensor", -3.0, 4.0)
    for dtype in (torch.float32, torch.bfloat16):
        # LayerNorm over 32 columns, affine, quantized input, weight and bias
        x = (torch.randn(6, 32, generator=gen) * 2 + 0.5).to(dtype)
        x[1, 3] = 0.0
        mod = torch.nn.LayerNorm(32, eps=1e-5).to(dtype)
        with torch.no_grad():
            mod.weight.copy_(torch.rand(32, generator=gen) + 0.5)
            mod.bias.copy_(torch.randn(32, generator=gen) * 0.1)
        weight, bias = mod.weight.detach().clone(), mod.bias.detach().clone()
        slots = {"input_quantizer": (8, False, "tensor", -4.0, 5.0), "weight_quantizer": (8, True, "tensor", -1.5, 1.5),
                 "bias_quantizer": (8, True, "tensor", -0.4, 0.4), "output_quantizer": out_spec}
        value, codes, deq, got = run(mod, slots, x)
        cases.append(dict(op="layer_norm", dtype=str(dtype), x=x, weight=weight, bias=bias, eps=1e-5, normalized_shape=[32], slots=slots,
                          params=got, value=value, codes=codes, dequantized=deq))
        # Embedding [16, 24], per-row table parameters, ids [3, 5]
        table = (torch.randn(16, 24, generator=gen)).to(dtype)
        ids = torch.randint(0, 16, (3, 5), generator=gen)
        mod = torch.nn.Embedding(16, 24).to(dtype)
        with torch.no_grad():
            mod.weight.copy_(table)
        lo = table.float().amin(1)
        hi = table.float().amax(1)
        slots = {"weight_quantizer": (8, True, ("channel", 0), lo, hi), "output_quantizer": out_spec}
        value, codes, deq, got = run(mod, slots, ids)
        cases.append(dict(op="embedding", dtype=str(dtype), ids=ids, weight=table, slots=slots, params=got, value=value, codes=codes, dequantized=deq))
        # ReLU / SiLU on [4, 40] with a quantized input
        for op, cls in (("relu", torch.nn.ReLU), ("silu", torch.nn.SiLU)):
            x = (torch.randn(4, 40, generator=gen) * 3).to(dtype)
            slots = {"input_quantizer": (8, False, "tensor", -6.0, 7.0), "output_quantizer": out_spec}
            value, codes, deq, got = run(cls(), slots, x)
            cases.append(dict(op=op, dtype=str(dtype), x=x, slots=slots, params=got, value=value, codes=codes, dequantized=deq))
    torch.save(cases, HERE / "g19_modules.pt")
    print(f"wrote {len(cases)} cases to {HERE / 'g19_modules.pt'}")


if __name__ == "__main__":
    main()
