"""Generate g21_elementwise.pt: the REFERENCE's ff.nn.functional.{add, sub, mul, div, softmax, sigmoid, gelu} on the CPU.

Run where the reference is importable, with the same two-line `optree` shim as gen_golden.py:

    PYTHONPATH=/root/reference/src:/tmp/ffshim python tests/golden/gen_elementwise.py

Each case holds the operator's float operands, the (num_bits, symmetric, granularity, lo, hi) of every quantizer with the scale /
offset it derived, the keyword arguments, the value the operator returns without an output quantizer (dequantized where that is
the rescale below), and the codes + dequantized value it returns with the output quantizer. Operands are plain or quantized (per tensor or per row), `other` is a tensor of the
same shape, a suffix of it, or a Python number. The last case is mul of a per-tensor quantized tensor by a number without an output
quantizer: the reference's rescale (codes unchanged, scale * other). fp32 and bf16 activations. Nothing of the reference travels:
inputs, parameters and the reference's outputs only.
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


def row_spec(x, symmetric=False):
    t = x.float().reshape(-1, x.shape[-1])
    return (8, symmetric, ("channel", 0), t.amin(1).clamp(max=-0.25), t.amax(1).clamp(min=0.25))


def main() -> None:
    gen = torch.Generator().manual_seed(21)
    cases = []
    out_spec = (8, False, "tensor", -3.0, 4.0)
    F = ff.nn.functional

    def case(name, op, inputs, slots, kwargs, out=out_spec):
        """inputs: {"input": tensor, "other": tensor or number}; slots: {operand: quantizer spec} for the quantized operands."""
        quantizers = {k: quantizer(v) for k, v in slots.items()}
        args = {k: quantizers[k](v) if k in quantizers else v for k, v in inputs.items()}
        fn = getattr(F, op)
        with torch.no_grad(), ff.strict_quantization(False):
            value = fn(**args, **kwargs)
            oq = quantizer(out)
            quantized = fn(**args, **kwargs, output_quantizer=oq)
        rescaled = isinstance(value, ff.QuantizedTensor)  # mul of a per-tensor quantized tensor by a number: the rescale
        value = value.dequantize() if rescaled else value
        cases.append(dict(name=name, op=op, dtype=str(inputs["input"].dtype), inputs=inputs, slots=slots, out_slot=out,
                          params={k: params(q) for k, q in quantizers.items()}, out_params=params(oq), kwargs=kwargs,
                          value=value.detach().clone(), value_rescaled=rescaled, codes=quantized.raw_data.detach().clone(),
                          dequantized=quantized.dequantize().detach().clone()))

    for dtype in (torch.float32, torch.bfloat16):
        tag = "bf16" if dtype == torch.bfloat16 else "fp32"
        a = (torch.randn(6, 32, generator=gen) * 2).to(dtype)
        b = (torch.randn(6, 32, generator=gen) * 1.5 + 0.25).to(dtype)
        b_nz = torch.where(b.abs() < 0.1, torch.full_like(b, 0.5), b)
        a3 = (torch.randn(3, 4, 16, generator=gen)).to(dtype)
        bias = (torch.randn(16, generator=gen) * 0.3).to(dtype)
        mat = (torch.randn(4, 16, generator=gen)).to(dtype)
        qa, qb = (8, False, "tensor", -4.0, 5.0), (8, True, "tensor", -2.5, 2.5)
        case(f"add q+q {tag}", "add", dict(input=a, other=b), dict(input=qa, other=qb), {})
        case(f"add q+q alpha=2 per-row other {tag}", "add", dict(input=a, other=b), dict(input=qa, other=row_spec(b)), dict(alpha=2))
        case(f"sub q-plain alpha=-0.5 {tag}", "sub", dict(input=a, other=b), dict(input=qa), dict(alpha=-0.5))
        case(f"sub per-row q - scalar {tag}", "sub", dict(input=a, other=0.75), dict(input=row_spec(a)), {})
        case(f"add plain + scalar alpha=3 {tag}", "add", dict(input=a, other=1.25), {}, dict(alpha=3))
        case(f"mul q*q {tag}", "mul", dict(input=a, other=b), dict(input=qa, other=qb), {})
        case(f"mul q*scalar with output quantizer {tag}", "mul", dict(input=a, other=-1.5), dict(input=qa), {})
        case(f"div q/q {tag}", "div", dict(input=a, other=b_nz), dict(input=qa, other=(8, False, "tensor", -3.0, 2.0)), {})
        case(f"div q/scalar {tag}", "div", dict(input=a, other=3.0), dict(input=qa), {})
        case(f"add suffix bias [16] {tag}", "add", dict(input=a3, other=bias), dict(input=(8, False, "tensor", -3.0, 3.0), other=(8, True, "tensor", -1.0, 1.0)), {})
        case(f"add suffix [4, 16] plain {tag}", "add", dict(input=a3, other=mat), dict(input=(8, False, "tensor", -3.0, 3.0)), {})
        case(f"softmax q {tag}", "softmax", dict(input=a), dict(input=qa), dict(dim=-1), out=(8, False, "tensor", 0.0, 1.0))
        case(f"softmax per-row q {tag}", "softmax", dict(input=a), dict(input=row_spec(a)), dict(dim=1), out=(8, False, "tensor", 0.0, 1.0))
        case(f"sigmoid q {tag}", "sigmoid", dict(input=a), dict(input=qa), {}, out=(8, False, "tensor", 0.0, 1.0))
        case(f"sigmoid per-row q {tag}", "sigmoid", dict(input=a), dict(input=row_spec(a)), {}, out=(8, False, "tensor", 0.0, 1.0))
        case(f"gelu q {tag}", "gelu", dict(input=a), dict(input=qa), {})
        case(f"gelu tanh q {tag}", "gelu", dict(input=a), dict(input=qa), dict(approximate="tanh"))
        case(f"gelu tanh plain {tag}", "gelu", dict(input=a), {}, dict(approximate="tanh"))
        # mul of a per-tensor quantized tensor by a number, no output quantizer: the reference's rescale of the scale
        q = quantizer(qa)
        with torch.no_grad():
            scaled = F.mul(q(a), 2.5, strict_quantization=False)
        cases.append(dict(name=f"scalar multiply {tag}", op="scalar_multiply", dtype=str(dtype), inputs=dict(input=a, other=2.5),
                          slots=dict(input=qa), params=dict(input=params(q)), codes=scaled.raw_data.detach().clone(),
                          scale=scaled.quant_args().scale.detach().clone(), dequantized=scaled.dequantize().detach().clone()))
    torch.save(cases, HERE / "g21_elementwise.pt")
    print(f"wrote {len(cases)} cases to {HERE / 'g21_elementwise.pt'}")


if __name__ == "__main__":
    main()
