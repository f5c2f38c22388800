"""Generate g23_math.pt: the REFERENCE's ff.nn.functional.{rms_norm, pow, exp, sin, cos, sum, cumsum} on the CPU.

Run where the reference is importable, with the same two-line `optree` shim as gen_golden.py:

    PYTHONPATH=/root/reference/src:/tmp/ffshim python tests/golden/gen_math.py

Each case holds the operator's float operands, the (num_bits, symmetric, granularity, lo, hi) of every quantizer with the scale /
offset it derived, the keyword arguments, the value the operator returns without an output quantizer, and the codes + dequantized
value it returns with the output quantizer. The input is plain or quantized (per tensor or per row); rms_norm runs with and without
a (quantized) weight and with eps=None; pow at 2, 3, 0.5, -1 and 1.7; sum / cumsum over the first, a middle and the last dim, and
sum over the whole tensor. fp32 and bf16 activations. Nothing of the reference travels: inputs, parameters and the reference's
outputs only.
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
    return (8, symmetric, ("channel", tuple(range(x.dim() - 1))), t.amin(1).clamp(max=-0.25), t.amax(1).clamp(min=0.25))


def main() -> None:
    gen = torch.Generator().manual_seed(23)
    cases = []
    F = ff.nn.functional

    def case(name, op, inputs, slots, kwargs, out):
        """inputs: {"input": tensor, "weight": tensor}; slots: {operand: quantizer spec} for the quantized operands."""
        quantizers = {k: quantizer(v) for k, v in slots.items()}
        args = {k: quantizers[k](v) if k in quantizers else v for k, v in inputs.items()}
        fn = getattr(F, op)
        with torch.no_grad(), ff.strict_quantization(False):
            value = fn(**args, **kwargs)
            oq = quantizer(out)
            quantized = fn(**args, **kwargs, output_quantizer=oq)
        cases.append(dict(name=name, op=op, dtype=str(inputs["input"].dtype), inputs=inputs, slots=slots, out_slot=out,
                          params={k: params(q) for k, q in quantizers.items()}, out_params=params(oq), kwargs=kwargs,
                          value=value.detach().clone(), codes=quantized.raw_data.detach().clone(),
                          dequantized=quantized.dequantize().detach().clone()))

    for dtype in (torch.float32, torch.bfloat16):
        tag = "bf16" if dtype == torch.bfloat16 else "fp32"
        a = (torch.randn(6, 32, generator=gen) * 2).to(dtype)
        pos = (torch.rand(6, 32, generator=gen) * 3 + 0.1).to(dtype)
        w = (torch.randn(32, generator=gen) * 0.5 + 1).to(dtype)
        a3 = (torch.randn(3, 4, 16, generator=gen)).to(dtype)
        qa, qw, qp = (8, False, "tensor", -4.0, 5.0), (8, True, "tensor", -2.0, 2.0), (8, False, "tensor", 0.0, 3.2)
        norm_out = (8, False, "tensor", -3.0, 3.0)
        case(f"rms_norm q eps=None {tag}", "rms_norm", dict(input=a), dict(input=qa), dict(normalized_shape=(32,)), norm_out)
        case(f"rms_norm per-row q, q weight, eps=1e-6 {tag}", "rms_norm", dict(input=a, weight=w), dict(input=row_spec(a), weight=qw),
             dict(normalized_shape=(32,), eps=1e-6), norm_out)
        case(f"rms_norm plain, plain weight, eps=None {tag}", "rms_norm", dict(input=a, weight=w), {}, dict(normalized_shape=(32,)), norm_out)
        case(f"rms_norm q, q weight, eps=None {tag}", "rms_norm", dict(input=a, weight=w), dict(input=qa, weight=qw),
             dict(normalized_shape=[32], eps=None), norm_out)
        for e in (2, 3, 0.5, -1, 1.7):
            x, slot = (a, qa) if e in (2, 3) else (pos, qp)
            case(f"pow {e} q {tag}", "pow", dict(input=x), dict(input=slot), dict(exponent=e), (8, False, "tensor", -4.0, 10.0))
        case(f"pow 2 per-row q {tag}", "pow", dict(input=a), dict(input=row_spec(a)), dict(exponent=2.0), (8, False, "tensor", 0.0, 16.0))
        for op, out in (("exp", (8, False, "tensor", 0.0, 8.0)), ("sin", (8, True, "tensor", -1.0, 1.0)), ("cos", (8, True, "tensor", -1.0, 1.0))):
            case(f"{op} q {tag}", op, dict(input=a), dict(input=qa), {}, out)
            if op == "exp":
                case(f"{op} per-row q {tag}", op, dict(input=a), dict(input=row_spec(a)), {}, out)
                case(f"{op} plain {tag}", op, dict(input=a), {}, {}, out)
        sum_out = (8, False, "tensor", -12.0, 12.0)
        for dim in (0, 1, -1):
            case(f"sum dim={dim} q {tag}", "sum", dict(input=a3), dict(input=(8, False, "tensor", -3.0, 3.0)), dict(dim=dim), sum_out)
            case(f"cumsum dim={dim} q {tag}", "cumsum", dict(input=a3), dict(input=(8, False, "tensor", -3.0, 3.0)), dict(dim=dim), sum_out)
        case(f"sum dim=1 per-row q {tag}", "sum", dict(input=a3), dict(input=row_spec(a3)), dict(dim=1), sum_out)
        case(f"cumsum dim=-1 per-row q {tag}", "cumsum", dict(input=a3), dict(input=row_spec(a3)), dict(dim=-1), sum_out)
        case(f"sum dim=None q {tag}", "sum", dict(input=a3), dict(input=(8, False, "tensor", -3.0, 3.0)), {}, (8, False, "tensor", -40.0, 40.0))
        case(f"sum dim=None plain {tag}", "sum", dict(input=a3), {}, dict(dim=None), (8, False, "tensor", -40.0, 40.0))
    torch.save(cases, HERE / "g23_math.pt")
    print(f"wrote {len(cases)} cases to {HERE / 'g23_math.pt'}")


if __name__ == "__main__":
    main()
