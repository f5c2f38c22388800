"""Generate g29_index.pt: the REFERENCE's ff.nn.functional.{index_add, permute} and its code-level expand / unsqueeze /
take_along_dim / topk on the CPU.

Run where the reference is importable, with the same two-line `optree` shim as gen_golden.py:

    PYTHONPATH=<reference>/src:<shim> python tests/golden/gen_index.py

Each case holds the operator's float inputs, the (num_bits, symmetric, granularity, lo, hi) of every input quantizer (None: a
plain input) with the scale / offset it derived, the keyword arguments, and what the reference returns without an output
quantizer and with one: for a float result its value, for a quantized one its type name, codes, dequantized value and the scale /
offset of its context.
index_add runs over dim 0 / 1 / -1 with an index of different values (a part of a permutation) and one with repeats (one row named
five times, rows that are not named), alpha 1 / 0.5 / -2, on quantized and plain operands. permute runs on 2- to 5-D inputs, plain,
per tensor and per channel (axis 0, 1 and the last). The code-level operators run on per-tensor tensors; topk's input has different
codes within every row, so its indices do not depend on how ties are broken. fp32 and bf16. Nothing of the reference travels:
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


def record(result):
    """What a test compares of one result of the reference."""
    if isinstance(result, ff.quantized_tensor.QuantizedTensor):
        p = result.quant_args()
        return dict(type="QuantizedTensor", codes=result.raw_data.detach().clone(), dequantized=result.dequantize().detach().clone(),
                    scale=torch.as_tensor(p.scale).detach().clone(), offset=None if p.offset is None else torch.as_tensor(p.offset).detach().clone())
    return dict(type="Tensor", value=result.detach().clone())


def channel_spec(x, axis):
    t = x.float().movedim(axis, 0).reshape(x.shape[axis], -1)
    return (8, False, ("channel", axis), t.amin(1).clamp(max=-0.25), t.amax(1).clamp(min=0.25))


A, B = (8, False, "tensor", -4.0, 5.0), (6, True, "tensor", -3.0, 3.0)
OUT = (8, False, "tensor", -6.0, 7.0)


def main() -> None:
    gen = torch.Generator().manual_seed(29)
    cases = []
    F = ff.nn.functional

    def case(name, op, inputs, slots, kwargs, index=None):
        quantizers = [None if s is None else quantizer(s) for s in slots]
        with torch.no_grad(), ff.strict_quantization(False):
            args = [x if q is None else q(x) for x, q in zip(inputs, quantizers)]
            if op == "index_add":
                call = lambda **k: F.index_add(args[0], kwargs["dim"], index, args[1], alpha=kwargs["alpha"], **k)  # noqa: E731
            else:
                call = lambda **k: F.permute(args[0], kwargs["dims"], **k)  # noqa: E731
            plain = record(call())
            oq = quantizer(OUT)
            quantized = record(call(output_quantizer=oq))
        cases.append(dict(name=name, op=op, dtype=str(inputs[0].dtype), inputs=list(inputs), index=index, slots=list(slots), out_slot=OUT,
                          params=[None if q is None else params(q) for q in quantizers], out_params=params(oq), kwargs=kwargs,
                          plain=plain, quantized=quantized))

    code_level = []

    def code_case(name, x, method, args, kwargs=None, through_torch=False):
        """`method` of the quantized `x` (or ``torch.<method>(q, ...)``) with plain arguments, which travel with the case."""
        q = quantizer(A)
        kwargs = kwargs or {}
        with torch.no_grad(), ff.strict_quantization(False):
            qx = q(x)
            result = getattr(torch, method)(qx, *args, **kwargs) if through_torch else getattr(qx, method)(*args, **kwargs)
        entry = dict(name=name, dtype=str(x.dtype), x=x, slot=A, params=params(q), method=method, args=args, kwargs=kwargs, through_torch=through_torch)
        if isinstance(result, torch.return_types.topk):
            entry.update(result=record(result.values), indices=result.indices.clone())
        else:
            entry.update(result=record(result), indices=None)
        code_level.append(entry)

    for dtype in (torch.float32, torch.bfloat16):
        tag = "bf16" if dtype == torch.bfloat16 else "fp32"

        def rand(*shape):
            return (torch.randn(*shape, generator=gen) * 2).to(dtype)

        # ---- index_add ----
        shape = (5, 6, 8)
        for dim in (0, 1, -1):
            rows = shape[dim]
            unique = torch.randperm(rows, generator=gen)[: rows - 2]
            repeated = torch.tensor([1, 0, 1, rows - 1, 1, 1, 0, rows - 1, 1])  # row 1 five times; rows 2 .. rows - 2 not at all
            for kind, index in (("unique", unique), ("repeated", repeated)):
                x = rand(*shape)
                source_shape = list(shape)
                source_shape[dim] = index.numel()
                source = rand(*source_shape)
                for slots, alpha in (([A, B], 1), ([A, B], 0.5), ([None, B], -2), ([A, None], 0.5), ([None, None], 1)):
                    forms = " ".join("plain" if s is None else "q" for s in slots)
                    case(f"index_add dim {dim} {kind} alpha {alpha} {forms} {tag}", "index_add", [x, source], slots, dict(dim=dim, alpha=alpha), index=index)
        # ---- permute ----
        for shape, dims in (((3, 5), (1, 0)), ((2, 5, 7), (2, 1, 0)), ((2, 3, 5, 7), (0, 2, 3, 1)), ((2, 5, 7, 3), (0, 3, 1, 2)),
                            ((2, 3, 4, 9), (0, 2, 1, 3)), ((2, 3, 2, 4, 5), (0, 2, 3, 4, 1))):
            x = rand(*shape)
            forms = [("plain", None), ("q", A), ("per-channel 0 q", channel_spec(x, 0)), ("per-channel 1 q", channel_spec(x, 1)),
                     ("per-channel last q", channel_spec(x, len(shape) - 1))]
            for form, slot in forms:
                case(f"permute {shape} -> {dims} {form} {tag}", "permute", [x], [slot], dict(dims=dims))
        # ---- expand / unsqueeze / take_along_dim / topk on the codes ----
        x = rand(4, 6)
        code_case(f"expand {tag}", rand(1, 4, 6), "expand", (3, 4, 6))
        code_case(f"expand -1 {tag}", rand(4, 1), "expand", (-1, 5))
        code_case(f"unsqueeze 1 {tag}", x, "unsqueeze", (1,))
        code_case(f"unsqueeze -1 {tag}", x, "unsqueeze", (-1,))
        picks = torch.randint(0, 6, (4, 3), generator=gen)
        code_case(f"take_along_dim dim 1 {tag}", x, "take_along_dim", (picks, 1))
        code_case(f"torch.take_along_dim dim 0 {tag}", x, "take_along_dim", (picks[:, :1].expand(4, 6) % 4,), dict(dim=0), through_torch=True)
        steps = torch.stack([torch.randperm(16, generator=gen) for _ in range(5)])  # different codes in a row: 0.25 apart, scale 9 / 255
        ranked = (steps.float() * 0.25 - 2.0).to(dtype)
        code_case(f"topk 3 {tag}", ranked, "topk", (3,))
        code_case(f"torch.topk 2 dim 0 smallest {tag}", ranked.t().contiguous(), "topk", (2,), dict(dim=0, largest=False), through_torch=True)
    torch.save(dict(cases=cases, code_level=code_level), HERE / "g29_index.pt")
    print(f"wrote {len(cases)} + {len(code_level)} cases to {HERE / 'g29_index.pt'}")


if __name__ == "__main__":
    main()
