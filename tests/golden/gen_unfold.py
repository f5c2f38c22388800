"""Generate g30_unfold.pt: the REFERENCE's ff.nn.functional.unfold on the CPU.

Run where the reference is importable, with the same two-line `optree` shim as gen_golden.py:

    PYTHONPATH=<reference>/src:<shim> python tests/golden/gen_unfold.py

Each case holds the operator's float input, the (num_bits, symmetric, granularity, lo, hi) of the input quantizer (None: a plain
input) with the scale / offset it derived, the geometry, and what the reference returns without an output quantizer and with one:
for a float result its value, for a quantized one its type name, codes and dequantized value (its context holds the output
quantizer's parameters, which the file holds once).
Eleven geometries — one element, every parameter asymmetric, groups of 8 columns that span two and three output rows, L = 8 and
L = 9, windows wholly in the padding, stride 2 on odd sizes, dilation, window = image, an unbatched input — each on a plain input,
on per-tensor codes (asymmetric 8-bit, symmetric 6-bit) and on per-channel codes (asymmetric 8-bit; ``PerChannel(1)``, or
``PerChannel(0)`` on the unbatched input). fp32 and bf16. Nothing of the reference travels: inputs, parameters and the reference's
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


def record(result):
    """What a test compares of one result of the reference."""
    if isinstance(result, ff.quantized_tensor.QuantizedTensor):
        return dict(type="QuantizedTensor", codes=result.raw_data.detach().clone(), dequantized=result.dequantize().detach().clone())
    return dict(type="Tensor", value=result.detach().clone())


def channel_spec(x, axis):
    t = x.float().movedim(axis, 0).reshape(x.shape[axis], -1)
    return (8, False, ("channel", axis), t.amin(1).clamp(max=-0.25), t.amax(1).clamp(min=0.25))


A, B = (8, False, "tensor", -4.0, 5.0), (6, True, "tensor", -3.0, 3.0)
OUT = (8, False, "tensor", -6.0, 7.0)  # (asymmetric: the codes of the +0.0 in the padding are not code 0)

# (shape, kernel_size, dilation, padding, stride)
GEOMETRIES = [
    ((1, 1, 1, 1), 1, 1, 0, 1),
    ((2, 3, 5, 7), (3, 2), (1, 2), (2, 1), (2, 1)),
    ((1, 2, 6, 6), 3, 1, 0, 1),
    ((1, 2, 10, 5), 3, 1, 0, 1),
    ((2, 1, 3, 10), 3, 1, 0, 1),
    ((1, 1, 3, 11), 3, 1, 0, 1),
    ((1, 3, 4, 4), 1, 1, 2, 1),
    ((1, 2, 7, 9), 3, 1, 1, 2),
    ((1, 2, 5, 5), 3, 2, 2, 1),
    ((1, 2, 4, 6), (4, 6), 1, 0, 1),
    ((3, 5, 6), (2, 3), 1, 0, 1),
]


def main() -> None:
    gen = torch.Generator().manual_seed(30)
    cases = []
    F = ff.nn.functional
    oq = quantizer(OUT)
    out_params = params(oq)

    def case(name, x, slot, kwargs):
        q = None if slot is None else quantizer(slot)
        with torch.no_grad(), ff.strict_quantization(False):
            arg = x if q is None else q(x)
            plain = record(F.unfold(arg, **kwargs))
            quantized = record(F.unfold(arg, **kwargs, output_quantizer=oq))
        cases.append(dict(name=name, dtype=str(x.dtype), input=x, slot=slot, params=None if q is None else params(q), kwargs=kwargs, plain=plain,
                          quantized=quantized))

    for dtype in (torch.float32, torch.bfloat16):
        tag = "bf16" if dtype == torch.bfloat16 else "fp32"
        for shape, kernel, dilation, padding, stride in GEOMETRIES:
            x = (torch.randn(*shape, generator=gen) * 2).to(dtype)
            kwargs = dict(kernel_size=kernel, dilation=dilation, padding=padding, stride=stride)
            channel = len(shape) - 3
            forms = [("plain", None), ("q", A), ("symmetric q", B), ("per-channel q", channel_spec(x, channel))]
            for form, slot in forms:
                case(f"unfold {shape} k{kernel} d{dilation} p{padding} s{stride} {form} {tag}".replace(" ", "_"), x, slot, kwargs)
    torch.save(dict(cases=cases, out_slot=OUT, out_params=out_params), HERE / "g30_unfold.pt")
    print(f"wrote {len(cases)} cases to {HERE / 'g30_unfold.pt'}")


if __name__ == "__main__":
    main()
