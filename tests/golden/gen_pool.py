"""Generate g24_pool.pt: the REFERENCE's ff.nn.functional.{avg_pool1d, avg_pool2d, max_pool2d, interpolate} on the CPU.

Run where the reference is importable, with the same two-line `optree` shim as gen_golden.py:

    PYTHONPATH=/root/reference/src:/tmp/ffshim python tests/golden/gen_pool.py

Each case holds the operator's float input, the (num_bits, symmetric, granularity, lo, hi) of every quantizer with the scale /
offset it derived, the keyword arguments, the value the operator returns without an output quantizer, and the codes + dequantized
value it returns with the output quantizer. The input is plain or quantized (per tensor or per channel). avg_pool2d runs k2 s2,
k3 s2 p1 with count_include_pad both ways, ceil_mode on an odd map, a non-square kernel and a global 7x7; avg_pool1d k4 s4 and
k3 s1 p1; max_pool2d k3 s2 p1, stride=None, dilation 2, ceil_mode and an input with NaN and +-inf; interpolate nearest x2, x1.5,
size=(13, 9), nearest-exact and a 3-D input. fp32 and bf16 activations. Nothing of the reference travels: inputs, parameters and the
reference's outputs only.
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


def channel_spec(x):
    t = x.float().transpose(0, 1).reshape(x.shape[1], -1)
    t = torch.nan_to_num(t, nan=0.0, posinf=4.0, neginf=-4.0)
    return (8, False, ("channel", 1), t.amin(1).clamp(max=-0.25), t.amax(1).clamp(min=0.25))


def main() -> None:
    gen = torch.Generator().manual_seed(24)
    cases = []
    F = ff.nn.functional
    per_tensor = (8, False, "tensor", -4.0, 5.0)
    out = (8, False, "tensor", -3.0, 3.5)

    def case(name, op, x, slot, kwargs):
        """slot: None for a plain input, else the input quantizer's spec."""
        slots = {} if slot is None else dict(input=slot)
        quantizers = {k: quantizer(v) for k, v in slots.items()}
        fn = getattr(F, op)
        with torch.no_grad(), ff.strict_quantization(False):
            arg = quantizers["input"](x) if quantizers else x
            value = fn(arg, **kwargs)
            oq = quantizer(out)
            quantized = fn(arg, **kwargs, output_quantizer=oq)
        cases.append(dict(name=name, op=op, dtype=str(x.dtype), inputs=dict(input=x), slots=slots, out_slot=out,
                          params={k: params(q) for k, q in quantizers.items()}, out_params=params(oq), kwargs=kwargs,
                          value=value.detach().clone(), codes=quantized.raw_data.detach().clone(),
                          dequantized=quantized.dequantize().detach().clone()))

    for dtype in (torch.float32, torch.bfloat16):
        tag = "bf16" if dtype == torch.bfloat16 else "fp32"
        a = (torch.randn(2, 3, 8, 6, generator=gen) * 2).to(dtype)      # an even map
        odd = (torch.randn(2, 3, 7, 9, generator=gen) * 2).to(dtype)    # an odd one
        head = (torch.randn(2, 3, 7, 7, generator=gen) * 2).to(dtype)
        row = (torch.randn(2, 3, 12, generator=gen) * 2).to(dtype)
        special = (torch.randn(2, 3, 9, 9, generator=gen) * 2).to(dtype)
        special[0, 0, 0, 0], special[0, 1, 4, 4], special[1, 2, 8, 8], special[1, 0, 3, 5] = float("nan"), float("inf"), float("-inf"), -0.0
        special[1, 1] = float("-inf")
        forms = (("plain", lambda x: None), ("q", lambda x: per_tensor), ("per-channel q", channel_spec))
        pools = [
            ("avg_pool2d k2 s2", "avg_pool2d", a, dict(kernel_size=2, stride=2)),
            ("avg_pool2d k3 s2 p1", "avg_pool2d", a, dict(kernel_size=3, stride=2, padding=1)),
            ("avg_pool2d k3 s2 p1 count_include_pad=False", "avg_pool2d", a, dict(kernel_size=3, stride=2, padding=1, count_include_pad=False)),
            ("avg_pool2d ceil_mode odd", "avg_pool2d", odd, dict(kernel_size=2, stride=2, ceil_mode=True)),
            ("avg_pool2d k(3, 2) s(2, 1) p(1, 0)", "avg_pool2d", odd, dict(kernel_size=(3, 2), stride=(2, 1), padding=(1, 0))),
            ("avg_pool2d global 7x7", "avg_pool2d", head, dict(kernel_size=7, stride=7)),
            ("avg_pool1d k4 s4", "avg_pool1d", row, dict(kernel_size=4, stride=4)),
            ("avg_pool1d k3 s1 p1", "avg_pool1d", row, dict(kernel_size=3, stride=1, padding=1)),
            ("max_pool2d k3 s2 p1", "max_pool2d", a, dict(kernel_size=3, stride=2, padding=1)),
            ("max_pool2d stride=None", "max_pool2d", a, dict(kernel_size=2)),
            ("max_pool2d dilation 2", "max_pool2d", odd, dict(kernel_size=3, stride=1, padding=1, dilation=2)),
            ("max_pool2d ceil_mode", "max_pool2d", odd, dict(kernel_size=3, stride=2, ceil_mode=True)),
            ("interpolate nearest x2", "interpolate", a, dict(scale_factor=2)),
            ("interpolate nearest x1.5", "interpolate", odd, dict(scale_factor=1.5)),
            ("interpolate size=(13, 9)", "interpolate", a, dict(size=(13, 9))),
            ("interpolate nearest-exact", "interpolate", odd, dict(scale_factor=(1.7, 0.6), mode="nearest-exact")),
            ("interpolate 3-D", "interpolate", row, dict(scale_factor=2.5)),
        ]
        for name, op, x, kwargs in pools:
            for form, slot in forms:
                case(f"{name} {form} {tag}", op, x, slot(x), kwargs)
        case(f"max_pool2d NaN inf plain {tag}", "max_pool2d", special, None, dict(kernel_size=3, stride=2, padding=1))
    torch.save(cases, HERE / "g24_pool.pt")
    print(f"wrote {len(cases)} cases to {HERE / 'g24_pool.pt'}")


if __name__ == "__main__":
    main()
