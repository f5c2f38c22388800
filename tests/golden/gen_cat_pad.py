"""Generate g25_cat_pad.pt: the REFERENCE's ff.nn.functional.{cat, pad} (and torch.cat on quantized tensors) on the CPU.

Run where the reference is importable, with the same two-line `optree` shim as gen_golden.py:

    PYTHONPATH=/root/reference/src:/tmp/ffshim python tests/golden/gen_cat_pad.py

Each case holds the operator's float inputs, the (num_bits, symmetric, granularity, lo, hi) of every input quantizer (None: a
plain input) with the scale / offset it derived, the keyword arguments, and what the reference returns without an output
quantizer and with one: for a float result its value, for a quantized one its type name, codes, dequantized value and the scale /
offset of its context. Inputs quantized by the SAME quantizer (``share``) carry one parameter object, as a module's outputs do.
cat runs over dim 0 / 1 / -1 with two, three and nine inputs: all quantized with different parameters, mixed plain and quantized,
the same parameters without an output quantizer (the reference keeps codes) and with one, and torch.cat of same-parameter
tensors. pad runs constant mode with the default and a non-zero value, negative pads, 1-, 2- and 3-D pads, reflect and replicate
in each rank ATen takes, on plain / per-tensor / per-channel inputs. fp32 and bf16. Nothing of the reference travels: inputs,
parameters and the reference's outputs only.
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


def channel_spec(x):
    t = x.float().transpose(0, 1).reshape(x.shape[1], -1)
    return (8, False, ("channel", 1), t.amin(1).clamp(max=-0.25), t.amax(1).clamp(min=0.25))


A, B, C = (8, False, "tensor", -4.0, 5.0), (8, False, "tensor", -2.0, 2.5), (6, True, "tensor", -3.0, 3.0)
OUT = (8, False, "tensor", -3.0, 3.5)


def main() -> None:
    gen = torch.Generator().manual_seed(25)
    cases = []
    F = ff.nn.functional

    def case(name, op, inputs, slots, kwargs, share=False, through_torch=False):
        """slots: one quantizer spec (or None for a plain input) per input; share: one quantizer object for all of them."""
        shared = quantizer(slots[0]) if share else None
        quantizers = [shared if share else (None if s is None else quantizer(s)) for s in slots]
        with torch.no_grad(), ff.strict_quantization(False):
            args = [x if q is None else q(x) for x, q in zip(inputs, quantizers)]
            if op == "cat":
                call = (lambda **k: torch.cat(args, **kwargs)) if through_torch else (lambda **k: F.cat(args, **kwargs, **k))
            else:
                call = lambda **k: F.pad(args[0], **kwargs, **k)  # noqa: E731
            plain = record(call())
            oq = quantizer(OUT)
            quantized = None if through_torch else record(call(output_quantizer=oq))
        cases.append(dict(name=name, op=op, dtype=str(inputs[0].dtype), inputs=list(inputs), slots=list(slots), share=share,
                          through_torch=through_torch, out_slot=OUT, params=[None if q is None else params(q) for q in quantizers],
                          out_params=params(oq), kwargs=kwargs, plain=plain, quantized=quantized))

    for dtype in (torch.float32, torch.bfloat16):
        tag = "bf16" if dtype == torch.bfloat16 else "fp32"

        def rand(*shape):
            return (torch.randn(*shape, generator=gen) * 2).to(dtype)

        # ---- cat ----
        for dim, shapes in ((0, [(2, 3, 8), (1, 3, 8), (3, 3, 8)]), (1, [(2, 3, 8), (2, 5, 8), (2, 1, 8)]), (-1, [(2, 3, 8), (2, 3, 5), (2, 3, 3)])):
            xs = [rand(*s) for s in shapes]
            case(f"cat dim {dim} two inputs all quantized {tag}", "cat", xs[:2], [A, B], dict(dim=dim))
            case(f"cat dim {dim} three inputs all quantized {tag}", "cat", xs, [A, B, C], dict(dim=dim))
            case(f"cat dim {dim} three inputs mixed plain and quantized {tag}", "cat", xs, [A, None, C], dict(dim=dim))
            case(f"cat dim {dim} three inputs plain {tag}", "cat", xs, [None, None, None], dict(dim=dim))
            nine = [xs[i % 3] for i in range(9)]
            case(f"cat dim {dim} nine inputs mixed plain and quantized {tag}", "cat", nine, [A, None, C, B, A, None, None, C, B], dict(dim=dim))
            case(f"cat dim {dim} same parameters {tag}", "cat", xs, [A, A, A], dict(dim=dim), share=True)
            case(f"cat dim {dim} same parameters of two quantizers {tag}", "cat", xs[:2], [A, A], dict(dim=dim))
            case(f"torch.cat dim {dim} same parameters {tag}", "cat", xs, [A, A, A], dict(dim=dim), share=True, through_torch=True)
        # ---- pad ----
        x4, x3, x5 = rand(2, 3, 5, 8), rand(2, 3, 7), rand(1, 2, 3, 4, 6)
        forms = (("plain", lambda x: None), ("q", lambda x: A), ("per-channel q", channel_spec))
        pads = [
            ("pad constant default value 1-D", x4, dict(pad=(1, 2), mode="constant")),
            ("pad constant value -1.5 2-D", x4, dict(pad=(1, 2, 3, 0), mode="constant", value=-1.5)),
            ("pad constant value 0.3 3-D", x4, dict(pad=(0, 8, 1, 1, 2, 0), mode="constant", value=0.3)),
            ("pad constant negative pads", x4, dict(pad=(-2, 3, 1, -1), mode="constant", value=2.0)),
            ("pad constant 3-D input", x3, dict(pad=(4, 5), mode="constant", value=1.0)),
            ("pad reflect 1-D on 3-D", x3, dict(pad=(3, 2), mode="reflect")),
            ("pad reflect 2-D on 4-D", x4, dict(pad=(3, 2, 1, 4), mode="reflect")),
            ("pad reflect 3-D on 5-D", x5, dict(pad=(2, 1, 3, 0, 1, 2), mode="reflect")),
            ("pad replicate 1-D on 3-D", x3, dict(pad=(2, 3), mode="replicate")),
            ("pad replicate 2-D on 4-D", x4, dict(pad=(0, 3, 2, 1), mode="replicate")),
            ("pad replicate 3-D on 5-D", x5, dict(pad=(1, 1, 0, 2, 2, 1), mode="replicate")),
        ]
        for name, x, kwargs in pads:
            for form, slot in forms:
                case(f"{name} {form} {tag}", "pad", [x], [slot(x)], kwargs)
        # the ranks without a batch dimension (per-tensor parameters: dim 1 is padded, or there is none)
        for name, x, kwargs in (("pad reflect 1-D on 2-D", x3[0], dict(pad=(2, 2), mode="reflect")), ("pad reflect 2-D on 3-D", x4[0], dict(pad=(1, 2, 2, 1), mode="reflect")),
                                ("pad reflect 3-D on 4-D", x5[0], dict(pad=(1, 1, 1, 1, 1, 1), mode="reflect")),
                                ("pad replicate 1-D on 2-D", x3[0], dict(pad=(1, 3), mode="replicate")), ("pad replicate 2-D on 3-D", x4[0], dict(pad=(2, 0, 1, 1), mode="replicate")),
                                ("pad replicate 3-D on 4-D", x5[0], dict(pad=(0, 1, 2, 0, 1, 1), mode="replicate"))):
            for form, slot in forms[:2]:
                case(f"{name} {form} {tag}", "pad", [x], [slot(x)], kwargs)
    torch.save(cases, HERE / "g25_cat_pad.pt")
    print(f"wrote {len(cases)} cases to {HERE / 'g25_cat_pad.pt'}")


if __name__ == "__main__":
    main()
