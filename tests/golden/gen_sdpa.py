"""Generate g22_sdpa.pt: the REFERENCE's ff.nn.functional.scaled_dot_product_attention on the CPU.

Run where the reference is importable, with the same two-line `optree` shim as gen_golden.py:

    PYTHONPATH=<reference>/src:<shim> python tests/golden/gen_sdpa.py

Each case holds q / k / v (plain, or the float values a per-tensor quantizer turns into codes), the mask, the keyword arguments,
the (num_bits, scale, offset) of every active quantizer and the value the reference returns. The last case is one
estimate_ranges(running_minmax) pass with the scale / offset every quantizer ended with. Inputs, parameters and outputs only.
"""

from __future__ import annotations

import pathlib

import torch

HERE = pathlib.Path(__file__).resolve().parent

try:
    import fastforward as ff
except ImportError as e:  # pragma: no cover
    raise SystemExit(f"the reference is not importable ({e}); see the module docstring")

NAMES = ("attn_scores_quantizer", "attn_mask_quantizer", "masked_scores_quantizer", "attn_weights_quantizer", "scaled_query_quantizer",
         "scaled_key_quantizer", "dropout_quantizer", "output_quantizer")


def quantizer(bits, scale, offset, container=None):
    q = ff.nn.LinearQuantizer(bits, symmetric=False, granularity=ff.PerTensor(), quantized_dtype=container)
    q.quantization_range = (torch.tensor(-1.0), torch.tensor(1.0))
    with torch.no_grad():
        q.scale.fill_(scale)
        q.offset.fill_(offset)
    return q


ALL8 = {"attn_scores_quantizer": (8, 2.0**-3, 0.0), "attn_mask_quantizer": (8, 2.0**-2, 0.0), "masked_scores_quantizer": (8, 0.07, 3.0),
        "attn_weights_quantizer": (8, 1 / 255, 128.0), "scaled_query_quantizer": (8, 0.013, -2.0), "scaled_key_quantizer": (8, 0.011, 1.0),
        "dropout_quantizer": (8, 2.0**-8, 128.0), "output_quantizer": (8, 0.01, 0.0)}
SETS = {
    "none": {},
    "qk": {k: ALL8[k] for k in ("scaled_query_quantizer", "scaled_key_quantizer")},
    "weights": {"attn_weights_quantizer": ALL8["attn_weights_quantizer"]},
    "all8": ALL8,
    "weights4": {"attn_weights_quantizer": (4, 1 / 15, 8.0)},
}


def main() -> None:
    gen = torch.Generator().manual_seed(22)
    F = ff.nn.functional
    cases = {}

    def case(name, dtype, B, H, HKV, L, S, E, qset, mask=None, quantized_qkv=False, **kwargs):
        q = torch.randn(B, H, L, E, generator=gen).to(dtype)
        k = torch.randn(B, HKV, S, E, generator=gen).to(dtype)
        v = torch.randn(B, HKV, S, E, generator=gen).to(dtype)
        spec = SETS[qset]
        quantizers = {n: quantizer(*spec[n]) for n in spec}
        operands = (q, k, v)
        if quantized_qkv:
            operands = tuple(quantizer(8, 2.0**-5, 0.0, container=torch.int8)(t) for t in operands)
        with torch.no_grad():
            out = F.scaled_dot_product_attention(*operands, attn_mask=mask, **kwargs, **quantizers)
        cases[name] = dict(q=q, k=k, v=v, mask=mask, kwargs=kwargs, quantizers=spec, quantized_qkv=quantized_qkv, out=out)

    nf = dict(strict_quantization=False)
    for dtype in (torch.float32, torch.bfloat16):
        tag = str(dtype).split(".")[-1]
        for qset in SETS:
            case(f"{tag}_self_{qset}", dtype, 2, 2, 2, 9, 9, 16, qset, **nf)
            case(f"{tag}_cross_causal_{qset}", dtype, 1, 2, 2, 7, 12, 16, qset, is_causal=True, **nf)
        case(f"{tag}_cross_causal_tall", dtype, 1, 2, 2, 12, 7, 16, "all8", is_causal=True, **nf)
        boolmask = torch.rand(7, 11, generator=gen) > 0.4
        boolmask[3] = False
        case(f"{tag}_bool_masked_row", dtype, 1, 2, 2, 7, 11, 16, "weights", mask=boolmask, **nf)
        case(f"{tag}_bool_all8", dtype, 1, 2, 2, 7, 11, 16, "all8", mask=boolmask, **nf)
        case(f"{tag}_float_mask_scale", dtype, 2, 2, 2, 5, 8, 16, "qk", mask=torch.randn(2, 1, 5, 8, generator=gen).to(dtype), scale=0.1, **nf)
        case(f"{tag}_gqa", dtype, 1, 4, 2, 6, 6, 16, "all8", enable_gqa=True, is_causal=True, **nf)
        case(f"{tag}_finite_neg_inf", dtype, 1, 2, 2, 7, 11, 16, "all8", mask=boolmask, neg_inf=-20.0, **nf)
        case(f"{tag}_finite_neg_inf_plain", dtype, 1, 2, 2, 7, 11, 16, "none", mask=boolmask, neg_inf=-1e4, **nf)
    case("strict_quantized_qkv", torch.float32, 1, 2, 2, 5, 6, 16, "all8", quantized_qkv=True, strict_quantization=True)

    # calibration: one estimate_ranges(running_minmax) pass (a finite neg_inf: min/max of an infinite bias is an error); the ranges every quantizer ended with
    q, k, v = (torch.randn(1, 2, 6, 16, generator=gen) for _ in range(3))
    qs = {n: ff.nn.LinearQuantizer(8, symmetric=False, granularity=ff.PerTensor()) for n in NAMES}
    with torch.no_grad(), ff.estimate_ranges(torch.nn.ModuleList(qs.values()), ff.range_setting.running_minmax):
        out = F.scaled_dot_product_attention(q, k, v, is_causal=True, neg_inf=-100.0, strict_quantization=False, **qs)
    ranges = {n: (qs[n].scale.detach().clone(), qs[n].offset.detach().clone()) for n in NAMES}
    cases["calibration"] = dict(q=q, k=k, v=v, out=out, ranges=ranges)
    torch.save(cases, HERE / "g22_sdpa.pt")
    print(f"wrote {len(cases)} cases to {HERE / 'g22_sdpa.pt'}")


if __name__ == "__main__":
    main()
