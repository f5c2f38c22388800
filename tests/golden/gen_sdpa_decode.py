"""Generate g31_sdpa_decode.pt: the REFERENCE's ff.nn.functional.scaled_dot_product_attention on the CPU for a short query over K / V
held as int8 codes (a quantized KV cache).

Run where the reference is importable, with the same two-line `optree` shim as gen_golden.py:

    PYTHONPATH=<reference>/src:<shim> python tests/golden/gen_sdpa_decode.py

Each case holds q, the float k / v that a per-tensor quantizer with an int8 container turns into codes, the (num_bits, scale,
offset) of those quantizers and of the output quantizer (None without one), the mask, the keyword arguments and the value the
reference returns. Inputs, parameters and outputs only.
"""

from __future__ import annotations

import pathlib

import torch

HERE = pathlib.Path(__file__).resolve().parent

try:
    import fastforward as ff
except ImportError as e:  # pragma: no cover
    raise SystemExit(f"the reference is not importable ({e}); see the module docstring")

K_SPEC = (8, 2.0**-5, 3.0)
V_SPEC = (8, 0.031, -7.0)
Q_SPEC = (8, 2.0**-5, 0.0)
OUT_SPEC = (8, 2.0**-6, 2.0)


def quantizer(bits, scale, offset, container=None):
    q = ff.nn.LinearQuantizer(bits, symmetric=False, granularity=ff.PerTensor(), quantized_dtype=container)
    q.quantization_range = (torch.tensor(-1.0), torch.tensor(1.0))
    with torch.no_grad():
        q.scale.fill_(scale)
        q.offset.fill_(offset)
    return q


def main() -> None:
    gen = torch.Generator().manual_seed(31)
    F = ff.nn.functional
    cases = {}

    def case(name, dtype, B, H, HKV, L, S, E, mask=None, out=False, q_codes=None, **kwargs):
        q = torch.randn(B, H, L, E, generator=gen).to(dtype)
        k = torch.randn(B, HKV, S, E, generator=gen).to(dtype)
        v = torch.randn(B, HKV, S, E, generator=gen).to(dtype)
        with torch.no_grad():
            qq = q if q_codes is None else quantizer(*Q_SPEC, container=q_codes)(q)
            kq, vq = quantizer(*K_SPEC, container=torch.int8)(k), quantizer(*V_SPEC, container=torch.int8)(v)
            assert kq.raw_data.dtype == torch.int8 and vq.raw_data.dtype == torch.int8
            extra = dict(output_quantizer=quantizer(*OUT_SPEC)) if out else {}
            got = F.scaled_dot_product_attention(qq, kq, vq, attn_mask=mask, enable_gqa=H != HKV, strict_quantization=False, **kwargs, **extra)
            if isinstance(got, ff.QuantizedTensor):
                got = got.dequantize()
        cases[name] = dict(q=q, k=k, v=v, mask=mask, kwargs=kwargs, k_spec=K_SPEC, v_spec=V_SPEC, q_spec=None if q_codes is None else Q_SPEC,
                           q_container=q_codes, out_spec=OUT_SPEC if out else None, out=got)

    bf, hf = torch.bfloat16, torch.float16
    case("bf16_L1_S1_mha", bf, 2, 2, 2, 1, 1, 64)
    case("bf16_L1_S65_gqa", bf, 2, 4, 2, 1, 65, 64)
    case("bf16_L1_S300_gqa_out", bf, 1, 8, 2, 1, 300, 64, out=True)
    case("bf16_L4_S65_mha_bool", bf, 1, 2, 2, 4, 65, 64, mask=torch.rand(4, 65, generator=gen) > 0.3)
    rowless = torch.rand(1, 1, 4, 300, generator=gen) > 0.3
    rowless[..., 2, :] = False
    case("bf16_L4_S300_gqa_bool_masked_row", bf, 1, 4, 2, 4, 300, 64, mask=rowless)
    case("bf16_L4_S300_gqa_float_out", bf, 1, 4, 2, 4, 300, 64, mask=torch.randn(1, 1, 4, 300, generator=gen).to(bf), out=True, scale=0.2)
    case("fp16_L1_S300_mha_float", hf, 1, 2, 2, 1, 300, 64, mask=torch.randn(1, 300, generator=gen))
    case("fp16_L4_S65_gqa_causal_out", hf, 1, 4, 2, 4, 65, 64, out=True, is_causal=True)
    case("bf16_L1_S65_gqa_q_int8", bf, 1, 4, 2, 1, 65, 64, q_codes=torch.int8)
    torch.save(cases, HERE / "g31_sdpa_decode.pt")
    print(f"wrote {len(cases)} cases to {HERE / 'g31_sdpa_decode.pt'}")


if __name__ == "__main__":
    main()
