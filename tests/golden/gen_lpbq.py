"""Generate ``g32_lpbq.pt`` by running the REFERENCE's LPBQ code (``fastforward.export._lpbq``, CPU eager).

Run with the reference's ``src`` directory and the ``optree`` shim of gen_golden.py on PYTHONPATH:

    PYTHONPATH=<reference>/src:<shim> python tests/golden/gen_lpbq.py

``fastforward.export``'s package ``__init__`` pulls in ``gguf`` / ``onnx``, which are not needed here: an empty stand-in module for
``fastforward.export`` (with its ``__path__`` set) goes into ``sys.modules`` first, so that ``fastforward.export._lpbq`` and
``_export_types`` import on their own. Nothing of the reference travels: the fixture holds inputs and the outputs it produced, as
tensors and plain Python values (``torch.load(..., weights_only=True)``).

Contents
    compress   ``grouped_dynamic_quantize`` for J in {1, 2, 5, 64, 65, 112}, bits 2 / 3 / 4, both orientations, fp32 and bf16 scales:
               seeded positive rows, rows of exact ties ``m * (k + 0.5) / 2^bits``, a row with entries below ``d / 2``, a constant row
    encodings  ``generate_lpbq_encoding`` for four weights quantized by the reference's own ``LinearQuantizer(4, symmetric=True,
               allow_one_sided=False, PerBlock(...))`` with ranges from the blocks' min / max: weight, codes, scale, the full dict
    errors     the ValueError texts of every refusal of ``LPBQProcessor.__new__`` and ``_lpbq_granularity_and_block_size``
"""

from __future__ import annotations

import importlib.util
import pathlib
import sys
import types

import torch

HERE = pathlib.Path(__file__).resolve().parent

spec = importlib.util.find_spec("fastforward")
if spec is None or not spec.submodule_search_locations:  # pragma: no cover
    sys.exit("the reference is not importable; see the module docstring")
stand_in = types.ModuleType("fastforward.export")
stand_in.__path__ = [str(pathlib.Path(list(spec.submodule_search_locations)[0]) / "export")]  # type: ignore[attr-defined]
sys.modules["fastforward.export"] = stand_in

import fastforward as ff  # noqa: E402

from fastforward.export._export_types import ProcessedQuantParams  # noqa: E402
from fastforward.export._lpbq import LPBQProcessor  # noqa: E402
from fastforward.quantization.tiled_tensor import tiles_to_rows  # noqa: E402

BLOCK_COUNTS = (1, 2, 5, 64, 65, 112)
BITS = (2, 3, 4)


def scale_rows(J: int, bits: int, gen: torch.Generator) -> torch.Tensor:
    """fp32 [rows, J]: three seeded rows, two rows of exact ties, a row with entries below d / 2, a constant row."""
    top = 2**bits
    seeded = torch.rand(3, J, generator=gen) * 0.1 + 1e-3
    ties = torch.empty(2, J)
    for r, (m, shift) in enumerate(((0.25, 0), (2.0, 1))):   # m a power of two: m * (k + 0.5) / 2^bits and its quotient by d are exact
        k = (torch.arange(J) + shift) % top
        ties[r] = m * (k.float() + 0.5) / top
        ties[r, J - 1] = m
    small = torch.full((1, J), 0.75)
    small[0, : J - 1] = 0.75 * torch.linspace(0.01, 0.49, max(J - 1, 1))[: J - 1] / top
    constant = torch.full((1, J), 0.0371)
    return torch.cat([seeded, ties, small, constant])


def compress_records() -> list[dict]:
    records = []
    gen = torch.Generator().manual_seed(32)
    for J in BLOCK_COUNTS:
        for bits in BITS:
            base = scale_rows(J, bits, gen)
            for dtype in (torch.float32, torch.bfloat16):
                for orientation, grouping in (("rows", [1, -1]), ("columns", [-1, 1])):
                    scales = base.to(dtype) if orientation == "rows" else base.to(dtype).t().contiguous()
                    q, d = LPBQProcessor(bits, 8).grouped_dynamic_quantize(scales, grouping, bits)
                    assert q.shape == scales.shape and d.dtype == dtype and d.numel() == base.shape[0]
                    records.append({"J": J, "bits": bits, "orientation": orientation, "dtype": str(dtype).removeprefix("torch."),
                                    "scales": scales.clone(), "q": q.to(torch.uint8), "d": d.flatten().clone()})
    return records


def check_coverage(records: list[dict]) -> None:
    """From the recorded outputs themselves: every q of 1 .. 16 occurs; a tie went each way; an entry was clamped to 1; every channel
    has an entry equal to 2^bits."""
    seen: set[int] = set()
    up = down = clamped = 0
    for r in records:
        axis = 1 if r["orientation"] == "rows" else 0
        q, top = r["q"].to(torch.int32), 2 ** r["bits"]
        assert bool((q.amax(dim=axis) == top).all()), (r["J"], r["bits"], r["orientation"], r["dtype"])
        assert int(q.min()) >= 1 and int(q.max()) <= top
        if r["bits"] == 4:
            seen |= set(q.flatten().tolist())
        d = r["d"].double().unsqueeze(axis)
        quotient = r["scales"].double() / d
        tie = ((quotient - quotient.floor()) == 0.5) & (quotient > 1)  # (0.5 itself rounds to 0 and is clamped: counted below)
        up += int((tie & (q.double() > quotient)).sum())
        down += int((tie & (q.double() < quotient)).sum())
        clamped += int(((quotient < 0.5) & (q == 1)).sum())
    assert seen == set(range(1, 17)), sorted(seen)
    assert up > 0 and down > 0 and clamped > 0, (up, down, clamped)


WEIGHTS = (  # (name, shape, block_dims, block_size, per_channel_dims)
    ("rows_g16", (8, 64), 1, 16, 0),
    ("rows_g32", (6, 96), 1, 32, 0),
    ("columns_g16", (64, 8), 0, 16, 1),
    ("columns_g24", (48, 6), 0, 24, 1),
)


def processed(scale: torch.Tensor, offset: torch.Tensor, bitwidth: int, shape, tile) -> ProcessedQuantParams:
    return ProcessedQuantParams(scale, offset, offset - 2 ** (bitwidth - 1), bitwidth, not bool(offset.any()), torch.Size(shape), torch.Size(tile))


def encoding_records() -> list[dict]:
    records = []
    gen = torch.Generator().manual_seed(33)
    for name, shape, block_dim, block_size, channel_dim in WEIGHTS:
        weight = torch.randn(*shape, generator=gen) * torch.rand(shape[0], 1, generator=gen).add(0.05)
        granularity = ff.PerBlock(block_dims=(block_dim,), block_sizes=(block_size,), per_channel_dims=(channel_dim,))
        tile = granularity.tile_size(weight.shape)
        quantizer = ff.nn.LinearQuantizer(4, symmetric=True, allow_one_sided=False, granularity=granularity)
        rows = tiles_to_rows(weight, tile)
        quantizer.quantization_range = (rows.min(-1).values, rows.max(-1).values)
        with torch.no_grad():
            quantized = quantizer(weight)
        scale = quantizer.scale.detach().clone()
        encoding = LPBQProcessor(4, 8).generate_lpbq_encoding(name, processed(scale, torch.zeros_like(scale), 4, shape, tile))
        records.append({"name": name, "shape": list(shape), "block_dims": [block_dim], "block_sizes": [block_size], "per_channel_dims": [channel_dim],
                        "weight": weight.clone(), "codes": quantized.raw_data.detach().to(torch.int8), "scale": scale, "encoding": encoding})
    return records


def error_records() -> list[dict]:
    records = []
    for compressed_bw, decompressed_bw in ((0, 8), (4, -1), (8, 8), (9, 8), (9, 16), (4, 33)):
        try:
            LPBQProcessor(compressed_bw, decompressed_bw)
        except ValueError as e:
            records.append({"kind": "bitwidths", "compressed_bw": compressed_bw, "decompressed_bw": decompressed_bw, "text": str(e)})
        else:  # pragma: no cover
            raise AssertionError((compressed_bw, decompressed_bw))
    scale = torch.full((8,), 0.1)
    zero = torch.zeros(8)
    unsuitable = {
        "per_channel": processed(scale, zero, 4, (8, 32), (1, 32)),
        "per_tensor": processed(scale[:1], zero[:1], 4, (8, 32), (8, 32)),
        "two_block_dims": processed(scale, zero, 4, (8, 32), (4, 8)),
        "asymmetric": processed(torch.full((16,), 0.1), torch.full((16,), 3.0), 4, (8, 32), (1, 16)),
        "bitwidth": processed(torch.full((16,), 0.1), torch.zeros(16), 8, (8, 32), (1, 16)),
    }
    for what, params in unsuitable.items():
        try:
            LPBQProcessor(4, 8)._lpbq_granularity_and_block_size(f"layer.{what}", params)
        except ValueError as e:
            records.append({"kind": "unsuitable", "what": what, "name": f"layer.{what}", "text": str(e)})
        else:  # pragma: no cover
            raise AssertionError(what)
    return records


def main() -> None:
    compress = compress_records()
    check_coverage(compress)
    fixture = {"compress": compress, "encodings": encoding_records(), "errors": error_records()}
    path = HERE / "g32_lpbq.pt"
    torch.save(fixture, path)
    torch.load(path, weights_only=True)
    print(f"wrote {path.name}: {len(compress)} compressions, {len(fixture['encodings'])} encodings, {len(fixture['errors'])} errors, {path.stat().st_size} bytes")


if __name__ == "__main__":
    main()
