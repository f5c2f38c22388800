"""Every launch route of the quantizer core at its smallest shape and on both sides of each threshold (tests/quantizer_routes.py):
the SHA-256 of what each case writes against tests/golden/quantizer_routes.json, recorded on the build before the host halves of
ffq_quantize.hip, ffq_dequantize.hip, ffq_minmax.hip, ffq_pack.hip and ffq_backward.hip were restated
(tests/golden/gen_quantizer_routes.py). Digests only: what the bits should be is the business of the parity and exact suites."""

import json

import pytest

import quantizer_routes as qr

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
FAMILIES = {"affine": qr.affine_cases, "minmax": qr.minmax_cases, "dynamic": qr.dynamic_cases, "pack": qr.pack_cases, "backward": qr.backward_cases}
COUNTS = {"affine": 205, "minmax": 79, "dynamic": 52, "pack": 33, "backward": 39}


def test_the_file_holds_every_case():
    want = json.loads((GOLDEN / "quantizer_routes.json").read_text())
    assert list(want) == [name for name, _ in qr.cases()], "the case list and the file disagree"
    assert {family: len(build()) for family, build in FAMILIES.items()} == COUNTS and len(want) == sum(COUNTS.values())


@pytest.mark.parametrize("family", list(FAMILIES))
def test_every_route_writes_the_recorded_bits(family, hip_backend):
    want = json.loads((GOLDEN / "quantizer_routes.json").read_text())
    wrong = [name for name, call in FAMILIES[family]() if qr.digest(call(hip_backend)) != want[name]]
    assert not wrong, f"{len(wrong)} cases differ from the recorded digests: {wrong[:8]}"
