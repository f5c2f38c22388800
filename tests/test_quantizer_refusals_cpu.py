"""The status, the order of the checks and the wording of every refusal of the quantizer core, without a GPU: each call of
tests/golden/gen_quantizer_refusals.py (every entry point of ffq_quantize.hip, ffq_dequantize.hip, ffq_minmax.hip, ffq_pack.hip
and ffq_backward.hip, one call per refusal a host-only call can reach, and calls that break two rules at once) against
tests/golden/quantizer_refusals.json, which was taken from the build before the host halves of those files were restated."""

import json

import gen_quantizer_refusals

from conftest import GOLDEN, HIP_SO

FFQ_ERR_LAUNCH = 9


def test_every_refusal_reads_as_recorded():
    want = json.loads((GOLDEN / "quantizer_refusals.json").read_text())
    got = gen_quantizer_refusals.records(HIP_SO)
    assert [r["call"] for r in got] == [r["call"] for r in want], "the list of calls and the file disagree"
    assert len(want) == 316 and sum(r["status"] != 0 for r in want) == 295
    assert all(r["message"] for r in want if r["status"])  # (every refusal says why)
    assert not [r for r in want if r["status"] == FFQ_ERR_LAUNCH], "a recorded call reached a launch"
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, f"{len(wrong)} records differ, the first (got, recorded): {wrong[0]}"
