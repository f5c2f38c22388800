"""The wording of every refusal of the decode-attention and KV-cache family, without a GPU: the status and the whole
``ffq_last_error()`` text of each row of the five C-ABI error tables, and the exception class and whole text of each call the
wrappers (ops/decode.py, ops/kv_cache.py) and the two cache classes (nn/kv_cache.py) refuse on host tensors, against
tests/golden/decode_refusals.json (taken from the build before the family's host side was restated:
tests/golden/gen_decode_refusals.py). The tables' own tests pin the statuses and the order of the checks; this pins the words."""

import json

import gen_decode_refusals

from conftest import GOLDEN, HIP_SO


def test_every_refusal_reads_as_recorded():
    want = json.loads((GOLDEN / "decode_refusals.json").read_text())
    got = gen_decode_refusals.records(HIP_SO)
    assert [(r["list"], r["index"]) for r in got] == [(r["list"], r["index"]) for r in want], "the lists the tests walk and the file disagree"
    assert sum("status" in r for r in want) == 246 and sum("type" in r for r in want) == 159
    assert all(r["message"] for r in want if r.get("status") or r.get("type"))  # (every refusal says why)
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, f"{len(wrong)} records differ, the first (got, recorded): {wrong[0]}"
