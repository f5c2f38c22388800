"""Generate decode_refusals.json: what the decode-attention and KV-cache entry points answer to every call they refuse, word for word.

    python tests/golden/gen_decode_refusals.py <path to libffq_hip.so> [output file]

Run on the build of the commit whose wording is to be pinned (the file in the tree was taken from the parent of the commit that
added it, before the host side of the family was restated). Two kinds of record, each walked from the list the tests themselves walk:

    {"list": "<test module>.<table>", "index": i, "status": <FFQ status>, "message": <the whole ffq_last_error() text>}

one per row of the five C-ABI error tables (``ERRORS`` of test_sdpa_decode_cpu, ``APPEND_ERRORS`` / ``DECODE_ERRORS`` of
test_kv_cache_cpu and test_kv_paged_cpu; "" for a row that returns FFQ_OK), and

    {"list": "<test module>.<builder>", "index": i, "type": <exception class>, "message": <its whole text>}

one per call the wrappers of ops/decode.py and ops/kv_cache.py and the two classes of nn/kv_cache.py refuse on host tensors.
tests/test_decode_refusals_cpu.py compares the tree with the file, record for record."""

from __future__ import annotations

import json
import pathlib
import sys

TESTS = pathlib.Path(__file__).resolve().parent.parent
for directory in (TESTS.parent, TESTS):  # the package, and the test modules whose lists are walked
    if str(directory) not in sys.path:
        sys.path.insert(0, str(directory))

TABLES = (("test_sdpa_decode_cpu", "ERRORS"), ("test_kv_cache_cpu", "APPEND_ERRORS"), ("test_kv_cache_cpu", "DECODE_ERRORS"),
          ("test_kv_paged_cpu", "APPEND_ERRORS"), ("test_kv_paged_cpu", "DECODE_ERRORS"))
BUILDERS = (("test_sdpa_decode_cpu", "wrapper_refusals"), ("test_sdpa_decode_cpu", "causal_with_a_mask"), ("test_kv_cache_cpu", "wrapper_refusals"),
            ("test_kv_paged_cpu", "wrapper_refusals"), ("test_kv_cache_cpu", "class_refusals"), ("test_kv_paged_cpu", "class_refusals"))


def _calls(module, builder):
    """The refused calls of one builder: a list of calls, a (..., [(call, words)]) tuple, or the one call the builder itself is."""
    fn = getattr(module, builder)
    if builder == "causal_with_a_mask":
        return [fn]
    built = fn()
    return built if isinstance(built, list) else [call for call, _ in built[-1]]


def records(library_path):
    import importlib

    from fastforward_amd._cabi import FFQLibrary

    out = []
    for name, table in TABLES:
        for index, (call, _) in enumerate(getattr(importlib.import_module(name), table)):
            lib = FFQLibrary(library_path)
            status = int(call(lib))
            out.append({"list": f"{name}.{table}", "index": index, "status": status, "message": lib.ffq_last_error().decode() if status else ""})
    for name, builder in BUILDERS:
        for index, call in enumerate(_calls(importlib.import_module(name), builder)):
            try:
                call()
            except Exception as refusal:  # noqa: BLE001 (the class is part of the record)
                out.append({"list": f"{name}.{builder}", "index": index, "type": type(refusal).__name__, "message": str(refusal)})
            else:
                out.append({"list": f"{name}.{builder}", "index": index, "type": None, "message": ""})
    return out


if __name__ == "__main__":
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    out = pathlib.Path(sys.argv[2]) if len(sys.argv) > 2 else pathlib.Path(__file__).resolve().parent / "decode_refusals.json"
    rows = records(pathlib.Path(sys.argv[1]))
    out.write_text("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]\n")
    print(f"{len(rows)} records, {sum('status' in r for r in rows)} from the C ABI -> {out}")
