"""Generate quantizer_routes.json: the SHA-256 of what every launch route of the quantizer core writes, on an MI355X.

    python tests/golden/gen_quantizer_routes.py <path to libffq_hip.so> [output file]

Run on the build of the commit whose bits are to be pinned (the file in the tree was taken from the parent of the commit that added
it, before the host halves of the five files were restated, twice, with equal results). The cases and their operands are those of
tests/quantizer_routes.py; tests/test_quantizer_routes_gpu.py compares the tree with the file, case by case."""

from __future__ import annotations

import json
import pathlib
import sys

TESTS = pathlib.Path(__file__).resolve().parent.parent
for directory in (TESTS.parent, TESTS):
    if str(directory) not in sys.path:
        sys.path.insert(0, str(directory))


def records(library_path, only=None):
    import quantizer_routes as qr

    from fastforward_amd._cabi import FFQLibrary

    lib = FFQLibrary(library_path)
    return {name: qr.digest(call(lib)) for name, call in qr.cases() if only is None or name.startswith(only)}


if __name__ == "__main__":
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    out = pathlib.Path(sys.argv[2]) if len(sys.argv) > 2 else pathlib.Path(__file__).resolve().parent / "quantizer_routes.json"
    rows = records(pathlib.Path(sys.argv[1]))
    out.write_text("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in rows.items()) + "\n}\n")
    print(f"{len(rows)} digests -> {out}")
