"""Stage the reference FastForward package as bytecode under oracle/_ref/ (test infrastructure only; never committed).

tests/test_adapter_reference.py installs this package's kernels into the reference's own operator table and dispatcher,
importing the reference from oracle/_ref/. Its sources are read from FASTFORWARD_REFERENCE_SRC (the src/ directory of a
FastForward checkout; default below). Every module is compiled to a sourceless .pyc by the interpreter running this
script (build() runs it with its own), and the package's data files are copied beside them. Where the sources are not
available nothing is staged, an earlier staging is kept, and those tests skip.

    python oracle/stage_reference.py
"""

from __future__ import annotations

import os
import pathlib
import py_compile
import shutil

OUT = pathlib.Path(__file__).resolve().parent / "_ref"
DEFAULT_SRC = "/root/reference/src"


def stage(src: str | os.PathLike) -> bool:
    package = pathlib.Path(src) / "fastforward"
    if not os.path.isfile(package / "__init__.py"):  # False (not an error) where the path cannot be reached
        return False
    staging = OUT / "fastforward.partial"
    shutil.rmtree(staging, ignore_errors=True)
    try:
        _compile_into(package, staging)
    except PermissionError:  # parts of the checkout are unreadable to this user: as if it were absent
        shutil.rmtree(staging, ignore_errors=True)
        return False
    shutil.rmtree(OUT / "fastforward", ignore_errors=True)
    staging.rename(OUT / "fastforward")
    return True


def _compile_into(package: pathlib.Path, staging: pathlib.Path) -> None:
    for path in sorted(package.rglob("*")):
        if not path.is_file() or "__pycache__" in path.parts or path.suffix == ".pyc":
            continue
        rel = path.relative_to(package)
        if path.suffix == ".py":
            py_compile.compile(str(path), cfile=str(staging / rel.with_suffix(".pyc")), dfile=str(pathlib.Path("fastforward") / rel), doraise=True)
        else:
            (staging / rel).parent.mkdir(parents=True, exist_ok=True)
            shutil.copyfile(path, staging / rel)


if __name__ == "__main__":
    src = os.environ.get("FASTFORWARD_REFERENCE_SRC") or DEFAULT_SRC
    if stage(src):
        print(f"staged the reference package from {src} into {OUT / 'fastforward'}")
    else:
        print(f"no reference package under {src}: nothing staged" + ("" if (OUT / "fastforward").is_dir() else "; tests/test_adapter_reference.py will skip"))
