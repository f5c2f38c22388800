"""`python bench.py` on one GPU at the tiny shapes: a plain run prints the headline and nothing else, `--full` adds every
side measurement to the same line."""

import json
import os
import pathlib
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
TINY = ("--gpus", "1", "--model", "tiny", "--steps", "2", "--warmup", "1", "--batch", "2", "--seq-len", "64", "--calib-seqs", "4")
SIDE = ("module_graph_drop_in", "roofline", "hbm_kernels", "attention_kernel", "host_us_per_op", "cpu_baseline", "summary")


def _bench(*args: str) -> dict:
    env = dict(os.environ)
    for key in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "FFQ_DIST_BACKEND"):
        env.pop(key, None)
    proc = subprocess.run([sys.executable, str(ROOT / "bench.py"), *TINY, *args], capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert proc.returncode == 0, proc.stderr[-3000:]
    lines = [line for line in proc.stdout.splitlines() if line.startswith("{")]
    assert len(lines) == 1, f"exactly one JSON line expected, got {len(lines)}"
    return json.loads(lines[0])


def test_plain_run_is_the_headline_only():
    line = _bench()
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["steps"] == 2 and line["warmup"] == 1
    assert line["unit"] == "tokens/s" and line["higher_is_better"] is True and line["dtype"] == "int8"
    assert line["calibration"]["sequences_per_gpu"] == 4
    assert line["module_graph_drop_in"] is None and not any(key in line for key in SIDE[1:])


def test_full_run_adds_the_side_measurements():
    line = _bench("--full")
    assert line["value"] > 0 and line["module_graph_drop_in"]["value"] > 0
    assert line["roofline"]["achieved"] > 0 and line["roofline"]["per_shape"]
    assert len(line["hbm_kernels"]) == 10 and all(row["achieved"] > 0 for row in line["hbm_kernels"])
    assert line["attention_kernel"] is None  # head_dim 32: the forward takes torch's SDPA, no attention launch to time
    assert line["host_us_per_op"]["calls"] > 0 and line["cpu_baseline"]["value"] > 0
    assert line["summary"]["tokens_per_s"] == line["value"]
