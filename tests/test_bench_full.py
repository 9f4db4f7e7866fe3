"""`bench.py` without `--full` does only what its headline needs; `--full` adds the measurements after the timed region
(popcount matcher, every stage alone, PCIe-inclusive, CPU baseline).  Small batches, so that both runs stay short."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
ARGS = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "8", "--unique", "16"]
FULL_ONLY = ("cpu_baseline", "value_popcount_matcher", "pcie_inclusive", "value_pcie_inclusive", "cfg3", "cfg5", "cfg2_k2000",
             "cfg4_one_rank", "latency_us", "exchange", "cfg4")


def _run(extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MSLAM_BENCH_DRY")}
    r = subprocess.run([sys.executable, BENCH] + ARGS + extra, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _headline_ok(j):
    assert j["metric"] == json.load(open(os.path.join(ROOT, "BASELINE.json")))["metric"]
    assert j["unit"] == "keypoints/s" and j["higher_is_better"] is True and j["dtype"] == "u8"
    assert j["steps"] == 2 and j["warmup"] == 1 and j["value"] > 0 and j["ms_per_step"] > 0


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only():
    j = _run([])
    _headline_ok(j)
    assert not [k for k in FULL_ONLY if k in j] and "extras_error" not in j
    assert "stages_ms_serialized" not in j["roofline"]


@pytest.mark.gpu
def test_full_run_adds_what_the_headline_does_not_need():
    j = _run(["--full", "--no-legs", "--cpu-seconds", "1"])
    _headline_ok(j)
    assert "extras_error" not in j, j["extras_error"]
    assert j["value_popcount_matcher"] > 0 and j["value_pcie_inclusive"] > 0 and j["cpu_baseline"]["value"] > 0
    assert "describe" in j["roofline"]["stages_ms_serialized"]
