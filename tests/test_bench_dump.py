"""`bench.py --dump-outputs DIR`: what the last timed step computed, as float32 / float64 .npy files under 64 MB in all.
Two runs with the same arguments write the same arrays, and the dumped keypoints are the CPU oracle's for those frames."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "8", "--unique", "16", "--no-extras", "--no-cpu-baseline"]


def _run(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MSLAM_BENCH_DRY")}
    r = subprocess.run([sys.executable, BENCH] + ARGS + ["--dump-outputs", str(out_dir)], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_dump_outputs_is_reproducible_and_matches_the_oracle(tmp_path, orc):
    import synth
    lines = [_run(tmp_path / "a"), _run(tmp_path / "b")]
    for j in lines:
        assert j["steps"] == 3 and j["ms_per_step"] > 0 and j["dump_outputs"]["bytes"] <= 64 << 20
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and "xy.npy" in names and "match_to.npy" in names
    d = {}
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64) and x.dtype == y.dtype and np.array_equal(x, y), n
        d[n[:-4]] = x
    assert sum(x.nbytes for x in d.values()) <= 64 << 20
    # the last timed step is step 2 + 3 - 1 = 4 of a 2-batch cycle: frames 0..7 of the stream, all of them sampled
    assert d["frames"].tolist() == list(range(8)) and d["kp_offset"][-1] == d["kp_count"].sum() > 0
    frames = synth.make_stream(16, 640, 480, seed=1234)
    for s, f in enumerate(d["frames"].astype(int).tolist()):
        ref = orc.detect(frames[f], orc.params())
        a, b = int(d["kp_offset"][s]), int(d["kp_offset"][s + 1])
        assert np.array_equal(d["xy"][a:b], ref["xy"]) and np.array_equal(d["desc"][a:b], ref["desc"].astype(np.float32)), f
