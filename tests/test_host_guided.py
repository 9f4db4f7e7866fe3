"""Guided matching through the plugin loader: `mslam_harness --track --guided <radius>` (IKeyframeTracker::setGuidedMatch)
over the synthetic sequence tests/test_host_track.py uses, against the Python tracker HipKeyframeTracker(guided_radius =
radius) on the same frames.  Both loops make the same library calls on the same inputs, so flags, ids and poses are equal
(the harness prints the poses with 17 digits).  Radius 15 is the setting DESIGN 4.13 measures; the camera of this sequence moves about
95 px per frame, which radius 150 covers."""
import os
import subprocess
import sys

import numpy as np
import pytest

import track_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "modular-slam_amd", "host")
HARNESS = os.path.join(HOST, "mslam_harness")
PLUGIN = os.path.join(HOST, "libmslam_hip_plugin.so")


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", HOST])
    return True


def test_harness_and_adapter_know_the_guided_mode(built):
    assert "--guided" in open(os.path.join(HOST, "harness.cpp")).read()
    assert "setGuidedMatch" in open(os.path.join(HOST, "mslam_interfaces.hpp")).read()
    out = subprocess.check_output(["nm", "-DC", PLUGIN]).decode()
    assert "mslam_hip_set_guided_match" in out                              # the plugin calls the new C ABI


@pytest.mark.gpu
@pytest.mark.parametrize("radius", [15, 150])
def test_harness_guided_equals_the_python_tracker(built, pkg, orc, tmp_path, radius):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth
    seq = tr.make_sequence(seed=0)
    voc = tmp_path / "orbvoc.dbow3"
    voc.write_bytes(synth.make_vocabulary(10, 4, seed=5))
    path = tmp_path / "scene.bin"
    tr.write_scene(str(path), seq, seed=0)
    r = subprocess.run([HARNESS, PLUGIN, "--track", str(voc), str(path), "--guided", str(radius)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("track frame ")]
    assert len(lines) == len(seq["frames"])
    c = pkg.Context(width=640, height=480)
    params = dict(tr.SEQ_PARAMS)
    trk = pkg.HipKeyframeTracker(c, focal=tr.CAM[:2], principal=tr.CAM[2:], factor=tr.FACTOR, seed=0, guided_radius=radius, **params)
    assert c.get_guided_match() == (float(radius), 256, 640, 480)
    tracked = 0
    for f, (line, fr) in enumerate(zip(lines, seq["frames"])):
        o = trk.processSensorData(fr["desc"], fr["xy"], fr["depth"])
        tok = line.split()
        rv, tv = np.array([float(x) for x in tok[8:11]]), np.array([float(x) for x in tok[12:15]])
        got = (bool(int(tok[4])), int(tok[6]), int(tok[16]), int(tok[18]), bool(int(tok[20])))
        assert got == (o["tracked"], o["n_inliers"], o["reference"], o["keyframe"], o["relocalized"]), (f, got, line)
        assert np.array_equal(rv, o["rvec"]) and np.array_equal(tv, o["tvec"]), (f, rv, o["rvec"])
        tracked += f > 0 and o["tracked"]
        if f > 0 and o["tracked"]:
            assert c.last_match_kernel() == "guided"
    print("radius", radius, "tracked", tracked, "of", len(lines) - 1)
    assert radius != 150 or tracked > 20
    c.close()
