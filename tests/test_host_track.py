"""The keyframe tracking step through the plugin loader: `mslam_harness --track` drives hipOrbRelocalizerFactory's
IKeyframeTracker extension (initFirstKeyframe, trackKeyframe; relocalizePose when tracking fails) over the synthetic
sequence of tests/track_ref.py, written as a scene file, against the numpy loop of the same module."""
import os
import subprocess
import sys

import numpy as np
import pytest

import reloc_ref as rr
import track_ref as tr
from reloc_ref import po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "modular-slam_amd", "host")
HARNESS = os.path.join(HOST, "mslam_harness")
PLUGIN = os.path.join(HOST, "libmslam_hip_plugin.so")


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", HOST])
    return True


def test_harness_knows_the_track_mode(built):
    src = open(os.path.join(HOST, "harness.cpp")).read()
    assert "--track" in src and "IKeyframeTracker" in src and "MSTK" in src
    hdr = open(os.path.join(HOST, "mslam_interfaces.hpp")).read()
    for name in ("IKeyframeTracker", "trackKeyframe", "visibleLandmarks", "initFirstKeyframe", "KeyframeTrackResult"):
        assert name in hdr, name
    out = subprocess.check_output(["nm", "-DC", PLUGIN]).decode()
    assert "mslam_hip_track" in out and "mslam_hip_kf_visible" in out        # the plugin calls the new C ABI
    assert b"MSTK" in open(HARNESS, "rb").read()                           # the scene file's magic


def test_scene_file_layout(tmp_path, orc):
    """what write_scene puts down is what the harness's reader expects: header of 76 bytes, then n, descriptors, f32
    coordinates and the depth image per frame"""
    seq = tr.make_sequence(seed=0, n_frames=2)
    path = tmp_path / "scene.bin"
    tr.write_scene(str(path), seq, seed=3)
    raw = path.read_bytes()
    assert raw[:4] == b"MSTK" and np.frombuffer(raw, "<i4", 4, 4).tolist() == [1, 2, 640, 480]
    assert np.frombuffer(raw, "<f8", 4, 20).tolist() == list(tr.CAM) and np.frombuffer(raw, "<f4", 1, 52)[0] == np.float32(tr.FACTOR)
    assert np.frombuffer(raw, "<i4", 3, 56).tolist() == [3, 10, tr.SEQ_PARAMS["new_keyframe_min_landmarks"]]
    assert np.frombuffer(raw, "<f8", 1, 68)[0] == 3.0
    off = 76
    for fr in seq["frames"]:
        n = int(np.frombuffer(raw, "<i4", 1, off)[0])
        assert n == len(fr["desc"])
        assert np.array_equal(np.frombuffer(raw, np.uint8, n * 32, off + 4).reshape(n, 32), fr["desc"])
        assert np.array_equal(np.frombuffer(raw, "<f4", n * 2, off + 4 + n * 32).reshape(n, 2), fr["xy"])
        assert np.array_equal(np.frombuffer(raw, "<u2", 640 * 480, off + 4 + n * 40).reshape(480, 640), fr["depth"])
        off += 4 + n * 40 + 640 * 480 * 2
    assert off == len(raw)


@pytest.mark.gpu
def test_plugin_tracks_the_sequence_as_the_reference_loop(built, orc, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth
    seq = tr.make_sequence(seed=0)
    rows, trk = tr.run_reference(seq)
    voc = tmp_path / "orbvoc.dbow3"
    voc.write_bytes(synth.make_vocabulary(10, 4, seed=5))
    path = tmp_path / "scene.bin"
    tr.write_scene(str(path), seq, seed=0)
    r = subprocess.run([HARNESS, PLUGIN, "--track", str(voc), str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("track frame ")]
    print("\n".join(lines))
    assert len(lines) == len(rows)
    got = []
    for f, (line, ref, fr) in enumerate(zip(lines, rows, seq["frames"])):
        tok = line.split()
        assert int(tok[2]) == f
        rv, tv = np.array([float(x) for x in tok[8:11]]), np.array([float(x) for x in tok[12:15]])
        o = dict(tracked=bool(int(tok[4])), n_inliers=int(tok[6]), R=po.rodrigues(rv), t=tv, reference=int(tok[16]),
                 keyframe=int(tok[18]), relocalized=bool(int(tok[20])))
        got.append(o)
        # each loop runs on its own poses (1e-7 apart after the first step): flags and ids equal, poses against ground truth
        assert (o["tracked"], o["reference"], o["keyframe"], o["relocalized"]) == (ref["tracked"], ref["reference"], ref["keyframe"],
                                                                                 ref["relocalized"]), f
        assert rr.rot_err(o["R"], fr["R"]) < 0.1 and np.linalg.norm(o["t"] - fr["t"]) < 0.02, f
    assert tr.summarize(got) == tr.summarize(rows)
    # frame 1 starts from the identity on both sides: the same step, the PnP kernel's bound against its oracle
    assert got[1]["n_inliers"] == rows[1]["n_inliers"]
    assert np.abs(got[1]["R"] - rows[1]["R"]).max() < 1e-7 and np.abs(got[1]["t"] - rows[1]["t"]).max() < 1e-7

    # a file that is not a scene
    bad = tmp_path / "bad.bin"
    bad.write_bytes(b"nope" * 100)
    r = subprocess.run([HARNESS, PLUGIN, "--track", str(voc), str(bad)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 5 and "not a tracking scene" in r.stderr
