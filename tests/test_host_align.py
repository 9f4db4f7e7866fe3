"""RANSAC rigid alignment through the plugin loader: `mslam_harness --align` drives hipRigidAlignerFactory on a scene written
by tests/align_ref.py, and `--track ... --align <max_distance>` drives the tracking loop with
IAlignedKeyframeTracker::setTrackPose — both against the Python path on the same data."""
import os
import subprocess
import sys

import numpy as np
import pytest

import align_ref as ar
import track_align_ref as tar
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


def test_harness_knows_the_align_modes(built):
    src = open(os.path.join(HOST, "harness.cpp")).read()
    assert "--align" in src and "IRigidAligner" in src and "IAlignedKeyframeTracker" in src
    hdr = open(os.path.join(HOST, "mslam_interfaces.hpp")).read()
    for name in ("IRigidAligner", "RigidAlignment", "IAlignedKeyframeTracker", "setTrackPose"):
        assert name in hdr, name
    out = subprocess.check_output(["nm", "-DC", PLUGIN]).decode()
    assert "mslam_hip_align_ransac" in out and "mslam_hip_set_track_pose" in out and "hipRigidAlignerFactory" in out


def test_scene_file_reads_back(tmp_path):
    """every float of the text scene reads back to the f32 it was written from"""
    src, dst = ar.scene(3, 50, 0.3, 0.005)[:2]
    path = tmp_path / "scene.txt"
    ar.write_scene(str(path), src, dst, 0.05, 77, 9)
    lines = path.read_text().splitlines()
    assert lines[0].split() == ["50", "77", "0.050000000000000003", "9"] and len(lines) == 51
    back = np.array([[float(x) for x in l.split()] for l in lines[1:]]).astype(np.float32)
    assert np.array_equal(back[:, :3], src) and np.array_equal(back[:, 3:], dst)


@pytest.mark.gpu
def test_plugin_aligns_as_the_python_path(built, pkg, tmp_path):
    c = pkg.Context(width=0, height=0)
    scenes = [("scene", ar.scene(21, 400, 0.3, 0.005)[:2] + (ar.MAX_DISTANCE,))]
    scenes += [(k, v[:3]) for k, v in ar.edge_scenes().items() if k in ("nan_point", "collinear", "rot180_z")]
    for name, (src, dst, dist) in scenes:
        path = tmp_path / (name + ".txt")
        ar.write_scene(str(path), src, dst, dist, 100, 5)
        r = subprocess.run([HARNESS, PLUGIN, "--align", str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        line = [l for l in r.stdout.splitlines() if l.startswith("align ")][0]
        got = c.align_ransac(src, dst, dist, 100, 5)
        if got is None:
            assert line == "align none", name
            continue
        tok = line.split()
        R = np.array([float(x) for x in tok[2:11]]).reshape(3, 3)
        t = np.array([float(x) for x in tok[12:15]])
        mask = np.array([ch == "1" for ch in tok[18]])
        assert int(tok[16]) == int(got[2].sum()) and np.array_equal(mask, got[2]), name
        assert np.array_equal(t, got[1]) and np.abs(R - po.rodrigues(got[0])).max() < 1e-12, name    # the same rvec, turned into R twice
    c.close()


@pytest.mark.gpu
def test_plugin_tracks_with_alignment_as_the_reference_loop(built, orc, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth
    seq = tr.make_sequence(seed=0)
    rows, trk = tar.run_reference(seq, 0.05)
    voc = tmp_path / "orbvoc.dbow3"
    voc.write_bytes(synth.make_vocabulary(10, 4, seed=5))
    path = tmp_path / "scene.bin"
    tr.write_scene(str(path), seq, seed=0)
    r = subprocess.run([HARNESS, PLUGIN, "--track", str(voc), str(path), "--align", "0.05"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("track frame ")]
    assert len(lines) == len(rows)
    got = []
    for f, (line, ref) in enumerate(zip(lines, rows)):
        tok = line.split()
        assert int(tok[2]) == f
        rv, tv = np.array([float(x) for x in tok[8:11]]), np.array([float(x) for x in tok[12:15]])
        o = dict(tracked=bool(int(tok[4])), n_inliers=int(tok[6]), R=po.rodrigues(rv), t=tv, reference=int(tok[16]), keyframe=int(tok[18]))
        assert o["tracked"] == ref["tracked"] and o["n_inliers"] == ref["n_inliers"], f
        assert np.abs(o["R"] - ref["R"]).max() <= 1e-9 and np.abs(o["t"] - ref["t"]).max() <= 1e-9, f
        got.append(o)
    # (the plugin numbers the keyframes it inserts from 2^30; the frames at which it does so are the reference's)
    assert [f for f, o in enumerate(got) if o["keyframe"] >= 0] == tr.summarize(rows)[1]
    bad = subprocess.run([HARNESS, PLUGIN, "--track", str(voc), str(path), "--align", "0"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2
