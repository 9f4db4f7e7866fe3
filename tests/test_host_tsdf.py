"""The dense TSDF map through the plugin loader: `mslam_harness --dense <scene>` drives hipDenseMapFactory (IDenseMap) on a
scene file written by tests/tsdf_ref.py::write_scene; its line and its dump equal the Python path byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import tsdf_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "modular-slam_amd", "host")
HARNESS = os.path.join(HOST, "mslam_harness")
PLUGIN = os.path.join(HOST, "libmslam_hip_plugin.so")


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", HOST])
    return True


def test_harness_knows_the_dense_mode(built):
    src = open(os.path.join(HOST, "harness.cpp")).read()
    assert "--dense" in src and "--dump" in src and "IDenseMap" in src and "hipDenseMapFactory" in src
    hdr = open(os.path.join(HOST, "mslam_interfaces.hpp")).read()
    for name in ("IDenseMap", "DenseMapParams", "addFrame", "updatePoses", "removeFrame", "extract"):
        assert name in hdr, name
    out = subprocess.check_output(["nm", "-DC", PLUGIN]).decode()
    assert "hipDenseMapFactory" in out and "mslam_hip_tsdf_update_poses" in out and "mslam_hip_tsdf_extract" in out


def test_harness_refuses_a_file_that_is_no_scene(built, tmp_path):
    """read before anything touches a GPU: exit code 5"""
    bad = tmp_path / "bad.bin"
    bad.write_bytes(b"MSTSDF0\0" + bytes(200))
    r = subprocess.run([HARNESS, PLUGIN, "--dense", str(bad)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 5, (r.returncode, r.stderr)


@pytest.mark.gpu
def test_plugin_maps_as_the_python_path(built, pkg, tmp_path):
    """the sphere scene with one update and one removal"""
    p, frames = tr.sphere_scene()
    ids = [5, 6, 7]
    R1, t1 = tr.rot(1, 0.23) @ frames[1][1], frames[1][2] + np.array([0.01, -0.02, 0.015])
    updates = [(6, R1, t1), (5, frames[0][1], frames[0][2])]      # one moved, one listed with the pose it has
    for min_weight in (1, 2):
        path, dump = tmp_path / ("scene%d.bin" % min_weight), tmp_path / ("dump%d.bin" % min_weight)
        tr.write_scene(str(path), p, [(i,) + f for i, f in zip(ids, frames)], updates, [7], min_weight)
        r = subprocess.run([HARNESS, PLUGIN, "--dense", str(path), "--dump", str(dump)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        line = [l for l in r.stdout.splitlines() if l.startswith("dense ")][0]
        c = pkg.Context(width=0, height=0)
        c.tsdf_create(**tr.create_kwargs(p))
        for i, f in zip(ids, frames):
            c.tsdf_add_frame(i, *f)
        moved = c.tsdf_update_poses([u[0] for u in updates], np.stack([u[1] for u in updates]), np.stack([u[2] for u in updates]))
        c.tsdf_remove_frame(7)
        S, W = c.tsdf_read()
        xyz, nrm = c.tsdf_extract(min_weight)
        assert moved == 1
        assert line == "dense frames %d moved %d points %d sumS %d sumW %d" % (c.tsdf_info()[1], moved, len(xyz),
                                                                                 int(S.astype(np.int64).sum()), int(W.astype(np.int64).sum()))
        assert dump.read_bytes() == S.tobytes() + W.tobytes() + xyz.tobytes() + nrm.tobytes()
        ref = tr.fresh(p, [frames[0], (frames[1][0], R1, t1)])
        assert np.array_equal(S, ref[0]) and np.array_equal(W, ref[1])
        assert len(xyz) == len(tr.extract(ref[0], ref[1], p, min_weight)[0]) > 0
        c.close()
    # a scene the library refuses (a frame id twice) ends with the adapter's exception: "error: ..." and exit code 1
    path = tmp_path / "twice.bin"
    tr.write_scene(str(path), p, [(1,) + frames[0], (1,) + frames[1]])
    r = subprocess.run([HARNESS, PLUGIN, "--dense", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "mslam_hip_tsdf_add_frame" in r.stderr
