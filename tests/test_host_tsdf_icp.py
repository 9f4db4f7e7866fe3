"""Frame-to-model alignment through the plugin loader: `mslam_harness --dense <scene> --icp <frames>` drives IDenseAligner (a
dynamic_cast of hipDenseMapFactory's object) on a frames file written by tests/tsdf_icp_ref.py::write_frames; its dump equals
the numpy reference byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import tsdf_ref as tr
import tsdf_raycast_ref as rr
import tsdf_icp_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "modular-slam_amd", "host")
HARNESS = os.path.join(HOST, "mslam_harness")
PLUGIN = os.path.join(HOST, "libmslam_hip_plugin.so")
ODD = ir.ODD


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", HOST])
    return True


def frame(p, depth, R0, t0, camera=None, levels=ir.LEVELS, dist_max=ir.DIST_MAX, cos_min=ir.COS_MIN, min_pairs=ir.MIN_PAIRS, rot_tol=0.0,
          trans_tol=0.0, **kw):
    cam = rr.camera_of(p) if camera is None else camera
    z_far, step, coarse = rr.defaults(p, R0, t0, 0.1, None, None, kw.get("coarse"))
    render = dict(cam, z_near=0.1, z_far=z_far, step=step, coarse=coarse, min_weight=1)
    return dict(render=render, levels=levels, dist_max=dist_max, cos_min=cos_min, min_pairs=min_pairs, rot_tol=rot_tol,
                trans_tol=trans_tol, R0=R0, t0=t0, depth=depth)


def test_harness_knows_the_icp_mode(built):
    src = open(os.path.join(HOST, "harness.cpp")).read()
    assert "--icp" in src and "IDenseAligner" in src and "dynamic_cast" in src
    hdr = open(os.path.join(HOST, "mslam_interfaces.hpp")).read()
    for name in ("IDenseAligner", "DenseAlignParams", "DenseAlignResult", "align"):
        assert name in hdr, name
    out = subprocess.check_output(["nm", "-DC", PLUGIN]).decode()
    assert "hipDenseMapFactory" in out and "mslam_hip_tsdf_icp" in out


def test_frames_file_layout(tmp_path):
    p, _ = ir.corner_scene("small")
    depth = np.arange(1200, dtype=np.uint16).reshape(30, 40)
    f = frame(p, depth, tr.rot(1, 0.1), np.array([0.1, 0.2, 0.3]), levels=((3, 2), (1, 7)), min_pairs=16, rot_tol=1e-6)
    path = tmp_path / "frames.bin"
    ir.write_frames(str(path), [f, f])
    raw = path.read_bytes()
    one = 72 + 40 + 32 + 96 + 2400
    assert raw[:8] == ir.FRAMES_MAGIC and len(raw) == 16 + 2 * one and np.frombuffer(raw[8:16], "<i4").tolist() == [2, 0]
    assert np.frombuffer(raw[16:24], "<i4").tolist() == [40, 30]
    assert np.frombuffer(raw[88:128], "<i4").tolist() == [2, 16, 3, 1, 0, 0, 2, 7, 0, 0]
    assert np.frombuffer(raw[128:160], "<f8").tolist() == [ir.DIST_MAX, ir.COS_MIN, 1e-6, 0.0]
    assert np.frombuffer(raw[232:256], "<f8").tolist() == [0.1, 0.2, 0.3] and raw[256:256 + 2400] == depth.tobytes()


def test_harness_refuses_a_file_that_is_no_frames_file(built, tmp_path):
    """both files are read before anything touches a GPU: exit code 5"""
    p, frames = ir.corner_scene("small")
    scene, bad = tmp_path / "scene.bin", tmp_path / "bad.bin"
    tr.write_scene(str(scene), p, [(q,) + f for q, f in enumerate(frames)])
    bad.write_bytes(b"MSTSDFI0" + bytes(200))
    r = subprocess.run([HARNESS, PLUGIN, "--dense", str(scene), "--icp", str(bad)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 5, (r.returncode, r.stderr)
    short = tmp_path / "short.bin"
    ir.write_frames(str(short), [frame(p, ir.render_corner(p, *ir.TRUE_POSE), np.eye(3), np.zeros(3))])
    short.write_bytes(short.read_bytes()[:-8])
    r = subprocess.run([HARNESS, PLUGIN, "--dense", str(scene), "--icp", str(short)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 5, (r.returncode, r.stderr)


@pytest.mark.gpu
def test_plugin_aligns_as_the_reference(built, tmp_path):
    """the small corner scene with one update and one removal; three frames: the defaults from the identity, an odd render camera
    from another guess with tolerances, and a blank depth image (DEGENERATE: the guess comes back)"""
    p, frames = ir.corner_scene("small")
    ids = [5, 6, 7]
    R1, t1 = tr.rot(1, 0.02) @ frames[1][1], frames[1][2] + np.array([0.01, -0.02, 0.015])
    scene, frames_path, dump = tmp_path / "scene.bin", tmp_path / "frames.bin", tmp_path / "dump.bin"
    tr.write_scene(str(scene), p, [(i,) + f for i, f in zip(ids, frames)], [(6, R1, t1)], [7], 1)
    depth = ir.render_corner(p, *ir.TRUE_POSE)
    todo = [frame(p, depth, np.eye(3), np.zeros(3), min_pairs=16),
            frame(p, depth, *ir.OFF, camera=ODD, coarse=1, levels=((2, 6), (1, 6)), min_pairs=16, rot_tol=2e-3, trans_tol=2e-3),
            frame(p, np.zeros_like(depth), *ir.OFF)]
    ir.write_frames(str(frames_path), todo)
    r = subprocess.run([HARNESS, PLUGIN, "--dense", str(scene), "--icp", str(frames_path), "--dump", str(dump)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    S, W = tr.fresh(p, [frames[0], (frames[1][0], R1, t1)])
    got = ir.read_dump(str(dump))
    lines = [l for l in r.stdout.splitlines() if l.startswith("icp frame ")]
    assert len(got) == len(lines) == 3 and any(l.startswith("dense frames 2 moved 1 ") for l in r.stdout.splitlines())
    for q, (f, g) in enumerate(zip(todo, got)):
        v = f["render"]
        _, xyz, nrm = rr.raycast(S, W, p, f["R0"], f["t0"], camera=v, z_near=v["z_near"], z_far=v["z_far"], step=v["step"],
                                 coarse=v["coarse"], min_weight=v["min_weight"])
        ref = ir.solve(f["depth"], ir.frame_camera(p), (xyz, nrm), v, f["R0"], f["t0"], f["R0"], f["t0"], levels=f["levels"],
                       dist_max=f["dist_max"], cos_min=f["cos_min"], min_pairs=f["min_pairs"], rot_tol=f["rot_tol"], trans_tol=f["trans_tol"])
        assert g["R"].tobytes() == np.ascontiguousarray(ref["R"]).tobytes() and g["t"].tobytes() == np.ascontiguousarray(ref["t"]).tobytes(), q
        assert g["result"] == ir.result_bytes(ref) and g["record"].tobytes() == ref["record"].tobytes(), q
        assert lines[q] == "icp frame %d status %d iterations %d pairs %d" % (q, ref["status"], ref["iterations"], ref["count"])
    assert got[0]["result"][:4] == b"\x01\x00\x00\x00" and got[2]["result"][:4] == b"\x02\x00\x00\x00"
    assert got[2]["R"].tobytes() == np.ascontiguousarray(ir.OFF[0]).tobytes()
    # without --dump the lines are the same; a frame the library refuses ends with the adapter's exception and exit code 1
    r2 = subprocess.run([HARNESS, PLUGIN, "--dense", str(scene), "--icp", str(frames_path)], capture_output=True, text=True, timeout=120)
    assert r2.returncode == 0 and r2.stdout == r.stdout
    ir.write_frames(str(frames_path), [dict(todo[0], min_pairs=5)])
    r3 = subprocess.run([HARNESS, PLUGIN, "--dense", str(scene), "--icp", str(frames_path)], capture_output=True, text=True, timeout=120)
    assert r3.returncode == 1 and "mslam_hip_tsdf_icp" in r3.stderr
