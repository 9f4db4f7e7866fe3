"""The ray-cast of the dense map through the plugin loader: `mslam_harness --dense <scene> --raycast <views>` drives
IDenseMapRenderer (a dynamic_cast of hipDenseMapFactory's object) on a views file written by
tests/tsdf_raycast_ref.py::write_views; its dump equals the numpy reference byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import tsdf_ref as tr
import tsdf_raycast_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "modular-slam_amd", "host")
HARNESS = os.path.join(HOST, "mslam_harness")
PLUGIN = os.path.join(HOST, "libmslam_hip_plugin.so")


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", HOST])
    return True


def view(p, R, t, camera=None, z_near=0.1, min_weight=1, **kw):
    cam = rr.camera_of(p) if camera is None else camera
    z_far, step, coarse = rr.defaults(p, R, t, z_near, kw.get("z_far"), kw.get("step"), kw.get("coarse"))
    return dict(cam, z_near=z_near, z_far=z_far, step=step, coarse=coarse, min_weight=min_weight, R=R, t=t)


def test_harness_knows_the_raycast_mode(built):
    src = open(os.path.join(HOST, "harness.cpp")).read()
    assert "--raycast" in src and "IDenseMapRenderer" in src and "dynamic_cast" in src
    hdr = open(os.path.join(HOST, "mslam_interfaces.hpp")).read()
    for name in ("IDenseMapRenderer", "DenseRenderParams", "DenseRender", "render"):
        assert name in hdr, name
    out = subprocess.check_output(["nm", "-DC", PLUGIN]).decode()
    assert "hipDenseMapFactory" in out and "mslam_hip_tsdf_raycast" in out


def test_harness_refuses_a_file_that_is_no_views_file(built, tmp_path):
    """both files are read before anything touches a GPU: exit code 5"""
    p, frames = tr.sphere_scene()
    scene, bad = tmp_path / "scene.bin", tmp_path / "bad.bin"
    tr.write_scene(str(scene), p, [(q,) + f for q, f in enumerate(frames)])
    bad.write_bytes(b"MSTSDFV0" + bytes(200))
    r = subprocess.run([HARNESS, PLUGIN, "--dense", str(scene), "--raycast", str(bad)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 5, (r.returncode, r.stderr)
    short = tmp_path / "short.bin"
    rr.write_views(str(short), [view(p, np.eye(3), np.zeros(3))])
    short.write_bytes(short.read_bytes()[:-8])
    r = subprocess.run([HARNESS, PLUGIN, "--dense", str(scene), "--raycast", str(short)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 5, (r.returncode, r.stderr)


@pytest.mark.gpu
def test_plugin_renders_as_the_reference(built, tmp_path):
    """the sphere scene with one update and one removal, seen from three views"""
    p, frames = tr.sphere_scene()
    ids = [5, 6, 7]
    R1, t1 = tr.rot(1, 0.23) @ frames[1][1], frames[1][2] + np.array([0.01, -0.02, 0.015])
    scene, views_path, dump = tmp_path / "scene.bin", tmp_path / "views.bin", tmp_path / "dump.bin"
    tr.write_scene(str(scene), p, [(i,) + f for i, f in zip(ids, frames)], [(6, R1, t1)], [7], 1)
    tilted = (tr.rot(1, -0.12) @ tr.rot(0, 0.07), np.array([-0.1, 0.05, 0.02]))
    odd = dict(width=23, height=17, focal=(22.0, 23.0), principal=(11.0, 8.0))
    views = [view(p, np.eye(3), np.zeros(3)), view(p, *tilted, camera=odd, coarse=1),
             view(p, tr.rot(1, np.pi), np.array([0.0, 0.0, -3.0]))]
    rr.write_views(str(views_path), views)
    r = subprocess.run([HARNESS, PLUGIN, "--dense", str(scene), "--raycast", str(views_path), "--dump", str(dump)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    S, W = tr.fresh(p, [frames[0], (frames[1][0], R1, t1)])
    got = rr.read_dump(str(dump))
    lines = [l for l in r.stdout.splitlines() if l.startswith("raycast view ")]
    assert len(got) == len(lines) == 3 and any(l.startswith("dense frames 2 moved 1 ") for l in r.stdout.splitlines())
    for q, (v, (depth, xyz, nrm, hits)) in enumerate(zip(views, got)):
        ref = rr.raycast(S, W, p, v["R"], v["t"], camera=v, z_near=v["z_near"], z_far=v["z_far"], step=v["step"], coarse=v["coarse"],
                         min_weight=v["min_weight"])
        assert depth.tobytes() == ref[0].tobytes() and xyz.tobytes() == ref[1].tobytes() and nrm.tobytes() == ref[2].tobytes(), q
        assert hits == int((ref[0] > 0).sum())
        assert lines[q] == "raycast view %d size %d x %d hits %d" % (q, v["width"], v["height"], hits)
    assert got[0][3] > 0 and got[1][3] > 0 and got[2][3] == 0
    # without --dump the lines are the same; a view the library refuses ends with the adapter's exception and exit code 1
    r2 = subprocess.run([HARNESS, PLUGIN, "--dense", str(scene), "--raycast", str(views_path)], capture_output=True, text=True, timeout=120)
    assert r2.returncode == 0 and r2.stdout == r.stdout
    rr.write_views(str(views_path), [dict(views[0], step=0.0)])
    r3 = subprocess.run([HARNESS, PLUGIN, "--dense", str(scene), "--raycast", str(views_path)], capture_output=True, text=True, timeout=120)
    assert r3.returncode == 1 and "mslam_hip_tsdf_raycast" in r3.stderr
