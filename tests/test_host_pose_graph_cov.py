"""Marginal covariances of the pose graph through the plugin loader: `mslam_harness <plugin> --pose-graph <scene> --covariance`
drives IPoseGraphCovariance::poseGraphCovariance of hipBundleAdjustBackendFactory's object (mslam_hip_pose_graph_covariance
behind it) and prints the block of every keyframe that is not constant and has an edge.  Source, export and usage checks on
the CPU; the runs need the GPU and stand under the rule of tests/test_gpu_pose_graph_cov.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_cov_cases as cc  # noqa: E402
import pose_graph_cov_ref as cr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "modular-slam_amd", "host")
HARNESS = os.path.join(HOST, "mslam_harness")
PLUGIN = os.path.join(HOST, "libmslam_hip_plugin.so")


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", HOST])
    return True


def write_scene(path, sc):
    """pose_graph_cases.write_scene's file ("MSPG", version 1) with the ids chosen so that the scene's one constant pose,
    wherever it stands, is keyframe 1 (the adapter holds that one constant); the others are index + 2"""
    K, E = len(sc["poses"]), len(sc["edge_a"])
    assert int(np.sum(sc["fixed"] != 0)) <= 1
    ids = np.where(sc["fixed"] != 0, 1, np.arange(K) + 2).astype("<i4")
    with open(path, "wb") as f:
        f.write(b"MSPG" + np.array([1, K, E, sc.get("max_iterations", 100), sc["sqrt_info"] is not None], "<i4").tobytes())
        f.write(ids.tobytes())
        for a, dt in ((sc["poses"], "<f8"), (sc["edge_a"], "<i4"), (sc["edge_b"], "<i4"), (sc["edge_meas"], "<f8")):
            f.write(np.ascontiguousarray(a, dt).tobytes())
        if sc["sqrt_info"] is not None:
            f.write(np.ascontiguousarray(sc["sqrt_info"], "<f8").tobytes())


def test_the_interface_is_declared_and_the_mirrored_ones_gain_no_virtual(built):
    hdr = open(os.path.join(HOST, "mslam_interfaces.hpp")).read()
    body = hdr[hdr.index("class IPoseGraphCovariance"):]
    body = body[:body.index("};")]
    assert "virtual PoseGraphCovariance poseGraphCovariance(" in body and "= 0;" in body and " : " not in body.splitlines()[0]
    for base in ("IBackend", "IGlobalBackend : public IBackend", "ILoopClosingBackend : public IGlobalBackend"):
        b = hdr[hdr.index("class " + base):]
        assert "ovariance" not in b[:b.index("};")], base
    src = open(os.path.join(HOST, "harness.cpp")).read()
    assert "--pose-graph <scene> --covariance" in src[:src.index("#include")]
    assert "dynamic_cast<mslam::IPoseGraphCovariance*>" in src
    out = subprocess.check_output(["nm", "-DC", PLUGIN]).decode()
    assert "typeinfo for mslam::IPoseGraphCovariance" in out and "mslam_hip_pose_graph_covariance" in out


def test_the_harness_parses_the_flag(built, tmp_path):
    none = str(tmp_path / "none.bin")
    run = lambda *a: subprocess.run([HARNESS, PLUGIN, *a], capture_output=True, text=True, timeout=60)
    assert run("--pose-graph", none, "--covariance").returncode == 5        # as far as the scene file, which is not there
    assert run("--pose-graph", none).returncode == 5 and run("--pose-graph", none, "--sparse").returncode == 5
    assert run("--pose-graph", none, "--covariances").returncode != 5        # not a form: usage


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chain:9", "star70", "info_dense"])
def test_harness_covariance_against_the_qr_reference(built, tmp_path, name):
    sc, ref = cc.reference(name)
    path = tmp_path / "scene.bin"
    write_scene(str(path), sc)
    out = subprocess.run([HARNESS, PLUGIN, "--pose-graph", str(path), "--covariance"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0] == "loaded ok" and lines[1] == "covariance blocks %d" % len(ref["poses_of"])
    rows = [l.split() for l in lines[2:]]
    assert [r[0] for r in rows] == ["cov"] * len(ref["poses_of"]) and [int(r[1]) for r in rows] == ref["poses_of"].tolist()
    got = np.array([[float(v) for v in r[2:]] for r in rows]).reshape(-1, 6, 6)
    dist = float(np.max(np.abs(got - ref["cov"])))
    top = float(np.max(np.abs(ref["sigma"])))
    print("PGC harness %-12s P %3d d %.3e reached %.3e (relative) bound %.3e" % (name, len(got), ref["d"], dist / top, ref["bound"] / top))
    assert ref["d"] <= cr.MAX_D and dist <= ref["bound"]
    assert got.tobytes() == np.ascontiguousarray(got.transpose(0, 2, 1)).tobytes()     # %.17g round-trips: symmetric bit for bit
