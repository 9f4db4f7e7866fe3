"""The SPARSE pose-graph solver through the plugin loader: `mslam_harness --pose-graph <scene> --sparse` reaches
ISparsePoseGraphBackend::setPoseGraphSolver and ILoopClosingBackend::closeLoop of hipBundleAdjustBackendFactory's object with
dynamic_cast.  Source and usage checks and the refused kind on the CPU (the backend throws before anything touches a device);
the run itself needs the GPU: it returns the bits of the Python mirror (Context.pose_graph after
set_pose_graph_solver("sparse")) and stays within the bound of tests/test_gpu_pose_graph_sparse.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_cases as pc  # noqa: E402
import pose_graph_sparse_cases as psc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "modular-slam_amd", "host")
HARNESS = os.path.join(HOST, "mslam_harness")
PLUGIN = os.path.join(HOST, "libmslam_hip_plugin.so")
SCENE = "loops:66"


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", HOST])
    return True


def test_harness_and_interfaces_know_the_solver(built):
    src = open(os.path.join(HOST, "harness.cpp")).read()
    assert "--pose-graph <scene> --sparse | --solver <kind>" in src[:src.index("#include")] and "ISparsePoseGraphBackend" in src
    hdr = open(os.path.join(HOST, "mslam_interfaces.hpp")).read()
    assert "class ISparsePoseGraphBackend" in hdr and "virtual void setPoseGraphSolver(int kind) = 0;" in hdr
    for base in ("IBackend", "IGlobalBackend : public IBackend", "ILoopClosingBackend : public IGlobalBackend", "IRobustBackend"):
        body = hdr[hdr.index("class " + base):]
        assert "setPoseGraphSolver" not in body[:body.index("};")], base       # the other interfaces gain no virtual
    out = subprocess.check_output(["nm", "-DC", PLUGIN]).decode()
    assert "hipBundleAdjustBackendFactory" in out and "mslam_hip_set_pose_graph_solver" in out
    assert b"--sparse" in open(HARNESS, "rb").read()


def test_a_kind_outside_0_1_throws(built, tmp_path):
    path = tmp_path / "scene.bin"
    pc.write_scene(str(path), psc.scene(SCENE))
    for kind in ("2", "-1"):
        out = subprocess.run([HARNESS, PLUGIN, "--pose-graph", str(path), "--solver", kind], capture_output=True, text=True, timeout=60)
        assert out.returncode == 1 and "setPoseGraphSolver: kind 0 (dense) or 1 (sparse)" in out.stderr, kind
        assert "pose_graph termination" not in out.stdout
    for text in ("abc", "1x", ""):                            # not an integer: a usage error, not kind 0
        out = subprocess.run([HARNESS, PLUGIN, "--pose-graph", str(path), "--solver", text], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and "--solver takes an integer kind" in out.stderr, text


@pytest.mark.gpu
def test_harness_sparse_returns_the_bits_of_the_python_mirror(built, pkg, tmp_path):
    sc, ref, aug, dist = psc.reference(SCENE)
    path = tmp_path / "scene.bin"
    pc.write_scene(str(path), sc)
    out = subprocess.run([HARNESS, PLUGIN, "--pose-graph", str(path), "--sparse"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0] == "loaded ok"
    head = lines[1].split()
    poses = np.array([[float(v) for v in l.split()[2:]] for l in lines if l.startswith("keyframe ")])
    c = pkg.Context(width=0, height=0)
    c.set_pose_graph_solver("sparse")
    mirror = c.pose_graph(sc["poses"], sc["edge_a"], sc["edge_b"], sc["edge_meas"], sc["sqrt_info"], sc["fixed"])
    c.close()
    assert head[0] == "pose_graph" and int(head[2]) == mirror["termination"] == ref["termination"] and int(head[4]) == mirror["iterations"]
    assert float(head[6]) == mirror["initial_cost"] and float(head[8]) == mirror["final_cost"]
    assert poses.shape == (len(sc["poses"]), 7) and poses.tobytes() == mirror["poses"].tobytes()
    assert abs(int(head[4]) - ref["iterations"]) <= 1
    assert pc.same_rotation_distance(poses, ref["poses"]) <= max(1e-9, 1000.0 * dist)
    assert np.array_equal(poses[0], sc["poses"][0])      # keyframe id 1 is constant
    # `--solver 0` is the plain call
    dense = subprocess.run([HARNESS, PLUGIN, "--pose-graph", str(path), "--solver", "0"], capture_output=True, text=True, timeout=120)
    plain = subprocess.run([HARNESS, PLUGIN, "--pose-graph", str(path)], capture_output=True, text=True, timeout=120)
    assert dense.returncode == 0 and dense.stdout == plain.stdout
