"""The pose-graph solve through the plugin loader: `mslam_harness --pose-graph` reaches ILoopClosingBackend::closeLoop of
hipBundleAdjustBackendFactory's object with dynamic_cast, on scene files written by tests/pose_graph_cases.py, against
tests/pose_graph_ref.py's QR solve; the bounds are those of tests/test_gpu_pose_graph.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_cases as pc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "modular-slam_amd", "host")
HARNESS = os.path.join(HOST, "mslam_harness")
PLUGIN = os.path.join(HOST, "libmslam_hip_plugin.so")


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", HOST])
    return True


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chain:17", "info_upper"])
def test_harness_pose_graph_against_the_reference(built, tmp_path, name):
    sc, qr, ch, dist = pc.reference(name)
    path = tmp_path / "scene.bin"
    pc.write_scene(str(path), sc)
    out = subprocess.run([HARNESS, PLUGIN, "--pose-graph", str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0] == "loaded ok"
    head = lines[1].split()
    bound = max(1e-9, 1000.0 * dist)
    assert head[0] == "pose_graph" and int(head[2]) == qr["termination"] and abs(int(head[4]) - qr["iterations"]) <= 1
    assert abs(float(head[6]) - qr["initial_cost"]) <= 1e-6 * qr["initial_cost"]
    second_order = len(sc["edge_a"]) * (pc.jacobian_row_bound(sc) * bound) ** 2 / 2.0
    assert head[7] == "final" and abs(float(head[8]) - qr["final_cost"]) <= 1e-6 * qr["final_cost"] + second_order
    assert int(head[10]) == len(sc["poses"]) and int(head[12]) == len(sc["edge_a"])
    poses = np.array([[float(v) for v in l.split()[2:]] for l in lines if l.startswith("keyframe ")])
    assert poses.shape == (len(sc["poses"]), 7) and pc.same_rotation_distance(poses, qr["poses"]) <= bound
    assert np.array_equal(poses[0], sc["poses"][0])      # keyframe id 1 is constant
