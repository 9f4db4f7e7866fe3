"""The SPARSE global bundle adjustment through the plugin loader: `mslam_harness --ba-global <scene> --sparse` reaches
ISparseGlobalBackend::setGlobalSolver of hipBundleAdjustBackendFactory's object with dynamic_cast, then
IGlobalBackend::globalBundleAdjustment, on scene files written from tests/ba_global_cases.py and
tests/ba_global_sparse_cases.py, in the manner and with the bounds of tests/test_host_ba_global.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_cases  # noqa: E402
import ba_global_cases as bg  # noqa: E402
import ba_global_sparse_cases as bc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "modular-slam_amd", "host")
HARNESS = os.path.join(HOST, "mslam_harness")
PLUGIN = os.path.join(HOST, "libmslam_hip_plugin.so")


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", HOST])
    return True


def test_harness_and_plugin_know_the_sparse_global_solver():
    """what build() left: nothing is compiled here"""
    src = open(os.path.join(HOST, "harness.cpp")).read()
    assert "--ba-global <scene> --sparse" in src and "ISparseGlobalBackend" in src and "setGlobalSolver(1)" in src
    hdr = open(os.path.join(HOST, "mslam_interfaces.hpp")).read()
    assert "class ISparseGlobalBackend" in hdr and "virtual void setGlobalSolver(int kind) = 0;" in hdr
    plugin = open(os.path.join(HOST, "mslam_hip_plugin.cpp")).read()
    assert "public ISparseGlobalBackend" in plugin and "void setGlobalSolver(int kind) override" in plugin
    out = subprocess.check_output(["nm", "-DC", PLUGIN]).decode()
    assert "hipBundleAdjustBackendFactory" in out and "mslam_hip_set_ba_global_solver" in out
    assert b"setGlobalSolver" in open(HARNESS, "rb").read()


def _reference(name):
    if name in bc.NEW:
        sc, ref, aug, dist, mask = bc.reference(name)
        return sc, ref, dist, mask
    sc, qr, sch, dist, mask, margin = bg.reference(name)
    return sc, qr, dist, mask


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["traj:66", "gross80", "loop_row"])
def test_harness_ba_global_sparse_against_the_reference(built, tmp_path, name):
    sc, ref, dist, mask = _reference(name)
    path = tmp_path / "scene.bin"
    ids = ba_cases.write_scene(str(path), sc)
    out = subprocess.run([HARNESS, PLUGIN, "--ba-global", str(path), "--sparse"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0] == "loaded ok"
    head = lines[1].split()
    assert head[0] == "ba" and int(head[2]) == ref["termination"] and abs(int(head[4]) - ref["iterations"]) <= 1
    assert abs(float(head[6]) - ref["initial_cost"]) <= 1e-6 * ref["initial_cost"]
    bound = max(1e-9, 1000.0 * dist)
    assert head[7] == "final" and abs(float(head[8]) - ref["final_cost"]) <= 1e-6 * ref["final_cost"] + len(sc["obs_kf"]) * (12.0 * bound) ** 2 / 2.0
    assert int(head[10]) == len(sc["poses"]) and int(head[12]) == len(sc["landmarks"]) and int(head[14]) == int(mask.sum())
    poses = np.array([[float(v) for v in l.split()[2:]] for l in lines if l.startswith("keyframe ")])
    lms = np.array([[float(v) for v in l.split()[2:]] for l in lines if l.startswith("landmark ")])
    assert np.max(np.abs(poses - ref["poses"])) <= bound and np.max(np.abs(lms - ref["landmarks"])) <= bound
    got = sorted((int(l.split()[1]), int(l.split()[2])) for l in lines if l.startswith("outlier "))
    assert got == sorted((int(ids[k]), int(l)) for k, l in zip(sc["obs_kf"][mask], sc["obs_lm"][mask]))
    assert np.array_equal(poses[0], sc["poses"][0])      # keyframe id 1 is constant
