"""mslam_hip_bundle_adjust_global without a GPU: the trajectory scenes of tests/ba_global_cases.py take the paths their GPU
tests rely on (both CPU solvers converge in the same number of iterations, `hard66` has rejected steps, almost no pair of
keyframes is covisible, the wrap pairs exist, `gross80` has outliers with a margin), and the new entry point is declared,
exported and wired: header, library, ABI list, HipBackend(global_solver=True)."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_global_cases as bg  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (M, iterations, rejected steps) of the QR solve
EXPECT = {"traj:8": (74, 3, 0), "traj:9": (83, 4, 0), "traj:10": (92, 4, 0), "traj:16": (146, 4, 0), "traj:17": (155, 4, 0),
          "traj:18": (164, 4, 0), "traj:32": (290, 4, 0), "traj:33": (299, 4, 0), "traj:34": (308, 4, 0), "traj:65": (587, 5, 0),
          "traj:66": (596, 5, 0), "traj:97": (875, 5, 0), "traj:130": (1172, 7, 0), "traj193": (1160, 6, 0), "free65": (587, 4, 0),
          "hard66": (596, 33, 6), "gross80": (722, 6, 0)}


@pytest.mark.parametrize("name", bg.WITH_QR)
def test_scene_takes_its_path(name):
    sc, qr, sch, dist, mask, margin = bg.reference(name)
    M, it, rej = EXPECT[name]
    covisible, every = bg.pairs(sc)
    K = len(sc["poses"])
    free = [k for k in range(K) if not sc["fixed"][k]]
    print("BAG %-9s K %d free %d M %d it %d/%d rejected %d dist %.2e pairs %d/%d outliers %d margin %.2e" % (
        name, K, len(free), len(sc["obs_kf"]), qr["iterations"], sch["iterations"], qr["trace"]["rejected"], dist, len(covisible),
        every, int(mask.sum()), margin))
    assert len(free) == bg.TABLE[name] and len(sc["obs_kf"]) == M
    assert qr["termination"] == sch["termination"] == 0
    assert qr["iterations"] == sch["iterations"] == it
    assert qr["trace"]["rejected"] == sch["trace"]["rejected"] == rej and qr["trace"]["invalid"] == sch["trace"]["invalid"] == 0
    assert dist <= 1e-12                               # 1000 x this is the GPU test's bound
    assert len(covisible) < every                      # a sparse reduced system: blocks that no pair writes
    assert (free[0], free[-1]) in covisible            # the loop: the last keyframes see what the first see
    assert (free[0], free[len(free) // 2]) not in covisible
    if name == "hard66":
        assert qr["trace"]["rejected"] > 0
    if name == "gross80":
        assert int(mask.sum()) == 2 and margin > 1e-6
    else:
        assert not mask.any()
    if name == "free65":
        assert not sc["fixed"].any()


def test_noise_free_300_reaches_the_truth():
    sc, sch = bg.schur_reference("traj300")
    covisible, every = bg.pairs(sc)
    assert len(sc["poses"]) == 300 and len(sc["obs_kf"]) == 1802 and len(covisible) < every // 20
    assert sch["termination"] == 0 and sch["iterations"] == 9
    err = max(np.max(np.abs(sch["poses"] - sc["truth_poses"])), np.max(np.abs(sch["landmarks"] - sc["truth_landmarks"])))
    assert err <= 1e-7


def test_header_declares_the_entry_point_and_the_bound():
    hdr = open(os.path.join(ROOT, "include", "mslam_hip.h")).read()
    assert re.search(r"^#define MSLAM_HIP_BA_GLOBAL_MAX_KEYFRAMES 1024$", hdr, re.M)
    assert re.search(r"^int mslam_hip_bundle_adjust_global\(mslam_hip_ctx\* ctx,", hdr, re.M)
    assert re.search(r"^#define MSLAM_HIP_ABI_VERSION 5$", hdr, re.M)      # an addition: the version stays


def test_library_exports_the_entry_point(pkg):
    assert "mslam_hip_bundle_adjust_global" in pkg.ABI_SYMBOLS
    assert getattr(pkg.lib(), "mslam_hip_bundle_adjust_global")
    assert pkg.lib().mslam_hip_abi_version() == 5
    assert hasattr(pkg.Context, "bundle_adjust_global")


def test_backend_capacity_is_checked_before_the_context_is_touched(pkg):
    be = pkg.HipBackend(None, global_solver=True)
    for id in range(1025):
        be.add_keyframe(id, [0, 0, 0, 1, 0, 0, 0], [], np.zeros((0, 3)))
    with pytest.raises(pkg.MslamHipError) as e:
        be.global_ba()                                  # there is no context: touching it would be an AttributeError
    assert e.value.code == pkg.E_CAPACITY
    assert be.neighbours(0, {0: set(range(1, 1025))}) == list(range(1025 - 64, 1025))      # local_ba's rule is unchanged
    be = pkg.HipBackend(None)
    for id in range(65):
        be.add_keyframe(id, [0, 0, 0, 1, 0, 0, 0], [], np.zeros((0, 3)))
    with pytest.raises(pkg.MslamHipError) as e:
        be.global_ba()
    assert e.value.code == pkg.E_CAPACITY
    assert pkg.HipBackend.MAX_KEYFRAMES == 64
