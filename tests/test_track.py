"""The keyframe tracking step without a GPU: the library exports the two calls, and the numpy reference of tests/track_ref.py
(the composition the GPU tests compare against) is itself right on a synthetic sequence with known poses."""
import ctypes
import os
import re

import numpy as np
import pytest

import track_ref as tr
from reloc_ref import po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# where the reference loop inserts keyframes / changes its reference without inserting one on make_sequence(seed=0):
# the camera slides out (keyframes when fewer than 100 inliers remain) and back (older keyframes see more again)
EXPECTED_KEYFRAMES = [0, 6, 11, 30]
EXPECTED_SWITCHES = [25]


@pytest.fixture(scope="module")
def sequence(orc):
    seq = tr.make_sequence(seed=0)
    rows, trk = tr.run_reference(seq)
    return seq, rows, trk


def test_library_exports_the_tracking_calls_and_keeps_its_abi_version(pkg):
    """(the shared object is cross-compiled: loading it by ctypes needs no GPU)"""
    assert {"mslam_hip_kf_visible", "mslam_hip_track"} <= set(pkg.ABI_SYMBOLS)
    text = open(os.path.join(ROOT, "include", "mslam_hip.h")).read()
    for name in ("mslam_hip_kf_visible", "mslam_hip_track"):
        assert re.search(r"^int %s\(" % name, text, re.M), name
    assert re.search(r"#define MSLAM_HIP_ABI_VERSION 5\b", text)
    try:
        L = pkg.lib()
    except OSError as e:                      # no HIP runtime to resolve against on this host: the symbol table still tells
        import subprocess
        syms = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH]).decode()
        assert " mslam_hip_kf_visible" in syms and " mslam_hip_track" in syms, e
        return
    assert L.mslam_hip_kf_visible and L.mslam_hip_track
    assert L.mslam_hip_abi_version() == 5
    assert ctypes.sizeof(pkg.TrackResult) == 4 * 4 + 15 * 8 + 7 * 4 + 4      # the header's struct, padded to 8 bytes


def test_reference_recovers_the_noise_free_sequence(sequence):
    seq, rows, _ = sequence
    for f, r in enumerate(rows):
        print(f, "tracked", r["tracked"], "inliers", r["n_inliers"], "reference", r["reference"], "keyframe", r["keyframe"],
              "error %.5f deg %.6f m" % (r["err_deg"], r["err_m"]))
    assert all(r["tracked"] for r in rows)
    assert max(r["err_deg"] for r in rows) < 0.1 and max(r["err_m"] for r in rows) < 0.02


def test_reference_inserts_keyframes_and_switches_its_reference(sequence):
    _, rows, trk = sequence
    tracked, inserted, switched = tr.summarize(rows)
    assert inserted == EXPECTED_KEYFRAMES and switched == EXPECTED_SWITCHES
    assert len(inserted) >= 3 and len(switched) >= 1            # at least two keyframes after the first, one switch
    assert not any(r["relocalized"] for r in rows)
    # a keyframe goes in exactly when fewer than new_keyframe_min_landmarks inliers remain
    for f, r in enumerate(rows[1:], 1):
        assert (r["keyframe"] >= 0) == (r["n_inliers"] < tr.SEQ_PARAMS["new_keyframe_min_landmarks"]), f
    assert trk.ids == [0, 1, 2, 3]


def test_vote_hand_cases():
    cam = (500.0, 500.0, 320.0, 240.0)
    R, t = np.eye(3), np.zeros(3)
    pts = np.array([[0.0, 0.0, 2.0],          # the principal point: visible
                    [0.0, 0.0, -2.0],         # behind the camera: u, v inside, c2 < 0
                    [-1.28, 0.0, 2.0],        # u = -0.64 * 500 + 320 = 0 exactly: visible (u >= 0)
                    [1.28, 0.0, 2.0],         # u = 640 = width exactly: not visible (u < width)
                    [0.0, -0.96, 2.0],        # v = 0 exactly: visible
                    [0.0, 0.96, 2.0],         # v = 480 = height exactly: not visible
                    [0.0, 0.0, 0.0]])         # c2 = 0: 0 / 0, nothing compares true
    u = (pts[:, 0] / np.where(pts[:, 2] == 0, 1, pts[:, 2])) * 500.0 + 320.0
    assert u[2] == 0.0 and u[3] == 640.0                            # the cases are exact in f64
    assert tr.visible(pts, R, t, cam).tolist() == [True, False, True, False, True, False, False]
    store = {1: (None, pts), 2: (None, pts[:1]), 3: (None, np.empty((0, 3))), 4: (None, pts[[0, 2, 4]])}
    counts, best = tr.vote(store, [3, 2, 1, 4], R, t, cam)
    assert counts.tolist() == [0, 1, 3, 3] and best == 2            # the first maximum in list order
    assert tr.vote(store, [4, 1], R, t, cam)[1] == 0
    assert tr.vote(store, [], R, t, cam)[1] == -1
    assert tr.vote(store, [3], R, t, cam)[1] == 0                  # an entry without landmarks still wins a list of one
    # a pose: the camera one metre to the right sees the u = width point inside
    assert tr.visible(pts[3:4], R, np.array([-1.0, 0.0, 0.0]), cam).tolist() == [True]


def test_entry_construction_parts():
    rng = np.random.default_rng(5)
    n = 12
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    xyz = rng.uniform(-1, 1, (n, 3)) + [0, 0, 2.0]
    valid = np.ones(n, bool)
    valid[[3, 9]] = False                       # 3 is matched, 9 is not: neither can be lifted
    xyz[10, 2] = 3.5                            # beyond z_max
    ref_world = rng.normal(size=(8, 3))
    # matches in `to` order: keypoints 5, 3, 7, 1, 11 against landmarks 0, 2, 4, 6, 7
    pairs = (np.array([5, 3, 7, 1, 11], np.int32), np.array([0, 2, 4, 6, 7], np.int32))
    mask = np.array([True, False, True, True])  # over the correspondences 5, 7, 1, 11: keypoint 7 is a PnP outlier
    R, t = po.rodrigues([0.1, -0.2, 0.05]), np.array([0.3, -0.1, 0.2])
    e = tr.build_entry(desc, xyz, valid, pairs, mask, ref_world, R, t, 3.0)
    assert e["n_inherited"] == 3
    assert e["kp"].tolist() == [5, 1, 11, 0, 2, 4, 6, 8]          # part A in correspondence order, part B in keypoint order
    assert e["src"].tolist() == [0, 6, 7, -1, -1, -1, -1, -1]
    a, b = set(e["kp"][:3].tolist()), set(e["kp"][3:].tolist())
    assert not a & b and 7 not in a | b                            # disjoint; the outlier with a valid depth is in neither
    assert 3 not in a | b and 9 not in a | b and 10 not in a | b
    assert np.array_equal(e["desc"], desc[e["kp"]])
    assert np.array_equal(e["world"][:3], ref_world[[0, 6, 7]])    # inherited as they are
    want = (xyz[e["kp"][3:]] - t) @ R                              # R^T (p - t)
    assert np.abs(e["world"][3:] - want).max() < 1e-14
    # the lift inverts the pose: the lifted points project back onto their camera points
    assert np.abs(e["world"][3:] @ R.T + t - xyz[e["kp"][3:]]).max() < 1e-14


def test_step_below_min_matched_points_is_not_tracked(sequence):
    seq, _, trk = sequence
    fr = seq["frames"][1]
    s = tr.track(fr["desc"], fr["xy"], fr["depth"], trk.store, 0, [0], min_matched_points=100000)
    assert not s["tracked"] and not s["keyframe_required"] and s["entry"] is None and s["vote_best"] == -1
    assert s["status"] == 1 and s["n_correspondences"] > 100
