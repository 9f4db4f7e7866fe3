"""The SPARSE global bundle adjustment's CPU side: tests/ba_global_sparse_ref.py (the Levenberg-Marquardt loop of
tests/ba_ref.py on a scipy.sparse Jacobian, two sparse linear solvers) pinned to ba_ref's QR solve on every scene of
ba_global_cases.WITH_QR, and the symbolic phase of the library (ba_global_analyze: no context, no GPU) pinned to the rule
restated in plain Python: the scenes of tests/ba_global_sparse_cases.py, the envelope table of the trajectories, nodes of
degree 0, the argument errors, E_CAPACITY with every output written."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_global_cases as bg  # noqa: E402
import ba_global_sparse_cases as bc  # noqa: E402
import ba_global_sparse_ref as bs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", bg.WITH_QR)
def test_sparse_reference_is_the_dense_reference(name):
    """the same termination, iteration count and per-step decisions; state within max(1e-9, 1000 x |x_schur - x_qr|) of the QR
    solve"""
    sc, qr, sch, dist, mask, margin = bg.reference(name)
    for solver in bs.SOLVERS:
        got = bs.solve(sc, solver)
        assert got["termination"] == qr["termination"] and got["iterations"] == qr["iterations"], solver
        for k in ("rejected", "accepted_after_rejected", "invalid", "dbl_max", "free_poses", "landmarks"):
            assert got["trace"][k] == qr["trace"][k], (solver, k)
        steps = got["trace"]["steps"]
        assert len(steps) == qr["iterations"] and steps.count("rejected") == qr["trace"]["rejected"]
        assert steps.count("invalid") == qr["trace"]["invalid"] and steps.count("converged") <= 1
        assert bs.distance(got, qr) <= max(1e-9, 1000.0 * dist), solver
        assert abs(got["initial_cost"] - qr["initial_cost"]) <= 1e-12 * qr["initial_cost"]
        assert abs(got["final_cost"] - qr["final_cost"]) <= 1e-9 * qr["final_cost"]


def _same_analysis(pkg, sc):
    K = len(sc["poses"])
    got = pkg.ba_global_analyze(sc["fixed"], K, sc["obs_kf"], sc["obs_lm"], len(sc["landmarks"]))
    want = bs.analyze(sc["fixed"], K, sc["obs_kf"], sc["obs_lm"])
    for k in ("n_free", "ordering", "envelope_blocks", "n_pairs", "fits"):
        assert got[k] == want[k], k
    assert got["order"].tolist() == want["order"].tolist() and got["first"].tolist() == want["first"].tolist()
    return got, want


@pytest.mark.parametrize("name", bc.NEW + ["ring:1100", "shuffled:1100", "thin:16384"])
def test_analyze_is_the_rule(pkg, name):
    sc = bc.scene(name)
    got, want = _same_analysis(pkg, sc)
    pairs, _ = bg.pairs(sc) if len(sc["poses"]) <= 1100 else (None, None)
    if pairs is not None:
        assert got["n_pairs"] == len(pairs)                       # the list the DENSE path reads out of its bit table
    if name.startswith("shuffled"):
        assert got["ordering"] == bs.RCM and want["natural_blocks"] > 2 * want["rcm_blocks"]
    if name == "loop_row":                                        # the late keyframe's row reaches back to keyframe 1
        assert got["ordering"] == bs.NATURAL and got["order"][-1] == 40 and got["first"][-1] == 0
        assert got["envelope_blocks"] > got["n_pairs"]            # fill-in inside it
    if name == "complete12":
        assert got["envelope_blocks"] == got["n_pairs"] == 11 * 12 // 2
    if name == "two_rings":
        assert got["n_free"] == 19 and got["first"].tolist()[10] == 10       # no block joins the two components


# measured with the pose graph's rule on the covisibility edges; both rules agree when no node is isolated
TABLE = {"traj:9": (27, 26, bs.RCM), "traj:66": (277, 476, bs.NATURAL), "traj193": (844, 1548, bs.NATURAL),
         "ring:1100": (4424, 5762, bs.NATURAL)}


@pytest.mark.parametrize("name", list(TABLE))
def test_envelope_table(pkg, name):
    sc = bc.scene(name)
    got, want = _same_analysis(pkg, sc)
    natural, rcm, chosen = TABLE[name]
    assert (want["natural_blocks"], want["rcm_blocks"]) == (natural, rcm)
    assert got["ordering"] == chosen and got["envelope_blocks"] == min(natural, rcm) and got["fits"]
    if name == "ring:1100":
        assert sc["poses"].shape == bg.trajectory(1100, 2, 3, 1100)["poses"].shape and got["n_free"] == 1099


def test_a_node_of_degree_0_is_a_row(pkg):
    """unlike in the pose graph: a free keyframe that shares no landmark with another free keyframe keeps its row; under RCM
    the nodes of degree 0 start first and end last"""
    for name in ("isolated", "fixed_only_partner"):
        sc = bc.scene(name)
        got, want = _same_analysis(pkg, sc)
        assert got["n_free"] == 12 and got["order"].tolist()[-1] == 12 and got["first"].tolist()[-1] == 11
    # a hub with the smallest index: RCM wins, and the two keyframes without a partner end last, the larger index first
    kf = [0, 1, 0, 2, 0, 3, 0, 4, 5, 6, 7, 7]
    lm = [0, 0, 1, 1, 2, 2, 3, 3, 4, 5, 6, 6]
    fixed = np.zeros(8, np.uint8)
    fixed[7] = 1
    got = pkg.ba_global_analyze(fixed, 8, kf, lm)
    want = bs.analyze(fixed, 8, kf, lm)
    assert got["ordering"] == want["ordering"] == bs.RCM and got["n_free"] == 7
    assert got["order"].tolist() == want["order"].tolist() and got["order"].tolist()[-2:] == [6, 5]
    assert got["first"].tolist() == want["first"].tolist() and got["first"].tolist()[-2:] == [5, 6]
    assert got["n_pairs"] == 7 + 4
    # only constant or unobserved keyframes: no node
    got = pkg.ba_global_analyze(np.ones(3, np.uint8), 3, [0, 1, 2], [0, 0, 0])
    assert got["n_free"] == 0 and got["envelope_blocks"] == 0 and got["n_pairs"] == 0 and got["fits"]
    got = pkg.ba_global_analyze(None, 5, [], [])
    assert got["n_free"] == 0 and got["n_pairs"] == 0
    # a landmark twice in a keyframe joins nothing new; a keyframe without an observation is no node
    got = pkg.ba_global_analyze(None, 4, [0, 0, 2, 2], [0, 0, 0, 1])
    assert got["order"].tolist() == [0, 2] and got["first"].tolist() == [0, 0] and got["n_pairs"] == 3


def test_analyze_argument_errors(pkg):
    ok = pkg.ba_global_analyze(None, 3, [0, 1, 1, 2], [0, 0, 1, 1])
    assert ok["n_free"] == 3 and ok["envelope_blocks"] == 5 and ok["n_pairs"] == 5
    for K, kf, lm, L in ((3, [0, 3], [0, 0], 1), (3, [0, -1], [0, 0], 1), (3, [0, 1], [0, 1], 1), (3, [0, 1], [0, -1], 1), (-1, [], [], 0),
                         (pkg.BA_GLOBAL_MAX_KEYFRAMES_SPARSE + 1, [0], [0], 1), (3, [0], [0], (1 << 24) + 1), (3, [0], [0], -1)):
        with pytest.raises(pkg.MslamHipError) as e:
            pkg.ba_global_analyze(None, K, kf, lm, L)
        assert e.value.code == pkg.E_INVALID, (K, kf, lm, L)
    with pytest.raises(pkg.MslamHipError) as e:
        pkg.ba_global_analyze(None, 3, [0, 1], [0])
    assert e.value.code == pkg.E_INVALID
    with pytest.raises(pkg.MslamHipError) as e:
        pkg.ba_global_analyze(np.zeros(4, np.uint8), 3, [0], [0])
    assert e.value.code == pkg.E_INVALID
    big = pkg.BA_GLOBAL_MAX_KEYFRAMES_SPARSE
    edge = pkg.ba_global_analyze(None, big, [0, big - 1], [0, 0])           # K at the bound: two nodes, one block below the diagonal
    assert edge["order"].tolist() == [0, big - 1] and edge["envelope_blocks"] == 3
    # nothing is written on E_INVALID; every output may be NULL
    lib, n = pkg.lib(), pkg.C.c_int(-7)
    kf, lm = np.array([0, 5], np.int32), np.array([0, 0], np.int32)
    assert lib.mslam_hip_bundle_adjust_global_analyze(None, 3, pkg._p(kf), pkg._p(lm), 2, 1, None, None, pkg.C.byref(n), None, None, None) == pkg.E_INVALID
    assert n.value == -7
    kf[1] = 2
    assert lib.mslam_hip_bundle_adjust_global_analyze(None, 3, pkg._p(kf), pkg._p(lm), 2, 1, None, None, None, None, None, None) == pkg.OK


def test_capacity_with_every_output_written(pkg):
    """one landmark 1500 keyframes see: both orders give the whole triangle, 1500 x 1501 / 2 blocks, above the bound"""
    sc = bc.scene("wide:1500")
    got, want = _same_analysis(pkg, sc)
    assert not got["fits"] and want["natural_blocks"] == want["rcm_blocks"] == 1500 * 1501 // 2 > pkg.POSE_GRAPH_MAX_ENVELOPE_BLOCKS
    assert got["envelope_blocks"] == 1500 * 1501 // 2 and got["ordering"] == bs.NATURAL and got["n_free"] == 1500
    assert got["order"].tolist() == list(range(1500)) and not got["first"].any() and got["n_pairs"] == 1500 * 1501 // 2
    blocks = pkg.C.c_int64(0)
    rc = pkg.lib().mslam_hip_bundle_adjust_global_analyze(None, 1500, pkg._p(sc["obs_kf"]), pkg._p(sc["obs_lm"]), 1500, 1, None, None, None,
                                                          None, pkg.C.byref(blocks), None)
    assert rc == pkg.E_CAPACITY and blocks.value == 1500 * 1501 // 2


def test_exports_and_abi(pkg):
    hdr = open(os.path.join(ROOT, "include", "mslam_hip.h")).read()
    assert re.search(r"^#define MSLAM_HIP_ABI_VERSION 5$", hdr, re.M) and pkg.lib().mslam_hip_abi_version() == 5
    assert re.search(r"^#define MSLAM_HIP_BA_GLOBAL_SOLVER_DENSE 0$", hdr, re.M)
    assert re.search(r"^#define MSLAM_HIP_BA_GLOBAL_SOLVER_SPARSE 1$", hdr, re.M)
    assert re.search(r"^#define MSLAM_HIP_BA_GLOBAL_MAX_KEYFRAMES_SPARSE 16384$", hdr, re.M)
    assert re.search(r"^#define MSLAM_HIP_BA_GLOBAL_MAX_KEYFRAMES 1024$", hdr, re.M)
    for name in ("mslam_hip_set_ba_global_solver", "mslam_hip_get_ba_global_solver", "mslam_hip_bundle_adjust_global_analyze"):
        assert name in pkg.ABI_SYMBOLS and name in hdr and hasattr(pkg.lib(), name), name
    assert (pkg.BA_GLOBAL_SOLVER_DENSE, pkg.BA_GLOBAL_SOLVER_SPARSE) == (0, 1)
    assert (pkg.BA_GLOBAL_MAX_KEYFRAMES, pkg.BA_GLOBAL_MAX_KEYFRAMES_SPARSE) == (1024, 16384)
    assert pkg.HipBackend.MAX_GLOBAL_KEYFRAMES_SPARSE == 16384
    with pytest.raises(pkg.MslamHipError) as e:
        pkg.HipBackend(None, global_linear_solver="skyline")
    assert e.value.code == pkg.E_INVALID


@pytest.mark.parametrize("name", bc.RECORDED)
def test_recorded_reference_belongs_to_its_scene(name):
    """the recorded solves carry the digest of the scene this tree builds; the two solvers agree; the noise-free twins are
    at the truth within the project's 1e-7"""
    sc, a, b, dist, truth = bc.recorded(name)
    assert a["poses"].shape == sc["poses"].shape and a["landmarks"].shape == sc["landmarks"].shape
    assert (a["termination"], a["iterations"], a["trace"]["rejected"]) == (b["termination"], b["iterations"], b["trace"]["rejected"])
    assert dist < 1e-10
    if name == "thin:16384":
        assert (a["termination"], a["iterations"]) == (1, 3)        # the iteration cap
    else:
        assert a["termination"] == 0
    if "0:" in name:
        assert truth <= 1e-7
