"""The CPU side of mslam_hip_set_ba_global_pcg: tests/ba_global_pcg_ref.py (the Levenberg-Marquardt loop of
tests/ba_global_sparse_ref.py with an explicit Schur complement and block-Jacobi PCG) pinned to the direct references at a
tight tolerance, the ground the solver is for (revisit:1900: above the envelope bound, few pairs) through the library's
symbolic phase, the header's constants, and the argument checks of HipBackend that need no context."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_global_cases as bg  # noqa: E402
import ba_global_pcg_cases as pc  # noqa: E402
import ba_global_pcg_ref as pr  # noqa: E402
import ba_global_sparse_cases as bc  # noqa: E402
import ba_global_sparse_ref as bs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIGHT = dict(cg_max_iterations=2000, cg_tolerance=1e-12)


@pytest.mark.parametrize("name", bg.WITH_QR + bc.NEW)
def test_tight_pcg_reference_is_the_direct_reference(name):
    """tolerance 1e-12: the decisions of the direct solve, iteration for iteration, and a state within max(1e-9, 1000 x the
    distance of the two direct solvers); no solve at the cap of 2000, none broken down"""
    sc, ref, dist, mask = pc.direct_reference(name)
    sc, got = pc.pcg_reference(name, **TIGHT)
    d = bs.distance(got, ref)
    print("PCG ref %-20s it %d/%d term %d/%d CG max %d total %d  d %.3e dist %.3e" % (
        name, got["iterations"], ref["iterations"], got["termination"], ref["termination"], max(got["cg"], default=0), sum(got["cg"]), d, dist))
    assert got["termination"] == ref["termination"] and got["iterations"] == ref["iterations"]
    for k in ("rejected", "accepted_after_rejected", "invalid", "dbl_max", "free_poses", "landmarks"):
        assert got["trace"][k] == ref["trace"][k], k
    if "steps" in ref["trace"]:
        assert got["trace"]["steps"] == ref["trace"]["steps"]
    assert d <= max(1e-9, 1000.0 * dist)
    # the longest solve: 517 CG iterations on traj:130, 954 on traj193 (rings cost about 4 to 5 iterations per keyframe),
    # both inside the tight tier's cap of 2000
    assert got["at_cap"] == 0 and got["breakdowns"] == 0 and max(got["cg"], default=0) < TIGHT["cg_max_iterations"] // 2
    assert len(got["cg"]) == got["iterations"]
    assert abs(got["final_cost"] - ref["final_cost"]) <= 1e-9 * ref["final_cost"]


def test_pcg_of_the_reference_against_a_dense_solve():
    """the CG routine alone: a random block system, against numpy's solve; b = 0; the cap; a breakdown"""
    import scipy.sparse as sp
    rng = np.random.default_rng(3)
    n = 6 * 7
    A = rng.normal(size=(n, n))
    S = sp.csr_matrix(A @ A.T + n * np.eye(n))
    b = rng.normal(size=n)
    y, its, end = pr.pcg(S, b, 500, 1e-12)
    assert end == "converged" and 0 < its <= n + 5
    assert np.max(np.abs(y - np.linalg.solve(S.toarray(), b))) <= 1e-12
    y, its, end = pr.pcg(S, np.zeros(n), 500, 1e-6)
    assert (its, end) == (0, "converged") and not y.any()
    y, its, end = pr.pcg(S, b, 2, 1e-12)
    assert (its, end) == (2, "cap") and np.all(np.isfinite(y))
    y, its, end = pr.pcg(sp.csr_matrix(np.eye(n) - 2.0 * np.outer(b, b) / (b @ b) + 1e-3 * np.diag(np.arange(n))), b, 50, 1e-12)
    assert end == "breakdown" and np.all(np.isnan(y))


def test_the_ground_no_other_solver_takes(pkg):
    """revisit:1900: above DENSE's K, above SPARSE's envelope bound in both orders, and about 6 blocks per keyframe"""
    sc = pc.scene("revisit:1900")
    K = len(sc["poses"])
    an = pkg.ba_global_analyze(sc["fixed"], K, sc["obs_kf"], sc["obs_lm"], len(sc["landmarks"]))
    print("revisit:1900 envelope %d (ordering %d) n_pairs %d" % (an["envelope_blocks"], an["ordering"], an["n_pairs"]))
    assert K == 1900 > pkg.BA_GLOBAL_MAX_KEYFRAMES and an["n_free"] == 1899
    assert not an["fits"] and an["envelope_blocks"] > pkg.POSE_GRAPH_MAX_ENVELOPE_BLOCKS
    assert an["n_pairs"] < pkg.POSE_GRAPH_MAX_ENVELOPE_BLOCKS // 50
    small = pc.scene("revisit:130")
    an = pkg.ba_global_analyze(small["fixed"], 130, small["obs_kf"], small["obs_lm"], len(small["landmarks"]))
    assert an["fits"] and an["n_pairs"] == len(bg.pairs(small)[0])
    twin = pc.scene("revisit0:130")
    assert np.array_equal(twin["obs_kf"], small["obs_kf"]) and np.array_equal(twin["obs_lm"], small["obs_lm"])
    assert np.max(np.abs(bs.solve(twin)["poses"] - twin["truth_poses"])) <= 1e-7


def test_exports_and_constants(pkg):
    hdr = open(os.path.join(ROOT, "include", "mslam_hip.h")).read()
    assert re.search(r"^#define MSLAM_HIP_BA_GLOBAL_PCG_MAX_ITERATIONS 500$", hdr, re.M)
    assert re.search(r"^#define MSLAM_HIP_BA_GLOBAL_PCG_TOLERANCE 1e-6$", hdr, re.M)
    assert (pkg.BA_GLOBAL_PCG_MAX_ITERATIONS, pkg.BA_GLOBAL_PCG_TOLERANCE) == (500, 1e-6) == (pr.MAX_ITERATIONS, pr.TOLERANCE)
    for name in ("mslam_hip_set_ba_global_pcg", "mslam_hip_get_ba_global_pcg", "mslam_hip_get_ba_global_pcg_stats"):
        assert name in pkg.ABI_SYMBOLS and name in hdr and hasattr(pkg.lib(), name), name
    fields = re.search(r"typedef struct mslam_hip_pcg_stats\s*\{(.*?)\}", hdr, re.S).group(1)
    assert re.findall(r"int64_t (\w+);", fields) == [k for k, _ in pkg.PcgStats._fields_]
    assert pkg.C.sizeof(pkg.PcgStats) == 40
    assert re.search(r"^#define MSLAM_HIP_ABI_VERSION 5$", hdr, re.M) and pkg.lib().mslam_hip_abi_version() == 5


def test_backend_rejects_bad_arguments_before_touching_a_context(pkg):
    for bad in ((0, 1e-6), (-3, 1e-6), (500, 0.0), (500, 1.0), (500, float("nan")), (500, -1e-3), (2.5, 1e-6), (500,), "cg", (2 ** 31, 0.5)):
        with pytest.raises(pkg.MslamHipError) as e:
            pkg.HipBackend(None, global_solver=True, global_pcg=bad)
        assert e.value.code == pkg.E_INVALID, bad
    with pytest.raises(pkg.MslamHipError) as e:
        pkg.HipBackend(None, global_pcg=(500, 1e-6))              # needs global_solver
    assert e.value.code == pkg.E_INVALID
    with pytest.raises(pkg.MslamHipError) as e:
        pkg.HipKeyframeTracker(None, ba_global_pcg=(500, 1e-6))   # needs loop_closure and loop_global_ba
    assert e.value.code == pkg.E_INVALID
    assert pkg.HipBackend(None, global_solver=True).global_pcg is None
    assert pkg.HipBackend(None, global_solver=True, global_pcg=True).global_pcg == (500, 1e-6)
    be = pkg.HipBackend(None, global_solver=True, global_pcg=(40, 1e-3))
    assert be.global_pcg == (40, 1e-3)
    be.poses = {k: None for k in range(pkg.BA_GLOBAL_MAX_KEYFRAMES_SPARSE + 1)}
    with pytest.raises(pkg.MslamHipError) as e:
        be.global_ba()
    assert e.value.code == pkg.E_CAPACITY and "16384" in str(e.value)
