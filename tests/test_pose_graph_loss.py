"""The loss on the pose graph's edges (mslam_hip_set_pose_graph_loss), on the CPU: the symbols, the restatement
tests/pose_graph_loss_ref.py against its own stated cost and against tests/pose_graph_ref.py, that every scene is what its
name says, and that the restatement alone shows what the loss is for.  The kernels are compared with it in
tests/test_gpu_pose_graph_loss.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_cases as pc  # noqa: E402
import pose_graph_loss_ref as pl  # noqa: E402
import pose_graph_ref as pg  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mslam_hip_set_pose_graph_loss", "mslam_hip_get_pose_graph_loss", "mslam_hip_pose_graph_edge_weights"]


def test_symbols_are_exported_declared_and_listed(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mslam_hip.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "modular-slam_amd", "libmslam_hip.so")]).decode()
    exported = {l.split()[-1] for l in out.splitlines()}
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in pkg.ABI_SYMBOLS and name in exported and hasattr(pkg.lib(), name), name
    assert pkg.lib().mslam_hip_abi_version() == 5
    assert (pkg.BA_LOSS_NONE, pkg.BA_LOSS_HUBER, pkg.BA_LOSS_CAUCHY) == (pl.NONE, pl.HUBER, pl.CAUCHY) == (0, 1, 2)
    assert not re.search(r"#define\s+MSLAM_HIP_(PG|POSE_GRAPH|PNP)\w*LOSS", hdr)          # no second set of numbers
    for name in ("set_pose_graph_loss", "get_pose_graph_loss", "pose_graph_edge_weights"):
        assert callable(getattr(pkg.Context, name))
    import inspect
    assert "pose_graph_loss" in inspect.signature(pkg.HipBackend.__init__).parameters
    assert "pose_graph_loss" in inspect.signature(pkg.HipKeyframeTracker.__init__).parameters


def test_loss_formulas():
    a = 0.5
    s = np.array([0.0, 0.1, 0.25, np.nextafter(0.25, 1.0), 4.0, 1e300])
    rho, w = pl.loss(pl.HUBER, a, s)
    assert rho[:3].tolist() == s[:3].tolist() and w[:3].tolist() == [1.0, 1.0, 1.0]        # s == b is the inlier branch
    assert rho[3] < s[3] and rho[4] == 2.0 * a * 2.0 - 0.25 and w[4] == a / 2.0       # one ulp above b: the other branch
    rho, w = pl.loss(pl.CAUCHY, a, s)
    assert rho[0] == 0.0 and w[0] == 1.0 and rho[4] == 0.25 * np.log(17.0) and w[4] == 1.0 / 17.0
    assert np.all(np.diff(w) <= 0.0) and w[-1] > 0.0
    assert pl.loss(pl.HUBER, a, np.inf)[1] == pl.DBL_MIN and pl.loss(pl.CAUCHY, a, np.inf)[1] == pl.DBL_MIN
    assert np.isnan(pl.loss(pl.HUBER, a, np.nan)[0]) and np.isnan(pl.loss(pl.CAUCHY, a, np.nan)[0])


@pytest.mark.parametrize("name", ["chain:9", "info_upper", "rejected", "duplicates"])
@pytest.mark.parametrize("solver", ["qr", "chol"])
def test_without_a_loss_it_is_pose_graph_ref_bit_for_bit(name, solver):
    sc = pc.scene(name)
    a, b = pc.solve(sc, solver), pl.solve(sc, solver, None)
    assert a["poses"].tobytes() == b["poses"].tobytes()
    for k in ("termination", "iterations", "reason"):
        assert a[k] == b[k]
    for k in ("initial_cost", "final_cost"):
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes()
    for k in ("rejected", "invalid", "dbl_max", "free_poses"):
        assert a["trace"][k] == b["trace"][k]


@pytest.mark.parametrize("name", ["dup3", "to_fixed", "info_dense", "false:12,4,1,1"])
@pytest.mark.parametrize("kind", pl.LOSSES)
def test_gradient_is_the_central_difference_of_half_sum_rho(name, kind):
    """the corrected pair's J^T f against (cost(Plus(x, h e_j)) - cost(Plus(x, -h e_j))) / 2 h of 1/2 sum rho, at the start,
    where the bad edges are on Huber's outer branch and the others inside.  h = 1e-6: the truncation term is h^2 times a third
    derivative of order 10, the rounding term eps cost / h = 1e-10 cost"""
    sc = pl.scene(name)
    how = (kind, pl.SCALE)
    x, ea, eb, meas, info = pg._arrays(sc["poses"], sc["edge_a"], sc["edge_b"], sc["edge_meas"], sc["sqrt_info"])
    prob = pl.LossProblem(len(x), ea, eb, meas, info, sc["fixed"].astype(bool), pl.KINDS[kind], pl.SCALE)
    ok, c, f, g, J = prob.evaluate(x)
    assert ok and abs(c - pl.cost(x, ea, eb, meas, info, how)) <= 1e-12 * c
    w = pl.weights(x, ea, eb, meas, info, how)
    assert w[sc["bad"]].max() < 1.0
    h = 1e-6
    num = np.zeros(prob.n)
    for j in range(prob.n):
        d = np.zeros(prob.n)
        d[j] = h
        num[j] = (pl.cost(prob.plus(x, d), ea, eb, meas, info, how) - pl.cost(prob.plus(x, -d), ea, eb, meas, info, how)) / (2.0 * h)
    assert np.max(np.abs(num - g)) <= 1e-6 * max(1.0, float(np.max(np.abs(g)))), np.max(np.abs(num - g))


def test_every_scene_is_what_its_name_says():
    bad_far = lambda sc: pl.chi2(sc["truth_poses"], sc["edge_a"], sc["edge_b"], sc["edge_meas"], None)
    for name in pl.SCENES:
        sc = pl.scene(name)
        E = len(sc["edge_a"])
        s = bad_far(sc)
        good = np.setdiff1d(np.arange(E), sc["bad"])
        # at the truth a bad edge is off by 1.5 m and 0.6 rad, a good one by the noise: 0.01 m and 0.01 rad
        assert s[sc["bad"]].min() > 1.0 and (len(good) == 0 or s[good].max() < 0.01), name
        assert sc["fixed"].sum() == 1 and len(sc["poses"]) <= 80, name
    assert len(pl.scene("one")["edge_a"]) == 1
    for E in (255, 256, 257):
        sc = pl.scene("edges:%d" % E)
        assert len(sc["edge_a"]) == E and sc["bad"][-1] == E - 1 and (256 in sc["bad"]) == (E > 256)
    assert (257 + 255) // 256 == 2 and 257 % 256 == 1                   # a tail block of one edge, and it is bad
    hub = pl.scene("hub")
    ends = np.stack([hub["edge_a"], hub["edge_b"]], 1)
    inc = np.flatnonzero((ends == 0).any(1))                            # the hub's incidence list, in edge order
    assert len(inc) == 70 and inc.tolist() == list(range(70)) and not hub["fixed"][0]
    assert all(np.searchsorted(inc, e) >= 64 for e in hub["bad"]) and len(hub["bad"]) == 3
    d = pl.scene("dup3")
    same = [e for e in range(len(d["edge_a"])) if (d["edge_a"][e], d["edge_b"][e]) == (1, 2)]
    assert same == [1, 2, 3] and d["bad"].tolist() == [2]
    t = pl.scene("to_fixed")
    e = int(t["bad"][0])
    assert t["fixed"][t["edge_a"][e]] == 1 and t["fixed"][t["edge_b"][e]] == 0
    i = pl.scene("info_dense")
    assert not i["sqrt_info"][-1].any() and not i["sqrt_info"][2, 3:].any() and i["sqrt_info"][0, 3:].any()
    s = pl.chi2(i["poses"], i["edge_a"], i["edge_b"], i["edge_meas"], i["sqrt_info"])
    assert s[-1] == 0.0
    for kind in pl.LOSSES:                                              # s = 0: w = 1 and rho = 0, no 0 / 0
        rho, w = pl.loss(pl.KINDS[kind], pl.SCALE, s[-1])
        assert rho == 0.0 and w == 1.0
    for name, (K, n_true, n_false) in {"false:12,4,1,1": (12, 4, 1), "false:40,10,3,2": (40, 10, 3), "false:70,12,3,5": (70, 12, 3)}.items():
        sc = pl.scene(name)
        E = K - 1 + n_true + n_false
        assert len(sc["poses"]) == K and len(sc["edge_a"]) == E and sc["bad"].tolist() == list(range(E - n_false, E))
        assert [(a, b) for a, b in zip(sc["edge_a"][:K - 1], sc["edge_b"][:K - 1])] == [(k, k + 1) for k in range(K - 1)]
        assert np.all(np.abs(sc["edge_b"][K - 1:] - sc["edge_a"][K - 1:]) >= 3)


@pytest.mark.parametrize("name", list(pl.SCENES))
@pytest.mark.parametrize("kind", pl.LOSSES)
def test_the_two_solvers_agree_and_no_step_is_invalid(name, kind):
    sc, qr, ch, dist = pl.reference(name, kind)
    assert qr["termination"] == ch["termination"] == pg.CONVERGENCE and qr["iterations"] == ch["iterations"]
    assert dist <= 1e-12 and qr["trace"]["invalid"] == ch["trace"]["invalid"] == 0
    # two states 1e-12 apart at a minimum differ in cost by the second-order term (tests/test_gpu_pose_graph.py's rule)
    second_order = len(sc["edge_a"]) * (pc.jacobian_row_bound(sc) * 1e-12) ** 2 / 2.0
    assert abs(qr["final_cost"] - ch["final_cost"]) <= 1e-12 * qr["final_cost"] + second_order
    how = (kind, pl.SCALE)
    assert abs(qr["final_cost"] - pl.cost(qr["poses"], sc["edge_a"], sc["edge_b"], sc["edge_meas"], sc["sqrt_info"], how)) <= 1e-12 * qr["final_cost"] + 1e-300
    assert qr["final_cost"] <= qr["initial_cost"]


@pytest.mark.parametrize("name", list(pl.FALSE_LOOPS))
def test_what_it_is_for_holds_in_the_restatement_alone(name):
    """with each loss the largest position error against the truth is below the one without; under Cauchy every false
    edge's weight at the solution is below every other edge's"""
    sc, none = pl.reference(name, "none")[:2]
    err0 = pl.position_error(sc, none["poses"])
    for kind in pl.LOSSES:
        qr = pl.reference(name, kind)[1]
        err = pl.position_error(sc, qr["poses"])
        w = pl.weights(qr["poses"], sc["edge_a"], sc["edge_b"], sc["edge_meas"], sc["sqrt_info"], (kind, pl.SCALE))
        others = np.setdiff1d(np.arange(len(w)), sc["bad"])
        print("%s %s: error %.3g (none %.3g), false w <= %.3g, others w >= %.3g, %d iterations" % (
            name, kind, err, err0, w[sc["bad"]].max(), w[others].min(), qr["iterations"]))
        assert err < err0
        if kind == "cauchy":
            assert w[sc["bad"]].max() < w[others].min()


def test_threshold_scene_sits_on_hubers_branch_point():
    sc = pl.threshold_scene()
    a = pl.THRESHOLD_A
    s = pl.chi2(sc["poses"], sc["edge_a"], sc["edge_b"], sc["edge_meas"])
    assert s.tolist() == [a * a]
    at = pl.solve(sc, "qr", ("huber", a))
    below = pl.solve(sc, "qr", ("huber", np.nextafter(a, 0.0)))
    assert at["initial_cost"] == a * a / 2.0
    b = np.nextafter(a, 0.0) ** 2
    assert below["initial_cost"] == 0.5 * (2.0 * np.nextafter(a, 0.0) * np.sqrt(s[0]) - b) and b < s[0]
