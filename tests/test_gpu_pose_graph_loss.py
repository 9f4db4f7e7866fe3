"""The loss on the pose graph's edges on the MI355X (mslam_hip_set_pose_graph_loss: k_pg_edges_loss, k_pg_eval_loss,
k_pg_edge_weights in k_posegraph.hip) through Context.pose_graph with both linear solvers, against
tests/pose_graph_loss_ref.py's QR solve on its scenes (tests/test_pose_graph_loss.py shows on the CPU that every scene is what
its name says and that the restatement alone meets the inequalities asked here).

Bounds: the rule of tests/test_gpu_pose_graph.py, unchanged.  State: |x_gpu - x_qr|_inf <= max(1e-9, 1000 |x_chol - x_qr|_inf),
quaternions compared up to sign.  Costs: 1e-6 relative, plus at the final state the second-order term that file derives, E (J
B)^2 / 2 with J = pose_graph_cases.jacobian_row_bound (a corrected row is a row times sqrt(w) <= 1, so J holds with a loss).
Same termination and iteration count, no invalid step.  The exact checks are derived, not measured: sqrt(1.0) is 1.0 and a
product with 1.0 keeps its bits, so a Huber loss that no edge reaches is the solve without a loss, byte for byte."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth  # noqa: E402  (tools/, on the path through conftest.py)

import ba_cases  # noqa: E402
import loop_walk  # noqa: E402
import pose_graph_cases as pc  # noqa: E402
import pose_graph_loss_ref as pl  # noqa: E402
import track_ref as tr  # noqa: E402

pytestmark = pytest.mark.gpu
SOLVERS = ("dense", "sparse")


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(width=0, height=0)
    yield c
    c.close()


def _solve(ctx, sc, how=None, solver="dense", **over):
    a = dict(sc)
    a.update(over)
    ctx.set_pose_graph_solver(solver)
    ctx.set_pose_graph_loss(*(how or ("none",)))
    try:
        return ctx.pose_graph(a["poses"], a["edge_a"], a["edge_b"], a["edge_meas"], a["sqrt_info"], a["fixed"],
                              max_iterations=a.get("max_iterations", 100))
    finally:
        ctx.set_pose_graph_loss("none")
        ctx.set_pose_graph_solver("dense")


def _weights(ctx, sc, poses, how=None):
    ctx.set_pose_graph_loss(*(how or ("none",)))
    try:
        return ctx.pose_graph_edge_weights(poses, sc["edge_a"], sc["edge_b"], sc["edge_meas"], sc["sqrt_info"])
    finally:
        ctx.set_pose_graph_loss("none")


def _same_bits(a, b):
    assert a["poses"].tobytes() == b["poses"].tobytes()
    for k in ("termination", "iterations", "rejected_steps", "invalid_steps", "n_outliers"):
        assert a[k] == b[k], k
    for k in ("initial_cost", "final_cost"):
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), k


def _check_weights(chi2, weight, sc, poses, how):
    """chi2 against the restatement's at the same poses: 1e-12 relative, plus what the number format leaves of a residual that
    is itself a difference of metres: a component of r_e is formed from p_b - p_a, p_meas and unit quaternions with an absolute
    error d = 8 ulp of (|p_b - p_a| + |p_meas| + 2), times sqrt_info's largest absolute row sum, on either side, and |r|^2 then
    moves by 2 |r| d + d^2.  At an edge the solve has fitted (|r| = 1e-8) that term is all there is; at an edge of the noise's
    size (|r| = 0.1) it is a third of the relative one.  The weights follow from chi2 by the formula: a / sqrt(s) and
    1 / (1 + s (1 / b)) are two and three correctly rounded operations on both sides, 4 ulp covers a library that is not"""
    want = pl.chi2(poses, sc["edge_a"], sc["edge_b"], sc["edge_meas"], sc["sqrt_info"])
    assert chi2.shape == weight.shape == want.shape
    x = np.asarray(poses, np.float64)
    extent = np.linalg.norm(x[sc["edge_b"], 4:] - x[sc["edge_a"], 4:], axis=1) + np.linalg.norm(sc["edge_meas"][:, 4:], axis=1) + 2.0
    rows = 1.0 if sc["sqrt_info"] is None else np.max(np.sum(np.abs(sc["sqrt_info"]), 2), 1)
    d = 8.0 * np.finfo(np.float64).eps * extent * rows
    slack = 1e-12 * want + 2.0 * np.sqrt(want) * d + d * d
    assert np.all(np.abs(chi2 - want) <= slack), float(np.max(np.abs(chi2 - want) / np.maximum(slack, 1e-300)))
    if how is None:
        assert np.all(weight == 1.0)
        return
    w = pl.loss(pl.KINDS[how[0]], how[1], chi2)[1]
    assert np.all(np.abs(weight - w) <= 4.0 * np.finfo(np.float64).eps * w) and np.all(weight > 0.0) and np.all(weight <= 1.0)


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("kind", pl.LOSSES)
@pytest.mark.parametrize("name", list(pl.SCENES))
def test_against_the_qr_reference(ctx, name, kind, solver):
    sc, qr, ch, dist = pl.reference(name, kind)
    how = (kind, pl.SCALE)
    got = _solve(ctx, sc, how, solver)
    bound = max(1e-9, 1000.0 * dist)
    dx = pc.same_rotation_distance(got["poses"], qr["poses"])
    second_order = len(sc["edge_a"]) * (pc.jacobian_row_bound(sc) * bound) ** 2 / 2.0
    print("PGL %-16s %-6s %-6s term %d/%d it %d/%d rejected %d/%d cost0 %.17g/%.17g cost %.9g/%.9g dx %.3e bound %.3e" % (
        name, kind, solver, got["termination"], qr["termination"], got["iterations"], qr["iterations"], got["rejected_steps"],
        qr["trace"]["rejected"], got["initial_cost"], qr["initial_cost"], got["final_cost"], qr["final_cost"], dx, bound))
    assert got["termination"] == qr["termination"]
    assert got["iterations"] == qr["iterations"]
    assert got["invalid_steps"] == 0 and got["n_outliers"] == 0
    assert abs(got["initial_cost"] - qr["initial_cost"]) <= 1e-6 * qr["initial_cost"]
    assert abs(got["final_cost"] - qr["final_cost"]) <= 1e-6 * qr["final_cost"] + second_order
    assert dx <= bound
    assert np.all(np.isfinite(got["poses"])) and np.isfinite(got["final_cost"])
    start = np.asarray(sc["poses"], np.float64)
    for k in np.flatnonzero(sc["fixed"]):                     # a constant pose comes back bit for bit
        assert got["poses"][k].tobytes() == start[k].tobytes(), k
    # the weights, at the input poses and at the result
    for poses in (start, got["poses"]):
        chi2, weight = _weights(ctx, sc, poses, how)
        _check_weights(chi2, weight, sc, poses, how)
    if name == "info_dense":                                  # the edge whose sqrt_info is zero: s = 0 gives w = 1
        assert chi2[-1] == 0.0 and weight[-1] == 1.0
    _same_bits(got, _solve(ctx, sc, how, solver))             # two calls return the same bits


@pytest.mark.parametrize("name", list(pl.FALSE_LOOPS))
def test_what_it_is_for(ctx, name):
    """a graph with false loop edges: with each loss the largest position error against the truth is below the one without
    (no factor is fixed), and under Cauchy every false edge's weight at the result is below every other edge's"""
    sc = pl.scene(name)
    for solver in SOLVERS:
        err0 = pl.position_error(sc, _solve(ctx, sc, None, solver)["poses"])
        for kind in pl.LOSSES:
            how = (kind, pl.SCALE)
            got = _solve(ctx, sc, how, solver)
            err = pl.position_error(sc, got["poses"])
            chi2, weight = _weights(ctx, sc, got["poses"], how)
            others = np.setdiff1d(np.arange(len(weight)), sc["bad"])
            print("PGL %s %s %s: error %.3g (none %.3g), false w <= %.3g, others w >= %.3g, %d iterations" % (
                name, kind, solver, err, err0, weight[sc["bad"]].max(), weight[others].min(), got["iterations"]))
            assert got["termination"] == 0 and err < err0
            if kind == "cauchy":
                assert weight[sc["bad"]].max() < weight[others].min()


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", ["edges:257", "hub", "info_dense", "false:12,4,1,1"])
def test_a_huber_loss_no_edge_reaches_is_no_loss_byte_for_byte(ctx, name, solver):
    sc = pl.scene(name)
    none, huge = _solve(ctx, sc, None, solver), _solve(ctx, sc, ("huber", 1e6), solver)
    assert pl.chi2(sc["poses"], sc["edge_a"], sc["edge_b"], sc["edge_meas"], sc["sqrt_info"]).max() < 1e6
    assert none["iterations"] >= 3
    _same_bits(none, huge)


def test_hubers_branch_point(ctx):
    """|r|^2 == b exactly is the inlier branch: initial_cost == b / 2; at nextafter the other branch is taken and the cost is
    held to the restatement's"""
    sc = pl.threshold_scene()
    a = pl.THRESHOLD_A
    for solver in SOLVERS:
        at = _solve(ctx, sc, ("huber", a), solver)
        assert at["initial_cost"] == a * a / 2.0
        chi2, weight = _weights(ctx, sc, sc["poses"], ("huber", a))
        assert chi2.tolist() == [a * a] and weight.tolist() == [1.0]
        lo = float(np.nextafter(a, 0.0))
        below, ref = _solve(ctx, sc, ("huber", lo), solver), pl.solve(sc, "qr", ("huber", lo))
        assert lo * lo < a * a
        assert abs(below["initial_cost"] - ref["initial_cost"]) <= 1e-6 * ref["initial_cost"]
        assert below["termination"] == ref["termination"] and at["termination"] == pl.solve(sc, "qr", ("huber", a))["termination"]


def test_the_setting_defaults_validates_and_resets(ctx, pkg):
    fresh = pkg.Context(width=0, height=0)
    assert fresh.get_pose_graph_loss() == (pkg.BA_LOSS_NONE, 0.0)
    sc = pl.scene("dup3")
    never = fresh.pose_graph(sc["poses"], sc["edge_a"], sc["edge_b"], sc["edge_meas"], sc["sqrt_info"], sc["fixed"])
    fresh.close()
    ctx.set_pose_graph_loss("cauchy", 0.25)
    assert ctx.get_pose_graph_loss() == (pkg.BA_LOSS_CAUCHY, 0.25)
    for bad in ((3, 0.1), (-1, 0.1), ("huber", 0.0), ("huber", -1.0), ("cauchy", np.nan), ("huber", np.inf), ("tukey", 0.1)):
        with pytest.raises(pkg.MslamHipError) as e:
            ctx.set_pose_graph_loss(*bad)
        assert e.value.code == pkg.E_INVALID, bad
        assert ctx.get_pose_graph_loss() == (pkg.BA_LOSS_CAUCHY, 0.25), bad       # the setting is as it was
    k = C.c_int(-1)
    assert ctx.L.mslam_hip_get_pose_graph_loss(ctx._h, C.byref(k), None) == 0 and k.value == pkg.BA_LOSS_CAUCHY
    assert ctx.L.mslam_hip_get_pose_graph_loss(ctx._h, None, None) == 0
    with_loss = ctx.pose_graph(sc["poses"], sc["edge_a"], sc["edge_b"], sc["edge_meas"], sc["sqrt_info"], sc["fixed"])
    assert with_loss["poses"].tobytes() != never["poses"].tobytes()
    ctx.set_pose_graph_loss("none", 7.0)                      # with NONE the scale is ignored and reported as 0
    assert ctx.get_pose_graph_loss() == (pkg.BA_LOSS_NONE, 0.0)
    _same_bits(ctx.pose_graph(sc["poses"], sc["edge_a"], sc["edge_b"], sc["edge_meas"], sc["sqrt_info"], sc["fixed"]), never)
    ctx.set_pose_graph_loss(pkg.BA_LOSS_HUBER, 0.1)           # the numbers are accepted as the names are
    assert ctx.get_pose_graph_loss() == (pkg.BA_LOSS_HUBER, 0.1)
    ctx.set_pose_graph_loss("none")


def test_the_settings_are_independent(ctx):
    """set_pose_graph_loss does not change a bundle_adjust result, the bundle adjustments' and the PnP's losses do not change a
    pose graph's"""
    ba = ba_cases.scene("fixed:3,65,5")
    run_ba = lambda: ctx.bundle_adjust(ba["poses"], ba["landmarks"], ba["obs_kf"], ba["obs_lm"], ba["obs_cam"], ba["fixed"])
    plain = run_ba()
    ctx.set_pose_graph_loss("huber", 0.01)
    try:
        other = run_ba()
        assert ctx.get_ba_loss() == (0, 0.0) and ctx.get_pnp_mse_loss() == (0, 0.0)
    finally:
        ctx.set_pose_graph_loss("none")
    assert plain["poses"].tobytes() == other["poses"].tobytes() and plain["landmarks"].tobytes() == other["landmarks"].tobytes()
    assert plain["final_cost"] == other["final_cost"] and plain["iterations"] == other["iterations"]
    sc = pl.scene("to_fixed")
    none = _solve(ctx, sc)
    ctx.set_ba_loss("cauchy", 0.01)
    ctx.set_pnp_mse_loss("huber", 0.5)
    try:
        _same_bits(none, _solve(ctx, sc))
        assert ctx.get_pose_graph_loss() == (0, 0.0)
    finally:
        ctx.set_ba_loss("none")
        ctx.set_pnp_mse_loss("none")


@pytest.mark.parametrize("kind", pl.LOSSES)
def test_failure_leaves_the_poses(ctx, kind):
    """tests/test_gpu_pose_graph.py's FAILURE inputs with a loss set: rho of a NaN is a NaN, the start cost is not finite,
    termination 2 is the result and nothing moves"""
    clean = pc.scene("chain:9")
    for spoil in ("meas", "pose"):
        sc = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in clean.items()}
        if spoil == "meas":
            sc["edge_meas"][3, 5] = np.nan
        else:
            sc["poses"][4, 6] = np.inf
        for solver in SOLVERS:
            got = _solve(ctx, sc, (kind, pl.SCALE), solver)
            with np.errstate(all="ignore"):
                ref = pl.solve(sc, "qr", (kind, pl.SCALE))
            assert ref["termination"] == 2 and ref["reason"] == "initial evaluation failed"
            assert got["termination"] == 2 and got["iterations"] == 0 and not np.isfinite(got["initial_cost"])
            assert got["poses"].tobytes() == sc["poses"].tobytes()
    _same_bits(_solve(ctx, clean, (kind, pl.SCALE)), _solve(ctx, clean, (kind, pl.SCALE)))


def test_edge_weights_arguments(ctx, pkg):
    sc = pl.scene("dup3")
    chi2, weight = _weights(ctx, sc, sc["poses"])             # NONE: every weight is 1.0
    _check_weights(chi2, weight, sc, sc["poses"], None)
    assert weight.tolist() == [1.0] * len(sc["edge_a"])
    x = np.ascontiguousarray(sc["poses"], np.float64)
    ea, eb, z = (np.ascontiguousarray(sc[k]) for k in ("edge_a", "edge_b", "edge_meas"))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    raw = lambda c2, w, E=len(ea), K=len(x): ctx.L.mslam_hip_pose_graph_edge_weights(ctx._h, p(x), K, p(ea), p(eb), p(z), None, E, c2, w)
    ctx.set_pose_graph_loss("cauchy", pl.SCALE)
    try:
        both_c, both_w = np.zeros(len(ea)), np.zeros(len(ea))
        assert raw(p(both_c), p(both_w)) == 0
        only_c, only_w = np.zeros(len(ea)), np.zeros(len(ea))
        assert raw(p(only_c), None) == 0 and raw(None, p(only_w)) == 0 and raw(None, None) == 0      # NULL outputs are accepted
        assert only_c.tobytes() == both_c.tobytes() and only_w.tobytes() == both_w.tobytes() and both_w.min() < 0.01
        guard_c, guard_w = np.full(2, -7.0), np.full(2, -7.0)
        assert raw(p(guard_c), p(guard_w), E=0) == 0 and raw(p(guard_c), p(guard_w), E=0, K=0) == 0  # E = 0 writes nothing
        assert guard_c.tolist() == [-7.0, -7.0] and guard_w.tolist() == [-7.0, -7.0]
        assert raw(p(both_c), p(both_w), K=2) == pkg.E_INVALID                                        # an edge names pose 4
        assert raw(p(both_c), p(both_w), E=-1) == pkg.E_INVALID
        # the cap on K is the SPARSE solver's although the context's solver is DENSE
        K = pkg.POSE_GRAPH_MAX_KEYFRAMES + 5
        many = np.tile([0, 0, 0, 1.0, 0, 0, 0], (K, 1))
        many[:, 4] = np.arange(K)
        c2, w = ctx.pose_graph_edge_weights(many, [0, K - 2], [1, K - 1], [[0, 0, 0, 1.0, 1, 0, 0], [0, 0, 0, 1.0, 0.5, 0, 0]])
        assert c2.tolist() == [0.0, 0.25] and w[0] == 1.0 and abs(w[1] - pl.loss(pl.CAUCHY, pl.SCALE, 0.25)[1]) <= 4.0 * np.finfo(np.float64).eps * w[1]
        too_many = np.tile([0, 0, 0, 1.0, 0, 0, 0], (pkg.POSE_GRAPH_MAX_KEYFRAMES_SPARSE + 1, 1))
        with pytest.raises(pkg.MslamHipError) as e:
            ctx.pose_graph_edge_weights(too_many, [0], [1], [[0, 0, 0, 1.0, 0, 0, 0]])
        assert e.value.code == pkg.E_INVALID
    finally:
        ctx.set_pose_graph_loss("none")
    e0 = ctx.pose_graph_edge_weights(x, [], [], np.zeros((0, 7)))
    assert len(e0[0]) == 0 and len(e0[1]) == 0


# ---- HipBackend and the tracker --------------------------------------------------------------------------------------------

def _tracker(pkg, seq_params, **kw):
    c = pkg.Context(width=0, height=0, max_keypoints=4096)
    c.bow_load(synth.make_vocabulary(10, 3))
    return c, pkg.HipKeyframeTracker(c, focal=tr.CAM[:2], principal=tr.CAM[2:], **dict(seq_params, **kw))


def test_tracker_without_a_loss_is_the_tracker(pkg):
    """pose_graph_loss = None is the default: on tests/track_ref.py's walk the tracker with the switch named computes what the
    tracker without it computes, bit for bit, and a loss without loop_closure is refused"""
    seq = tr.make_sequence()
    runs = []
    for kw in (dict(), dict(pose_graph_loss=None)):
        c, t = _tracker(pkg, dict(tr.SEQ_PARAMS, local_map_depth=2, local_ba=True, loop_closure=True, loop_min_gap=2), **kw)
        runs.append((c, t, [t.processSensorData(fr["desc"], fr["xy"], fr["depth"]) for fr in seq["frames"]]))
        assert t.backend.pose_graph_loss is None and c.get_pose_graph_loss() == (0, 0.0)
    (c0, t0, a), (c1, t1, b) = runs
    assert t0.ids == t1.ids and len(t0.ids) >= 3
    for f, (x, y) in enumerate(zip(a, b)):
        assert sorted(x) == sorted(y)
        assert (x["tracked"], x["n_inliers"], x["keyframe"], x["reference"], x["relocalized"]) == \
               (y["tracked"], y["n_inliers"], y["keyframe"], y["reference"], y["relocalized"]), f
        assert x["R"].tobytes() == y["R"].tobytes() and x["tvec"].tobytes() == y["tvec"].tobytes() and x["rvec"].tobytes() == y["rvec"].tobytes(), f
    for k in t0.ids:
        assert c0.kf_read(k)[1].tobytes() == c1.kf_read(k)[1].tobytes() and t0.backend.poses[k].tobytes() == t1.backend.poses[k].tobytes()
    with pytest.raises(pkg.MslamHipError) as e:
        pkg.HipKeyframeTracker(c0, local_map_depth=2, local_ba=True, pose_graph_loss=("huber", 0.1))      # needs loop_closure
    assert e.value.code == pkg.E_INVALID
    c0.close()
    c1.close()


def test_tracker_passes_the_loss_to_close_loop(pkg):
    """tests/loop_walk.py's ring walk, which closes one loop: every close_loop result of the tracker equals a direct
    HipBackend(pose_graph_loss = ...) solve of the state the backend held at that moment, and the context carries no pose-graph
    loss between calls.  Nothing is claimed about the trajectory"""
    import copy
    how = ("cauchy", pl.SCALE)
    seq = loop_walk.ring_sequence()
    c, t = _tracker(pkg, dict(local_map_depth=2, local_ba=True, new_keyframe_min_landmarks=200), loop_closure=True, loop_min_gap=5,
                    pose_graph_loss=how)
    assert t.backend.pose_graph_loss == how
    held, inner = [], t.backend.close_loop

    def recording(*args, **kw):
        be = t.backend
        held.append((copy.deepcopy((be.poses, be.obs, be.landmarks, be.anchor, be.first)), copy.deepcopy((args, kw))))
        return inner(*args, **kw)
    t.backend.close_loop = recording
    for fr in seq["frames"]:
        t.processSensorData(fr["desc"], fr["xy"], fr["depth"])
        assert c.get_pose_graph_loss() == (0, 0.0)
    closed = [a for a in t.loop_results if a["loop"] is not None]
    assert len(closed) == len(held) == 1
    c2 = pkg.Context(width=0, height=0)
    for attempt, (state, (args, kw)) in zip(closed, held):
        be = pkg.HipBackend(c2, pose_graph_loss=how)
        be.poses, be.obs, be.landmarks, be.anchor, be.first = state
        want, got = be.close_loop(*args, **kw), attempt["result"]
        _same_bits(got, want)
        assert got["landmarks"].tobytes() == want["landmarks"].tobytes() and got["keyframes"] == want["keyframes"]
        E = len(got["edge_weight"])
        assert got["edge_chi2"].tobytes() == want["edge_chi2"].tobytes() and got["edge_weight"].tobytes() == want["edge_weight"].tobytes()
        assert E == len(got["edge_chi2"]) >= len(got["keyframes"]) and np.all(got["edge_weight"] > 0.0) and np.all(got["edge_weight"] <= 1.0)
        w = pl.loss(pl.CAUCHY, pl.SCALE, got["edge_chi2"])[1]
        assert np.all(np.abs(got["edge_weight"] - w) <= 4.0 * np.finfo(np.float64).eps * w)
        assert got["termination"] in (0, 1) and got["final_cost"] <= got["initial_cost"]
        assert c2.get_pose_graph_loss() == (0, 0.0)
    # without a loss the result has no weights
    plain = pkg.HipBackend(c2)
    plain.poses, plain.obs, plain.landmarks, plain.anchor, plain.first = copy.deepcopy(held[0][0])
    args, kw = held[0][1]
    assert "edge_weight" not in plain.close_loop(*args, **kw)
    c.close()
    c2.close()
