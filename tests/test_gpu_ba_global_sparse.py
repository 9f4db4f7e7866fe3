"""mslam_hip_bundle_adjust_global with the SPARSE linear solver on the MI355X (k_bag_schur_env of k_ba.hip writing the
covisible pairs' Schur blocks into the block envelope, the factor and substitution of k_pg_sparse.hip) through
Context.set_ba_global_solver("sparse") and Context.bundle_adjust_global.

Bounds, those of tests/test_gpu_ba_global.py (its _check is used as it is): |x_gpu - x_ref|_inf <= max(1e-9, 1000 dist), dist
the distance of two correct CPU solvers on the scene: "qr" and "schur" of tests/ba_ref.py where they exist, "normal" and
"augmented" of tests/ba_global_sparse_ref.py (tests/test_ba_global_sparse.py pins those to "qr") on the new scenes and above
the dense cap, where the solves are recorded under tests/golden/ba_global_sparse/.  Against ground truth (the noise-free
1100-keyframe rings) the bound is max(1e-7, 10 x the recorded distance of the sparse CPU reference to the truth): the dense CPU
Schur reference reaches 4.0e-8 at 1040 and 6.2e-8 at 1100 keyframes, inside the project's 1e-7 with little room.  No test
asserts a time."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_cases  # noqa: E402
import ba_global_cases as bg  # noqa: E402
import ba_global_sparse_cases as bc  # noqa: E402
import ba_loss_ref as lr  # noqa: E402
import ba_ref  # noqa: E402
import loop_walk  # noqa: E402
import pose_graph_sparse_cases as psc  # noqa: E402
import test_gpu_ba_global as tg  # noqa: E402
import test_gpu_pose_graph as tpg  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(width=0, height=0)
    c.set_ba_global_solver("sparse")
    yield c
    c.close()


@pytest.fixture(autouse=True)
def sparse_again(ctx):
    yield
    ctx.set_ba_global_solver("sparse")
    ctx.set_ba_loss("none")


def _solve(ctx, sc, **kw):
    return tg._solve(ctx, sc, **kw)


def _fixed_and_unobserved_stay(got, sc):
    seen = np.zeros(len(sc["poses"]), bool)
    seen[sc["obs_kf"]] = True
    for k in np.flatnonzero((np.asarray(sc["fixed"]) != 0) | ~seen):
        assert got["poses"][k].tobytes() == np.asarray(sc["poses"], np.float64)[k].tobytes(), k


# ---- against the references, the same rule -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", bg.WITH_QR)
def test_against_the_qr_reference(ctx, name):
    sc, qr, sch, dist, mask, margin = bg.reference(name)
    got = _solve(ctx, sc)
    tg._check("BAGS", name, got, sc, qr, dist, mask)
    _fixed_and_unobserved_stay(got, sc)
    if name == "hard66":
        assert got["rejected_steps"] > 0
    if name == "gross80":
        assert got["n_outliers"] == 2


@pytest.mark.parametrize("name", tg.OLD_GROUND)
def test_the_old_ground(ctx, name):
    sc, qr, sch, dist, mask, margin = ba_cases.reference(name)
    got = _solve(ctx, sc)
    tg._check("BAGS old", name, got, sc, qr, dist, mask)
    _fixed_and_unobserved_stay(got, sc)
    if name in ("all_fixed", "k1_fixed", "empty"):
        assert np.array_equal(got["poses"], sc["poses"])
    if name.startswith("cap"):
        assert got["iterations"] == qr["iterations"]
    if name in ("cap0", "at_minimum"):
        assert got["iterations"] == 0
        assert got["poses"].tobytes() == np.asarray(sc["poses"], np.float64).tobytes()
        assert got["landmarks"].tobytes() == np.asarray(sc["landmarks"], np.float64).tobytes()


@pytest.mark.parametrize("name", bc.NEW)
def test_the_new_scenes_against_the_sparse_references(ctx, pkg, name):
    sc, ref, aug, dist, mask = bc.reference(name)
    an = pkg.ba_global_analyze(sc["fixed"], len(sc["poses"]), sc["obs_kf"], sc["obs_lm"], len(sc["landmarks"]))
    got = _solve(ctx, sc)
    tg._check("BAGS new", name, got, sc, ref, dist, mask)
    _fixed_and_unobserved_stay(got, sc)
    assert aug["termination"] == ref["termination"] and aug["iterations"] == ref["iterations"]
    if name == "shuffled:66":
        assert an["ordering"] == pkg.PG_ORDER_RCM
    if name == "loop_row":
        assert an["ordering"] == pkg.PG_ORDER_NATURAL and an["envelope_blocks"] > an["n_pairs"]


def test_an_unobserved_keyframe_comes_back_bit_for_bit(ctx):
    sc, ref, aug, dist, mask = bc.reference("open:33")
    extra = np.array([[0.1, -0.2, 0.3, 0.0, 1.0, 2.0, 3.0]])
    extra[0, 3] = np.sqrt(1.0 - 0.14)
    more = dict(sc, poses=np.vstack([sc["poses"][:20], extra, sc["poses"][20:]]), fixed=np.r_[sc["fixed"][:20], 0, sc["fixed"][20:]].astype(np.uint8),
                obs_kf=(sc["obs_kf"] + (sc["obs_kf"] >= 20)).astype(np.int32))
    got = _solve(ctx, more)
    assert got["poses"][20].tobytes() == extra.tobytes()
    got["poses"] = np.delete(got["poses"], 20, 0)
    tg._check("BAGS unobserved", "open:33", got, sc, ref, dist, mask)


# ---- beyond the dense cap -----------------------------------------------------------------------------------------------------------

def _recorded(name):
    sc, ref, aug, dist, truth = bc.recorded(name)
    mask = ba_ref.outliers(ref["poses"], ref["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"])
    return sc, ref, aug, dist, truth, mask


def _truth_error(got, sc):
    seen = np.zeros(len(sc["landmarks"]), bool)
    seen[sc["obs_lm"]] = True
    return max(float(np.max(np.abs(got["poses"] - sc["truth_poses"]))),
               float(np.max(np.abs(got["landmarks"][seen] - sc["truth_landmarks"][seen]))))


@pytest.mark.parametrize("name", ["ring", "shuffled"])
def test_beyond_the_dense_cap(ctx, pkg, name):
    """1100 keyframes: DENSE rejects the call as before; SPARSE agrees with the recorded sparse reference, and on the
    noise-free twin reaches the truth.  shuffled: the same ring under a permutation, RCM chosen"""
    sc, ref, aug, dist, truth, mask = _recorded(name + ":1100")
    an = pkg.ba_global_analyze(sc["fixed"], 1100, sc["obs_kf"], sc["obs_lm"], len(sc["landmarks"]))
    assert an["ordering"] == (pkg.PG_ORDER_RCM if name == "shuffled" else pkg.PG_ORDER_NATURAL) and an["n_free"] == 1099
    ctx.set_ba_global_solver("dense")
    with pytest.raises(pkg.MslamHipError) as e:
        _solve(ctx, sc)
    assert e.value.code == pkg.E_INVALID
    ctx.set_ba_global_solver("sparse")
    got = _solve(ctx, sc)
    tg._check("BAGS", name + ":1100", got, sc, ref, dist, mask)
    _fixed_and_unobserved_stay(got, sc)
    sc0, ref0, aug0, dist0, truth0, mask0 = _recorded(name + "0:1100")
    got0 = _solve(ctx, sc0)
    err = _truth_error(got0, sc0)
    print("BAGS %s0:1100 term %d it %d/%d err %.3e, the reference's %.3e" % (name, got0["termination"], got0["iterations"], ref0["iterations"], err, truth0))
    assert got0["termination"] == 0 and abs(got0["iterations"] - ref0["iterations"]) <= 1 and got0["invalid_steps"] == 0
    assert err <= max(1e-7, 10.0 * truth0)
    assert not got0["outlier"].any()


# ---- the cap --------------------------------------------------------------------------------------------------------------------------

def test_the_sparse_cap(ctx, pkg):
    """16384 keyframes in a thin ring under an iteration cap of 3, against the recorded sparse reference; 16385 is rejected"""
    sc, ref, aug, dist, truth, mask = _recorded("thin:16384")
    assert len(sc["poses"]) == pkg.BA_GLOBAL_MAX_KEYFRAMES_SPARSE and len(sc["obs_kf"]) == 32770 and sc["max_iterations"] == 3
    got = _solve(ctx, sc)
    tg._check("BAGS", "thin:16384", got, sc, ref, dist, mask)
    assert got["termination"] == 1 and got["iterations"] == 3 and got["final_cost"] < got["initial_cost"]
    over = np.tile([0, 0, 0, 1.0, 0, 0, 0], (pkg.BA_GLOBAL_MAX_KEYFRAMES_SPARSE + 1, 1))
    none = np.zeros(0, np.int32)
    with pytest.raises(pkg.MslamHipError) as e:
        ctx.bundle_adjust_global(over, np.zeros((1, 3)), none, none, np.zeros((0, 3)))
    assert e.value.code == pkg.E_INVALID
    ok = ctx.bundle_adjust_global(over[:-1], np.zeros((1, 3)), none, none, np.zeros((0, 3)))
    assert ok["termination"] == 0 and ok["final_cost"] == 0.0


# ---- capacity, then reuse ---------------------------------------------------------------------------------------------------------------

def test_capacity_then_a_small_solve(ctx, pkg):
    """one landmark that 1500 keyframes see: the envelope is the whole triangle in both orders: E_CAPACITY, the message names
    the blocks, poses, landmarks and the outlier array keep their bytes; the context then solves as a fresh one does"""
    sc = bc.scene("wide:1500")
    x, lm = np.ascontiguousarray(sc["poses"], np.float64), np.ascontiguousarray(sc["landmarks"], np.float64)
    x[:, 4] = 1e-3 * np.arange(len(x))                        # off the minimum: a solve would move them
    out = np.full(len(sc["obs_kf"]), 7, np.uint8)
    before = (x.copy(), lm.copy())
    summary = pkg.BaSummary()
    rc = ctx.L.mslam_hip_bundle_adjust_global(ctx._h, pkg._p(x), pkg._p(sc["fixed"]), len(x), pkg._p(lm), len(lm), pkg._p(sc["obs_kf"]),
                                              pkg._p(sc["obs_lm"]), pkg._p(sc["obs_cam"]), len(sc["obs_kf"]), 100, pkg.C.c_double(0.15),
                                              pkg._p(out), pkg.C.byref(summary))
    assert rc == pkg.E_CAPACITY
    assert x.tobytes() == before[0].tobytes() and lm.tobytes() == before[1].tobytes() and np.all(out == 7)
    with pytest.raises(pkg.MslamHipError) as e:
        _solve(ctx, sc)
    assert e.value.code == pkg.E_CAPACITY and str(1500 * 1501 // 2) in str(e.value)
    small = bc.scene("shuffled:66")
    got = _solve(ctx, small)
    c = pkg.Context(width=0, height=0)
    c.set_ba_global_solver("sparse")
    tg._same_bits(got, _solve(c, small))
    c.close()


# ---- state on one context ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["shuffled:66", "loop_row", "complete12", "hard66", "gross80"])
def test_a_second_call_returns_the_same_bits(ctx, name):
    sc = bc.scene(name)
    a = _solve(ctx, sc)
    assert a["termination"] == 0
    if name == "hard66":
        assert a["rejected_steps"] > 0
    if name == "gross80":
        assert a["n_outliers"] == 2
    tg._same_bits(a, _solve(ctx, sc))


def test_dense_sparse_dense_on_one_context(ctx, pkg):
    sc, qr, sch, dist, mask, margin = bg.reference("traj:66")
    ctx.set_ba_global_solver("dense")
    assert ctx.get_ba_global_solver() == pkg.BA_GLOBAL_SOLVER_DENSE
    d0 = _solve(ctx, sc)
    ctx.set_ba_global_solver("sparse")
    assert ctx.get_ba_global_solver() == pkg.BA_GLOBAL_SOLVER_SPARSE
    s0 = _solve(ctx, sc)
    ctx.set_ba_global_solver(pkg.BA_GLOBAL_SOLVER_DENSE)
    d1 = _solve(ctx, sc)
    ctx.set_ba_global_solver("sparse")
    s1 = _solve(ctx, sc)
    tg._same_bits(d0, d1)
    tg._same_bits(s0, s1)
    tg._check("BAGS dsd sparse", "traj:66", s0, sc, qr, dist, mask)
    tg._check("BAGS dsd dense", "traj:66", d0, sc, qr, dist, mask)
    fresh = pkg.Context(width=0, height=0)                    # a fresh context is DENSE and returns the bits of d0
    assert fresh.get_ba_global_solver() == pkg.BA_GLOBAL_SOLVER_DENSE
    tg._same_bits(_solve(fresh, sc), d0)
    fresh.set_ba_global_solver("sparse")                      # and SPARSE on a fresh context the bits of s0
    tg._same_bits(_solve(fresh, sc), s0)
    fresh.close()


def test_a_sparse_pose_graph_solve_in_between(ctx, pkg):
    """both envelopes live in one buffer: what the pose graph's factor left there must not reach the next bundle adjustment;
    bundle_adjust (at most 64 keyframes) does not read the setting"""
    sc = bc.scene("loop_row")
    a = _solve(ctx, sc)
    graph = psc.scene("revisit200")
    ctx.set_pose_graph_solver("sparse")
    try:
        pg = ctx.pose_graph(graph["poses"], graph["edge_a"], graph["edge_b"], graph["edge_meas"], graph["sqrt_info"], graph["fixed"])
    finally:
        ctx.set_pose_graph_solver("dense")
    assert pg["termination"] == 0
    tg._same_bits(a, _solve(ctx, sc))
    small = bg.scene("traj:34")
    local = ctx.bundle_adjust(*tg._args(small))
    ctx.set_ba_global_solver("dense")
    tg._same_bits(local, ctx.bundle_adjust(*tg._args(small)))


# ---- loss, failure, setter ----------------------------------------------------------------------------------------------------------------

def test_huber_against_the_corrector_on_the_sparse_reference(ctx):
    """gross80 (three gross observations) with Huber at ba_loss_ref.SCALE: the weights reach the envelope through U, V and W"""
    sc, ref, aug, dist, mask = bc.reference("gross80", ("huber", lr.SCALE))
    plain = bc.reference("gross80")[1]
    assert ref["final_cost"] < 0.5 * plain["final_cost"]        # the loss is active on this scene
    ctx.set_ba_loss("huber", lr.SCALE)
    got = _solve(ctx, sc)
    tg._check("BAGS huber", "gross80", got, sc, ref, dist, mask)
    tg._same_bits(got, _solve(ctx, sc))


def test_failure_leaves_the_state_and_judges_the_outliers_at_the_input(ctx, pkg):
    for name in ("traj:66", "gross80"):
        clean = bg.scene(name)
        sc = {k: np.array(v) for k, v in clean.items()}
        sc["obs_cam"][5, 1] = np.nan
        got = _solve(ctx, sc)
        assert got["termination"] == 2 and got["iterations"] == 0 and not np.isfinite(got["initial_cost"])
        assert got["poses"].tobytes() == sc["poses"].tobytes() and got["landmarks"].tobytes() == sc["landmarks"].tobytes()
        with np.errstate(all="ignore"):
            mask = ba_ref.outliers(sc["poses"], sc["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"])
        assert mask.any() or name != "gross80"
        assert np.array_equal(got["outlier"], mask) and got["n_outliers"] == int(mask.sum())
    c = pkg.Context(width=0, height=0)
    c.set_ba_global_solver("sparse")
    tg._same_bits(_solve(ctx, clean), _solve(c, clean))         # the context is usable afterwards
    c.close()


def test_the_setter_rejects_an_unknown_kind(ctx, pkg):
    for bad in (2, -1, "skyline"):
        with pytest.raises(pkg.MslamHipError) as e:
            ctx.set_ba_global_solver(bad)
        assert e.value.code == pkg.E_INVALID
        assert ctx.get_ba_global_solver() == pkg.BA_GLOBAL_SOLVER_SPARSE
    assert ctx.L.mslam_hip_set_ba_global_solver(ctx._h, 2) == pkg.E_INVALID
    assert ctx.get_ba_global_solver() == pkg.BA_GLOBAL_SOLVER_SPARSE
    assert ctx.get_pose_graph_solver() == pkg.PG_SOLVER_DENSE          # two settings, not one


# ---- backend and tracker ------------------------------------------------------------------------------------------------------------------

def test_backend_global_ba_on_1100_keyframes(pkg):
    """HipBackend(global_solver=True, global_linear_solver="sparse") on the 1100-keyframe ring, on a context whose own setting
    is DENSE and stays DENSE; the default backend's E_CAPACITY on the same map"""
    sc, ref, aug, dist, truth, mask = _recorded("ring:1100")
    K = len(sc["poses"])
    c = pkg.Context(width=0, height=0, max_keypoints=64)
    be = pkg.HipBackend(c, global_solver=True, global_linear_solver="sparse")
    order = np.argsort(sc["obs_kf"], kind="stable")
    start = np.searchsorted(sc["obs_kf"][order], np.arange(K + 1))
    for k in range(K):                                        # ids = indices, keyframe 0 first: it is the constant one
        m = order[start[k]:start[k + 1]]
        be.add_keyframe(k, sc["poses"][k], sc["obs_lm"][m].astype(np.int64), sc["obs_cam"][m])
    for l in list(be.landmarks):
        be.landmarks[l] = sc["landmarks"][l].copy()
    got = be.global_ba()
    assert c.get_ba_global_solver() == pkg.BA_GLOBAL_SOLVER_DENSE
    bound = max(1e-9, 1000.0 * dist)
    dx = max(float(np.max(np.abs(got["poses"] - ref["poses"]))),
             float(np.max(np.abs(got["landmarks"] - ref["landmarks"][got["landmark_ids"]]))))
    print("BAGS backend ring:1100 term %d it %d/%d cost %.6g -> %.6g / %.6g dx %.3e bound %.3e" % (
        got["termination"], got["iterations"], ref["iterations"], got["initial_cost"], got["final_cost"], ref["final_cost"], dx, bound))
    assert got["termination"] == 0 and abs(got["iterations"] - ref["iterations"]) <= 1 and got["invalid_steps"] == 0
    assert got["keyframes"] == list(range(K)) and dx <= bound and got["n_outliers"] == int(mask.sum())
    assert abs(got["final_cost"] - ref["final_cost"]) <= 1e-6 * ref["final_cost"] + len(sc["obs_kf"]) * (12.0 * bound) ** 2 / 2.0
    assert be.poses[0].tobytes() == sc["poses"][0].tobytes() and be.poses[7].tobytes() == got["poses"][7].tobytes()
    for kw in (dict(global_linear_solver=pkg.BA_GLOBAL_SOLVER_DENSE), dict(global_solver=False)):
        for k, v in kw.items():
            setattr(be, k, v)
        with pytest.raises(pkg.MslamHipError) as e:
            be.global_ba()
        assert e.value.code == pkg.E_CAPACITY
    big = pkg.HipBackend(None, global_solver=True, global_linear_solver="sparse")
    big.poses = {k: None for k in range(pkg.BA_GLOBAL_MAX_KEYFRAMES_SPARSE + 1)}
    with pytest.raises(pkg.MslamHipError) as e:
        big.global_ba()
    assert e.value.code == pkg.E_CAPACITY and "16384" in str(e.value)
    c.close()


def test_tracker_ring_walk_with_the_sparse_global_solve(pkg):
    """tests/test_gpu_pose_graph.py's ring walk with loop_global_ba and ba_global_solver = "sparse": the loop closes, the
    global solve runs on the envelope and ends usable, the context's own setting stays DENSE"""
    seq = loop_walk.ring_sequence()
    c, t, rows = tpg._run_ring(pkg, seq, loop_closure=True, loop_min_gap=5, loop_global_ba=True, ba_global_solver="sparse")
    assert t.backend.global_linear_solver == pkg.BA_GLOBAL_SOLVER_SPARSE and t.backend.global_solver
    closed = [a for a in t.loop_results if a["loop"] is not None]
    assert len(closed) == 1 and all(r["tracked"] for r in rows)
    res, ba = closed[0]["result"], closed[0]["global_ba"]
    print("BAGS ring walk: closure %s, global BA term %d it %d cost %.6g -> %.6g" % (
        closed[0]["loop"], ba["termination"], ba["iterations"], ba["initial_cost"], ba["final_cost"]))
    assert res["termination"] == 0
    assert ba["termination"] in (0, 1) and ba["invalid_steps"] == 0 and ba["final_cost"] <= ba["initial_cost"]
    assert ba["keyframes"] == res["keyframes"] and ba["n_written"] >= len(ba["landmark_ids"]) > 0
    assert c.get_ba_global_solver() == pkg.BA_GLOBAL_SOLVER_DENSE
    c.close()
