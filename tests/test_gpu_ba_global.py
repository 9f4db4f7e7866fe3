"""mslam_hip_bundle_adjust_global on the MI355X (k_bag_schur of k_ba.hip and the k_bag_* kernels of k_chol.hip: covisible-pair
Schur complement, blocked Cholesky, blocked substitution) through Context.bundle_adjust_global: against tests/ba_ref.py's QR solve on the trajectory
scenes of tests/ba_global_cases.py (tests/test_ba_global.py shows on the CPU that every scene takes the path it is named
for); both solvers on cases of tests/ba_cases.py; determinism, also of a small solve after a large one; 300 keyframes against
ground truth; arguments and FAILURE; HipBackend(global_solver=True).

Bounds, restated from tests/test_gpu_ba.py.  State: |x_gpu - x_qr|_inf <= max(1e-9, 1000 |x_schur - x_qr|_inf): the distance
of two correct CPU solvers, times 1000 for the kernels' other summation orders.  Costs: 1e-6 relative, plus the second-order
term the state bound allows at a minimum, M (12 B)^2 / 2 (12 bounds the row norm of a residual's Jacobian: |X - p| <= 5 m).
A start cost of exactly 0 in the reference (at_minimum) has no relative precision: it takes M 3 ROUNDING^2 / 2 with
ROUNDING = 20 eps 5 m, the rounding of one residual component."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_cases  # noqa: E402
import ba_global_cases as bg  # noqa: E402
import ba_ref  # noqa: E402

pytestmark = pytest.mark.gpu
ROUNDING = 20 * np.finfo(np.float64).eps * 5.0
OLD_GROUND = ["fixed:8,200,10", "free:5,150,10", "rejected", "k64", "k64_dense", "fixed_middle", "fixed_two", "twice_in_keyframe",
              "fixed_only_landmarks", "all_fixed", "k1_fixed", "empty", "cap0", "cap1", "cap4_stops", "at_minimum", "blocks:16385"]


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(width=0, height=0)
    yield c
    c.close()


def _args(sc):
    return sc["poses"], sc["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"], sc["fixed"]


def _solve(ctx, sc, **kw):
    return ctx.bundle_adjust_global(*_args(sc), max_iterations=sc.get("max_iterations", 100), **kw)


def _check(tag, name, got, sc, qr, dist, mask):
    bound = max(1e-9, 1000.0 * dist)
    dx = max(float(np.max(np.abs(got["poses"] - qr["poses"]), initial=0.0)),
             float(np.max(np.abs(got["landmarks"] - qr["landmarks"]), initial=0.0)))
    M = len(sc["obs_kf"])
    second_order = M * (12.0 * bound) ** 2 / 2.0
    zero_cost = 0.0 if qr["initial_cost"] > 0.0 else M * 3 * ROUNDING ** 2 / 2.0
    print("%s %-22s term %d/%d it %d/%d rejected %d/%d invalid %d cost0 %.17g/%.17g cost %.6g/%.6g dx %.3e bound %.3e" % (
        tag, name, got["termination"], qr["termination"], got["iterations"], qr["iterations"], got["rejected_steps"],
        qr["trace"]["rejected"], got["invalid_steps"], got["initial_cost"], qr["initial_cost"], got["final_cost"], qr["final_cost"],
        dx, bound))
    assert got["termination"] == qr["termination"]
    assert abs(got["iterations"] - qr["iterations"]) <= 1
    assert got["invalid_steps"] == 0
    assert abs(got["initial_cost"] - qr["initial_cost"]) <= 1e-6 * qr["initial_cost"] + zero_cost
    assert abs(got["final_cost"] - qr["final_cost"]) <= 1e-6 * qr["final_cost"] + second_order
    assert dx <= bound
    assert np.array_equal(got["outlier"], mask) and got["n_outliers"] == int(mask.sum())


@pytest.mark.parametrize("name", bg.WITH_QR)
def test_against_the_qr_reference(ctx, name):
    sc, qr, sch, dist, mask, margin = bg.reference(name)
    got = _solve(ctx, sc)
    _check("BAG", name, got, sc, qr, dist, mask)
    if sc["fixed"][0]:
        assert got["poses"][0].tobytes() == sc["poses"][0].tobytes()
    if name == "hard66":
        assert got["rejected_steps"] > 0
    if name == "gross80":
        assert got["n_outliers"] == 2


@pytest.mark.parametrize("name", OLD_GROUND)
def test_both_solvers_on_the_old_ground(ctx, name):
    sc, qr, sch, dist, mask, margin = ba_cases.reference(name)
    got = _solve(ctx, sc)
    _check("BAG old", name, got, sc, qr, dist, mask)
    old = ctx.bundle_adjust(*_args(sc), max_iterations=sc.get("max_iterations", 100))
    assert (got["termination"], got["iterations"]) == (old["termination"], old["iterations"])
    assert np.array_equal(got["outlier"], old["outlier"])
    if name == "empty":
        assert got["final_cost"] == 0.0
    if name in ("all_fixed", "k1_fixed", "empty"):
        assert np.array_equal(got["poses"], sc["poses"])
    if name.startswith("cap"):
        assert got["iterations"] == qr["iterations"]
    if name in ("cap0", "at_minimum"):
        assert got["iterations"] == 0
        assert got["poses"].tobytes() == np.asarray(sc["poses"], np.float64).tobytes()
        assert got["landmarks"].tobytes() == np.asarray(sc["landmarks"], np.float64).tobytes()
    if name in ("fixed_middle", "fixed_two"):
        for k in (1,) + tuple(np.flatnonzero(sc["fixed"])):
            assert got["poses"][k].tobytes() == sc["poses"][k].tobytes(), k


def _same_bits(a, b):
    for k in ("poses", "landmarks", "outlier"):
        assert a[k].tobytes() == b[k].tobytes(), k
    for k in ("termination", "iterations", "rejected_steps", "invalid_steps", "n_outliers"):
        assert a[k] == b[k], k
    for k in ("initial_cost", "final_cost"):
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), k


@pytest.mark.parametrize("name", ["traj:66", "traj:130", "hard66", "k64_dense"])
def test_a_second_call_returns_the_same_bits(ctx, name):
    sc = ba_cases.scene(name) if name == "k64_dense" else bg.scene(name)
    a = _solve(ctx, sc)
    assert a["termination"] == 0
    _same_bits(a, _solve(ctx, sc))


def test_a_smaller_problem_after_a_larger_one(ctx, pkg):
    """the reduced system's block only grows: what 192 free keyframes left in it (fill-in, pad, another leading dimension)
    must not reach a solve of 8"""
    small = bg.scene("traj:9")
    c = pkg.Context(width=0, height=0)
    fresh = _solve(c, small)
    c.close()
    c = pkg.Context(width=0, height=0)
    assert _solve(c, bg.scene("traj193"))["termination"] == 0
    _same_bits(_solve(c, small), fresh)
    _same_bits(_solve(c, small), fresh)
    c.close()


def test_stage_timers_nest(pkg):
    """the solver's stages are timed inside the batch of iterations: on a fresh context (an empty timer list, so the inner
    scopes make it grow while the outer one is open) every stage of both entries comes back with a sane time, and timing
    changes no bit"""
    sc = bg.scene("traj:66")
    c = pkg.Context(width=0, height=0)
    c.set_profiling(2)
    c.stage_times()
    timed = _solve(c, sc)
    new = c.stage_times()
    small = bg.scene("traj:34")                 # the old entry takes at most 64 keyframes
    old_res = c.bundle_adjust(*_args(small))
    old = c.stage_times()
    c.set_profiling(0)
    _same_bits(timed, _solve(c, sc))
    _same_bits(old_res, c.bundle_adjust(*_args(small)))
    c.close()
    for stages, inner in ((new, {"solver_schur", "solver_factor", "solver_subst"}), (old, {"solver_schur", "solver_factor_subst"})):
        names = [n for n, _ in stages]
        batches = names.count("ba_iterations")
        assert batches >= 1 and names.count("ba_start_cost") == 1 and inner <= set(names)
        assert all(np.isfinite(ms) and 0.0 <= ms < 1000.0 for _, ms in stages), stages
        outer = sum(ms for n, ms in stages if n == "ba_iterations")
        assert 0.0 < sum(ms for n, ms in stages if n in inner) <= outer + 0.05      # nested on one stream; 0.05 ms for the events' resolution


def test_300_keyframes_reach_the_truth(ctx):
    """38 panels, no QR reference: the noise-free trajectory against ground truth, the rule of tests/test_ba.py"""
    sc, sch = bg.schur_reference("traj300")
    got = _solve(ctx, sc)
    seen_l = np.zeros(len(sc["landmarks"]), bool)
    seen_l[sc["obs_lm"]] = True
    err = max(float(np.max(np.abs(got["poses"] - sc["truth_poses"]))),
              float(np.max(np.abs(got["landmarks"][seen_l] - sc["truth_landmarks"][seen_l]))))
    print("BAG traj300 term %d it %d/%d rejected %d invalid %d cost %.6g -> %.6g err %.3e" % (
        got["termination"], got["iterations"], sch["iterations"], got["rejected_steps"], got["invalid_steps"], got["initial_cost"],
        got["final_cost"], err))
    assert got["termination"] == 0 and abs(got["iterations"] - sch["iterations"]) <= 1 and got["invalid_steps"] == 0
    assert err <= 1e-7
    assert not got["outlier"].any()


def test_invalid_arguments_then_a_clean_call(ctx, pkg):
    sc, qr, sch, dist, mask, margin = bg.reference("traj:9")
    many = np.tile([0, 0, 0, 1.0, 0, 0, 0], (1025, 1))
    with pytest.raises(pkg.MslamHipError) as e:
        ctx.bundle_adjust_global(many, sc["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"])
    assert e.value.code == pkg.E_INVALID
    with pytest.raises(pkg.MslamHipError) as e:
        ctx.bundle_adjust_global(sc["poses"], sc["landmarks"], np.where(np.arange(len(sc["obs_kf"])) == 7, 9, sc["obs_kf"]),
                                 sc["obs_lm"], sc["obs_cam"], sc["fixed"])
    assert e.value.code == pkg.E_INVALID
    _check("BAG clean", "traj:9", _solve(ctx, sc), sc, qr, dist, mask)
    none = np.zeros(0, np.int32)
    ok = ctx.bundle_adjust_global(many[:1024], sc["landmarks"], none, none, np.zeros((0, 3)))     # K = 1024 is inside the bound
    assert ok["termination"] == 0 and ok["final_cost"] == 0.0


def test_failure_leaves_the_state_and_judges_the_outliers_at_the_input(ctx, pkg):
    for name in ("traj:66", "gross80"):
        clean = bg.scene(name)
        sc = {k: np.array(v) for k, v in clean.items()}
        sc["obs_cam"][5, 1] = np.nan
        got = _solve(ctx, sc)
        assert got["termination"] == 2 and got["iterations"] == 0 and not np.isfinite(got["initial_cost"])
        assert got["poses"].tobytes() == sc["poses"].tobytes() and got["landmarks"].tobytes() == sc["landmarks"].tobytes()
        with np.errstate(all="ignore"):
            r = ba_ref.residuals(sc["poses"], sc["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"])
            norms = np.sqrt(np.sum(r * r, 1))
            mask = ba_ref.outliers(sc["poses"], sc["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"])
        assert not np.all(np.isfinite(norms)) and np.min(np.abs(norms[np.isfinite(norms)] - 0.15)) > 1e-6
        assert mask.any() or name != "gross80"
        assert np.array_equal(got["outlier"], mask) and got["n_outliers"] == int(mask.sum())
    c = pkg.Context(width=0, height=0)
    _same_bits(_solve(ctx, clean), _solve(c, clean))         # the context is usable afterwards
    c.close()


def test_backend_global_ba(pkg):
    sc = bg.scene("traj:66")
    K = len(sc["poses"])
    c = pkg.Context(width=0, height=0, max_keypoints=64)
    be = pkg.HipBackend(c, global_solver=True)
    rng = np.random.default_rng(66)
    kf_id = np.concatenate([[5000], rng.permutation(np.arange(100, 100 + K - 1))])       # the constant keyframe: first added, sorted last
    lm_id = 10 ** 12 + 7 * rng.permutation(len(sc["landmarks"]))
    for k in range(K):
        m = np.flatnonzero(sc["obs_kf"] == k)
        be.add_keyframe(int(kf_id[k]), sc["poses"][k], lm_id[sc["obs_lm"][m]], sc["obs_cam"][m])
    ids = sorted(int(v) for v in kf_id)
    poses, fixed, lids, lm, okf, olm, ocam = be.problem(ids)
    assert fixed.tolist() == [0] * (K - 1) + [1] and len(okf) == len(sc["obs_kf"])
    qr = ba_ref.bundle_adjust(poses, lm, okf, olm, ocam, fixed, linear_solver="qr")
    sch = ba_ref.bundle_adjust(poses, lm, okf, olm, ocam, fixed, linear_solver="schur")
    dist = max(np.max(np.abs(qr["poses"] - sch["poses"])), np.max(np.abs(qr["landmarks"] - sch["landmarks"])))
    mask = ba_ref.outliers(qr["poses"], qr["landmarks"], okf, olm, ocam)
    before = be.poses[ids[0]].copy()
    got = be.global_ba()
    _check("BAG backend", "traj:66", got, dict(obs_kf=okf), qr, dist, mask)
    assert got["keyframes"] == ids and got["landmark_ids"].tolist() == lids
    for k, id in enumerate(ids):
        assert be.poses[id].tobytes() == got["poses"][k].tobytes()
    assert be.poses[5000].tobytes() == sc["poses"][0].tobytes() and be.poses[ids[0]].tobytes() != before.tobytes()
    for i, l in enumerate(lids):
        assert be.landmarks[l].tobytes() == got["landmarks"][i].tobytes()
    # the refined landmarks reach a keyframe store that holds some of the same ids
    store = {3: np.array(lids[:40], np.int64), 4: np.array(lids[20:60] + [7], np.int64)}
    for k, l in store.items():
        c.kf_add(k, rng.integers(0, 256, (len(l), 32), dtype=np.uint8), rng.normal(size=(len(l), 3)), lids=l)
    assert c.kf_update_world(got["landmark_ids"], got["landmarks"]) == 80
    back = {l: i for i, l in enumerate(lids)}
    for k, l in store.items():
        world = c.kf_read(k)[1]
        for j, v in enumerate(l.tolist()):
            if v in back:
                assert world[j].tobytes() == got["landmarks"][back[v]].tobytes(), (k, j)
    # the default backend keeps its cap on the same map
    be.global_solver = False
    with pytest.raises(pkg.MslamHipError) as e:
        be.global_ba()
    assert e.value.code == pkg.E_CAPACITY
    c.close()
