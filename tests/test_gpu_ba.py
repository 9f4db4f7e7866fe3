"""Bundle adjustment on the MI355X (k_ba.hip) through Context.bundle_adjust, against tests/ba_ref.py's QR solve on the cases
of tests/ba_cases.py (tests/test_ba.py shows on the CPU that every case takes the path it is named for and that the two
CPU solvers agree on it); determinism, also of a small solve after a large one on one context; FAILURE and non-finite values
outside the problem; outlier thresholds; HipBackend's problem / global_ba / neighbours; mslam_hip_kf_update_world against a
numpy restatement; HipKeyframeTracker(local_ba).

Bounds.  State: |x_gpu - x_qr|_inf <= max(1e-9, 1000 |x_schur - x_qr|_inf), the rule of tests/test_gpu_mse_pnp_edges.py: the
distance of two correct CPU solvers, times 1000 for the kernels' other summation orders.  Costs: 1e-6 relative, plus what
the state bound itself allows at a minimum: there the cost is stationary, so two states B apart differ in cost by the
second-order term only, at most M (j B)^2 / 2 with j = 2 |X - p| + 2 <= 12 the largest row norm of a residual's Jacobian
in these scenes (|X - p| <= 5 m).  On a noise-free scene the final cost is the square of the last step's leftover (1e-18
and below) and has no relative precision at all; on the noisy scenes the extra term is below 1e-13 and changes nothing.
A start cost of exactly 0 in the reference (at_minimum: the observations were made by the reference's own residual at the
very state the solve starts from, so they cancel to the last bit there) has no relative precision either.  The kernels divide
by |q|^2 where the reference's jets multiply by its reciprocal, so their residuals are rounded otherwise: each component of
rot(q^-1, X) - rot(q^-1, p) - obs is some 20 operations on values of at most 5 m, an error of at most ROUNDING = 20 eps 5 m
= 2.2e-14, and the start cost at most M 3 ROUNDING^2 / 2 (1.4e-25 for the 195 observations; measured 1.7e-30).  Only that
case takes this term: every other start cost is positive and keeps the relative bound alone."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_cases  # noqa: E402
import ba_ref  # noqa: E402
import track_ref as tr  # noqa: E402

pytestmark = pytest.mark.gpu
ROUNDING = 20 * np.finfo(np.float64).eps * 5.0


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(width=0, height=0)
    yield c
    c.close()


def _solve(ctx, sc, **kw):
    return ctx.bundle_adjust(sc["poses"], sc["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"], sc["fixed"],
                             max_iterations=sc.get("max_iterations", 100), **kw)


@pytest.mark.parametrize("name", ba_cases.ALL)
def test_against_the_qr_reference(ctx, name):
    sc, qr, sch, dist, mask, margin = ba_cases.reference(name)
    got = _solve(ctx, sc)
    bound = max(1e-9, 1000.0 * dist)
    dx = max(float(np.max(np.abs(got["poses"] - qr["poses"]), initial=0.0)),
             float(np.max(np.abs(got["landmarks"] - qr["landmarks"]), initial=0.0)))
    second_order = len(sc["obs_kf"]) * (12.0 * bound) ** 2 / 2.0
    zero_cost = 0.0 if qr["initial_cost"] > 0.0 else len(sc["obs_kf"]) * 3 * ROUNDING ** 2 / 2.0
    print("BA %-28s family %-9s term %d/%d it %d/%d rejected %d/%d cost0 %.17g/%.17g cost %.6g/%.6g dx %.3e bound %.3e" % (
        name, ba_cases.family(name), got["termination"], qr["termination"], got["iterations"], qr["iterations"],
        got["rejected_steps"], qr["trace"]["rejected"], got["initial_cost"], qr["initial_cost"], got["final_cost"],
        qr["final_cost"], dx, bound))
    assert got["termination"] == qr["termination"]
    assert abs(got["iterations"] - qr["iterations"]) <= 1
    assert got["invalid_steps"] == 0
    assert abs(got["initial_cost"] - qr["initial_cost"]) <= 1e-6 * qr["initial_cost"] + zero_cost
    assert abs(got["final_cost"] - qr["final_cost"]) <= 1e-6 * qr["final_cost"] + second_order
    assert dx <= bound
    assert np.array_equal(got["outlier"], mask) and got["n_outliers"] == int(mask.sum())
    if name == "cap3":      # NO_CONVERGENCE, and the state reached is written
        assert got["termination"] == 1 and got["iterations"] == 3
        assert np.max(np.abs(got["poses"] - sc["poses"])) > 1e-3
    if name == "empty":
        assert got["final_cost"] == 0.0 and np.array_equal(got["poses"], sc["poses"]) and np.array_equal(got["landmarks"], sc["landmarks"])
    if name in ("all_fixed", "k1_fixed"):
        assert np.array_equal(got["poses"], sc["poses"])
    if name.startswith("cap"):        # the cap is exact: one iteration more or fewer is another solve
        assert got["iterations"] == qr["iterations"]
    if name == "cap0":                # nothing may move
        assert got["termination"] == 1 and got["iterations"] == 0 and got["final_cost"] == got["initial_cost"]
        assert got["poses"].tobytes() == np.asarray(sc["poses"], np.float64).tobytes()
        assert got["landmarks"].tobytes() == np.asarray(sc["landmarks"], np.float64).tobytes()
    if name == "at_minimum":          # the gradient test of iteration 0, with `successful` as the host set it
        assert got["termination"] == 0 and got["iterations"] == 0
        assert got["poses"].tobytes() == sc["poses"].tobytes() and got["landmarks"].tobytes() == sc["landmarks"].tobytes()
    if name in ("fixed_middle", "fixed_two"):
        for k in (1,) + tuple(np.flatnonzero(sc["fixed"])):
            assert got["poses"][k].tobytes() == sc["poses"][k].tobytes(), k


def test_constant_and_unobserved_blocks_are_untouched(ctx):
    sc = ba_cases.scene("fixed:3,65,5")
    poses = np.concatenate([sc["poses"], [[0, 0, 0, 1, 9, 9, 9]]])        # a keyframe and a landmark without observations
    lms = np.concatenate([sc["landmarks"], [[7.0, 7.0, 7.0]]])
    got = ctx.bundle_adjust(poses, lms, sc["obs_kf"], sc["obs_lm"], sc["obs_cam"], np.append(sc["fixed"], 0))
    base = _solve(ctx, sc)
    assert np.array_equal(got["poses"][0], sc["poses"][0]) and np.array_equal(got["poses"][3], poses[3])
    assert np.array_equal(got["landmarks"][65], lms[65])
    assert np.array_equal(got["poses"][:3], base["poses"]) and np.array_equal(got["landmarks"][:65], base["landmarks"])


def _same_bits(a, b):
    for k in ("poses", "landmarks", "outlier"):
        assert a[k].tobytes() == b[k].tobytes(), k
    for k in ("termination", "iterations", "rejected_steps", "invalid_steps", "n_outliers"):
        assert a[k] == b[k], k
    for k in ("initial_cost", "final_cost"):
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), k


@pytest.mark.parametrize("name", ["fixed:8,200,10", "rejected", "k64", "twice_in_keyframe", "blocks:16385", "k64_dense", "fixed_middle"])
def test_a_second_call_returns_the_same_bits(ctx, name):
    sc = ba_cases.scene(name)
    _same_bits(_solve(ctx, sc), _solve(ctx, sc))


def test_invalid_arguments_then_a_clean_call(ctx, pkg):
    sc = ba_cases.scene("fixed:2,20,5")

    def call(**over):
        a = dict(sc)
        a.update(over)
        return _solve(ctx, a)
    for bad in (dict(obs_kf=np.where(np.arange(40) == 7, 2, sc["obs_kf"])), dict(obs_lm=np.where(np.arange(40) == 0, -1, sc["obs_lm"])),
                dict(obs_lm=np.where(np.arange(40) == 39, 20, sc["obs_lm"]))):
        with pytest.raises(pkg.MslamHipError) as e:
            call(**bad)
        assert e.value.code == pkg.E_INVALID
    q = sc["poses"].copy()
    q[1, :4] *= 1.0 + 3e-6
    with pytest.raises(pkg.MslamHipError) as e:
        call(poses=q)
    assert e.value.code == pkg.E_INVALID
    many = np.tile([0, 0, 0, 1.0, 0, 0, 0], (65, 1))
    with pytest.raises(pkg.MslamHipError) as e:
        ctx.bundle_adjust(many, sc["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"])
    assert e.value.code == pkg.E_INVALID
    qr = ba_cases.reference("fixed:2,20,5")[1]
    got = call()
    assert got["termination"] == qr["termination"] and np.max(np.abs(got["poses"] - qr["poses"])) <= 1e-9
    q[1, :4] = sc["poses"][1, :4] * (1.0 + 5e-7)          # inside the 1e-6 band: accepted
    assert call(poses=q)["termination"] == 0


def test_a_smaller_problem_after_a_larger_one(ctx, pkg):
    """the workspace only grows and is carved afresh per call: what a larger solve left in it must not reach a smaller one.
    Every result equals, bit for bit, the same case's on a context that has solved nothing else."""
    fresh = {}
    for name in ("blocks:16385", "fixed:2,20,5", "k64_dense"):
        c = pkg.Context(width=0, height=0)
        fresh[name] = _solve(c, ba_cases.scene(name))
        c.close()
    c = pkg.Context(width=0, height=0)
    for name in ("blocks:16385", "fixed:2,20,5", "k64_dense", "fixed:2,20,5"):
        _same_bits(_solve(c, ba_cases.scene(name)), fresh[name])
    c.close()


def _bad_obs(v):
    def f(sc):
        sc["obs_cam"][5, 1] = v
    return f


def _bad_landmark(sc):
    assert np.any(sc["obs_lm"] == 9)
    sc["landmarks"][9, 0] = np.nan


def _bad_constant_pose(sc):
    assert sc["fixed"][0] and np.any(sc["obs_kf"] == 0)
    sc["poses"][0, 4] = np.nan


def test_failure_leaves_the_state_and_judges_the_outliers_at_the_input(ctx, pkg):
    """termination 2 (MSLAM_HIP_E_NO_MODEL) is a result: a non-finite cost at the start.  NaN != NaN, so bytes are compared."""
    clean = ba_cases.scene("gross_outliers")
    for spoil in (_bad_obs(np.nan), _bad_obs(np.inf), _bad_landmark, _bad_constant_pose):
        sc = {k: np.array(v) for k, v in clean.items()}
        spoil(sc)
        got = _solve(ctx, sc)
        assert got["termination"] == 2 and got["iterations"] == 0
        assert got["poses"].tobytes() == sc["poses"].tobytes() and got["landmarks"].tobytes() == sc["landmarks"].tobytes()
        assert not np.isfinite(got["initial_cost"])
        with np.errstate(all="ignore"):
            r = ba_ref.residuals(sc["poses"], sc["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"])
            norms = np.sqrt(np.sum(r * r, 1))
            mask = ba_ref.outliers(sc["poses"], sc["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"])
            ref = ba_ref.solve_scene(sc)
        assert not np.all(np.isfinite(norms))
        assert np.min(np.abs(norms[np.isfinite(norms)] - 0.15)) > 1e-6 and mask.any()
        assert np.array_equal(got["outlier"], mask) and got["n_outliers"] == int(mask.sum())
        assert ref["termination"] == ba_ref.FAILURE and ref["reason"] == "initial evaluation failed"
    c = pkg.Context(width=0, height=0)
    _same_bits(_solve(ctx, clean), _solve(c, clean))
    c.close()


def test_non_finite_values_outside_the_problem_do_not_matter(ctx):
    sc = ba_cases.scene("fixed:3,65,5")
    poses = np.concatenate([sc["poses"], [[0, 0, 0, 1, np.nan, 0, 0]]])       # unobserved and not constant
    lms = np.concatenate([sc["landmarks"], [[np.nan, np.inf, 0.0]]])          # unobserved
    got = ctx.bundle_adjust(poses, lms, sc["obs_kf"], sc["obs_lm"], sc["obs_cam"], np.append(sc["fixed"], 0))
    base = _solve(ctx, sc)
    assert base["termination"] == 0
    assert got["poses"][:3].tobytes() == base["poses"].tobytes() and got["landmarks"][:65].tobytes() == base["landmarks"].tobytes()
    assert got["poses"][3].tobytes() == poses[3].tobytes() and got["landmarks"][65].tobytes() == lms[65].tobytes()
    for k in ("termination", "iterations", "rejected_steps", "invalid_steps", "n_outliers"):
        assert got[k] == base[k], k
    for k in ("initial_cost", "final_cost"):
        assert np.float64(got[k]).tobytes() == np.float64(base[k]).tobytes(), k
    assert np.array_equal(got["outlier"], base["outlier"])


def _widest_gap(norms):
    """-> (a threshold in the middle of the widest gap between two adjacent sorted norms, the gap)"""
    s = np.sort(norms)
    i = int(np.argmax(np.diff(s)))
    return float((s[i] + s[i + 1]) / 2.0), float(s[i + 1] - s[i])


def test_outlier_threshold_and_fixed_none(ctx):
    sc, qr = ba_cases.reference("gross_outliers")[:2]
    r = ba_ref.residuals(qr["poses"], qr["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"])
    norms = np.sqrt(np.sum(r * r, 1))
    assert norms.min() > 1e-6             # 1000 x the state bound: no residual is zero at the kernels' solution either
    got = _solve(ctx, sc, outlier_threshold=0.0)
    assert got["outlier"].all() and got["n_outliers"] == len(norms)
    got = _solve(ctx, sc, outlier_threshold=1e9)
    assert not got["outlier"].any() and got["n_outliers"] == 0
    thr, gap = _widest_gap(norms)
    assert gap > 1e-6
    got = _solve(ctx, sc, outlier_threshold=thr)
    assert 0 < int(np.sum(norms > thr)) < len(norms)
    assert np.array_equal(got["outlier"], norms > thr) and got["n_outliers"] == int(np.sum(norms > thr))
    sc = ba_cases.scene("free:3,65,5")
    assert not sc["fixed"].any()
    a = ctx.bundle_adjust(sc["poses"], sc["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"], None)
    _same_bits(a, _solve(ctx, sc))


# ---- HipBackend ---------------------------------------------------------------------------------------------------------------

def _rotate(q, v):
    """R(q) v for a unit quaternion x y z w, rows of v"""
    u, w = q[:3], q[3]
    uv = 2.0 * np.cross(u, v)
    return v + w * uv + np.cross(u, uv)


def test_backend_problem_global_ba_and_neighbours(pkg):
    sc = ba_cases.scene("fixed:3,65,5")
    c = pkg.Context(width=0, height=0)
    be = pkg.HipBackend(c)
    kf_id = (40, 7, 19)                                  # the constant keyframe is added first and sorts last
    lm_id = 10 ** 12 + 7 * (64 - np.arange(65))
    first = {}
    for k, id in enumerate(kf_id):
        m = np.flatnonzero(sc["obs_kf"] == k)
        be.add_keyframe(id, sc["poses"][k], lm_id[sc["obs_lm"][m]], sc["obs_cam"][m])
        for l, cam in zip(sc["obs_lm"][m].tolist(), sc["obs_cam"][m]):
            first.setdefault(l, _rotate(sc["poses"][k, :4], cam) + sc["poses"][k, 4:])
    order = [1, 2, 0]                                    # scene keyframes in the order of their sorted ids 7, 19, 40
    poses, fixed, lids, lm, okf, olm, ocam = be.problem(sorted(kf_id))
    assert poses.tobytes() == sc["poses"][order].tobytes() and fixed.tolist() == [0, 0, 1]
    assert sorted(lids) == sorted(lm_id.tolist()) and len(lids) == 65
    back = {int(v): l for l, v in enumerate(lm_id)}
    for i, l in enumerate(lids):
        assert np.max(np.abs(lm[i] - first[back[l]])) <= 1e-12, l
    assert np.bincount(okf, minlength=3).tolist() == [int(np.sum(sc["obs_kf"] == k)) for k in order]
    for k, id in enumerate(sorted(kf_id)):               # every keyframe's observations, in the order they were added
        m, mine = np.flatnonzero(sc["obs_kf"] == order[k]), okf == k
        assert [lids[i] for i in olm[mine]] == lm_id[sc["obs_lm"][m]].tolist() and ocam[mine].tobytes() == sc["obs_cam"][m].tobytes()

    qr = ba_ref.bundle_adjust(poses, lm, okf, olm, ocam, fixed, linear_solver="qr")
    sch = ba_ref.bundle_adjust(poses, lm, okf, olm, ocam, fixed, linear_solver="schur")
    bound = max(1e-9, 1000.0 * max(np.max(np.abs(qr["poses"] - sch["poses"])), np.max(np.abs(qr["landmarks"] - sch["landmarks"]))))
    r = ba_ref.residuals(qr["poses"], qr["landmarks"], okf, olm, ocam)
    thr, gap = _widest_gap(np.sqrt(np.sum(r * r, 1)))    # a threshold that marks some observations and not others
    mask = np.sqrt(np.sum(r * r, 1)) > thr
    assert gap > 1e-6 and 0 < mask.sum() < len(mask)
    be.outlier_threshold = thr
    got = be.global_ba()
    dx = max(np.max(np.abs(got["poses"] - qr["poses"])), np.max(np.abs(got["landmarks"] - qr["landmarks"])))
    print("BA backend term %d/%d it %d/%d cost %.6g/%.6g dx %.3e bound %.3e" % (
        got["termination"], qr["termination"], got["iterations"], qr["iterations"], got["final_cost"], qr["final_cost"], dx, bound))
    assert got["termination"] == qr["termination"] == 0 and abs(got["iterations"] - qr["iterations"]) <= 1 and got["invalid_steps"] == 0
    assert abs(got["initial_cost"] - qr["initial_cost"]) <= 1e-6 * qr["initial_cost"]
    assert abs(got["final_cost"] - qr["final_cost"]) <= 1e-6 * qr["final_cost"] + len(okf) * (12.0 * bound) ** 2 / 2.0
    assert dx <= bound
    assert got["keyframes"] == sorted(kf_id) and got["landmark_ids"].tolist() == lids
    for k, id in enumerate(sorted(kf_id)):
        assert be.poses[id].tobytes() == got["poses"][k].tobytes()
    assert be.poses[40].tobytes() == sc["poses"][0].tobytes()
    for i, l in enumerate(lids):
        assert be.landmarks[l].tobytes() == got["landmarks"][i].tobytes()
    assert np.array_equal(got["outlier"], mask)
    assert got["outlier_observations"] == [(sorted(kf_id)[k], lids[l]) for k, l in zip(okf[mask], olm[mask])]

    # FAILURE keeps the stored state
    be.add_keyframe(50, [0, 0, 0, 1, 0.1, 0, 0], [lids[3]], [[np.nan, 0.0, 2.0]])
    before = ({k: v.tobytes() for k, v in be.poses.items()}, {l: v.tobytes() for l, v in be.landmarks.items()})
    got = be.global_ba()
    assert got["termination"] == 2 and got["keyframes"] == [7, 19, 40, 50]
    assert before == ({k: v.tobytes() for k, v in be.poses.items()}, {l: v.tobytes() for l, v in be.landmarks.items()})
    c.close()

    # a star of 70 keyframes: the neighbourhood is all of them, the 64 largest ids are kept; 65 keyframes are too many for
    # global_ba, which says so before it touches the context (there is none)
    be = pkg.HipBackend(None)
    for id in range(70):
        be.add_keyframe(id, [0, 0, 0, 1, 0, 0, 0], [], np.zeros((0, 3)))
        if id == 63:
            assert be.neighbours(0, {0: set(range(1, 64))}) == list(range(64))
        if id == 64:
            with pytest.raises(pkg.MslamHipError) as e:
                be.global_ba()
            assert e.value.code == pkg.E_CAPACITY
    graph = {0: set(range(1, 70))}
    graph.update({k: {0} for k in range(1, 70)})
    assert be.neighbours(0, graph) == list(range(6, 70))
    assert be.neighbours(3, graph) == list(range(6, 70))      # a leaf reaches the centre, and through it every other leaf
    assert be.neighbours(3, graph, deep_level=0) == [0, 3]


# ---- mslam_hip_kf_update_world ------------------------------------------------------------------------------------------------

def _update_ref(store, ids, xyz):
    """every landmark whose id is listed takes the point of the id's last place in the list -> (store, count)"""
    last = {int(l): i for i, l in enumerate(ids)}
    out, n = {}, 0
    for k, (lids, w) in store.items():
        w = w.copy()
        for i, l in enumerate(lids.tolist()):
            if l in last:
                w[i] = xyz[last[l]]
                n += 1
        out[k] = (lids, w)
    return out, n


def test_kf_update_world(pkg):
    c = pkg.Context(width=0, height=0, max_keypoints=320)
    rng = np.random.default_rng(5)
    lids = {3: np.arange(0, 300), 4: np.concatenate([np.arange(200, 400), [250, 250]]), 9: np.arange(1000, 1070)}
    store = {k: (np.asarray(v, np.int64), rng.normal(size=(len(v), 3))) for k, v in lids.items()}
    for k, (l, w) in store.items():
        c.kf_add(k, rng.integers(0, 256, (len(l), 32), dtype=np.uint8), w, lids=l)

    def check(ids, xyz):
        nonlocal store
        store, n = _update_ref(store, ids, xyz)
        assert c.kf_update_world(ids, xyz) == n
        for k, (l, w) in store.items():
            assert np.array_equal(c.kf_read_ids(k), l)
            assert c.kf_read(k)[1].tobytes() == w.tobytes(), k
        return n
    assert check(np.zeros(0, np.int64), np.zeros((0, 3))) == 0                                     # n = 0
    assert check(np.array([5000, 6000]), rng.normal(size=(2, 3))) == 0                            # ids the store does not hold
    ids = np.concatenate([np.arange(190, 260), [250, 1069, 7777]])                                # shared ids, a repeat inside entry 4, an id listed twice
    assert check(ids, rng.normal(size=(len(ids), 3))) == 70 + 60 + 2 + 1
    c.kf_remove(3)
    del store[3]
    assert check(np.arange(0, 400), rng.normal(size=(400, 3))) == 202                              # a removed entry's slot is not counted
    c.close()


# ---- the tracker --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sequence():
    return tr.make_sequence()


def _run(pkg, seq, **kw):
    c = pkg.Context(width=0, height=0, max_keypoints=4096)
    t = pkg.HipKeyframeTracker(c, focal=tr.CAM[:2], principal=tr.CAM[2:], **dict(tr.SEQ_PARAMS, **kw))
    return c, t, [t.processSensorData(fr["desc"], fr["xy"], fr["depth"]) for fr in seq["frames"]]


def test_tracker_with_local_ba(pkg, sequence):
    c, t, rows = _run(pkg, sequence, local_map_depth=2, local_ba=True)
    assert len(t.ba_results) == len(t.ids) - 1 >= 1
    solved = {}
    for ba in t.ba_results:
        print("local BA keyframes %s M %d term %d it %d cost %.6g -> %.6g outliers %d written %d" % (
            ba["keyframes"], len(ba["outlier"]), ba["termination"], ba["iterations"], ba["initial_cost"], ba["final_cost"],
            ba["n_outliers"], ba.get("n_written", -1)))
        assert ba["termination"] in (0, 1)
        assert ba["final_cost"] < ba["initial_cost"]
        assert ba["n_written"] >= len(ba["landmark_ids"])
        solved.update(zip(ba["landmark_ids"].tolist(), ba["landmarks"]))
    assert solved
    for k in t.ids:          # the store holds the refined points, bit for bit
        lids, world = c.kf_read_ids(k), c.kf_read(k)[1]
        for l, w in zip(lids.tolist(), world):
            if l in solved:
                assert w.tobytes() == solved[l].tobytes() == t.backend.landmarks[l].tobytes(), (k, l)
    assert t.backend.poses[0].tolist() == [0, 0, 0, 1, 0, 0, 0]      # the first keyframe is constant
    c.close()


def test_tracker_with_local_ba_over_windows(pkg, sequence):
    c = pkg.Context(width=0, height=0, max_keypoints=4096)
    t = pkg.HipKeyframeTracker(c, focal=tr.CAM[:2], principal=tr.CAM[2:], local_map_depth=2, local_ba=True, **tr.SEQ_PARAMS)
    fr = sequence["frames"]
    rows = t.process_window([f["desc"] for f in fr], [f["xy"] for f in fr], [f["depth"] for f in fr], window=4)
    assert len(rows) == len(fr) and len(t.ba_results) == len(t.ids) - 1 >= 1
    for ba in t.ba_results:
        assert ba["termination"] in (0, 1) and ba["final_cost"] < ba["initial_cost"] and ba["n_written"] >= len(ba["landmark_ids"])
    c.close()


def test_tracker_without_local_ba_is_todays_tracker(pkg, sequence):
    c0, t0, a = _run(pkg, sequence, local_map_depth=2)
    c1, t1, b = _run(pkg, sequence, local_map_depth=2, local_ba=False)
    assert t1.backend is None and t1.ba_results == []
    for f, (x, y) in enumerate(zip(a, b)):
        assert (x["tracked"], x["n_inliers"], x["keyframe"], x["reference"], x["relocalized"]) == \
               (y["tracked"], y["n_inliers"], y["keyframe"], y["reference"], y["relocalized"]), f
        assert x["R"].tobytes() == y["R"].tobytes() and x["tvec"].tobytes() == y["tvec"].tobytes() and x["rvec"].tobytes() == y["rvec"].tobytes(), f
    for k in t0.ids:
        assert c0.kf_read(k)[1].tobytes() == c1.kf_read(k)[1].tobytes()
    with pytest.raises(pkg.MslamHipError):
        pkg.HipKeyframeTracker(c0, local_ba=True)           # needs the graph
    c0.close()
    c1.close()
