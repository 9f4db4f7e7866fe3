"""Bundle adjustment on the MI355X (k_ba.hip) through Context.bundle_adjust, against tests/ba_ref.py's QR solve on the cases
of tests/ba_cases.py (tests/test_ba.py shows on the CPU that every case takes the path it is named for and that the two
CPU solvers agree on it); determinism; mslam_hip_kf_update_world against a numpy restatement; HipKeyframeTracker(local_ba).

Bounds.  State: |x_gpu - x_qr|_inf <= max(1e-9, 1000 |x_schur - x_qr|_inf), the rule of tests/test_gpu_mse_pnp_edges.py: the
distance of two correct CPU solvers, times 1000 for the kernels' other summation orders.  Costs: 1e-6 relative, plus what
the state bound itself allows at a minimum: there the cost is stationary, so two states B apart differ in cost by the
second-order term only, at most M (j B)^2 / 2 with j = 2 |X - p| + 2 <= 12 the largest row norm of a residual's Jacobian
in these scenes (|X - p| <= 5 m).  On a noise-free scene the final cost is the square of the last step's leftover (1e-18
and below) and has no relative precision at all; on the noisy scenes the extra term is below 1e-13 and changes nothing."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_cases  # noqa: E402
import ba_ref  # noqa: E402
import track_ref as tr  # noqa: E402

pytestmark = pytest.mark.gpu


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
    print("BA %-28s family %-9s term %d/%d it %d/%d rejected %d/%d cost0 %.17g/%.17g cost %.6g/%.6g dx %.3e bound %.3e" % (
        name, ba_cases.family(name), got["termination"], qr["termination"], got["iterations"], qr["iterations"],
        got["rejected_steps"], qr["trace"]["rejected"], got["initial_cost"], qr["initial_cost"], got["final_cost"],
        qr["final_cost"], dx, bound))
    assert got["termination"] == qr["termination"]
    assert abs(got["iterations"] - qr["iterations"]) <= 1
    assert got["invalid_steps"] == 0
    assert abs(got["initial_cost"] - qr["initial_cost"]) <= 1e-6 * qr["initial_cost"]
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


def test_constant_and_unobserved_blocks_are_untouched(ctx):
    sc = ba_cases.scene("fixed:3,65,5")
    poses = np.concatenate([sc["poses"], [[0, 0, 0, 1, 9, 9, 9]]])        # a keyframe and a landmark without observations
    lms = np.concatenate([sc["landmarks"], [[7.0, 7.0, 7.0]]])
    got = ctx.bundle_adjust(poses, lms, sc["obs_kf"], sc["obs_lm"], sc["obs_cam"], np.append(sc["fixed"], 0))
    base = _solve(ctx, sc)
    assert np.array_equal(got["poses"][0], sc["poses"][0]) and np.array_equal(got["poses"][3], poses[3])
    assert np.array_equal(got["landmarks"][65], lms[65])
    assert np.array_equal(got["poses"][:3], base["poses"]) and np.array_equal(got["landmarks"][:65], base["landmarks"])


@pytest.mark.parametrize("name", ["fixed:8,200,10", "rejected", "k64", "twice_in_keyframe"])
def test_a_second_call_returns_the_same_bits(ctx, name):
    sc = ba_cases.scene(name)
    a, b = _solve(ctx, sc), _solve(ctx, sc)
    for k in ("poses", "landmarks", "outlier"):
        assert a[k].tobytes() == b[k].tobytes(), k
    for k in ("termination", "iterations", "rejected_steps", "invalid_steps", "n_outliers"):
        assert a[k] == b[k], k
    assert np.float64(a["initial_cost"]).tobytes() == np.float64(b["initial_cost"]).tobytes()
    assert np.float64(a["final_cost"]).tobytes() == np.float64(b["final_cost"]).tobytes()


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
