"""Bundle adjustment with a loss function on the MI355X (k_ba.hip's *_loss kernels, mslam_hip_set_ba_loss) through
Context.set_ba_loss / bundle_adjust / bundle_adjust_global, against tests/ba_loss_ref.py's QR solve (tests/test_ba_loss.py
shows on the CPU that the restatement minimises the stated cost and that its scenes are what they are named for).

Bounds: the rule of tests/test_gpu_ba.py, unchanged.  State: |x_gpu - x_qr|_inf <= max(1e-9, 1000 |x_schur - x_qr|_inf).
Costs: 1e-6 relative plus the second-order term M (12 B)^2 / 2 that file derives for two states B apart at a minimum; a loss
only lowers the curvature (rho' <= 1, rho'' <= 0), so the term still bounds it.  The outlier mask is compared where the
restatement's |r| is further than 1e-6 (1000 x the 1e-9 state bound) from the threshold.

Exact checks, derived from the formulas and not measured: Huber with a = 1e6 has s <= b for every observation, so rho = s and
w = 1.0, and a product with 1.0 keeps its bits: the result equals loss NONE's byte for byte although other kernels ran.  In
threshold_scene the start cost is one term, rho / 2, and every other residual is exactly 0: with |r|^2 == b Huber's inlier
branch gives b / 2 exactly.  Huber's two branches join with equal value and slope at b, so at nextafter the two costs agree to
rounding and the cost cannot tell the branch: the restatement's predicate s > b tells it, and the kernel's cost is held to
the restatement's on both sides."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_cases  # noqa: E402
import ba_loss_ref as lr  # noqa: E402
import ba_ref  # noqa: E402
import pose_graph_cases as pc  # noqa: E402
import track_ref as tr  # noqa: E402

pytestmark = pytest.mark.gpu
A = lr.SCALE
KINDS = ["huber", "cauchy"]
ENTRIES = ["bundle_adjust", "bundle_adjust_global"]


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(width=0, height=0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def no_loss_left_behind(ctx):
    yield
    ctx.set_ba_loss("none")


def _solve(ctx, sc, entry="bundle_adjust", **kw):
    return getattr(ctx, entry)(sc["poses"], sc["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"], sc["fixed"], **kw)


def _same_bits(a, b):
    for k in ("poses", "landmarks", "outlier"):
        assert a[k].tobytes() == b[k].tobytes(), k
    for k in ("termination", "iterations", "rejected_steps", "invalid_steps", "n_outliers"):
        assert a[k] == b[k], k
    for k in ("initial_cost", "final_cost"):
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), k


def _against(ctx, name, kind, entry):
    sc, qr, dist, mask, margin = lr.reference(name, kind)
    ctx.set_ba_loss(kind, A)
    got = _solve(ctx, sc, entry)
    bound = max(1e-9, 1000.0 * dist)
    dx = max(float(np.max(np.abs(got["poses"] - qr["poses"]))), float(np.max(np.abs(got["landmarks"] - qr["landmarks"]))))
    second_order = len(sc["obs_kf"]) * (12.0 * bound) ** 2 / 2.0
    sure = margin > 1e-6
    print("BA loss %-17s %-6s %-20s term %d/%d it %d/%d rejected %d/%d cost0 %.17g/%.17g cost %.17g/%.17g dx %.3e bound %.3e unsure %d" % (
        name, kind, entry, got["termination"], qr["termination"], got["iterations"], qr["iterations"], got["rejected_steps"],
        qr["trace"]["rejected"], got["initial_cost"], qr["initial_cost"], got["final_cost"], qr["final_cost"], dx, bound,
        int(np.sum(~sure))))
    assert got["termination"] == qr["termination"] and got["iterations"] == qr["iterations"]
    assert got["invalid_steps"] == 0
    assert abs(got["initial_cost"] - qr["initial_cost"]) <= 1e-6 * qr["initial_cost"]
    assert abs(got["final_cost"] - qr["final_cost"]) <= 1e-6 * qr["final_cost"] + second_order
    assert dx <= bound
    assert np.array_equal(got["outlier"][sure], mask[sure])
    return sc, qr, got


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["out:3,24", "out:4,40"])
def test_against_the_restatement(ctx, name, kind, entry):
    _against(ctx, name, kind, entry)


@pytest.mark.parametrize("kind", KINDS)
def test_block_and_stride_edges(ctx, kind):
    """K = 2, L = 300, M = 600: bad observations at positions >= 256 of the free keyframe's row, on landmarks >= 256, and on
    the last observation of a tail block (tests/test_ba_loss.py checks the scene is that)"""
    _against(ctx, "edges", kind, "bundle_adjust")


@pytest.mark.parametrize("kind", KINDS)
def test_constant_keyframe_weights(ctx, kind):
    """bad observations on the constant keyframe only: k_ba_landmarks alone sees their weights.  Unweighted there, the
    landmarks they touch would land more than 1e-3 from the restatement's (tests/test_ba_loss.py: the distance of the
    solutions with and without a loss)"""
    sc, qr, got = _against(ctx, "fixed_only", kind, "bundle_adjust")
    touched = np.unique(sc["obs_lm"][sc["bad"]])
    assert np.max(np.abs(got["landmarks"][touched] - qr["landmarks"][touched])) <= 1e-9


@pytest.mark.parametrize("kind", KINDS)
def test_a_landmark_whose_every_observation_is_bad(ctx, kind):
    sc, qr, got = _against(ctx, "all_bad_landmark", kind, "bundle_adjust")
    assert np.all(np.isfinite(got["poses"])) and np.all(np.isfinite(got["landmarks"])) and np.isfinite(got["final_cost"])


@pytest.mark.parametrize("kind", KINDS)
def test_threshold_edges(ctx, kind):
    b = A * A
    costs = []
    for offset in (A, np.nextafter(A, np.inf)):
        sc = lr.threshold_scene(offset)
        ref = lr.solve_scene(sc, loss=(kind, A), max_iterations=0)
        ctx.set_ba_loss(kind, A)
        got = _solve(ctx, sc, max_iterations=0)
        print("BA loss threshold %-6s offset %s: cost0 %s / %s" % (kind, float(offset).hex(), float(got["initial_cost"]).hex(), float(ref["initial_cost"]).hex()))
        assert np.isfinite(got["initial_cost"]) and got["termination"] == ref["termination"] == 1      # r = 0 rows: no 0 / 0
        assert abs(got["initial_cost"] - ref["initial_cost"]) <= 1e-6 * ref["initial_cost"]
        assert got["poses"].tobytes() == sc["poses"].tobytes() and got["landmarks"].tobytes() == sc["landmarks"].tobytes()
        costs.append((got["initial_cost"], ref["initial_cost"]))
    s = [offset * offset for offset in (A, np.nextafter(A, np.inf))]
    assert s[0] == b and s[1] > b                              # the restatement's predicate: the two sides of the branch
    if kind == "huber":
        assert costs[0][0] == 0.5 * b == costs[0][1]           # the inlier branch: rho = s, exactly
    assert costs[1][1] > costs[0][1] and costs[1][0] >= costs[0][0]


@pytest.mark.parametrize("entry", ENTRIES)
def test_an_inactive_huber_is_loss_none_byte_for_byte(ctx, entry):
    for name in ("out:4,40", "edges"):
        sc = lr.scene(name)
        ctx.set_ba_loss("none")
        base = _solve(ctx, sc, entry)
        ctx.set_ba_loss("huber", 1e6)
        assert ctx.get_ba_loss() == (1, 1e6)
        _same_bits(_solve(ctx, sc, entry), base)
        assert base["iterations"] >= 2


def test_set_then_reset_is_a_context_that_never_set_one(ctx, pkg):
    sc = lr.scene("out:4,40")
    fresh = pkg.Context(width=0, height=0)
    assert fresh.get_ba_loss() == (pkg.BA_LOSS_NONE, 0.0)
    base = {e: _solve(fresh, sc, e) for e in ENTRIES}
    fresh.close()
    for kind, code in (("huber", pkg.BA_LOSS_HUBER), ("cauchy", pkg.BA_LOSS_CAUCHY), (1, 1), (2, 2)):
        ctx.set_ba_loss(kind, 0.25)
        assert ctx.get_ba_loss() == (code, 0.25)
    changed = _solve(ctx, sc)
    assert changed["final_cost"] != base["bundle_adjust"]["final_cost"]
    ctx.set_ba_loss("none", 123.0)                             # the scale of NONE is ignored and reported as 0
    assert ctx.get_ba_loss() == (0, 0.0)
    for e in ENTRIES:
        _same_bits(_solve(ctx, sc, e), base[e])
    ctx.set_ba_loss(pkg.BA_LOSS_HUBER, A)
    ctx.set_ba_loss(pkg.BA_LOSS_NONE)
    assert ctx.get_ba_loss() == (0, 0.0)


def test_invalid_arguments_then_a_clean_call(ctx, pkg):
    ctx.set_ba_loss("cauchy", 0.5)
    bad = [(3, 0.1), (-1, 0.1), (3, 0.0), (-1, np.nan)]
    for kind in (1, 2):
        bad += [(kind, 0.0), (kind, -0.02), (kind, np.inf), (kind, -np.inf), (kind, np.nan)]
    for kind, scale in bad:
        with pytest.raises(pkg.MslamHipError) as e:
            ctx.set_ba_loss(kind, scale)
        assert e.value.code == pkg.E_INVALID, (kind, scale)
        assert ctx.get_ba_loss() == (2, 0.5), (kind, scale)     # unchanged
    with pytest.raises(pkg.MslamHipError) as e:
        ctx.set_ba_loss("tukey", 0.1)
    assert e.value.code == pkg.E_INVALID and ctx.get_ba_loss() == (2, 0.5)
    _against(ctx, "out:3,24", "huber", "bundle_adjust")


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("kind", KINDS)
def test_a_second_call_returns_the_same_bits(ctx, kind, entry):
    sc = lr.scene("edges")
    ctx.set_ba_loss(kind, A)
    _same_bits(_solve(ctx, sc, entry), _solve(ctx, sc, entry))


@pytest.mark.parametrize("kind", KINDS)
def test_failure_leaves_the_state_and_judges_the_outliers_at_the_input(ctx, kind):
    """the non-finite observation tests/test_gpu_ba.py uses for FAILURE, with a loss set"""
    sc = {k: np.array(v) for k, v in ba_cases.scene("gross_outliers").items()}
    sc["obs_cam"][5, 1] = np.nan
    ctx.set_ba_loss(kind, A)
    got = _solve(ctx, sc, max_iterations=sc.get("max_iterations", 100))
    assert got["termination"] == 2 and got["iterations"] == 0 and not np.isfinite(got["initial_cost"])
    assert got["poses"].tobytes() == sc["poses"].tobytes() and got["landmarks"].tobytes() == sc["landmarks"].tobytes()
    with np.errstate(all="ignore"):
        r = ba_ref.residuals(sc["poses"], sc["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"])
        norms = np.sqrt(np.sum(r * r, 1))
        mask = ba_ref.outliers(sc["poses"], sc["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"])
        ref = lr.solve_scene(sc, loss=(kind, A))
    assert np.min(np.abs(norms[np.isfinite(norms)] - 0.15)) > 1e-6 and mask.any()
    assert np.array_equal(got["outlier"], mask) and got["n_outliers"] == int(mask.sum())
    assert ref["termination"] == ba_ref.FAILURE and ref["reason"] == "initial evaluation failed"


def test_the_pose_graph_ignores_the_setting(ctx):
    sc = pc.scene("chain:9")

    def run():
        return ctx.pose_graph(sc["poses"], sc["edge_a"], sc["edge_b"], sc["edge_meas"], sc["sqrt_info"], sc["fixed"])
    ctx.set_ba_loss("none")
    base = run()
    ctx.set_ba_loss("cauchy", 1e-3)                            # a scale far below the edges' residuals: it would show
    got = run()
    assert got["poses"].tobytes() == base["poses"].tobytes() and base["iterations"] >= 1
    for k in ("termination", "iterations", "rejected_steps", "invalid_steps"):
        assert got[k] == base[k], k
    for k in ("initial_cost", "final_cost"):
        assert np.float64(got[k]).tobytes() == np.float64(base[k]).tobytes(), k


def test_a_loss_keeps_the_good_observations(ctx):
    """what the feature is for.  The restatement satisfies the three conditions on its own (tests/test_ba_loss.py)"""
    sc = lr.scene("out:4,40")
    good = np.ones(len(sc["obs_kf"]), bool)
    good[sc["bad"]] = False
    flagged = {}
    for kind in ("none", "huber", "cauchy"):
        ctx.set_ba_loss(kind, A)
        got = _solve(ctx, sc)
        flagged[kind] = (int(got["outlier"][good].sum()), int(got["outlier"][~good].sum()))
        print("BA loss out:4,40 %-6s good flagged %d bad flagged %d of %d" % (kind, flagged[kind][0], flagged[kind][1], len(sc["bad"])))
    assert flagged["none"][0] >= 1 and flagged["huber"][0] == 0 and flagged["cauchy"][0] == 0


# ---- the tracker --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sequence():
    return tr.make_sequence()


def _run(pkg, seq, wrap=None, **kw):
    c = pkg.Context(width=0, height=0, max_keypoints=4096)
    t = pkg.HipKeyframeTracker(c, focal=tr.CAM[:2], principal=tr.CAM[2:], **dict(tr.SEQ_PARAMS, **kw))
    if wrap:
        wrap(t)
    return c, t, [t.processSensorData(fr["desc"], fr["xy"], fr["depth"]) for fr in seq["frames"]]


def test_tracker_without_ba_loss_is_todays_tracker(pkg, sequence):
    c0, t0, a = _run(pkg, sequence, local_map_depth=2, local_ba=True)
    c1, t1, b = _run(pkg, sequence, local_map_depth=2, local_ba=True, ba_loss=None)
    assert t1.ba_loss is None and t1.backend.loss is None and len(t0.ba_results) == len(t1.ba_results) >= 1
    for f, (x, y) in enumerate(zip(a, b)):
        assert (x["tracked"], x["n_inliers"], x["keyframe"], x["reference"], x["relocalized"]) == \
               (y["tracked"], y["n_inliers"], y["keyframe"], y["reference"], y["relocalized"]), f
        assert x["R"].tobytes() == y["R"].tobytes() and x["tvec"].tobytes() == y["tvec"].tobytes() and x["rvec"].tobytes() == y["rvec"].tobytes(), f
    assert t0.ids == t1.ids
    for k in t0.ids:
        assert c0.kf_read(k)[1].tobytes() == c1.kf_read(k)[1].tobytes() and np.array_equal(c0.kf_read_ids(k), c1.kf_read_ids(k))
    c0.close()
    c1.close()


def test_tracker_with_ba_loss(pkg, sequence):
    """every ba_results entry equals a direct HipBackend(loss = ...) solve of the problem the tracker's backend held at that
    moment, and the store holds the refined points bit for bit.  Nothing is claimed about the trajectory: nobody has
    measured the sequence's outlier rate"""
    loss = ("huber", A)
    seen = []

    def wrap(t):
        inner = t.backend._solve

        def recording(kf_ids, blocked=False):
            be = t.backend
            seen.append((list(kf_ids), blocked, copy.deepcopy((be.poses, be.obs, be.landmarks, be.anchor, be.first))))
            assert t.ctx.get_ba_loss() == (0, 0.0)              # between solves the context has no loss
            return inner(kf_ids, blocked)
        t.backend._solve = recording
    c, t, rows = _run(pkg, sequence, wrap=wrap, local_map_depth=2, local_ba=True, ba_loss=loss)
    assert t.ba_loss == loss and t.backend.loss == loss and c.get_ba_loss() == (0, 0.0)
    assert len(t.ba_results) == len(seen) == len(t.ids) - 1 >= 1
    c2 = pkg.Context(width=0, height=0)
    solved = {}
    for ba, (kf_ids, blocked, state) in zip(t.ba_results, seen):
        be = pkg.HipBackend(c2, loss=loss)
        be.poses, be.obs, be.landmarks, be.anchor, be.first = copy.deepcopy(state)      # a solve writes its result back
        direct = be._solve(kf_ids, blocked)
        _same_bits(ba, direct)
        assert ba["keyframes"] == direct["keyframes"] and np.array_equal(ba["landmark_ids"], direct["landmark_ids"])
        plain = pkg.HipBackend(c2)
        plain.poses, plain.obs, plain.landmarks, plain.anchor, plain.first = copy.deepcopy(state)
        none = plain._solve(kf_ids, blocked)
        print("local BA huber keyframes %s M %d term %d it %d cost %.6g -> %.6g (no loss: %.6g -> %.6g) outliers %d / %d" % (
            ba["keyframes"], len(ba["outlier"]), ba["termination"], ba["iterations"], ba["initial_cost"], ba["final_cost"],
            none["initial_cost"], none["final_cost"], ba["n_outliers"], none["n_outliers"]))
        assert ba["termination"] in (0, 1) and ba["final_cost"] < ba["initial_cost"]
        assert ba["initial_cost"] <= none["initial_cost"]      # rho(s) <= s
        solved.update(zip(ba["landmark_ids"].tolist(), ba["landmarks"]))
    assert solved
    for k in t.ids:
        lids, world = c.kf_read_ids(k), c.kf_read(k)[1]
        for l, w in zip(lids.tolist(), world):
            if l in solved:
                assert w.tobytes() == solved[l].tobytes() == t.backend.landmarks[l].tobytes(), (k, l)
    c.close()
    c2.close()
