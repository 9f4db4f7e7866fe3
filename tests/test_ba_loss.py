"""The loss function of bundle adjustment (mslam_hip_set_ba_loss) on the CPU: the symbols and constructors, the loss
formulas on hand values, tests/ba_loss_ref.py (the restatement the GPU tests compare with) against tests/ba_ref.py with an
inactive loss and against scipy's robust least squares at its own result, the condition the GPU tests rest on (a loss keeps
the good observations unflagged where no loss does not), and HipBackend's set / restore bookkeeping on a stub context."""
import inspect
import os
import re

import numpy as np
import pytest

import ba_loss_ref as lr
import ba_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mslam_hip_set_ba_loss", "mslam_hip_get_ba_loss"]
A = lr.SCALE


def test_symbols_are_exported_declared_and_listed(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mslam_hip.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr)
        assert name in pkg.ABI_SYMBOLS and hasattr(pkg.lib(), name)
    for name, value in (("NONE", 0), ("HUBER", 1), ("CAUCHY", 2)):
        assert re.search(r"#define MSLAM_HIP_BA_LOSS_%s %d\b" % (name, value), hdr)
        assert getattr(pkg, "BA_LOSS_" + name) == value
    assert pkg.lib().mslam_hip_abi_version() == 5
    assert callable(pkg.Context.set_ba_loss) and callable(pkg.Context.get_ba_loss)
    assert inspect.signature(pkg.Context.set_ba_loss).parameters["scale"].default == 0.0


def test_constructor_defaults(pkg):
    assert inspect.signature(pkg.HipBackend.__init__).parameters["loss"].default is None
    assert inspect.signature(pkg.HipKeyframeTracker.__init__).parameters["ba_loss"].default is None
    assert pkg.HipBackend(None).loss is None and pkg.HipBackend(None, loss=("huber", 0.02)).loss == ("huber", 0.02)
    t = pkg.HipKeyframeTracker(None)
    assert t.ba_loss is None and t.backend is None
    with pytest.raises(pkg.MslamHipError) as e:
        pkg.HipKeyframeTracker(None, ba_loss=("huber", 0.02))               # needs local_ba
    assert e.value.code == pkg.E_INVALID
    t = pkg.HipKeyframeTracker(None, local_map_depth=2, local_ba=True, ba_loss=("cauchy", 0.05))
    assert t.ba_loss == ("cauchy", 0.05) and t.backend.loss == ("cauchy", 0.05)
    assert pkg.HipKeyframeTracker(None, local_map_depth=2, local_ba=True).backend.loss is None
    doc = pkg.HipKeyframeTracker.__doc__
    assert "ba_loss = " in doc and "lm_cull = True" in doc and "found / visible" in doc
    assert "loss = " in pkg.HipBackend.__doc__


# ---- the formulas on hand values ----------------------------------------------------------------------------------------
def test_loss_formulas_on_hand_values():
    b = A * A
    up = np.nextafter(b, np.inf)
    for kind in (lr.HUBER, lr.CAUCHY):
        rho, w = lr.loss(kind, A, 0.0)
        assert rho == 0.0 and w == 1.0                                       # no 0 / 0 from a / sqrt(s)
        rho, w = lr.loss(kind, A, 1e300)
        assert np.isfinite(rho) and 0.0 < w < 1e-140
        rho, w = lr.loss(kind, A, np.array([0.0, b, up, 1e300]))             # arrays go the scalar's way
        assert [lr.loss(kind, A, s)[0] for s in (0.0, b, up, 1e300)] == rho.tolist()
        assert np.all(np.diff(rho) >= 0.0) and np.all(np.diff(w) <= 0.0)     # rho grows, rho' falls: rho'' <= 0
    rho, w = lr.loss(lr.HUBER, A, b)
    assert rho == b and w == 1.0                                             # s == b is the inlier branch
    rho_up, w_up = lr.loss(lr.HUBER, A, up)
    assert rho_up == 2.0 * A * np.sqrt(up) - b and w_up == A / np.sqrt(up)   # the outlier branch
    assert abs(rho_up - b) <= 4 * np.spacing(b) and 1.0 - w_up <= 4 * np.finfo(np.float64).eps      # continuous at b
    rho, w = lr.loss(lr.HUBER, A, 1e300)
    assert rho == 2.0 * A * 1e150 - b and w == A / 1e150
    rho, w = lr.loss(lr.HUBER, A, 4.0 * b)                                   # |r| = 2 a: rho = 3 b, rho' = 1 / 2
    assert abs(rho - 3.0 * b) <= 4 * np.spacing(b) and abs(w - 0.5) <= 1e-15
    rho, w = lr.loss(lr.CAUCHY, A, b)                                        # rho = b log 2, rho' = 1 / 2
    assert abs(rho - b * np.log(2.0)) <= 4 * np.spacing(b) and abs(w - 0.5) <= 1e-15
    rho, w = lr.loss(lr.CAUCHY, A, 1e300)
    assert abs(rho - b * (np.log(1e300) - np.log(b))) <= 1e-12 * rho
    rho, w = lr.loss(lr.CAUCHY, A, np.inf)
    assert rho == np.inf and w == lr.DBL_MIN                                 # the floor of rho'
    assert np.isnan(lr.loss(lr.HUBER, A, np.nan)[0]) and np.isnan(lr.loss(lr.CAUCHY, A, np.nan)[0])


def _same_result(a, b):
    assert a["poses"].tobytes() == b["poses"].tobytes() and a["landmarks"].tobytes() == b["landmarks"].tobytes()
    for k in ("termination", "iterations", "reason", "trace"):
        assert a[k] == b[k], k
    for k in ("initial_cost", "final_cost", "gradient_max_norm"):
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), k


@pytest.mark.parametrize("solver", ["qr", "schur"])
def test_an_inactive_loss_is_ba_ref(solver):
    """Huber with a = 1e6: every s is below b, so rho = s and every weight is exactly 1; multiplying by sqrt(1) changes no
    bit.  The restated loop must then return what ba_ref.bundle_adjust returns, and so must loss = None"""
    sc = ba_ref.make_scene(3, 30, 4, noise=0.003)
    base = ba_ref.solve_scene(sc, linear_solver=solver)
    assert base["iterations"] >= 2 and base["final_cost"] > 0.0
    _same_result(lr.solve_scene(sc, linear_solver=solver, loss=("huber", 1e6)), base)
    _same_result(lr.solve_scene(sc, linear_solver=solver), base)


@pytest.mark.parametrize("kind", ["huber", "cauchy"])
def test_the_restatement_minimises_the_stated_cost(kind):
    """scipy.optimize.least_squares, one scalar residual |r_m| per observation, loss = kind, f_scale = a (scipy's rho on a
    scalar residual is Ceres's on s = |r_m|^2), over the tangent at the restatement's result through _Problem.plus, started
    at that result.  The restatement stops when one step changes the cost by less than 1e-6 of it; ten of those is the bound
    on what scipy may still gain.  scipy runs with tolerances of 1e-10, a hundred times tighter than its defaults, and at
    most 60 evaluations (each with a finite-difference Jacobian): Huber ends by itself after 25; Cauchy's gain is 9.5e-8 at
    the cap and 1.01e-7 after 100 evaluations and after 200.  Measured: 7.6e-9 (huber), 9.5e-8 (cauchy); printed below."""
    from scipy.optimize import least_squares
    sc, qr = lr.reference("out:4,40", kind)[:2]
    prob = ba_ref._Problem(qr["poses"], qr["landmarks"], sc["obs_kf"].astype(np.int64), sc["obs_lm"].astype(np.int64),
                           sc["obs_cam"], sc["fixed"].astype(bool))

    def norms(delta):
        p, l = prob.plus(qr["poses"], qr["landmarks"], delta)
        r = ba_ref.residuals(p, l, sc["obs_kf"], sc["obs_lm"], sc["obs_cam"])
        return np.sqrt(np.sum(r * r, 1))
    mine = lr.cost(qr["poses"], qr["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"], lr.KINDS[kind], A)
    assert abs(mine - qr["final_cost"]) <= 1e-12 * mine
    res = least_squares(norms, np.zeros(prob.n), loss=kind, f_scale=A, xtol=1e-10, ftol=1e-10, gtol=1e-10, max_nfev=60)
    start = 0.5 * np.sum(A * A * (lr.loss(lr.KINDS[kind], 1.0, (norms(np.zeros(prob.n)) / A) ** 2)[0]))
    assert abs(start - mine) <= 1e-9 * mine                                   # scipy's cost is the stated cost
    drop = (mine - res.cost) / mine
    print("BA loss %s: restatement cost %.12g, scipy from there %.12g, relative drop %.3e, nfev %d" % (kind, mine, res.cost, drop, res.nfev))
    assert drop <= 1e-5


@pytest.mark.parametrize("name", ["out:3,24", "out:4,40", "out:6,70"])
def test_a_loss_keeps_the_good_observations(name):
    """what the feature is for, on the restatement alone: the GPU test of the same name rests on it"""
    sc = lr.scene(name)
    good = np.ones(len(sc["obs_kf"]), bool)
    good[sc["bad"]] = False
    row = {}
    for kind in ("none", "huber", "cauchy"):
        qr, mask = lr.reference(name, kind)[1], lr.reference(name, kind)[3]
        assert qr["termination"] == ba_ref.CONVERGENCE
        err = float(np.max(np.linalg.norm(qr["landmarks"] - sc["truth_landmarks"], axis=1)))
        row[kind] = (err, int(mask[good].sum()), int(mask[~good].sum()))
        print("BA loss %-9s %-6s M %d bad %d: landmark error max %.4f m, good flagged %d, bad flagged %d" % (
            name, kind, len(good), len(sc["bad"]), err, row[kind][1], row[kind][2]))
    assert row["none"][1] >= 1
    for kind in ("huber", "cauchy"):
        assert row[kind][1] == 0 and row[kind][2] >= 0.9 * len(sc["bad"]) and row[kind][0] < row["none"][0]


def test_hand_scenes_are_what_they_are_named_for():
    sc = lr.scene("edges")
    K, L, M = len(sc["poses"]), len(sc["landmarks"]), len(sc["obs_kf"])
    assert (K, L, M) == (2, 300, 600) and M % 256 != 0 and sc["bad"][-1] == M - 1
    row1 = np.flatnonzero(sc["obs_kf"] == 1)                                  # keyframe 1's row, sorted by landmark
    assert len(row1) > 256 and np.all(np.diff(sc["obs_lm"][row1]) > 0) and not sc["fixed"][1]
    assert np.intersect1d(row1[256:], sc["bad"]).size >= 4                    # bad at row positions >= 256
    assert np.sum(sc["obs_lm"][sc["bad"]] >= 256) >= 8 and np.sum(sc["obs_lm"][sc["bad"]] < 256) >= 2
    sc = lr.scene("fixed_only")
    assert sc["fixed"][0] and np.all(sc["obs_kf"][sc["bad"]] == 0) and len(sc["bad"]) >= 4
    huber, none = lr.reference("fixed_only", "huber")[1], lr.reference("fixed_only", "none")[1]
    touched = np.unique(sc["obs_lm"][sc["bad"]])
    assert np.min(np.linalg.norm(huber["landmarks"][touched] - none["landmarks"][touched], axis=1)) > 1e-3     # the weights matter
    sc = lr.scene("all_bad_landmark")
    assert np.array_equal(sc["bad"], np.flatnonzero(sc["obs_lm"] == 5))
    for off, outlier in ((A, False), (np.nextafter(A, np.inf), True)):
        sc = lr.threshold_scene(off)
        r = ba_ref.residuals(sc["poses"], sc["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"])
        s = np.sum(r * r, 1)
        assert (s[0] == A * A) == (not outlier) and (s[0] > A * A) == outlier and not s[1:].any()


# ---- HipBackend's bookkeeping -------------------------------------------------------------------------------------------
class StubContext:
    """Context.set_ba_loss / get_ba_loss / bundle_adjust on a recorded setting"""

    def __init__(self, setting=(0, 0.0), fail=False):
        self.setting, self.fail, self.calls, self.at_solve = setting, fail, [], []

    def get_ba_loss(self):
        self.calls.append("get")
        return self.setting

    def set_ba_loss(self, kind, scale=0.0):
        self.calls.append(("set", kind, scale))
        self.setting = (kind, scale)

    def bundle_adjust(self, poses, lm, okf, olm, ocam, fixed, max_iterations, outlier_threshold):
        self.calls.append("solve")
        self.at_solve.append(self.setting)
        if self.fail:
            raise RuntimeError("the solve raised")
        return dict(poses=poses.copy(), landmarks=lm.copy(), outlier=np.zeros(len(okf), bool), termination=0)

    bundle_adjust_global = bundle_adjust


def _backend(pkg, ctx, **kw):
    be = pkg.HipBackend(ctx, **kw)
    be.add_keyframe(1, [0, 0, 0, 1, 0, 0, 0], [5, 6], [[0, 0, 2.0], [0.5, 0, 2.0]])
    be.add_keyframe(2, [0, 0, 0, 1, 0.1, 0, 0], [5, 6], [[-0.1, 0, 2.0], [0.4, 0, 2.0]])
    return be


def test_backend_sets_its_loss_and_restores_the_previous_setting(pkg):
    ctx = StubContext(setting=(2, 0.5))                    # somebody else's Cauchy
    be = _backend(pkg, ctx, loss=("huber", 0.02))
    be.global_ba()
    assert ctx.calls == ["get", ("set", "huber", 0.02), "solve", ("set", 2, 0.5)]
    assert ctx.at_solve == [("huber", 0.02)] and ctx.setting == (2, 0.5)
    ctx.calls.clear()
    be.local_ba(2, {1: {2}, 2: {1}}, prune=True)          # nothing flagged: one solve
    assert ctx.calls == ["get", ("set", "huber", 0.02), "solve", ("set", 2, 0.5)]
    be.global_solver = True                                # the blocked entry goes the same way
    be.global_ba()
    assert ctx.at_solve == [("huber", 0.02)] * 3 and ctx.setting == (2, 0.5)


def test_backend_restores_the_setting_when_the_solve_raises(pkg):
    ctx = StubContext(setting=(0, 0.0), fail=True)
    be = _backend(pkg, ctx, loss=("cauchy", 0.1))
    with pytest.raises(RuntimeError):
        be.global_ba()
    assert ctx.calls == ["get", ("set", "cauchy", 0.1), "solve", ("set", 0, 0.0)] and ctx.setting == (0, 0.0)


def test_backend_without_a_loss_never_touches_the_setting(pkg):
    ctx = StubContext(setting=(1, 0.3))
    be = _backend(pkg, ctx)
    be.global_ba()
    be.local_ba(2, {1: {2}, 2: {1}})
    assert ctx.calls == ["solve", "solve"] and ctx.at_solve == [(1, 0.3)] * 2
