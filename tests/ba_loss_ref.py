"""CPU restatement of bundle adjustment with a loss function (mslam_hip_set_ba_loss), for the tests.

tests/ba_ref.py restates the solve the reference makes, which passes lossFunction = nullptr.  This module adds what Ceres 2.2
does when a loss is given, each piece from the published source named beside it, and shares nothing with the HIP kernels:

  * loss_function.h, HuberLoss::Evaluate and CauchyLoss::Evaluate at s = |r_m|^2 (the residual block's squared norm: the
    three camera-frame components together), with scale a and b = a^2:
        Huber   s > b:  rho = 2 a sqrt(s) - b, rho' = max(DBL_MIN, a / sqrt(s));   else rho = s, rho' = 1
        Cauchy  rho = b log(1 + s c), rho' = max(DBL_MIN, 1 / (1 + s c)), c = 1 / b
  * corrector.cc: rho'' <= 0 for both, so the constructor takes `sq_norm == 0 || rho[2] <= 0`: residual_scaling =
    jacobian_scaling = sqrt(rho'), no curvature term; residual_block.cc: the block's cost is rho / 2.

LossProblem is ba_ref._Problem with evaluate() corrected that way: f and the rows of J scaled by sqrt(rho') per observation,
cost 1/2 sum rho, gradient J^T f of the corrected pair.  ba_ref.bundle_adjust builds its _Problem itself, so its
trust-region loop is restated here with the problem as the one difference; with loss = None, or with a loss whose every
weight is 1, it returns what ba_ref.bundle_adjust returns, bit for bit (tests/test_ba_loss.py).  Both linear solvers of
ba_ref work on the corrected pair unchanged.  The outlier mask is ba_ref.outliers: the uncorrected residual.

PARITY UNPINNED, as ba_ref: no Ceres build exists here.  The restatement is pinned to its own stated cost instead: started at
its result, scipy.optimize.least_squares with the same loss finds nothing lower (tests/test_ba_loss.py).
This is test infrastructure (not a conftest.py, not under oracle/).
"""
import functools

import numpy as np

import ba_ref
from ba_ref import (CONVERGENCE, DBL_MAX, FAILURE, FUNCTION_TOLERANCE, GRADIENT_TOLERANCE, INITIAL_TRUST_REGION_RADIUS,
                    MAX_LM_DIAGONAL, MAX_NUM_CONSECUTIVE_INVALID_STEPS, MAX_TRUST_REGION_RADIUS, MIN_LM_DIAGONAL,
                    MIN_RELATIVE_DECREASE, MIN_TRUST_REGION_RADIUS, NO_CONVERGENCE, PARAMETER_TOLERANCE)

DBL_MIN = np.finfo(np.float64).tiny
NONE, HUBER, CAUCHY = 0, 1, 2
KINDS = {"none": NONE, "huber": HUBER, "cauchy": CAUCHY}


def loss(kind, a, s):
    """-> (rho, rho') at s (array or scalar), kind HUBER or CAUCHY, scale a"""
    s = np.asarray(s, np.float64)
    b = a * a
    with np.errstate(all="ignore"):
        if kind == HUBER:
            outlier = s > b
            r = np.sqrt(s)
            rho = np.where(outlier, 2.0 * a * r - b, s)
            w = np.where(outlier, np.maximum(DBL_MIN, a / r), 1.0)
        elif kind == CAUCHY:
            total = 1.0 + s * (1.0 / b)
            rho = b * np.log(total)
            w = np.maximum(DBL_MIN, 1.0 / total)
        else:
            raise ValueError(kind)
    return rho, w


def cost(poses, landmarks, obs_kf, obs_lm, obs_cam, kind, a):
    """1/2 sum rho(|r_m|^2)"""
    r = ba_ref.residuals(poses, landmarks, obs_kf, obs_lm, obs_cam)
    s = np.sum(r * r, 1)
    return float(np.sum(0.5 * (s if kind == NONE else loss(kind, a, s)[0])))


class LossProblem(ba_ref._Problem):
    def __init__(self, poses, landmarks, obs_kf, obs_lm, obs_cam, fixed, kind, a):
        super().__init__(poses, landmarks, obs_kf, obs_lm, obs_cam, fixed)
        self.kind, self.a = kind, a

    def evaluate(self, poses, landmarks):
        ok, c, f, g, J = super().evaluate(poses, landmarks)
        if self.kind == NONE:
            return ok, c, f, g, J
        with np.errstate(all="ignore"):
            r = f.reshape(-1, 3)
            rho, w = loss(self.kind, self.a, np.sum(r * r, 1))
            scaling = np.sqrt(w)
            f = (r * scaling[:, None]).reshape(-1)
            J = J * np.repeat(scaling, 3)[:, None]
            ok = bool(np.all(np.isfinite(f)) and np.all(np.isfinite(J)))
            return ok, float(np.sum(0.5 * rho)), f, J.T @ f, J


def bundle_adjust(poses, landmarks, obs_kf, obs_lm, obs_cam, fixed=None, max_iterations=100, linear_solver="qr", loss=None):
    """ba_ref.bundle_adjust's loop and result dict on a LossProblem.  loss = None or (kind, a) with kind "huber" / "cauchy"
    or the integers"""
    kind, a = (NONE, 0.0) if loss is None else (KINDS.get(loss[0], loss[0]), float(loss[1]))
    lm_step = {"qr": ba_ref._lm_step_qr, "schur": ba_ref._lm_step_schur}[linear_solver]
    poses0 = np.array(poses, np.float64).reshape(-1, 7)
    lms0 = np.array(landmarks, np.float64).reshape(-1, 3)
    obs_kf, obs_lm = np.asarray(obs_kf, np.int64).reshape(-1), np.asarray(obs_lm, np.int64).reshape(-1)
    obs_cam = np.asarray(obs_cam, np.float64).reshape(-1, 3)
    fixed = np.zeros(len(poses0), bool) if fixed is None else np.asarray(fixed).astype(bool)
    trace = dict(rejected=0, accepted_after_rejected=0, invalid=0, dbl_max=0)
    x_p, x_l = poses0.copy(), lms0.copy()

    def out(term, it, c0, c, reason, gmax=np.nan, usable=True):
        return dict(poses=x_p if usable else poses0, landmarks=x_l if usable else lms0, termination=term, iterations=it,
                    initial_cost=c0, final_cost=c, gradient_max_norm=gmax, reason=reason, trace=trace)

    if len(obs_kf) == 0:
        return out(CONVERGENCE, 0, 0.0, 0.0, "no parameter blocks", 0.0)
    prob = LossProblem(poses0, lms0, obs_kf, obs_lm, obs_cam, fixed, kind, a)
    seen_k = np.zeros(len(poses0), bool)
    seen_k[obs_kf] = True
    free_of_obs = prob.col_k[obs_kf] >= 0
    lm_has_free = np.zeros(len(lms0), bool)
    lm_has_free[obs_lm[free_of_obs]] = True
    trace.update(free_poses=len(prob.free_k), constant_poses=int(np.sum(seen_k & fixed)), landmarks=len(prob.act_l),
                 landmarks_fixed_only=int(np.sum(~lm_has_free[prob.act_l])))

    def gradient_max_norm(g):
        xp, xl = prob.plus(x_p, x_l, -g)
        return float(np.max(np.abs(prob.ambient(x_p, x_l) - prob.ambient(xp, xl))))

    ok, x_cost, f, g, J = prob.evaluate(x_p, x_l)
    initial_cost = x_cost
    if not ok or not np.isfinite(x_cost):
        return out(FAILURE, 0, initial_cost, initial_cost, "initial evaluation failed", usable=False)
    scale = 1.0 / (1.0 + np.sqrt(np.sum(J * J, axis=0)))
    gmax = gradient_max_norm(g)
    radius, decrease_factor = INITIAL_TRUST_REGION_RADIUS, 2.0
    invalid = iteration = 0
    successful = True
    while True:
        if iteration >= max_iterations:
            return out(NO_CONVERGENCE, iteration, initial_cost, x_cost, "max iterations", gmax)
        if successful and gmax <= GRADIENT_TOLERANCE:
            return out(CONVERGENCE, iteration, initial_cost, x_cost, "gradient tolerance", gmax)
        if radius <= MIN_TRUST_REGION_RADIUS:
            return out(CONVERGENCE, iteration, initial_cost, x_cost, "min trust region radius", gmax)
        iteration += 1
        successful = False
        Js = J * scale
        diagonal = np.minimum(np.maximum(np.sum(Js * Js, axis=0), MIN_LM_DIAGONAL), MAX_LM_DIAGONAL)
        D = np.sqrt(diagonal / radius)
        with np.errstate(all="ignore"):
            step, model_cost_change = lm_step(prob, Js, D, f)
        if not (np.all(np.isfinite(step)) and model_cost_change > 0.0):
            invalid += 1
            trace["invalid"] += 1
            if invalid >= MAX_NUM_CONSECUTIVE_INVALID_STEPS:
                return out(FAILURE, iteration, initial_cost, x_cost, "too many invalid steps", gmax, usable=False)
            radius /= decrease_factor
            decrease_factor *= 2.0
            continue
        invalid = 0
        c_p, c_l = prob.plus(x_p, x_l, step * scale)
        c_ok, candidate_cost, c_f, c_g, c_J = prob.evaluate(c_p, c_l)
        if not np.isfinite(candidate_cost):
            candidate_cost = DBL_MAX
            trace["dbl_max"] += 1
        x_amb = prob.ambient(x_p, x_l)
        step_norm = np.linalg.norm(x_amb - prob.ambient(c_p, c_l))
        if step_norm <= PARAMETER_TOLERANCE * (np.linalg.norm(x_amb) + PARAMETER_TOLERANCE):
            return out(CONVERGENCE, iteration, initial_cost, x_cost, "parameter tolerance", gmax)
        if abs(x_cost - candidate_cost) <= FUNCTION_TOLERANCE * x_cost:
            return out(CONVERGENCE, iteration, initial_cost, x_cost, "function tolerance", gmax)
        relative_decrease = -DBL_MAX if candidate_cost >= DBL_MAX else (x_cost - candidate_cost) / model_cost_change
        if relative_decrease > MIN_RELATIVE_DECREASE:
            if not c_ok:
                return out(FAILURE, iteration, initial_cost, x_cost, "evaluation at the accepted point failed", gmax, usable=False)
            x_p, x_l = c_p, c_l
            x_cost, f, g, J = candidate_cost, c_f, c_g, c_J
            gmax = gradient_max_norm(g)
            successful = True
            radius = min(MAX_TRUST_REGION_RADIUS, radius / max(1.0 / 3.0, 1.0 - (2.0 * relative_decrease - 1.0) ** 3))
            trace["accepted_after_rejected"] += decrease_factor != 2.0
            decrease_factor = 2.0
        else:
            trace["rejected"] += 1
            radius /= decrease_factor
            decrease_factor *= 2.0


def solve_scene(sc, **kw):
    return bundle_adjust(sc["poses"], sc["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"], sc["fixed"], **kw)


# ---- scenes -----------------------------------------------------------------------------------------------------------
SCALE = 0.02          # a of the tests, metres
THRESHOLD = 0.15      # the reference's outlier threshold


def spoil(sc, bad, sigma, rng):
    """sigma N(0, 1) per coordinate on the observations `bad` -> the scene with `bad` (sorted indices) recorded"""
    bad = np.sort(np.asarray(bad, np.int64))
    sc = dict(sc, obs_cam=sc["obs_cam"].copy())
    sc["obs_cam"][bad] += sigma * rng.normal(size=(len(bad), 3))
    sc["bad"] = bad
    return sc


def make_outlier_scene(K, L, seed, noise=0.003, every=12, sigma=0.4, **kw):
    """ba_ref.make_scene plus sigma N(0, 1) m per coordinate on M // every observations, drawn without replacement by a
    generator seeded with (seed, every) -> the scene dict with bad = their indices, ascending"""
    sc = ba_ref.make_scene(K, L, seed, noise=noise, **kw)
    rng = np.random.default_rng([seed, every])
    M = len(sc["obs_kf"])
    return spoil(sc, rng.choice(M, size=M // every, replace=False), sigma, rng)


def _edges():
    """K = 2, L = 300, every landmark seen from both keyframes: M = 600 in the order (l, k), keyframe 0 constant.  The row
    of keyframe 1 holds 300 observations sorted by landmark, so its positions >= 256 are the landmarks >= 256: bad there
    (k_ba_cameras' lane stride wraps; the second block of k_ba_landmarks), on both keyframes; a few bad ones in the first
    block; the last observation (l = 299, k = 1) bad and M = 600 = 2 x 256 + 88 (k_ba_eval's tail block)"""
    sc = ba_ref.make_scene(2, 300, 11, noise=0.003)
    assert sc["obs_kf"].tolist() == [0, 1] * 300
    bad = [2 * l + 1 for l in range(256, 300, 4)] + [2 * l for l in range(258, 300, 8)] + [2 * 7 + 1, 2 * 130, 599]
    return spoil(sc, sorted(set(bad)), 0.4, np.random.default_rng(12))


def _fixed_only():
    """bad observations on the constant keyframe only: its k_ba_cameras workgroup never runs, so their weights reach the
    solve through k_ba_landmarks alone"""
    sc = ba_ref.make_scene(3, 24, 5, noise=0.003)
    of_fixed = np.flatnonzero(sc["obs_kf"] == 0)
    return spoil(sc, of_fixed[::3], 0.4, np.random.default_rng(6))


def _all_bad_landmark():
    """every observation of landmark 5 is bad"""
    sc = ba_ref.make_scene(3, 24, 7, noise=0.003)
    return spoil(sc, np.flatnonzero(sc["obs_lm"] == 5), 0.4, np.random.default_rng(8))


SCENES = {
    "out:3,24": lambda: make_outlier_scene(3, 24, 2),
    "out:4,40": lambda: make_outlier_scene(4, 40, 2),
    "out:6,70": lambda: make_outlier_scene(6, 70, 2),
    "edges": _edges,
    "fixed_only": _fixed_only,
    "all_bad_landmark": _all_bad_landmark,
}


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def reference(name, kind):
    """-> (scene, qr result, distance of the schur result from it, outlier mask at the qr state, the smallest distance of a
    residual norm from the threshold).  kind "none" / "huber" / "cauchy" at SCALE.  Computed once and shared: do not write
    into what this returns"""
    sc = scene(name)
    how = None if kind == "none" else (kind, SCALE)
    qr = solve_scene(sc, linear_solver="qr", loss=how)
    sch = solve_scene(sc, linear_solver="schur", loss=how)
    dist = max(float(np.max(np.abs(qr["poses"] - sch["poses"]))), float(np.max(np.abs(qr["landmarks"] - sch["landmarks"]))))
    r = ba_ref.residuals(qr["poses"], qr["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"])
    norms = np.sqrt(np.sum(r * r, 1))
    return sc, qr, dist, norms > THRESHOLD, np.abs(norms - THRESHOLD)


def threshold_scene(offset):
    """A problem on exact grid values whose start is its solution: unit-quaternion identity rotations, positions and
    landmarks on a grid of 1/8 m, noise-free, start = truth, so every residual is 0 exactly (the rotation by (0, 0, 0, 1) adds
    only zeros) — except observation 0, of landmark 0 on the optical axis of keyframe 0 (X - p has x = 0): its observed x
    is -offset, so r = (offset, 0, 0) and |r|^2 = offset^2, each exactly."""
    poses = np.array([[0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 0.5, 0.125, 0], [0, 0, 0, 1, -0.25, 0.375, 0.125]], np.float64)
    g = np.arange(12)
    lms = np.stack([(g % 4) * 0.5 - 0.75, (g // 4) * 0.625 - 0.5, 2.0 + (g % 3) * 0.25], 1)
    lms[0] = (0.0, 0.25, 2.5)
    okf, olm = np.repeat(np.arange(3), 12).astype(np.int32), np.tile(np.arange(12), 3).astype(np.int32)
    cam = lms[olm] - poses[okf, 4:]
    assert cam[0, 0] == 0.0
    cam[0, 0] = -offset
    r = ba_ref.residuals(poses, lms, okf, olm, cam)
    assert r[0].tolist() == [offset, 0.0, 0.0] and not r[1:].any()
    return dict(poses=poses, landmarks=lms, fixed=np.array([1, 0, 0], np.uint8), obs_kf=okf, obs_lm=olm, obs_cam=cam)
