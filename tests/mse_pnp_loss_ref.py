"""CPU restatement of min-MSE PnP with a loss function (mslam_hip_set_pnp_mse_loss), for the tests.

tests/mse_pnp_ref.py restates the solve the reference makes, which gives its residual blocks no loss.  This module adds what
Ceres 2.2 does when a loss is given, each piece from the published source named beside it, and shares nothing with the HIP
kernel:

  * loss_function.h, HuberLoss::Evaluate and CauchyLoss::Evaluate at s = |residual_i|^2 (the residual block's squared norm:
    both pixel components of a point together), with scale a (pixels) and b = a^2:
        Huber   s <= b: rho = s, rho' = 1;   else rho = 2 a sqrt(s) - b, rho' = max(DBL_MIN, a / sqrt(s))
        Cauchy  rho = b log(1 + s c), rho' = max(DBL_MIN, 1 / (1 + s c)), c = 1 / b
  * corrector.cc: rho'' <= 0 for both, so the constructor takes `sq_norm == 0 || rho[2] <= 0`: residual_scaling =
    jacobian_scaling = sqrt(rho'), no curvature term; residual_block.cc: the block's cost is rho / 2.

evaluate() is mse_pnp_ref._evaluate corrected that way: f and the rows of J scaled by sqrt(rho') per point, cost 1/2 sum rho,
gradient J^T f of the corrected pair.  mse_pnp_ref.min_mse_pnp calls its _evaluate itself, so its trust-region loop is
restated here with the evaluation as the one difference; with loss = None it returns what mse_pnp_ref.min_mse_pnp returns, bit
for bit (tests/test_mse_pnp_loss.py).  Both linear solvers of mse_pnp_ref work on the corrected pair unchanged.  (The kernel
keeps no rows and puts rho' on the products of its sums instead: the same numbers up to rounding.)

The scenes are tests/test_mse_pnp.py's scene64 with a fifth of the image points replaced by uniform ones and half a pixel of
noise on the rest, at the point counts where the kernel's lane stride turns, and a few with the bad points placed by hand.
The scale of the tests is 2 px.

PARITY UNPINNED, as mse_pnp_ref: no Ceres build exists here.  This is test infrastructure (not a conftest.py, not under
oracle/)."""
import functools

import numpy as np

import mse_pnp_ref as mr
from mse_pnp_ref import (CONVERGENCE, DBL_MAX, FAILURE, FUNCTION_TOLERANCE, GRADIENT_TOLERANCE, INITIAL_TRUST_REGION_RADIUS,
                         MAX_LM_DIAGONAL, MAX_NUM_CONSECUTIVE_INVALID_STEPS, MAX_NUM_ITERATIONS, MAX_TRUST_REGION_RADIUS,
                         MIN_LM_DIAGONAL, MIN_RELATIVE_DECREASE, MIN_TRUST_REGION_RADIUS, NO_CONVERGENCE, PARAMETER_TOLERANCE)
from test_mse_pnp import CAM, perturbed, scene64

DBL_MIN = np.finfo(np.float64).tiny
NONE, HUBER, CAUCHY = 0, 1, 2
KINDS = {"none": NONE, "huber": HUBER, "cauchy": CAUCHY}
SCALE = 2.0           # a of the tests, pixels
LOSSES = ("huber", "cauchy")


def loss(kind, a, s):
    """-> (rho, rho') at s (array or scalar), kind HUBER or CAUCHY, scale a"""
    s = np.asarray(s, np.float64)
    b = a * a
    with np.errstate(all="ignore"):
        if kind == HUBER:
            inlier = s <= b
            r = np.sqrt(s)
            rho = np.where(inlier, s, 2.0 * a * r - b)
            w = np.where(inlier, 1.0, np.maximum(DBL_MIN, a / r))
        elif kind == CAUCHY:
            total = 1.0 + s * (1.0 / b)
            rho = b * np.log(total)
            w = np.maximum(DBL_MIN, 1.0 / total)
        else:
            raise ValueError(kind)
    return rho, w


def _how(how):
    return (NONE, 0.0) if how is None else (KINDS.get(how[0], how[0]), float(how[1]))


def cost(x, obj, img, cam, how=None):
    """1/2 sum rho(|residual_i|^2)"""
    kind, a = _how(how)
    with np.errstate(all="ignore"):
        res = np.asarray(img, np.float64).reshape(-1, 2) - mr.project(x, obj, cam)
        s = res[:, 0] ** 2 + res[:, 1] ** 2
        return float(np.sum(0.5 * (s if kind == NONE else loss(kind, a, s)[0])))


def evaluate(x, obj, img, cam, kind, a, trace=None):
    ok, c, f, g, J = mr._evaluate(x, obj, img, cam, trace)
    if kind == NONE:
        return ok, c, f, g, J
    with np.errstate(all="ignore"):
        r = f.reshape(-1, 2)
        rho, w = loss(kind, a, r[:, 0] ** 2 + r[:, 1] ** 2)
        scaling = np.sqrt(w)
        f = (r * scaling[:, None]).reshape(-1)
        J = J * np.repeat(scaling, 2)[:, None]
        ok = bool(np.all(np.isfinite(f)) and np.all(np.isfinite(J)))
        return ok, float(np.sum(0.5 * rho)), f, J.T @ f, J


def min_mse_pnp(obj, img, cam, x0, linear_solver="qr", loss=None):
    """mse_pnp_ref.min_mse_pnp's loop and result dict on the corrected evaluation.  loss = None or (kind, a) with kind
    "huber" / "cauchy" or the integers"""
    kind, a = _how(loss)
    lm_step = {"qr": mr._lm_step_qr, "normal": mr._lm_step_normal}[linear_solver]
    trace = dict(small_angle=0, rodrigues=0, rejected=0, accepted_after_rejected=0, invalid=0, dbl_max=0, branches="")
    obj = np.asarray(obj, np.float64).reshape(-1, 3)
    img = np.asarray(img, np.float64).reshape(-1, 2)
    x = np.array(x0, np.float64).reshape(6)

    def out(term, it, c0, c, reason, gmax=np.nan, xr=None):
        return dict(x=x.copy() if xr is None else xr, termination=term, iterations=it, initial_cost=c0, final_cost=c,
                    gradient_max_norm=gmax, reason=reason, trace=trace)

    if len(obj) == 0:
        return out(CONVERGENCE, 0, 0.0, 0.0, "no parameter blocks", 0.0)
    x_start = x.copy()
    ok, x_cost, f, g, J = evaluate(x, obj, img, cam, kind, a, trace)
    initial_cost = x_cost
    if not ok or not np.isfinite(x_cost):
        return out(FAILURE, 0, initial_cost, initial_cost, "initial evaluation failed", xr=x_start)
    with np.errstate(all="ignore"):
        scale = 1.0 / (1.0 + np.sqrt(np.sum(J * J, axis=0)))
    gmax = mr._gradient_max_norm(x, g)
    radius, decrease_factor = INITIAL_TRUST_REGION_RADIUS, 2.0
    invalid = 0
    iteration = 0
    successful = True
    while True:
        if iteration >= MAX_NUM_ITERATIONS:
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
            step, model_cost_change = lm_step(Js, D, f)
        if not (np.all(np.isfinite(step)) and model_cost_change > 0.0):
            invalid += 1
            trace["invalid"] += 1
            if invalid >= MAX_NUM_CONSECUTIVE_INVALID_STEPS:
                return out(FAILURE, iteration, initial_cost, x_cost, "too many invalid steps", gmax, xr=x_start)
            radius /= decrease_factor
            decrease_factor *= 2.0
            continue
        invalid = 0
        candidate = x + step * scale
        c_ok, candidate_cost, c_f, c_g, c_J = evaluate(candidate, obj, img, cam, kind, a, trace)
        if not np.isfinite(candidate_cost):
            candidate_cost = DBL_MAX
            trace["dbl_max"] += 1
        step_norm = np.linalg.norm(x - candidate)
        if step_norm <= PARAMETER_TOLERANCE * (np.linalg.norm(x) + PARAMETER_TOLERANCE):
            return out(CONVERGENCE, iteration, initial_cost, x_cost, "parameter tolerance", gmax)
        if abs(x_cost - candidate_cost) <= FUNCTION_TOLERANCE * x_cost:
            return out(CONVERGENCE, iteration, initial_cost, x_cost, "function tolerance", gmax)
        relative_decrease = -DBL_MAX if candidate_cost >= DBL_MAX else (x_cost - candidate_cost) / model_cost_change
        if relative_decrease > MIN_RELATIVE_DECREASE:
            if not c_ok:
                return out(FAILURE, iteration, initial_cost, x_cost, "evaluation at the accepted point failed", gmax, xr=x_start)
            x = candidate
            x_cost, f, g, J = candidate_cost, c_f, c_g, c_J
            gmax = mr._gradient_max_norm(x, g)
            successful = True
            radius = min(MAX_TRUST_REGION_RADIUS, radius / max(1.0 / 3.0, 1.0 - (2.0 * relative_decrease - 1.0) ** 3))
            trace["accepted_after_rejected"] += decrease_factor != 2.0
            decrease_factor = 2.0
        else:
            trace["rejected"] += 1
            radius /= decrease_factor
            decrease_factor *= 2.0


# ---- scenes -----------------------------------------------------------------------------------------------------------
SIZES, SEEDS = (6, 63, 64, 65, 129, 400), (0, 1)
MIXED = ["mixed:%d:%d" % (n, seed) for n in SIZES for seed in SEEDS]
PLACED = ["from64", "last", "all_bad", "n1", "n0"]
CASES = MIXED + PLACED


def _placed(n, seed, bad):
    """scene64 with half a pixel of noise and no outliers; then the image points `bad` drawn uniformly over the frame"""
    obj, img, x = scene64(seed, n=n, noise=0.5)
    bad = np.asarray(bad, np.int64)
    img[bad] = np.random.default_rng([seed, 5]).uniform(0, [640, 480], (len(bad), 2))
    return dict(obj=obj, img=img, truth=x, start=perturbed(x, seed), bad=bad)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(obj, img, truth, start, bad): bad = the indices of the points whose image point is not the projection's"""
    kind, _, rest = name.partition(":")
    if kind == "mixed":                # the issue's table: scene64(100 n + seed, n, outliers = 0.2, noise = 0.5)
        n, seed = (int(v) for v in rest.split(":"))
        obj, img, x = scene64(100 * n + seed, n=n, outliers=0.2, noise=0.5)
        rng = np.random.default_rng(100 * n + seed)          # scene64's own draws, again, up to its outlier mask
        rng.normal(size=3), rng.normal(size=3), [rng.uniform(-1, 1, n) for _ in range(3)], rng.normal(size=(n, 2))
        return dict(obj=obj, img=img, truth=x, start=perturbed(x, seed), bad=np.flatnonzero(rng.random(n) < 0.2))
    if kind == "from64":               # n = 129: the bad points are on the lanes' second and third trip only
        return _placed(129, 7, [64, 70, 100, 127, 128])
    if kind == "last":                 # n = 65: the one bad point is the only point of lane 0's second trip
        return _placed(65, 8, [64])
    if kind == "all_bad":              # every image point is uniform: no pose explains them
        return _placed(30, 9, np.arange(30))
    if kind == "n1":                   # one point: underdetermined
        return _placed(1, 10, [])
    if kind == "n0":
        return _placed(0, 11, [])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name, kind):
    """-> (case, qr result, normal-equations result); kind "none" / "huber" / "cauchy" at SCALE.  Computed once and shared: do
    not write into what this returns"""
    c = case(name)
    how = None if kind == "none" else (kind, SCALE)
    return c, min_mse_pnp(c["obj"], c["img"], CAM, c["start"], "qr", how), min_mse_pnp(c["obj"], c["img"], CAM, c["start"], "normal", how)


THRESHOLD_A = 2.0


def threshold_case():
    """one point (0, 0, 1) seen from r = t = 0 (the small-angle branch returns the point itself: X / Z = 0 exactly) at
    (cx + 2, cy): the residual is (2, 0) and s = 4 = THRESHOLD_A^2, each exactly: Huber's inlier branch at a = 2 (cost 2), the
    other at nextafter(2, 0)"""
    obj, img = np.array([[0.0, 0.0, 1.0]]), np.array([[CAM[2] + 2.0, CAM[3]]])
    res, _ = mr.residuals_and_jacobian(np.zeros(6), obj, img, CAM)
    assert res.tolist() == [[2.0, 0.0]]
    return obj, img, np.zeros(6)
