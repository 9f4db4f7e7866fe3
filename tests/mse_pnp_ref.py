"""CPU restatement of MinMseTracker::solvePnp (reference ceres_reprojection_error_pnp.cpp:18-110) for the tests.

The reference minimises, with Ceres, the reprojection error of all correspondences over x = (r, t) (angle-axis r,
translation t), from the caller's pose:

    residual_i(x) = observed_i - (f * X/Z + c),   (X, Y, Z) = ceres::AngleAxisRotatePoint(r, P_i) + t
    cost(x)       = 1/2 sum_i |residual_i|^2       (no loss function; ReprojectionErrorFunctor, :18-60)

with Solver::Options defaults except gradient / function / parameter tolerance 1e-8 (:85-91).  This module restates,
in numpy and independently of the HIP kernel (modular-slam_amd/csrc/k_pnp_mse.hip), the pieces of Ceres 2.2 that the
call exercises, each from the published source named beside it:

  * ceres::AngleAxisRotatePoint (rotation.h), both branches: Rodrigues' formula for theta^2 > DBL_EPSILON, p + r x p
    below it;
  * ceres::AutoDiffCostFunction<_, 2, 6> (autodiff_cost_function.h, jet.h): forward-mode dual numbers with 6 derivative
    slots; the landmark, the intrinsics and the observation enter as constant jets (T(point.x()) ...), and every
    operation uses jet.h's formula (a / b = (a.a / b.a, (a.v - (a.a / b.a) b.v) / b.a), sqrt, sin, cos, ...);
  * TrustRegionMinimizer (trust_region_minimizer.cc): IterationZero, the Jacobi scaling 1 / (1 + |J_col|) computed once
    from the Jacobian at the start, the model cost change -(J d)^T (f + J d / 2), step validity (model cost change > 0),
    HandleInvalidStep (5 in a row: FAILURE), a candidate that fails to evaluate as cost DBL_MAX, ParameterToleranceReached
    (|x - x_candidate| <= tol (|x| + tol)), FunctionToleranceReached (|cost change| <= tol cost), IsStepSuccessful
    (relative decrease > min_relative_decrease 1e-3), HandleSuccessfulStep, and the checks of
    FinalizeIterationAndCheckIfMinimizerCanContinue in their order (max_num_iterations 50, gradient tolerance on
    |x - Plus(x, -g)|_inf after a successful step, min_trust_region_radius 1e-32);
  * TrustRegionStepEvaluator (trust_region_step_evaluator.cc) with max_consecutive_nonmonotonic_steps 0 (monotonic):
    the step quality is (cost - candidate cost) / model cost change;
  * LevenbergMarquardtStrategy (levenberg_marquardt_strategy.cc): radius 1e4 (initial) .. 1e16, diagonal
    clamp(diag(J^T J), 1e-6, 1e32) of the scaled Jacobian, D = sqrt(diagonal / radius), StepAccepted
    (radius /= max(1/3, 1 - (2 rho - 1)^3), decrease factor 2), StepRejected / StepIsInvalid (radius /= decrease factor,
    decrease factor *= 2);
  * DenseQRSolver (dense_qr_solver.cc): the step solves min |J y - f|^2 + |D y|^2 by a QR factorisation of [J; D]
    (the kernel uses normal equations instead: the two differ in rounding only);
  * solver.cc Minimize(): a problem without parameter blocks (n = 0) is CONVERGENCE at cost 0, parameters untouched.

min_mse_pnp(..., linear_solver="normal") is a second solver for the same step, written from DESIGN.md's description of
what the kernel does and not from the kernel: Cholesky of (Js^T Js + diag(D^2)) y = Js^T f, the model cost change from
the normal equations.  The two solvers are both correct and differ in rounding only, so their distance on a case says how
far two correct implementations may drift apart there; the GPU tests take their bound from it.  Every solve also
returns `trace`, which counts the paths it took (see min_mse_pnp).

PARITY UNPINNED: no Ceres build exists here, so nothing pins this restatement to Ceres itself; it is pinned to ground
truth (noise-free scenes) and to finite differences (derivatives), and the GPU tests pin the kernel to it.
This is test infrastructure (not a conftest.py, not under oracle/).
"""
import numpy as np

DBL_EPSILON = np.finfo(np.float64).eps
DBL_MAX = np.finfo(np.float64).max
CONVERGENCE, NO_CONVERGENCE, FAILURE = 0, 1, 2          # ceres::TerminationType

# Solver::Options defaults (solver.h) + the call site's tolerances (ceres_reprojection_error_pnp.cpp:88-90)
MAX_NUM_ITERATIONS = 50
MAX_NUM_CONSECUTIVE_INVALID_STEPS = 5
INITIAL_TRUST_REGION_RADIUS = 1e4
MAX_TRUST_REGION_RADIUS = 1e16
MIN_TRUST_REGION_RADIUS = 1e-32
MIN_LM_DIAGONAL, MAX_LM_DIAGONAL = 1e-6, 1e32
MIN_RELATIVE_DECREASE = 1e-3
GRADIENT_TOLERANCE = FUNCTION_TOLERANCE = PARAMETER_TOLERANCE = 1e-8


# ---- jets: (a, v) with a of shape S and v of shape S + (6,) ---------------------------------------------------------
def _const(a, slots=6):
    a = np.asarray(a, np.float64)
    return a, np.zeros(a.shape + (slots,))


def _add(f, g):
    return f[0] + g[0], f[1] + g[1]


def _sub(f, g):
    return f[0] - g[0], f[1] - g[1]


def _mul(f, g):                                          # jet.h: (f.a g.a, f.a g.v + f.v g.a)
    return f[0] * g[0], f[0][..., None] * g[1] + f[1] * g[0][..., None]


def _div(f, g):                                          # jet.h operator/(Jet, Jet)
    g_a_inverse = 1.0 / g[0]
    f_a_by_g_a = f[0] * g_a_inverse
    return f_a_by_g_a, (f[1] - f_a_by_g_a[..., None] * g[1]) * g_a_inverse[..., None]


def _sqrt(f):
    tmp = np.sqrt(f[0])
    two_a_inverse = 1.0 / (2.0 * tmp)
    return tmp, f[1] * two_a_inverse[..., None]


def _cos(f):
    return np.cos(f[0]), -np.sin(f[0])[..., None] * f[1]


def _sin(f):
    return np.sin(f[0]), np.cos(f[0])[..., None] * f[1]


def angle_axis_rotate_point_jet(aa, pt):
    """ceres::AngleAxisRotatePoint (rotation.h) on jets: aa = 3 jets, pt = 3 jets -> 3 jets"""
    theta2 = _add(_add(_mul(aa[0], aa[0]), _mul(aa[1], aa[1])), _mul(aa[2], aa[2]))     # DotProduct
    if theta2[0] > DBL_EPSILON:                          # the comparison looks at the scalar part only
        theta = _sqrt(theta2)
        costheta, sintheta = _cos(theta), _sin(theta)
        one = _const(np.ones_like(theta[0]), theta[1].shape[-1])
        theta_inverse = _div(one, theta)
        w = [_mul(aa[k], theta_inverse) for k in range(3)]
        w_cross_pt = [_sub(_mul(w[1], pt[2]), _mul(w[2], pt[1])),
                      _sub(_mul(w[2], pt[0]), _mul(w[0], pt[2])),
                      _sub(_mul(w[0], pt[1]), _mul(w[1], pt[0]))]
        tmp = _mul(_add(_add(_mul(w[0], pt[0]), _mul(w[1], pt[1])), _mul(w[2], pt[2])), _sub(one, costheta))
        return [_add(_add(_mul(pt[k], costheta), _mul(w_cross_pt[k], sintheta)), _mul(w[k], tmp)) for k in range(3)]
    w_cross_pt = [_sub(_mul(aa[1], pt[2]), _mul(aa[2], pt[1])),
                  _sub(_mul(aa[2], pt[0]), _mul(aa[0], pt[2])),
                  _sub(_mul(aa[0], pt[1]), _mul(aa[1], pt[0]))]
    return [_add(pt[k], w_cross_pt[k]) for k in range(3)]


def angle_axis_rotate_point(r, p):
    """value (3,) and derivative d/dr (3, 3) of AngleAxisRotatePoint(r, p) for one point, as autodiff gives it"""
    r = np.asarray(r, np.float64)
    aa = [(np.array(r[k]), np.eye(3)[k]) for k in range(3)]
    pt = [_const(np.array(float(p[k])), 3) for k in range(3)]
    out = angle_axis_rotate_point_jet(aa, pt)
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def rotate_plain(r, P):
    """AngleAxisRotatePoint on plain doubles (n, 3) -> (n, 3): the value part of the jets, for finite differences"""
    out = angle_axis_rotate_point_jet([_const(np.float64(rk), 0) for rk in r], [_const(P[:, k], 0) for k in range(3)])
    return np.stack([o[0] for o in out], 1)


def residuals_and_jacobian(x, obj, img, cam):
    """ReprojectionErrorFunctor::operator() (:26-55) through AutoDiffCostFunction<_, 2, 6>: residuals (n, 2) and their
    Jacobian (n, 2, 6) at x = (r, t)"""
    fx, fy, cx, cy = cam
    obj = np.asarray(obj, np.float64).reshape(-1, 3)
    img = np.asarray(img, np.float64).reshape(-1, 2)
    x = np.asarray(x, np.float64)
    state = [(np.array(x[k]), np.eye(6)[k]) for k in range(6)]           # the parameter block, seeded e_k
    pt1 = [_const(obj[:, k]) for k in range(3)]
    with np.errstate(all="ignore"):
        pt2 = angle_axis_rotate_point_jet(state[:3], pt1)
        pt2 = [_add(pt2[k], state[3 + k]) for k in range(3)]
        xp = _add(_mul(_const(np.full(len(obj), fx)), _div(pt2[0], pt2[2])), _const(np.full(len(obj), cx)))
        yp = _add(_mul(_const(np.full(len(obj), fy)), _div(pt2[1], pt2[2])), _const(np.full(len(obj), cy)))
        r0 = _sub(_const(img[:, 0]), xp)
        r1 = _sub(_const(img[:, 1]), yp)
    res = np.stack([r0[0], r1[0]], 1)
    J = np.stack([r0[1], r1[1]], 1)
    return res, J


def project(x, obj, cam):
    """the projection of the functor on plain doubles (for scenes and costs)"""
    fx, fy, cx, cy = cam
    X = rotate_plain(np.asarray(x[:3], np.float64), np.asarray(obj, np.float64).reshape(-1, 3)) + np.asarray(x[3:6])
    return np.stack([fx * (X[:, 0] / X[:, 2]) + cx, fy * (X[:, 1] / X[:, 2]) + cy], 1)


def cost(x, obj, img, cam):
    with np.errstate(all="ignore"):
        res = np.asarray(img, np.float64).reshape(-1, 2) - project(x, obj, cam)
        return float(np.sum(0.5 * (res[:, 0] ** 2 + res[:, 1] ** 2)))


def _evaluate(x, obj, img, cam, trace=None):
    """Evaluator::Evaluate: (ok, cost, residuals f (2n), gradient J^T f, Jacobian (2n, 6)); ok is False when a residual or
    a Jacobian entry is not finite (ResidualBlock::Evaluate's IsEvaluationValid)"""
    if trace is not None:                                 # the branch AngleAxisRotatePoint takes at x
        small = not (x[0] * x[0] + x[1] * x[1] + x[2] * x[2] > DBL_EPSILON)
        trace["small_angle" if small else "rodrigues"] += 1
        trace["branches"] += "s" if small else "R"
    res, J = residuals_and_jacobian(x, obj, img, cam)
    f = res.reshape(-1)
    Jm = J.reshape(-1, 6)
    ok = bool(np.all(np.isfinite(f)) and np.all(np.isfinite(Jm)))
    with np.errstate(all="ignore"):
        c = float(np.sum(0.5 * (res[:, 0] ** 2 + res[:, 1] ** 2)))
        g = Jm.T @ f
    return ok, c, f, g, Jm


def _gradient_max_norm(x, g):
    return float(np.max(np.abs(x - (x + (-g))))) if len(x) else 0.0       # |x - Plus(x, -g)|_inf


def _lm_step_qr(Js, D, f):
    """DenseQRSolver on the D-augmented system: (step, model cost change -(Js d)^T (f + Js d / 2))"""
    A = np.vstack([Js, np.diag(D)])
    b = np.concatenate([f, np.zeros(6)])
    q, rr = np.linalg.qr(A)
    y = np.linalg.solve(rr, q.T @ b) if np.all(np.isfinite(rr)) else np.full(6, np.nan)
    step = -y
    model_residuals = Js @ step
    return step, -model_residuals.dot(f + model_residuals / 2.0)


def _lm_step_normal(Js, D, f):
    """the normal equations (Js^T Js + diag(D^2)) y = Js^T f by Cholesky; the model cost change
    -(f^T Js d + |Js d|^2 / 2) from Js^T f and the undamped Js^T Js.  A failed factorisation is a non-finite step, which
    the caller counts as an invalid one."""
    H = Js.T @ Js
    gs = Js.T @ f
    try:
        L = np.linalg.cholesky(H + np.diag(D * D))
    except np.linalg.LinAlgError:
        return np.full(6, np.nan), np.nan
    step = -np.linalg.solve(L.T, np.linalg.solve(L, gs))
    return step, -(gs.dot(step) + 0.5 * step.dot(H @ step))


def min_mse_pnp(obj, img, cam, x0, linear_solver="qr"):
    """MinMseTracker::solvePnp's ceres::Solve -> dict(x, termination, iterations, initial_cost, final_cost,
    gradient_max_norm, reason, trace).  `iterations` is the index of the trust-region iteration that ended the solve (0
    when the start already met a test); x is the start when termination is FAILURE.  linear_solver: "qr" (Ceres's
    DENSE_QR) or "normal" (Cholesky of the normal equations, see the module's text).  trace counts the paths taken:
    evaluations on the small-angle / Rodrigues branch of AngleAxisRotatePoint (`small_angle`, `rodrigues`; `branches` is
    their sequence, one letter s / R per evaluation, the start first), `rejected` steps, accepted steps that reset a
    grown decrease factor (`accepted_after_rejected`), `invalid` steps and candidates whose cost was replaced by DBL_MAX
    (`dbl_max`)."""
    lm_step = {"qr": _lm_step_qr, "normal": _lm_step_normal}[linear_solver]
    trace = dict(small_angle=0, rodrigues=0, rejected=0, accepted_after_rejected=0, invalid=0, dbl_max=0, branches="")
    obj = np.asarray(obj, np.float64).reshape(-1, 3)
    img = np.asarray(img, np.float64).reshape(-1, 2)
    x = np.array(x0, np.float64).reshape(6)

    def out(term, it, c0, c, reason, gmax=np.nan, xr=None):
        return dict(x=x.copy() if xr is None else xr, termination=term, iterations=it, initial_cost=c0, final_cost=c,
                    gradient_max_norm=gmax, reason=reason, trace=trace)

    if len(obj) == 0:                                     # solver.cc Minimize(): no parameter blocks
        return out(CONVERGENCE, 0, 0.0, 0.0, "no parameter blocks", 0.0)
    x_start = x.copy()
    # IterationZero
    ok, x_cost, f, g, J = _evaluate(x, obj, img, cam, trace)
    initial_cost = x_cost
    if not ok or not np.isfinite(x_cost):
        return out(FAILURE, 0, initial_cost, initial_cost, "initial evaluation failed", xr=x_start)
    with np.errstate(all="ignore"):
        scale = 1.0 / (1.0 + np.sqrt(np.sum(J * J, axis=0)))              # jacobian_scaling_, once
    gmax = _gradient_max_norm(x, g)
    radius, decrease_factor = INITIAL_TRUST_REGION_RADIUS, 2.0
    invalid = 0
    iteration = 0
    successful = True
    while True:
        # FinalizeIterationAndCheckIfMinimizerCanContinue
        if iteration >= MAX_NUM_ITERATIONS:
            return out(NO_CONVERGENCE, iteration, initial_cost, x_cost, "max iterations", gmax)
        if successful and gmax <= GRADIENT_TOLERANCE:
            return out(CONVERGENCE, iteration, initial_cost, x_cost, "gradient tolerance", gmax)
        if radius <= MIN_TRUST_REGION_RADIUS:
            return out(CONVERGENCE, iteration, initial_cost, x_cost, "min trust region radius", gmax)
        iteration += 1
        successful = False
        # ComputeTrustRegionStep -> LevenbergMarquardtStrategy::ComputeStep on the scaled Jacobian
        Js = J * scale
        diagonal = np.minimum(np.maximum(np.sum(Js * Js, axis=0), MIN_LM_DIAGONAL), MAX_LM_DIAGONAL)
        D = np.sqrt(diagonal / radius)
        with np.errstate(all="ignore"):
            step, model_cost_change = lm_step(Js, D, f)
        if not (np.all(np.isfinite(step)) and model_cost_change > 0.0):
            # HandleInvalidStep
            invalid += 1
            trace["invalid"] += 1
            if invalid >= MAX_NUM_CONSECUTIVE_INVALID_STEPS:
                return out(FAILURE, iteration, initial_cost, x_cost, "too many invalid steps", gmax, xr=x_start)
            radius /= decrease_factor
            decrease_factor *= 2.0
            continue
        invalid = 0
        delta = step * scale
        candidate = x + delta
        # ComputeCandidatePointAndEvaluateCost
        c_ok, candidate_cost, c_f, c_g, c_J = _evaluate(candidate, obj, img, cam, trace)
        if not np.isfinite(candidate_cost):
            candidate_cost = DBL_MAX
            trace["dbl_max"] += 1
        # ParameterToleranceReached
        step_norm = np.linalg.norm(x - candidate)
        if step_norm <= PARAMETER_TOLERANCE * (np.linalg.norm(x) + PARAMETER_TOLERANCE):
            return out(CONVERGENCE, iteration, initial_cost, x_cost, "parameter tolerance", gmax)
        # FunctionToleranceReached
        if abs(x_cost - candidate_cost) <= FUNCTION_TOLERANCE * x_cost:
            return out(CONVERGENCE, iteration, initial_cost, x_cost, "function tolerance", gmax)
        # IsStepSuccessful (TrustRegionStepEvaluator::StepQuality, monotonic)
        if candidate_cost >= DBL_MAX:
            relative_decrease = -DBL_MAX
        else:
            relative_decrease = (x_cost - candidate_cost) / model_cost_change
        if relative_decrease > MIN_RELATIVE_DECREASE:
            # HandleSuccessfulStep: residuals + Jacobian at the new point
            if not c_ok:
                return out(FAILURE, iteration, initial_cost, x_cost, "evaluation at the accepted point failed", gmax,
                           xr=x_start)
            x = candidate
            x_cost, f, g, J = candidate_cost, c_f, c_g, c_J
            gmax = _gradient_max_norm(x, g)
            successful = True
            radius = radius / max(1.0 / 3.0, 1.0 - (2.0 * relative_decrease - 1.0) ** 3)
            radius = min(MAX_TRUST_REGION_RADIUS, radius)
            trace["accepted_after_rejected"] += decrease_factor != 2.0
            decrease_factor = 2.0
        else:
            trace["rejected"] += 1
            radius /= decrease_factor                     # StepRejected
            decrease_factor *= 2.0
