"""CPU restatement of CeresBackend::bundleAdjustment's solve (reference ceres_backend.cpp:19-60, :185-240) for the tests.

The reference minimises, with Ceres, over the keyframes' states (orientation q as x y z w, position p; camera -> world) and
the landmarks X

    residual_m = rot(q^-1, X) - rot(q^-1, p) - observation_m          (ReprojectionError::operator(), :31-47)
    cost       = 1/2 sum_m |residual_m|^2                             (no loss function)

with q on an EigenQuaternionManifold, keyframe 1 constant (:155-159), max_num_iterations from a parameter and every other
Solver::Options at its default (:193-195).  This module restates, in numpy and sharing nothing with the HIP kernels
(modular-slam_amd/csrc/k_ba.hip), what that call exercises, each piece from the published source named beside it:

  * the residual through ceres::AutoDiffCostFunction<_, 3, 4, 3, 3> (jet.h): forward-mode dual numbers, ten slots (the four
    quaternion coefficients, p, X); Eigen's Quaternion::inverse() = conjugate / squared norm and _transformVector
    (v + w uv + u x uv with uv = 2 u x v), as Eigen evaluates them on jets;
  * EigenQuaternionManifold (manifold.h): Plus(q, d) = q_delta (x) q with q_delta = (sin|d| d / |d|, cos|d|), q unchanged for
    d = 0; PlusJacobian in x, y, z, w order; the tangent Jacobian of a residual is J_q * PlusJacobian;
  * TrustRegionMinimizer, TrustRegionStepEvaluator (monotonic), LevenbergMarquardtStrategy: as tests/mse_pnp_ref.py
    restates them, with solver.h's defaults: function tolerance 1e-6, gradient tolerance 1e-10, parameter tolerance 1e-8,
    initial radius 1e4, Jacobi scaling.  The norms of the parameter and gradient tests run over the ambient parameters (seven
    per pose) of the blocks that are in the problem: a constant block, or one without a residual, is not;
  * solver.cc Minimize(): a problem without residuals is CONVERGENCE at cost 0.

linear_solver="qr" solves min |J_s y - f|^2 + |D y|^2 by a dense QR of the D-augmented full system (every pose and landmark
column at once).  linear_solver="schur" is a second solver for the same step, written from DESIGN.md 4.14's description
of what the kernels do and not from the kernels: per-landmark blocks V_l + D^2 inverted, the reduced camera system
S = U + D^2 - W V^-1 W^T by Cholesky, back-substitution, the model cost change summed per observation.  Both are correct and
differ in rounding only; their distance on a case says how far two correct implementations may drift apart there, and the
GPU tests take their bound from it.  Every solve returns `trace`, the paths it took.

PARITY UNPINNED: no Ceres build exists here, so nothing pins this restatement to Ceres itself; it is pinned to ground truth
(noise-free scenes) and to central differences (derivatives), and the GPU tests pin the kernels to it.
This is test infrastructure (not a conftest.py, not under oracle/).
"""
import numpy as np

DBL_MAX = np.finfo(np.float64).max
CONVERGENCE, NO_CONVERGENCE, FAILURE = 0, 1, 2
MAX_NUM_CONSECUTIVE_INVALID_STEPS = 5
INITIAL_TRUST_REGION_RADIUS, MAX_TRUST_REGION_RADIUS, MIN_TRUST_REGION_RADIUS = 1e4, 1e16, 1e-32
MIN_LM_DIAGONAL, MAX_LM_DIAGONAL = 1e-6, 1e32
MIN_RELATIVE_DECREASE = 1e-3
FUNCTION_TOLERANCE, GRADIENT_TOLERANCE, PARAMETER_TOLERANCE = 1e-6, 1e-10, 1e-8


# ---- jets: (a, v), a of shape (M,), v of shape (M, slots) ---------------------------------------------------------------
def _const(a, slots):
    a = np.asarray(a, np.float64)
    return a, np.zeros(a.shape + (slots,))


def _add(f, g):
    return f[0] + g[0], f[1] + g[1]


def _sub(f, g):
    return f[0] - g[0], f[1] - g[1]


def _neg(f):
    return -f[0], -f[1]


def _mul(f, g):
    return f[0] * g[0], f[0][..., None] * g[1] + f[1] * g[0][..., None]


def _div(f, g):
    g_a_inverse = 1.0 / g[0]
    f_a_by_g_a = f[0] * g_a_inverse
    return f_a_by_g_a, (f[1] - f_a_by_g_a[..., None] * g[1]) * g_a_inverse[..., None]


def _cross(a, b):
    return [_sub(_mul(a[1], b[2]), _mul(a[2], b[1])), _sub(_mul(a[2], b[0]), _mul(a[0], b[2])),
            _sub(_mul(a[0], b[1]), _mul(a[1], b[0]))]


def _inverse(q):
    """Eigen Quaternion::inverse(): conjugate / squaredNorm"""
    n2 = _add(_add(_mul(q[0], q[0]), _mul(q[1], q[1])), _add(_mul(q[2], q[2]), _mul(q[3], q[3])))
    return [_div(_neg(q[0]), n2), _div(_neg(q[1]), n2), _div(_neg(q[2]), n2), _div(q[3], n2)]


def _transform_vector(q, v):
    """Eigen QuaternionBase::_transformVector"""
    uv = _cross(q[:3], v)
    uv = [_add(c, c) for c in uv]
    cr = _cross(q[:3], uv)
    return [_add(_add(v[k], _mul(q[3], uv[k])), cr[k]) for k in range(3)]


def residual_jets(q, p, X, obs, slots=10):
    """ReprojectionError::operator() on jets: q [M, 4], p, X, obs [M, 3] -> residuals [M, 3], Jacobian [M, 3, 10] over
    (q, p, X); slots = 0 evaluates plain doubles"""
    M = len(q)
    eye = np.eye(10)[:, :slots]

    def seed(a, k):
        return np.asarray(a, np.float64), np.broadcast_to(eye[k], (M, slots)).copy()
    qj = [seed(q[:, k], k) for k in range(4)]
    pj = [seed(p[:, k], 4 + k) for k in range(3)]
    Xj = [seed(X[:, k], 7 + k) for k in range(3)]
    inv = _inverse(qj)
    a, b = _transform_vector(inv, Xj), _transform_vector(inv, pj)
    r = [_sub(_sub(a[k], b[k]), _const(obs[:, k], slots)) for k in range(3)]
    return np.stack([c[0] for c in r], 1), np.stack([c[1] for c in r], 1)


def residuals(poses, landmarks, obs_kf, obs_lm, obs_cam):
    poses, landmarks = np.asarray(poses, np.float64).reshape(-1, 7), np.asarray(landmarks, np.float64).reshape(-1, 3)
    if len(obs_kf) == 0:
        return np.zeros((0, 3))
    with np.errstate(all="ignore"):
        return residual_jets(poses[obs_kf, :4], poses[obs_kf, 4:], landmarks[obs_lm], np.asarray(obs_cam, np.float64), 0)[0]


def cost(poses, landmarks, obs_kf, obs_lm, obs_cam):
    r = residuals(poses, landmarks, obs_kf, obs_lm, obs_cam)
    return float(np.sum(0.5 * np.sum(r * r, 1)))


def outliers(poses, landmarks, obs_kf, obs_lm, obs_cam, threshold=0.15):
    """createOutput (:212-230): squared residual norm > threshold^2"""
    r = residuals(poses, landmarks, obs_kf, obs_lm, obs_cam)
    return np.sum(r * r, 1) > threshold * threshold


def quaternion_plus(q, d):
    """EigenQuaternionManifold::Plus (manifold.h, QuaternionPlus with x y z w storage)"""
    q, d = np.asarray(q, np.float64), np.asarray(d, np.float64)
    norm = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    if not norm > 0.0:
        return q.copy()
    sbd = np.sin(norm) / norm
    ax, ay, az, aw = sbd * d[0], sbd * d[1], sbd * d[2], np.cos(norm)
    x, y, z, w = q
    return np.array([aw * x + ax * w + ay * z - az * y, aw * y + ay * w + az * x - ax * z,
                     aw * z + az * w + ax * y - ay * x, aw * w - ax * x - ay * y - az * z])


def plus_jacobian(q):
    """EigenQuaternionManifold::PlusJacobian (4 x 3), x y z w order"""
    x, y, z, w = q
    return np.array([[w, z, -y], [-z, w, x], [y, -x, w], [-x, -y, -z]], np.float64)


def tangent_jacobians(poses, landmarks, obs_kf, obs_lm, obs_cam):
    """-> residuals [M, 3], J_delta [M, 3, 3] (= J_q PlusJacobian), J_p [M, 3, 3], J_X [M, 3, 3]"""
    r, J = residual_jets(poses[obs_kf, :4], poses[obs_kf, 4:], landmarks[obs_lm], obs_cam)
    PJ = np.stack([plus_jacobian(q) for q in poses[:, :4]])[obs_kf]        # [M, 4, 3]
    return r, np.einsum("mij,mjk->mik", J[:, :, :4], PJ), J[:, :, 4:7], J[:, :, 7:10]


class _Problem:
    def __init__(self, poses, landmarks, obs_kf, obs_lm, obs_cam, fixed):
        self.kf, self.lm, self.cam = obs_kf, obs_lm, obs_cam
        K, L = len(poses), len(landmarks)
        seen_k, seen_l = np.zeros(K, bool), np.zeros(L, bool)
        seen_k[obs_kf], seen_l[obs_lm] = True, True
        self.free_k = np.flatnonzero(seen_k & ~fixed)      # the reduced program's pose blocks, in index order
        self.act_l = np.flatnonzero(seen_l)
        self.col_k = -np.ones(K, np.int64)
        self.col_k[self.free_k] = 6 * np.arange(len(self.free_k))
        self.nc = 6 * len(self.free_k)
        self.col_l = -np.ones(L, np.int64)
        self.col_l[self.act_l] = self.nc + 3 * np.arange(len(self.act_l))
        self.n = self.nc + 3 * len(self.act_l)

    def evaluate(self, poses, landmarks):
        """Evaluator::Evaluate -> ok, cost, f [3M], gradient [n], J [3M, n] (tangent columns: per free pose delta, p; then
        per landmark)"""
        with np.errstate(all="ignore"):
            r, Jd, Jp, JX = tangent_jacobians(poses, landmarks, self.kf, self.lm, self.cam)
            M = len(r)
            J = np.zeros((3 * M, self.n))
            rows = 3 * np.arange(M)[:, None, None] + np.arange(3)[None, :, None]
            ck = self.col_k[self.kf]
            m = ck >= 0
            for blk, off in ((Jd, 0), (Jp, 3)):
                cols = ck[m][:, None, None] + off + np.arange(3)[None, None, :]
                J[np.broadcast_to(rows[m], blk[m].shape), np.broadcast_to(cols, blk[m].shape)] = blk[m]
            cols = self.col_l[self.lm][:, None, None] + np.arange(3)[None, None, :]
            np.add.at(J, (np.broadcast_to(rows, JX.shape), np.broadcast_to(cols, JX.shape)), JX)
            f = r.reshape(-1)
            ok = bool(np.all(np.isfinite(f)) and np.all(np.isfinite(J)))
            c = float(np.sum(0.5 * np.sum(r * r, 1)))
            return ok, c, f, J.T @ f, J

    def plus(self, poses, landmarks, delta):
        poses, landmarks = poses.copy(), landmarks.copy()
        for k in self.free_k:
            d = delta[self.col_k[k]:self.col_k[k] + 6]
            poses[k, :4] = quaternion_plus(poses[k, :4], d[:3])
            poses[k, 4:] = poses[k, 4:] + d[3:]
        for l in self.act_l:
            landmarks[l] = landmarks[l] + delta[self.col_l[l]:self.col_l[l] + 3]
        return poses, landmarks

    def ambient(self, poses, landmarks):
        return np.concatenate([poses[self.free_k].reshape(-1), landmarks[self.act_l].reshape(-1)])


def _lm_step_qr(prob, Js, D, f):
    # the R factor of [A | b], A = [Js; D], b = [f; 0]: its last column is Q^T b, so R y = Q^T b needs no Q
    n = len(D)
    Ab = np.vstack([np.hstack([Js, f[:, None]]), np.hstack([np.diag(D), np.zeros((n, 1))])])
    rr = np.linalg.qr(Ab, mode="r")
    y = np.linalg.solve(rr[:n, :n], rr[:n, n]) if np.all(np.isfinite(rr)) else np.full(n, np.nan)
    step = -y
    m = Js @ step
    return step, -m.dot(f + m / 2.0)


def _lm_step_schur(prob, Js, D, f):
    """H = Js^T Js split into camera blocks U (6 x 6), landmark blocks V (3 x 3) and W; the landmark blocks
    with their damping are inverted one by one, the reduced system S y_c = g_c - W V^-1 g_l is solved by Cholesky (a failed
    factorisation is a non-finite, hence invalid, step), y_l = V^-1 (g_l - W^T y_c); the model cost change is
    -(Js s) . (f + Js s / 2) summed per observation"""
    nc, n = prob.nc, prob.n
    H, g = Js.T @ Js, Js.T @ f
    Vinv = np.zeros((n - nc, n - nc))
    for i in range(0, n - nc, 3):
        s = slice(nc + i, nc + i + 3)
        Vinv[i:i + 3, i:i + 3] = np.linalg.inv(H[s, s] + np.diag(D[s] ** 2))
    y = np.zeros(n)
    if nc:
        W = H[:nc, nc:]
        S = H[:nc, :nc] + np.diag(D[:nc] ** 2) - W @ Vinv @ W.T
        try:
            Lc = np.linalg.cholesky(S)
        except np.linalg.LinAlgError:
            return np.full(n, np.nan), np.nan
        y[:nc] = np.linalg.solve(Lc.T, np.linalg.solve(Lc, g[:nc] - W @ (Vinv @ g[nc:])))
        y[nc:] = Vinv @ (g[nc:] - W.T @ y[:nc])
    else:
        y[nc:] = Vinv @ g[nc:]
    step = -y
    m = (Js @ step).reshape(-1, 3)
    return step, float(np.sum(-np.sum(m * (f.reshape(-1, 3) + m / 2.0), 1)))


def bundle_adjust(poses, landmarks, obs_kf, obs_lm, obs_cam, fixed=None, max_iterations=100, linear_solver="qr"):
    """-> dict(poses, landmarks, termination, iterations, initial_cost, final_cost, gradient_max_norm, reason, trace).
    poses / landmarks are the inputs when termination is FAILURE.  trace counts `rejected` steps, accepted steps that reset a
    grown decrease factor (`accepted_after_rejected`), `invalid` steps, candidates whose cost became DBL_MAX (`dbl_max`), and
    describes the reduced program: `free_poses`, `constant_poses` (in the problem but constant), `landmarks`, and
    `landmarks_fixed_only` (seen from constant keyframes only)."""
    lm_step = {"qr": _lm_step_qr, "schur": _lm_step_schur}[linear_solver]
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
    prob = _Problem(poses0, lms0, obs_kf, obs_lm, obs_cam, fixed)
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


# ---- scenes -----------------------------------------------------------------------------------------------------------
def random_rotation_quaternion(rng, angle):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    return np.concatenate([np.sin(angle / 2.0) * axis, [np.cos(angle / 2.0)]])


def make_scene(K, L, seed, noise=0.0, views=None, start_angle=0.05, start_shift=0.05, fix_first=True, perturb_fixed=False):
    """K keyframes near the origin looking down +z at L landmarks 1.5 .. 4 m away; every landmark is seen from `views`
    keyframes (default: all, at least two).  -> dict(truth_poses, truth_landmarks, poses, landmarks (the start: every free
    pose moved by Plus with a tangent of length start_angle — a turn by twice that angle — and shifted by start_shift m in a random direction, every landmark
    shifted by start_shift), fixed, obs_kf, obs_lm, obs_cam (exact camera-frame points + N(0, noise) per coordinate))."""
    rng = np.random.default_rng(seed)
    tp = np.zeros((K, 7))
    for k in range(K):
        tp[k, :4] = random_rotation_quaternion(rng, rng.uniform(0.0, 0.25)) if k else (0, 0, 0, 1)
        tp[k, 4:] = rng.uniform(-0.4, 0.4, 3) if k else 0.0
    tl = np.stack([rng.uniform(-1.5, 1.5, L), rng.uniform(-1.0, 1.0, L), rng.uniform(1.5, 4.0, L)], 1)
    views = K if views is None else min(views, K)
    okf, olm = [], []
    for l in range(L):
        ks = np.sort(rng.choice(K, size=views, replace=False)) if views < K else np.arange(K)
        okf += ks.tolist()
        olm += [l] * len(ks)
    okf, olm = np.array(okf, np.int32), np.array(olm, np.int32)
    cam = residuals(tp, tl, okf, olm, np.zeros((len(okf), 3))) + noise * rng.normal(size=(len(okf), 3))
    fixed = np.zeros(K, np.uint8)
    fixed[0] = 1 if fix_first else 0
    sp, sl = tp.copy(), tl.copy()
    for k in range(K):
        if fixed[k] and not perturb_fixed:
            continue
        axis = rng.normal(size=3)
        q = quaternion_plus(tp[k, :4], start_angle * axis / np.linalg.norm(axis))
        sp[k, :4] = q / np.linalg.norm(q)
        d = rng.normal(size=3)
        sp[k, 4:] += start_shift * d / np.linalg.norm(d)
    d = rng.normal(size=(L, 3))
    sl += start_shift * d / np.linalg.norm(d, axis=1)[:, None]
    return dict(truth_poses=tp, truth_landmarks=tl, poses=sp, landmarks=sl, fixed=fixed, obs_kf=okf, obs_lm=olm, obs_cam=cam)


def solve_scene(sc, **kw):
    return bundle_adjust(sc["poses"], sc["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"], sc["fixed"], **kw)
