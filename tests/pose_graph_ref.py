"""CPU restatement of mslam_hip_pose_graph's solve (modular-slam_amd/csrc/k_posegraph.hip) and of HipBackend.close_loop,
for the tests.

The cost is 1/2 sum_e |r_e|^2 over the edges e = (a, b) with, as in Ceres's published pose_graph_3d example
(pose_graph_3d_error_term.h),

    p_ab = rot(q_a^-1, p_b - p_a)    q_ab = q_a^-1 (x) q_b    delta = q_meas (x) q_ab^-1
    r_e  = sqrt_info_e [p_ab - p_meas ; 2 vec(delta)]                      (no sign fix on delta)

poses (q as x y z w, p; camera -> world) on an EigenQuaternionManifold.  This module restates, in numpy and sharing nothing
with the HIP kernels:

  * the residual on jets (tests/ba_ref.py's forward-mode helpers, fourteen slots: q_a, p_a, q_b, p_b), Eigen's inverse(),
    quaternion product and _transformVector; the tangent Jacobian of a residual is the jets' times PlusJacobian;
  * analytic_jacobians(): the matrices DESIGN.md 4.17 writes down, for the test that compares them with the jets;
  * the trust region of tests/ba_ref.py (TrustRegionMinimizer, monotonic step evaluator, LevenbergMarquardtStrategy, the
    defaults of solver.h, Jacobi scaling), its norms over the ambient parameters of the free poses that have an edge;
  * two linear solvers for the damped step: "qr" on the stacked damped Jacobian, "chol" on the normal equations.  Both are
    correct and differ in rounding only; the GPU tests take their bound from the distance of the two;
  * close_loop(): what HipBackend.close_loop builds of a covisibility graph and a loop measurement, and the rigid move of the
    landmarks with their anchor keyframes.

PARITY UNPINNED: no Ceres build exists here; the restatement is pinned to ground truth and the analytic derivatives to the
jets.  This is test infrastructure (not a conftest.py, not under oracle/)."""
import numpy as np

import ba_ref
from ba_ref import (CONVERGENCE, DBL_MAX, FAILURE, FUNCTION_TOLERANCE, GRADIENT_TOLERANCE, INITIAL_TRUST_REGION_RADIUS,  # noqa: F401
                    MAX_LM_DIAGONAL, MAX_NUM_CONSECUTIVE_INVALID_STEPS, MAX_TRUST_REGION_RADIUS, MIN_LM_DIAGONAL,
                    MIN_RELATIVE_DECREASE, MIN_TRUST_REGION_RADIUS, NO_CONVERGENCE, PARAMETER_TOLERANCE, plus_jacobian,
                    quaternion_plus)
from ba_ref import _add, _const, _inverse, _mul, _sub, _transform_vector


def _product(a, b):
    """Eigen's quaternion product on jets, x y z w"""
    w = _sub(_sub(_sub(_mul(a[3], b[3]), _mul(a[0], b[0])), _mul(a[1], b[1])), _mul(a[2], b[2]))
    x = _sub(_add(_add(_mul(a[3], b[0]), _mul(a[0], b[3])), _mul(a[1], b[2])), _mul(a[2], b[1]))
    y = _sub(_add(_add(_mul(a[3], b[1]), _mul(a[1], b[3])), _mul(a[2], b[0])), _mul(a[0], b[2]))
    z = _sub(_add(_add(_mul(a[3], b[2]), _mul(a[2], b[3])), _mul(a[0], b[1])), _mul(a[1], b[0]))
    return [x, y, z, w]


def error_jets(xa, xb, meas, info=None, slots=14):
    """xa, xb, meas [E, 7] -> residuals [E, 6], Jacobian [E, 6, slots] over (q_a, p_a, q_b, p_b); slots = 0: plain doubles"""
    E = len(xa)
    eye = np.eye(14)[:, :slots]

    def seed(a, k):
        return np.asarray(a, np.float64), np.broadcast_to(eye[k], (E, slots)).copy()
    qa, pa = [seed(xa[:, k], k) for k in range(4)], [seed(xa[:, 4 + k], 4 + k) for k in range(3)]
    qb, pb = [seed(xb[:, k], 7 + k) for k in range(4)], [seed(xb[:, 4 + k], 11 + k) for k in range(3)]
    qm = [_const(meas[:, k], slots) for k in range(4)]
    qai = _inverse(qa)
    pab = _transform_vector(qai, [_sub(pb[k], pa[k]) for k in range(3)])
    dq = _product(qm, _inverse(_product(qai, qb)))
    u = [_sub(pab[k], _const(meas[:, 4 + k], slots)) for k in range(3)] + [_add(dq[k], dq[k]) for k in range(3)]
    r, J = np.stack([c[0] for c in u], 1), np.stack([c[1] for c in u], 1)
    if info is not None:
        W = np.asarray(info, np.float64).reshape(E, 6, 6)
        r, J = np.einsum("eij,ej->ei", W, r), np.einsum("eij,ejk->eik", W, J)
    return r, J


def _arrays(poses, edge_a, edge_b, edge_meas, sqrt_info):
    poses = np.array(poses, np.float64).reshape(-1, 7)
    ea, eb = np.asarray(edge_a, np.int64).reshape(-1), np.asarray(edge_b, np.int64).reshape(-1)
    meas = np.asarray(edge_meas, np.float64).reshape(-1, 7)
    info = None if sqrt_info is None else np.asarray(sqrt_info, np.float64).reshape(-1, 6, 6)
    return poses, ea, eb, meas, info


def residuals(poses, edge_a, edge_b, edge_meas, sqrt_info=None):
    poses, ea, eb, meas, info = _arrays(poses, edge_a, edge_b, edge_meas, sqrt_info)
    if len(ea) == 0:
        return np.zeros((0, 6))
    with np.errstate(all="ignore"):
        return error_jets(poses[ea], poses[eb], meas, info, 0)[0]


def cost(poses, edge_a, edge_b, edge_meas, sqrt_info=None):
    r = residuals(poses, edge_a, edge_b, edge_meas, sqrt_info)
    return float(np.sum(0.5 * np.sum(r * r, 1)))


def tangent_jacobians(poses, ea, eb, meas, info=None):
    """-> residuals [E, 6], J_a [E, 6, 6], J_b [E, 6, 6] over each pose's tangent (delta, dp): the jets' times PlusJacobian"""
    r, J = error_jets(poses[ea], poses[eb], meas, info)
    PJ = np.stack([plus_jacobian(q) for q in poses[:, :4]])
    Ja = np.concatenate([np.einsum("eij,ejk->eik", J[:, :, 0:4], PJ[ea]), J[:, :, 4:7]], 2)
    Jb = np.concatenate([np.einsum("eij,ejk->eik", J[:, :, 7:11], PJ[eb]), J[:, :, 11:14]], 2)
    return r, Ja, Jb


# ---- plain quaternions and rigid motions (x y z w; T = (q, p)) ------------------------------------------------------------
def q_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def q_inv(q):
    q = np.asarray(q, np.float64)
    return np.array([-q[0], -q[1], -q[2], q[3]]) / np.dot(q, q)


def q_matrix(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def compose(Ta, Tb):
    """T_a o T_b"""
    q = q_mul(Ta[:4], Tb[:4])
    return np.concatenate([q / np.linalg.norm(q), q_matrix(Ta[:4]) @ Tb[4:] + Ta[4:]])


def inverse(T):
    qi = q_inv(T[:4])
    return np.concatenate([qi, -(q_matrix(qi) @ T[4:])])


def relative(Ta, Tb):
    """T_a^-1 o T_b: pose b in a's frame, the measurement of an edge (a, b)"""
    return compose(inverse(np.asarray(Ta, np.float64)), np.asarray(Tb, np.float64))


def analytic_jacobians(poses, ea, eb, meas, info=None):
    """with P = the matrix of v -> rot(q_a^-1, v), v = p_b - p_a, A = q_meas (x) q_b^-1, B = q_a and M the
    matrix of u -> vec(A (x) (u, 0) (x) B):  J_a = W [[2 P [v]x, -P], [2 M, 0]],  J_b = W [[0, P], [-2 M, 0]]"""
    E = len(ea)
    Ja, Jb = np.zeros((E, 6, 6)), np.zeros((E, 6, 6))
    for e in range(E):
        xa, xb = poses[ea[e]], poses[eb[e]]
        P = q_matrix(q_inv(xa[:4]))
        v = xb[4:] - xa[4:]
        vx = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
        A, B = q_mul(meas[e, :4], q_inv(xb[:4])), xa[:4]
        M = np.stack([q_mul(q_mul(A, np.append(u, 0.0)), B)[:3] for u in np.eye(3)], 1)
        Ja[e, :3, :3], Ja[e, :3, 3:], Ja[e, 3:, :3] = 2.0 * P @ vx, -P, 2.0 * M
        Jb[e, :3, 3:], Jb[e, 3:, :3] = P, -2.0 * M
        if info is not None:
            Ja[e], Jb[e] = info[e] @ Ja[e], info[e] @ Jb[e]
    return Ja, Jb


class _Problem:
    def __init__(self, K, ea, eb, meas, info, fixed):
        self.ea, self.eb, self.meas, self.info = ea, eb, meas, info
        seen = np.zeros(K, bool)
        seen[ea], seen[eb] = True, True
        self.free = np.flatnonzero(seen & ~fixed)          # the program's pose blocks, in index order
        self.col = -np.ones(K, np.int64)
        self.col[self.free] = 6 * np.arange(len(self.free))
        self.n = 6 * len(self.free)

    def evaluate(self, poses):
        """-> ok, cost, f [6E], gradient [n], J [6E, n]"""
        with np.errstate(all="ignore"):
            r, Ja, Jb = tangent_jacobians(poses, self.ea, self.eb, self.meas, self.info)
            E = len(r)
            J = np.zeros((6 * E, self.n))
            for blk, ends in ((Ja, self.ea), (Jb, self.eb)):
                for e in np.flatnonzero(self.col[ends] >= 0):
                    c = self.col[ends[e]]
                    J[6 * e:6 * e + 6, c:c + 6] = blk[e]
            f = r.reshape(-1)
            ok = bool(np.all(np.isfinite(f)) and np.all(np.isfinite(Ja)) and np.all(np.isfinite(Jb)))
            return ok, float(np.sum(0.5 * np.sum(r * r, 1))), f, J.T @ f, J

    def plus(self, poses, delta):
        poses = poses.copy()
        for k in self.free:
            d = delta[self.col[k]:self.col[k] + 6]
            poses[k, :4] = quaternion_plus(poses[k, :4], d[:3])
            poses[k, 4:] = poses[k, 4:] + d[3:]
        return poses

    def ambient(self, poses):
        return poses[self.free].reshape(-1)


def _step_qr(Js, D, f):
    n = len(D)
    Ab = np.vstack([np.hstack([Js, f[:, None]]), np.hstack([np.diag(D), np.zeros((n, 1))])])
    rr = np.linalg.qr(Ab, mode="r")
    y = np.linalg.solve(rr[:n, :n], rr[:n, n]) if np.all(np.isfinite(rr)) else np.full(n, np.nan)
    step = -y
    m = Js @ step
    return step, -m.dot(f + m / 2.0)


def _step_chol(Js, D, f):
    """the normal equations (Js^T Js + D^2) y = Js^T f by Cholesky (a failed factorisation is an invalid step); the model
    cost change summed per edge"""
    n = len(D)
    try:
        Lc = np.linalg.cholesky(Js.T @ Js + np.diag(D * D))
    except np.linalg.LinAlgError:
        return np.full(n, np.nan), np.nan
    step = -np.linalg.solve(Lc.T, np.linalg.solve(Lc, Js.T @ f))
    m = (Js @ step).reshape(-1, 6)
    return step, float(np.sum(-np.sum(m * (f.reshape(-1, 6) + m / 2.0), 1)))


def pose_graph(poses, edge_a, edge_b, edge_meas, sqrt_info=None, fixed=None, max_iterations=100, linear_solver="qr"):
    """-> dict(poses, termination, iterations, initial_cost, final_cost, gradient_max_norm, reason, trace).  poses are the
    inputs when termination is FAILURE.  trace counts `rejected`, `accepted_after_rejected`, `invalid`, `dbl_max` and gives
    `free_poses`; trace["steps"] has one entry per iteration, the decisions of the loop: `parameter_ratio` = step_norm /
    (PARAMETER_TOLERANCE (|x| + PARAMETER_TOLERANCE)) and `function_ratio` = |x_cost - candidate_cost| / (FUNCTION_TOLERANCE
    x_cost) (a test fires at a ratio <= 1; both None for an invalid step) and `decision`: "accepted", "rejected", "invalid",
    or "converged" for the iteration one of the two tests ended."""
    lm_step = {"qr": _step_qr, "chol": _step_chol}[linear_solver]
    poses0, ea, eb, meas, info = _arrays(poses, edge_a, edge_b, edge_meas, sqrt_info)
    fixed = np.zeros(len(poses0), bool) if fixed is None else np.asarray(fixed).astype(bool)
    trace = dict(rejected=0, accepted_after_rejected=0, invalid=0, dbl_max=0, free_poses=0, steps=[])
    x = poses0.copy()

    def out(term, it, c0, c, reason, gmax=np.nan, usable=True):
        return dict(poses=x if usable else poses0, termination=term, iterations=it, initial_cost=c0, final_cost=c,
                    gradient_max_norm=gmax, reason=reason, trace=trace)

    if len(ea) == 0:
        return out(CONVERGENCE, 0, 0.0, 0.0, "no parameter blocks", 0.0)
    prob = _Problem(len(poses0), ea, eb, meas, info, fixed)
    trace["free_poses"] = len(prob.free)

    def gradient_max_norm(g):
        return float(np.max(np.abs(prob.ambient(x) - prob.ambient(prob.plus(x, -g))), initial=0.0))

    ok, x_cost, f, g, J = prob.evaluate(x)
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
            step, model_cost_change = lm_step(Js, D, f)
        if not (np.all(np.isfinite(step)) and model_cost_change > 0.0):
            invalid += 1
            trace["invalid"] += 1
            trace["steps"].append(dict(parameter_ratio=None, function_ratio=None, decision="invalid"))
            if invalid >= MAX_NUM_CONSECUTIVE_INVALID_STEPS:
                return out(FAILURE, iteration, initial_cost, x_cost, "too many invalid steps", gmax, usable=False)
            radius /= decrease_factor
            decrease_factor *= 2.0
            continue
        invalid = 0
        c_x = prob.plus(x, step * scale)
        c_ok, candidate_cost, c_f, c_g, c_J = prob.evaluate(c_x)
        if not np.isfinite(candidate_cost):
            candidate_cost = DBL_MAX
            trace["dbl_max"] += 1
        x_amb = prob.ambient(x)
        step_norm = np.linalg.norm(x_amb - prob.ambient(c_x))
        with np.errstate(all="ignore"):
            entry = dict(parameter_ratio=float(step_norm / (PARAMETER_TOLERANCE * (np.linalg.norm(x_amb) + PARAMETER_TOLERANCE))),
                         function_ratio=float(np.float64(abs(x_cost - candidate_cost)) / np.float64(FUNCTION_TOLERANCE * x_cost)),
                         decision="converged")
        trace["steps"].append(entry)
        if step_norm <= PARAMETER_TOLERANCE * (np.linalg.norm(x_amb) + PARAMETER_TOLERANCE):
            return out(CONVERGENCE, iteration, initial_cost, x_cost, "parameter tolerance", gmax)
        if abs(x_cost - candidate_cost) <= FUNCTION_TOLERANCE * x_cost:
            return out(CONVERGENCE, iteration, initial_cost, x_cost, "function tolerance", gmax)
        relative_decrease = -DBL_MAX if candidate_cost >= DBL_MAX else (x_cost - candidate_cost) / model_cost_change
        if relative_decrease > MIN_RELATIVE_DECREASE:
            entry["decision"] = "accepted"
            if not c_ok:
                return out(FAILURE, iteration, initial_cost, x_cost, "evaluation at the accepted point failed", gmax, usable=False)
            x = c_x
            x_cost, f, g, J = candidate_cost, c_f, c_g, c_J
            gmax = gradient_max_norm(g)
            successful = True
            radius = min(MAX_TRUST_REGION_RADIUS, radius / max(1.0 / 3.0, 1.0 - (2.0 * relative_decrease - 1.0) ** 3))
            trace["accepted_after_rejected"] += decrease_factor != 2.0
            decrease_factor = 2.0
        else:
            trace["rejected"] += 1
            entry["decision"] = "rejected"
            radius /= decrease_factor
            decrease_factor *= 2.0


# ---- HipBackend.close_loop, restated ----------------------------------------------------------------------------------------
def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th < 1e-300:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)


def matrix_to_quaternion(R):
    """unit quaternion x y z w, w >= 0 (the branch with the largest divisor)"""
    t = [R[0, 0] - R[1, 1] - R[2, 2], R[1, 1] - R[0, 0] - R[2, 2], R[2, 2] - R[0, 0] - R[1, 1], R[0, 0] + R[1, 1] + R[2, 2]]
    i = int(np.argmax(t))
    r = np.sqrt(1.0 + t[i])
    if i == 3:
        q = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], r * r]) / (2.0 * r)
    else:
        j, k = (i + 1) % 3, (i + 2) % 3
        q = np.zeros(4)
        q[i], q[j], q[k], q[3] = r * r, R[j, i] + R[i, j], R[k, i] + R[i, k], R[k, j] - R[j, k]
        q /= 2.0 * r
    q /= np.linalg.norm(q)
    return q if q[3] >= 0 else -q


def loop_measurement(T_loop, rvec, tvec):
    """Z = T_loop^-1 o T_cur*, T_cur* = (R^T, -R^T t) the camera -> world pose PnP found for the current keyframe"""
    R = rodrigues(rvec)
    T_cur = np.concatenate([matrix_to_quaternion(R.T), -R.T @ np.asarray(tvec, np.float64)])
    return relative(T_loop, T_cur)


def loop_problem(poses, first, graph, cur_id, loop_id, rvec, tvec, sqrt_info=None):
    """poses: id -> [7]; graph: id -> set of ids.  -> (ids, poses [K, 7], fixed, edge_a, edge_b, edge_meas, sqrt_info): every
    graph edge i < j with both ends in poses, sorted, measured on the current poses; the loop edge last"""
    ids = sorted(poses)
    index = {id: k for k, id in enumerate(ids)}
    x = np.array([poses[id] for id in ids], np.float64).reshape(-1, 7)
    ea, eb, meas = [], [], []
    for i in ids:
        for j in sorted(graph.get(i, ())):
            if i < j and j in index:
                ea.append(index[i]), eb.append(index[j]), meas.append(relative(poses[i], poses[j]))
    ea.append(index[loop_id]), eb.append(index[cur_id]), meas.append(loop_measurement(poses[loop_id], rvec, tvec))
    info = None
    if sqrt_info is not None:
        info = np.tile(np.eye(6), (len(ea), 1, 1))
        info[-1] = np.asarray(sqrt_info, np.float64).reshape(6, 6)
    fixed = np.array([id == first for id in ids], np.uint8)
    return ids, x, fixed, np.array(ea, np.int32), np.array(eb, np.int32), np.array(meas).reshape(-1, 7), info


def move_landmarks(ids, before, after, anchor, landmarks):
    """X' = T_a' T_a^-1 X for the landmark's anchor keyframe a -> (landmark ids sorted, points)"""
    index = {id: k for k, id in enumerate(ids)}
    lids = sorted(l for l in landmarks if anchor.get(l) in index)
    out = np.zeros((len(lids), 3))
    for i, l in enumerate(lids):
        k = index[anchor[l]]
        local = q_matrix(q_inv(before[k, :4])) @ (np.asarray(landmarks[l], np.float64) - before[k, 4:])
        out[i] = q_matrix(after[k, :4]) @ local + after[k, 4:]
    return lids, out


def close_loop(poses, first, graph, anchor, landmarks, cur_id, loop_id, rvec, tvec, sqrt_info=None, max_iterations=100,
               linear_solver="qr"):
    ids, x, fixed, ea, eb, meas, info = loop_problem(poses, first, graph, cur_id, loop_id, rvec, tvec, sqrt_info)
    res = pose_graph(x, ea, eb, meas, info, fixed, max_iterations, linear_solver)
    lids, lm = move_landmarks(ids, x, res["poses"], anchor, landmarks)
    res.update(keyframes=ids, poses_before=x, landmark_ids=np.array(lids, np.int64), landmarks=lm,
               edge_a=ea, edge_b=eb, edge_meas=meas, sqrt_info=info, fixed=fixed)
    return res
