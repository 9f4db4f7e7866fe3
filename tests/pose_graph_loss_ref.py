"""CPU restatement of the pose-graph solve with a loss function (mslam_hip_set_pose_graph_loss), for the tests.

tests/pose_graph_ref.py restates the solve without a loss.  This module adds what Ceres 2.2 does when a loss is given, each
piece from the published source named beside it, and shares nothing with the HIP kernels:

  * loss_function.h, HuberLoss::Evaluate and CauchyLoss::Evaluate at s = |r_e|^2 (the residual block's squared norm: all six
    weighted components of an edge together), with scale a and b = a^2:
        Huber   s <= b: rho = s, rho' = 1;   else rho = 2 a sqrt(s) - b, rho' = max(DBL_MIN, a / sqrt(s))
        Cauchy  rho = b log(1 + s c), rho' = max(DBL_MIN, 1 / (1 + s c)), c = 1 / b
  * corrector.cc: rho'' <= 0 for both, so the constructor takes `sq_norm == 0 || rho[2] <= 0`: residual_scaling =
    jacobian_scaling = sqrt(rho'), no curvature term; residual_block.cc: the block's cost is rho / 2.

LossProblem is pose_graph_ref._Problem with evaluate() corrected that way: f and the rows of J scaled by sqrt(rho') per edge,
cost 1/2 sum rho, gradient J^T f of the corrected pair.  pose_graph_ref.pose_graph builds its _Problem itself, so its
trust-region loop is restated here with the problem as the one difference; with loss = None it returns what
pose_graph_ref.pose_graph returns, bit for bit (tests/test_pose_graph_loss.py).  Both linear solvers of pose_graph_ref work
on the corrected pair unchanged.

The scenes: every kernel shape at which a per-edge weight can go wrong (SHAPES), and the three graphs with false loop edges
that show what the loss is for (FALSE_LOOPS).  A bad edge's measurement is pose_graph_cases._perturb(meas, rng, 0.6, 1.5):
turned by 0.6 rad and moved by 1.5 m.  The scale of the tests is 0.1 in the unit of the weighted residual.

PARITY UNPINNED, as pose_graph_ref: no Ceres build exists here.  This is test infrastructure (not a conftest.py, not under
oracle/)."""
import functools

import numpy as np

import pose_graph_cases as pc
import pose_graph_ref as pg
from pose_graph_ref import (CONVERGENCE, DBL_MAX, FAILURE, FUNCTION_TOLERANCE, GRADIENT_TOLERANCE, INITIAL_TRUST_REGION_RADIUS,
                            MAX_LM_DIAGONAL, MAX_NUM_CONSECUTIVE_INVALID_STEPS, MAX_TRUST_REGION_RADIUS, MIN_LM_DIAGONAL,
                            MIN_RELATIVE_DECREASE, MIN_TRUST_REGION_RADIUS, NO_CONVERGENCE, PARAMETER_TOLERANCE)

DBL_MIN = np.finfo(np.float64).tiny
NONE, HUBER, CAUCHY = 0, 1, 2
KINDS = {"none": NONE, "huber": HUBER, "cauchy": CAUCHY}
SCALE = 0.1           # a of the tests, in the unit of the weighted residual


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


def chi2(poses, edge_a, edge_b, edge_meas, sqrt_info=None):
    """|r_e|^2 per edge"""
    r = pg.residuals(poses, edge_a, edge_b, edge_meas, sqrt_info)
    return np.sum(r * r, 1)


def weights(poses, edge_a, edge_b, edge_meas, sqrt_info=None, how=None):
    """rho'(|r_e|^2) per edge, 1.0 without a loss"""
    kind, a = _how(how)
    s = chi2(poses, edge_a, edge_b, edge_meas, sqrt_info)
    return np.ones(len(s)) if kind == NONE else loss(kind, a, s)[1]


def cost(poses, edge_a, edge_b, edge_meas, sqrt_info=None, how=None):
    """1/2 sum rho(|r_e|^2)"""
    kind, a = _how(how)
    s = chi2(poses, edge_a, edge_b, edge_meas, sqrt_info)
    return float(np.sum(0.5 * (s if kind == NONE else loss(kind, a, s)[0])))


class LossProblem(pg._Problem):
    def __init__(self, K, ea, eb, meas, info, fixed, kind, a):
        super().__init__(K, ea, eb, meas, info, fixed)
        self.kind, self.a = kind, a

    def evaluate(self, poses):
        ok, c, f, g, J = super().evaluate(poses)
        if self.kind == NONE:
            return ok, c, f, g, J
        with np.errstate(all="ignore"):
            r = f.reshape(-1, 6)
            rho, w = loss(self.kind, self.a, np.sum(r * r, 1))
            scaling = np.sqrt(w)
            f = (r * scaling[:, None]).reshape(-1)
            J = J * np.repeat(scaling, 6)[:, None]
            ok = bool(np.all(np.isfinite(f)) and np.all(np.isfinite(J)))
            return ok, float(np.sum(0.5 * rho)), f, J.T @ f, J


def pose_graph(poses, edge_a, edge_b, edge_meas, sqrt_info=None, fixed=None, max_iterations=100, linear_solver="qr", loss=None):
    """pose_graph_ref.pose_graph's loop and result dict (trace: the counters) on a LossProblem.  loss = None or (kind, a) with
    kind "huber" / "cauchy" or the integers"""
    kind, a = _how(loss)
    lm_step = {"qr": pg._step_qr, "chol": pg._step_chol}[linear_solver]
    poses0, ea, eb, meas, info = pg._arrays(poses, edge_a, edge_b, edge_meas, sqrt_info)
    fixed = np.zeros(len(poses0), bool) if fixed is None else np.asarray(fixed).astype(bool)
    trace = dict(rejected=0, accepted_after_rejected=0, invalid=0, dbl_max=0, free_poses=0)
    x = poses0.copy()

    def out(term, it, c0, c, reason, gmax=np.nan, usable=True):
        return dict(poses=x if usable else poses0, termination=term, iterations=it, initial_cost=c0, final_cost=c,
                    gradient_max_norm=gmax, reason=reason, trace=trace)

    if len(ea) == 0:
        return out(CONVERGENCE, 0, 0.0, 0.0, "no parameter blocks", 0.0)
    prob = LossProblem(len(poses0), ea, eb, meas, info, fixed, kind, a)
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
        if step_norm <= PARAMETER_TOLERANCE * (np.linalg.norm(x_amb) + PARAMETER_TOLERANCE):
            return out(CONVERGENCE, iteration, initial_cost, x_cost, "parameter tolerance", gmax)
        if abs(x_cost - candidate_cost) <= FUNCTION_TOLERANCE * x_cost:
            return out(CONVERGENCE, iteration, initial_cost, x_cost, "function tolerance", gmax)
        relative_decrease = -DBL_MAX if candidate_cost >= DBL_MAX else (x_cost - candidate_cost) / model_cost_change
        if relative_decrease > MIN_RELATIVE_DECREASE:
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
            radius /= decrease_factor
            decrease_factor *= 2.0


def solve(sc, linear_solver="qr", loss=None):
    return pose_graph(sc["poses"], sc["edge_a"], sc["edge_b"], sc["edge_meas"], sc["sqrt_info"], sc["fixed"],
                      sc.get("max_iterations", 100), linear_solver=linear_solver, loss=loss)


# ---- scenes -----------------------------------------------------------------------------------------------------------
def spoil(sc, bad, seed):
    """the measurements of the edges `bad` turned by 0.6 rad and moved by 1.5 m, by a generator of its own -> the scene with
    `bad` (sorted indices) recorded"""
    bad = np.sort(np.asarray(bad, np.int64))
    rng = np.random.default_rng([seed, 77])
    sc = dict(sc, edge_meas=sc["edge_meas"].copy())
    for e in bad:
        sc["edge_meas"][e] = pc._perturb(sc["edge_meas"][e], rng, 0.6, 1.5)
    sc["bad"] = bad
    return sc


def _edges(E):
    """pose_graph_cases' edges:E (E random ordered pairs among 20 poses): blocks of 256 edges in k_pg_edges_loss and
    k_pg_eval_loss.  Bad: edge 3, the last edge (the tail block's partial sum when E = 257) and, when there is one, edge 256"""
    return spoil(pc.scene("edges:%d" % E), sorted({3, E - 1} | ({256} if E > 256 else set())), E)


def _hub():
    """pose_graph_cases' star70 (the hub, pose 0, free, is an end of the first 70 edges; leaf 1 constant) with a ring through
    the leaves listed after them, so that a bad spoke disagrees with its neighbours and stays down-weighted.  Edge e < 70 is
    the hub's incidence e and a lane of k_pg_poses takes incidences l and l + 64.  Bad: 64, 67 and 69, the second trip of
    lanes 0, 3 and 5"""
    spokes = [(0, k) if k % 2 else (k, 0) for k in range(1, 71)]
    return spoil(pc.make_scene(71, spokes + [(k, k + 1) for k in range(1, 70)], 5, fixed=(1,)), [64, 67, 69], 70)


def _dup3():
    """three edges on the pair (1, 2), the middle one bad: the pair's serial loop sums three products of three weights"""
    return spoil(pc.make_scene(5, [(0, 1), (1, 2), (1, 2), (1, 2), (2, 3), (3, 4), (4, 0), (0, 2)], 41), [2], 41)


def _to_fixed():
    """the bad edge (0, 3) ends at the constant pose 0: its weight reaches pose 3's diagonal block and gradient, no pair"""
    return spoil(pc.make_scene(6, pc.chain(6, 1) + [(0, 3)], 42), [6], 42)


def _info_dense():
    """pose_graph_cases' info_dense (a full sqrt_info; edge 2 weighs the position only; the last edge's matrix is zero: s = 0
    there, whatever the measurement) with edge 4 bad"""
    return spoil(pc.scene("info_dense"), [4], 43)


def false_loops(K, n_true, n_false, seed):
    """a chain of K poses with n_true extra loop edges and n_false grossly wrong ones after them, pose 0 constant: edges and
    noise from pose_graph_cases.make_scene (noise 0.01); the loop edges join pairs at least 3 apart, drawn by a generator
    seeded with (seed, K)"""
    rng = np.random.default_rng([seed, K])
    loops = []
    while len(loops) < n_true + n_false:
        a, b = sorted(rng.integers(0, K, 2).tolist())
        if b - a >= 3 and (a, b) not in loops:
            loops.append((a, b))
    sc = pc.make_scene(K, pc.chain(K, 0) + loops, seed, noise=0.01)
    return spoil(sc, np.arange(K - 1 + n_true, K - 1 + n_true + n_false), seed)


SHAPES = {
    "one": lambda: spoil(pc.scene("pair"), [0], 1),
    "edges:255": lambda: _edges(255),
    "edges:256": lambda: _edges(256),
    "edges:257": lambda: _edges(257),
    "hub": _hub,
    "dup3": _dup3,
    "to_fixed": _to_fixed,
    "info_dense": _info_dense,
}
FALSE_LOOPS = {
    "false:12,4,1,1": lambda: false_loops(12, 4, 1, 1),
    "false:40,10,3,2": lambda: false_loops(40, 10, 3, 2),
    "false:70,12,3,5": lambda: false_loops(70, 12, 3, 5),
}
SCENES = dict(SHAPES, **FALSE_LOOPS)
LOSSES = ("huber", "cauchy")


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def reference(name, kind):
    """-> (scene, qr result, chol result, |x_chol - x_qr|_inf up to the quaternions' signs); kind "none" / "huber" / "cauchy"
    at SCALE.  Computed once and shared: do not write into what this returns"""
    sc = scene(name)
    how = None if kind == "none" else (kind, SCALE)
    qr, ch = solve(sc, "qr", how), solve(sc, "chol", how)
    return sc, qr, ch, pc.same_rotation_distance(qr["poses"], ch["poses"])


def position_error(sc, poses):
    """the largest distance of a position from the truth's"""
    return float(np.max(np.linalg.norm(np.asarray(poses)[:, 4:] - sc["truth_poses"][:, 4:], axis=1)))


THRESHOLD_A = 0.5


def threshold_scene():
    """pose_graph_cases' pair shape on exact values: identity rotations, pose 0 at the origin (constant), pose 1 at (1, 0, 0),
    the measurement (0, 0, 0, 1; 0.5, 0, 0).  A rotation by (0, 0, 0, 1) adds only zeros, so r = (0.5, 0, 0, 0, 0, 0) and
    |r|^2 = 0.25 = THRESHOLD_A^2, each exactly: Huber's inlier branch at a = 0.5 (cost 0.125), the other at nextafter(0.5, 0)"""
    poses = np.array([[0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 1.0, 0, 0]], np.float64)
    sc = dict(truth_poses=poses.copy(), poses=poses, fixed=np.array([1, 0], np.uint8), edge_a=np.array([0], np.int32),
              edge_b=np.array([1], np.int32), edge_meas=np.array([[0, 0, 0, 1, 0.5, 0, 0]], np.float64), sqrt_info=None)
    r = pg.residuals(poses, sc["edge_a"], sc["edge_b"], sc["edge_meas"])
    assert r.tolist() == [[0.5, 0.0, 0.0, 0.0, 0.0, 0.0]]
    return sc
