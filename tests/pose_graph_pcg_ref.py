"""CPU reference for mslam_hip_pose_graph with mslam_hip_set_pose_graph_pcg (k_pg_assemble_pairs of
modular-slam_amd/csrc/k_posegraph.hip, the kernels of k_pcg.hip), for the tests.

pose_graph() is tests/pose_graph_sparse_ref.py's Levenberg-Marquardt loop (its _Problem, the same order of the tests, the same
trust region: the code itself, not a copy) with one other step: the damped, scaled normal equations A = Js^T Js + D^2 and
b = Js^T f are formed explicitly (scipy.sparse) and A y = b is solved by tests/ba_global_pcg_ref.py's pcg(): block-Jacobi
preconditioned conjugate gradients from y = 0, M = the 6 x 6 diagonal blocks of A, stop at |r|_2 <= tol |b|_2 or at the cap,
whose iterate is taken; b = 0 gives 0 without an iteration; p . q not > 0 or not finite is an invalid step.  The result gains
cg = the CG iterations of every linear solve, at_cap and breakdowns.  The step is inexact; the model cost change is taken from
Js step as for any step.  loss = ("huber" | "cauchy", a): Ceres's corrector on the rows and the cost 1/2 sum rho, with
tests/pose_graph_loss_ref.py's formulas, as k_pg_edges_loss / k_pg_eval_loss apply them before the assembly.
The loop takes its step from the module attribute pose_graph_sparse_ref._step_normal, which pose_graph() replaces for the
length of one call.  This is test infrastructure (not a conftest.py, not under oracle/)."""
import numpy as np
import scipy.sparse as sp

import ba_global_pcg_ref as bp
import pose_graph_loss_ref as pl
import pose_graph_sparse_ref as ps

MAX_ITERATIONS, TOLERANCE = 500, 1e-6      # the defaults of mslam_hip_set_pose_graph_pcg
TIGHT = (2000, 1e-12)                      # the tests' tight tier


class _LossProblem(ps._Problem):
    """pose_graph_sparse_ref._Problem with the corrector on the rows: f and J times sqrt(rho'(|r_e|^2)), cost 1/2 sum rho"""
    kind, a = pl.NONE, 0.0

    def evaluate(self, poses):
        ok, cost, f, g, J = super().evaluate(poses)
        with np.errstate(all="ignore"):
            r = f.reshape(-1, 6)
            rho, w = pl.loss(self.kind, self.a, np.sum(r * r, 1))
            sw = np.repeat(np.sqrt(w), 6)
            J = (sp.diags(sw) @ J).tocsr()
            f = sw * f
            return ok, float(np.sum(0.5 * rho)), f, J.T @ f, J


def pose_graph(poses, edge_a, edge_b, edge_meas, sqrt_info=None, fixed=None, max_iterations=100, cg_max_iterations=MAX_ITERATIONS,
               cg_tolerance=TOLERANCE, loss=None):
    """pose_graph_sparse_ref.pose_graph with the PCG step -> the same dict and cg = [CG iterations per linear solve], at_cap,
    breakdowns"""
    cg, ends = [], dict(cap=0, breakdown=0, converged=0)

    def step_pcg(Js, D, f):
        A = (Js.T @ Js + sp.diags(D * D)).tocsr()
        y, its, end = bp.pcg(A, Js.T @ f, cg_max_iterations, cg_tolerance)
        cg.append(its)
        ends[end] += 1
        step = -y
        return step, ps._model(Js, step, f)

    kept_step, kept_problem = ps._step_normal, ps._Problem
    ps._step_normal = step_pcg
    if loss is not None:
        ps._Problem = type("_Problem", (_LossProblem,), dict(kind=pl.KINDS.get(loss[0], loss[0]), a=float(loss[1])))
    try:
        res = ps.pose_graph(poses, edge_a, edge_b, edge_meas, sqrt_info, fixed, max_iterations, linear_solver="normal")
    finally:
        ps._step_normal, ps._Problem = kept_step, kept_problem
    res.update(cg=cg, at_cap=ends["cap"], breakdowns=ends["breakdown"])
    return res


def solve(sc, **kw):
    kw.setdefault("max_iterations", sc.get("max_iterations", 100))
    return pose_graph(sc["poses"], sc["edge_a"], sc["edge_b"], sc["edge_meas"], sc["sqrt_info"], sc["fixed"], **kw)
