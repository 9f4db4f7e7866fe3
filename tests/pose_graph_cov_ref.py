"""CPU references for mslam_hip_pose_graph_covariance (modular-slam_amd/csrc/k_pg_cov.hip), for the tests.

Sigma = (J^T J)^-1 over the free poses that have an edge, J the tangent Jacobian of tests/pose_graph_ref.py's _Problem (jets
times PlusJacobian; under a loss pose_graph_loss_ref.LossProblem's corrected rows).  Nothing here is shared with the HIP
kernels:

  * dense_pair(): two independent dense inverses, R^-1 R^-T from a QR of J (never forms J^T J) and L^-T L^-1 from a Cholesky
    of J^T J, and d = max|Sigma_chol - Sigma_qr| / max|Sigma_qr|.  The GPU tests take their bound from d (bound());
  * selected_inverse(): the Takahashi / Erisman-Tinney recursion restated on the block envelope that
    pose_graph_sparse_ref.analyze returns: a block Cholesky on the envelope, then the backward sweep.  It reaches 16384 poses;
  * splu_columns(): scipy.sparse.linalg.splu solves of unit vectors for the requested poses, where a dense inverse is out of
    reach.

The tangent of a pose is (delta, dp) with Plus(q, delta) = (sin|delta| delta / |delta|, cos|delta|) (x) q: delta is half a
rotation vector (tests/test_pose_graph_cov.py checks that against pose_graph_sparse_ref._quaternion_plus).

PARITY UNPINNED: no Ceres build exists here.  This is test infrastructure (not a conftest.py, not under oracle/)."""
import numpy as np
import scipy.linalg as sl
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import pose_graph_loss_ref as pl
import pose_graph_ref as pg
import pose_graph_sparse_ref as ps

FLOOR, FACTOR, MAX_D = 1e-9, 1000.0, 1e-6    # the rule: max(FLOOR, FACTOR d) max|Sigma_qr|; a case with d > MAX_D tests nothing


def problem(sc, loss=None, sparse=False):
    """the scene's problem: pose_graph_ref._Problem, LossProblem under loss = (kind, a), or the sparse twin"""
    poses, ea, eb, meas, info = pg._arrays(sc["poses"], sc["edge_a"], sc["edge_b"], sc["edge_meas"], sc["sqrt_info"])
    fixed = np.asarray(sc["fixed"]).astype(bool)
    if sparse:
        assert loss is None
        return ps._Problem(len(poses), ea, eb, meas, info, fixed)
    kind, a = pl._how(loss)
    return pl.LossProblem(len(poses), ea, eb, meas, info, fixed, kind, a)


def jacobian(prob, poses):
    ok, _, _, _, J = prob.evaluate(np.asarray(poses, np.float64).reshape(-1, 7))
    assert ok
    return J


def dense_pair(J):
    """-> (Sigma_qr, Sigma_chol, d)"""
    R = np.linalg.qr(J, mode="r")
    Ri = sl.solve_triangular(R, np.eye(R.shape[1]), lower=False)
    s_qr = Ri @ Ri.T
    L = np.linalg.cholesky(J.T @ J)
    Li = sl.solve_triangular(L, np.eye(len(L)), lower=True)
    s_ch = Li.T @ Li
    return s_qr, s_ch, float(np.max(np.abs(s_ch - s_qr)) / np.max(np.abs(s_qr)))


def bound(d, sigma_max):
    return max(FLOOR, FACTOR * d) * sigma_max


def block(sigma, prob, a, b):
    """the 6 x 6 block (a, b) of a dense Sigma over prob.free; zeros when either pose is constant"""
    ca, cb = prob.col[a], prob.col[b]
    if ca < 0 or cb < 0:
        return np.zeros((6, 6))
    return sigma[ca:ca + 6, cb:cb + 6]


def requests(sc):
    """what the tests ask of a scene: every free pose that has an edge, and for every edge between two of them the pair in
    both orientations -> (poses_of [P], pairs [Q, 2])"""
    fixed = np.asarray(sc["fixed"]).astype(bool)
    ea, eb = np.asarray(sc["edge_a"], np.int64), np.asarray(sc["edge_b"], np.int64)
    seen = np.zeros(len(fixed), bool)
    seen[ea], seen[eb] = True, True
    free = seen & ~fixed
    pairs = [p for a, b in zip(ea, eb) if free[a] and free[b] for p in ((a, b), (b, a))]
    return np.flatnonzero(free).astype(np.int32), np.array(pairs, np.int32).reshape(-1, 2)


def expected(sigma, prob, poses_of, pairs):
    cov = np.array([block(sigma, prob, k, k) for k in poses_of]).reshape(-1, 6, 6)
    cross = np.array([block(sigma, prob, a, b) for a, b in pairs]).reshape(-1, 6, 6)
    return cov, cross


# ---- the recursion, restated on analyze()'s envelope -------------------------------------------------------------------------
def _blocks_of(A, prob, an):
    """the 6 x 6 blocks of A (dense or sparse, over prob.free in index order) at the positions of the order: {(row, col)}, the
    lower triangle, zero blocks of the envelope included"""
    B = sp.bsr_matrix(sp.csr_matrix(A), blocksize=(6, 6))
    pos_of_free = np.empty(len(prob.free), np.int64)
    pos_of_free[prob.col[an["order"]] // 6] = np.arange(len(an["order"]))
    out = {}
    for i, f in enumerate(an["first"]):
        for j in range(int(f), i + 1):
            out[(i, j)] = np.zeros((6, 6))
    for br in range(B.shape[0] // 6):
        for at in range(B.indptr[br], B.indptr[br + 1]):
            i, j = pos_of_free[br], pos_of_free[B.indices[at]]
            if i >= j:
                assert (i, j) in out, "a block of A outside the envelope"
                out[(i, j)] = B.data[at].copy()
    return out


def selected_inverse(A, prob, an):
    """-> {(row, col): block} of A^-1 for every block of the envelope, positions in an["order"]"""
    n = len(an["order"])
    S = _blocks_of(A, prob, an)
    rows = [[] for _ in range(n)]     # column j's rows below the diagonal, ascending
    for i, f in enumerate(an["first"]):
        for j in range(int(f), i):
            rows[j].append(i)
    for j in range(n):                # the factor: L over S
        Ljj = np.linalg.cholesky(S[(j, j)])
        S[(j, j)] = Ljj
        for i in rows[j]:
            S[(i, j)] = sl.solve_triangular(Ljj, S[(i, j)].T, lower=True).T
        for x, i in enumerate(rows[j]):
            for k in rows[j][:x + 1]:
                S[(i, k)] = S[(i, k)] - S[(i, j)] @ S[(k, j)].T
    for i in range(n - 1, -1, -1):    # the sweep: Z over L
        W = sl.solve_triangular(S[(i, i)], np.eye(6), lower=True)
        G = {k: S[(k, i)] @ W for k in rows[i]}
        col = {j: -sum((S[(j, k)] if j >= k else S[(k, j)].T) @ G[k] for k in rows[i]) for j in rows[i]}
        Zii = W.T @ W - sum((G[k].T @ col[k] for k in rows[i]), np.zeros((6, 6)))
        S[(i, i)] = np.tril(Zii) + np.tril(Zii, -1).T
        for j in rows[i]:
            S[(j, i)] = col[j]
    return S


def envelope_block(Z, an, prob, a, b):
    """block (a, b) by pose index out of selected_inverse's result; zeros for a constant pose"""
    if prob.col[a] < 0 or prob.col[b] < 0:
        return np.zeros((6, 6))
    pos = {int(k): i for i, k in enumerate(an["order"])}
    i, j = pos[int(a)], pos[int(b)]
    return Z[(i, j)] if i >= j else Z[(j, i)].T


def splu_columns(J, prob, poses):
    """{pose: the six columns of (J^T J)^-1 that belong to it, [n, 6]} by a sparse LU of J^T J (J sparse)"""
    lu = spl.splu((J.T @ J).tocsc())
    out = {}
    for k in poses:
        E = np.zeros((prob.n, 6))
        E[prob.col[k] + np.arange(6), np.arange(6)] = 1.0
        out[int(k)] = lu.solve(E)
    return out
