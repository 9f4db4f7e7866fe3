// k_posegraph.hip — pose-graph optimisation: the body of RgbdFeatureFrontend::closeLoop (reference
// rgbd_feature_frontend.cpp:577-580, empty there; the call site is :198-205).
//
// Levenberg-Marquardt over keyframe poses (q, p; camera -> world) of cost = 1/2 sum_e |r_e|^2 with, for the edge e = (a, b)
// and its measurement (q_meas, p_meas) = pose b expressed in a's frame, the error term of Ceres's published pose_graph_3d
// example (pose_graph_3d_error_term.h):
//     p_ab = rot(q_a^-1, p_b - p_a)     q_ab = q_a^-1 (x) q_b     delta = q_meas (x) q_ab^-1
//     r_e  = sqrt_info_e [p_ab - p_meas ; 2 vec(delta)]
// No sign fix is applied on delta: a measurement entered as -q_meas, or a pose as -q, turns vec(delta) round.  Inverses are
// Eigen's inverse() (conjugate / squared norm), products Eigen's quaternion product, as in k_ba.hip.
// The trust-region loop is k_ba.hip's without the landmarks: its control block, decisions, reductions, quaternions and host
// driver are trust_region.hpp's, and this file holds the blocks of the problem.  The SAME / DEVIATES table is in
// include/mslam_hip.h, the walk-through in DESIGN.md 4.17.  PARITY UNPINNED: no Ceres build exists here;
// tests/pose_graph_ref.py restates the algorithm in numpy (jets, two linear solvers).
//
// A free pose has the tangent (delta, dp) of k_ba.hip: Plus = q_delta (x) q and the position.  With R_a^T the matrix of
// v -> rot(q_a^-1, v), v = p_b - p_a, and M the 3 x 3 matrix of u -> vec(A (x) (u, 0) (x) B), A = q_meas (x) q_b^-1, B = q_a
// (delta moves by A (x) (d_a - d_b, 0) (x) B to first order), the unweighted derivatives of [p_ab ; 2 vec(delta)] are
//     pose a: [ 2 R_a^T [v]x   -R_a^T ]        pose b: [  0     R_a^T ]
//             [ 2 M             0     ]                [ -2 M   0     ]
// and the edge's Jacobians are sqrt_info times these.
//
// One trust-region iteration on the context's stream; every launch reads the control block first and returns when the solve
// has ended, so the host enqueues iterations ahead and looks at a mapped word between batches:
//   k_pg_edges      a lane per edge: r_e and the two 6 x 6 tangent Jacobians (skipped after a rejected step: the state has
//                   not moved)
//   k_pg_poses      a wave per free pose: U_k = sum J^T J (21 entries) and g_k = sum J^T r over the pose's incidence list
//                   (edge order, built on the host) by lane stride, then a fixed butterfly; the column scaling at the first pass
//   k_pg_check      one wave: FinalizeIterationAndCheckIfMinimizerCanContinue
//   ba_blocked_solve (chol_solver.hpp): k_bag_clear; k_pg_assemble — a wave per unique sorted pair (i <= j) of free poses: the
//                   diagonal pair writes the scaled U_i with the damping and the scaled gradient into the right-hand-side row,
//                   an off-diagonal pair sums J_i^T J_j over the edges the host listed for it, in that order (a serial loop
//                   of one wave: the slow shape when thousands of duplicate edges join one pair), lane (r, c)
//                   keeping entry (r, c), and writes the scaled block into the lower triangle; the blocked Cholesky, the
//                   back-substitution.  With MSLAM_HIP_PG_SOLVER_SPARSE (mslam_hip_set_pose_graph_solver) pg_sparse_solve
//                   (pg_sparse.hpp) stands here instead: the factor on the block envelope, with k_pg_assemble_env, the same
//                   body (pg_assemble_pair) storing to the permuted envelope position; ci[k] is then the pose's
//                   position in the chosen order (every sum of the other kernels runs over k, none over ci).  Where an
//                   entry goes is SysView's, which solver runs LinearSolve's (both reduced_system.hpp)
//   k_pg_candidate  Plus on every pose
//   k_pg_eval       a lane per edge: the model cost change -(J_s s) . (f + J_s s / 2) and the cost at the candidate, summed per
//                   block by a fixed tree
//   k_pg_control    one wave: sums the block partials in a fixed order, step validity, parameter / function tolerance,
//                   accept or reject, radius
// mslam_hip_set_pose_graph_loss (an extension, NONE by default): with HUBER or CAUCHY k_pg_edges_loss and k_pg_eval_loss stand
// where k_pg_edges and k_pg_eval stand: the stored r_e and Jacobians are multiplied by sqrt(rho'(|r_e|^2)), Ceres's corrector on
// the rows, the cost is 1/2 sum rho, and every other kernel of the list runs unchanged on the corrected blocks.
// k_pg_edge_weights (mslam_hip_pose_graph_edge_weights) reports |r_e|^2 and rho' per edge at given poses.
// mslam_hip_pose_graph_covariance runs k_pg_edges (or _loss) and k_pg_poses under a control block at its start,
// k_pg_assemble_env_undamped (pg_assemble_pair without the damping term, a right-hand side of zeros), the factor of
// k_pg_sparse.hip and the two kernels of k_pg_cov.hip: blocks of (J^T J)^-1 inside the envelope.
// mslam_hip_set_pose_graph_pcg (an extension, off by default, read by mslam_hip_pose_graph alone): the normal equations are kept
// as their non-zero blocks, the diagonal ones and one per pair an edge joins (pg_pairs's list, no order, no envelope), written
// by k_pg_assemble_pairs, the fourth store of pg_assemble_pair, and solved by the block-Jacobi preconditioned conjugate
// gradients of k_pcg.hip, unchanged.  CG's length is the device's to decide, so tr_run_pcg (reduced_system.hpp) drives one
// trust-region iteration at a time instead of tr_run's batches.  Every other kernel is the one DENSE launches.  DESIGN.md 4.30.
// No sum uses an atomic and every sum has one order: two calls on the same input return the same bits.  No kernel waits on
// another workgroup; every device loop is bounded by a count the host validated.  All arithmetic is f64.
#include "reduced_system.hpp"

#include <algorithm>
#include <map>

namespace mslam
{

constexpr int kPgMaxEdges = MSLAM_HIP_POSE_GRAPH_MAX_EDGES;

struct PgArgs
{
    int K, E, n;           // n = 6 x (free poses with an edge): the size of the normal equations
    int n_pairs, n_blocks; // pairs of free poses; blocks of k_pg_eval
    int n_pad, ld;         // the blocked solver's padded size and leading dimension (CholArgs)
    // the problem
    const int32_t *ea, *eb; // [E]
    const double* meas;     // [E] x 7: q then p
    const double* info;     // [E] x 36 row-major, nullptr: identity
    const int32_t *inc_ptr, *inc; // incidences by pose, in edge order: 2 e + (0: the pose is the edge's a, 1: its b)
    const int32_t* ci;            // [K] the pose's block in the normal equations, -1: constant or without an edge
    const int32_t* pairs;         // [n_pairs][2] poses k1 <= k2, sorted
    const int32_t *pair_ptr, *pair_edge; // the edges between k1 and k2, in edge order (none for k1 == k2)
    // state and candidate
    double *pose, *cand;
    // blocks
    double *r, *J;       // [E] x 6; [E] x 72: J_a then J_b, 6 x 6 row-major
    double *U, *gc, *sc; // [K] x 21, 6, 6
    double *S, *yc;      // the padded normal equations (the context's d_ba_S); the solution, n
    // MSLAM_HIP_PG_SOLVER_SPARSE: S is the block envelope; row i's first block and first column, the right-hand side
    const int32_t *env_off, *env_first;
    double* rhs;
    double* part;        // [2][n_blocks]: model cost change, candidate cost
    TrCtrl* ctrl;
    int32_t* h_done; // mapped
    // mslam_hip_set_pose_graph_pcg: S holds the pairs' blocks themselves (SysLayout::Pairs), ci the index order; the block of
    // pair i of `pairs`.  The right-hand side is rhs
    const int32_t* pair_slot;
};

// entry (i, k) of the edge's sqrt_info
__device__ __forceinline__ double pg_info(const double* __restrict__ info, int i, int k)
{
    return info ? info[i * 6 + k] : (i == k ? 1.0 : 0.0);
}

// u = [p_ab - p_meas ; 2 vec(delta)], the unweighted error of edge e at the poses xa, xb
__device__ __forceinline__ void pg_error(const double* __restrict__ xa, const double* __restrict__ xb, const double* __restrict__ z, double u[6])
{
    double qai[4], qab[4], qabi[4], dq[4], pab[3];
    quat_inverse(xa, qai);
    const double v[3] = {xb[4] - xa[4], xb[5] - xa[5], xb[6] - xa[6]};
    quat_rotate(qai, v, pab);
    const double qb[4] = {xb[0], xb[1], xb[2], xb[3]}, qm[4] = {z[0], z[1], z[2], z[3]};
    quat_product(qai, qb, qab);
    quat_inverse(qab, qabi);
    quat_product(qm, qabi, dq);
    u[0] = pab[0] - z[4], u[1] = pab[1] - z[5], u[2] = pab[2] - z[6];
    u[3] = 2.0 * dq[0], u[4] = 2.0 * dq[1], u[5] = 2.0 * dq[2];
}
__device__ __forceinline__ void pg_residual(const double* __restrict__ xa, const double* __restrict__ xb, const double* __restrict__ z,
                                            const double* __restrict__ info, double r[6])
{
    double u[6];
    pg_error(xa, xb, z, u);
#pragma unroll
    for(int i = 0; i < 6; ++i)
    {
        double s = 0.0;
#pragma unroll
        for(int k = 0; k < 6; ++k)
            s += pg_info(info, i, k) * u[k];
        r[i] = s;
    }
}

// s = |r_e|^2 over the six weighted components, in the order of the cost
__device__ __forceinline__ double pg_sq_norm(const double r[6])
{
    return ((r[0] * r[0] + r[1] * r[1]) + (r[2] * r[2] + r[3] * r[3])) + (r[4] * r[4] + r[5] * r[5]);
}

// ---- blocks ------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_pg_edges(PgArgs a)
{
    const TrCtrl* ct = a.ctrl;
    if(ct->done || !ct->need_jac)
        return;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if(e >= a.E)
        return;
    const double* xa = a.pose + (size_t)a.ea[e] * 7;
    const double* xb = a.pose + (size_t)a.eb[e] * 7;
    const double* z = a.meas + (size_t)e * 7;
    const double* info = a.info ? a.info + (size_t)e * 36 : nullptr;
    double r[6];
    pg_residual(xa, xb, z, info, r);
#pragma unroll
    for(int i = 0; i < 6; ++i)
        a.r[(size_t)e * 6 + i] = r[i];
    // P = R_a^T, G = 2 P [v]x, M2 = 2 M
    double qai[4], qbi[4], A[4], P[9], G[9], M2[9];
    quat_inverse(xa, qai);
    quat_inverse(xb, qbi);
    quat_matrix(qai, P);
    const double v[3] = {xb[4] - xa[4], xb[5] - xa[5], xb[6] - xa[6]};
    const double vx[9] = {0.0, -v[2], v[1], v[2], 0.0, -v[0], -v[1], v[0], 0.0};
#pragma unroll
    for(int i = 0; i < 3; ++i)
#pragma unroll
        for(int j = 0; j < 3; ++j)
            G[i * 3 + j] = 2.0 * (P[i * 3] * vx[j] + P[i * 3 + 1] * vx[3 + j] + P[i * 3 + 2] * vx[6 + j]);
    const double qm[4] = {z[0], z[1], z[2], z[3]}, B[4] = {xa[0], xa[1], xa[2], xa[3]};
    quat_product(qm, qbi, A);
#pragma unroll
    for(int j = 0; j < 3; ++j)
    {
        const double ej[4] = {j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0, 0.0};
        double t[4], w[4];
        quat_product(A, ej, t);
        quat_product(t, B, w);
        M2[j] = 2.0 * w[0], M2[3 + j] = 2.0 * w[1], M2[6 + j] = 2.0 * w[2];
    }
    double* Ja = a.J + (size_t)e * 72;
    double* Jb = Ja + 36;
#pragma unroll
    for(int i = 0; i < 6; ++i)
    {
        const double w0 = pg_info(info, i, 0), w1 = pg_info(info, i, 1), w2 = pg_info(info, i, 2);
        const double w3 = pg_info(info, i, 3), w4 = pg_info(info, i, 4), w5 = pg_info(info, i, 5);
#pragma unroll
        for(int j = 0; j < 3; ++j)
        {
            const double wp = w0 * P[j] + w1 * P[3 + j] + w2 * P[6 + j];
            const double wm = w3 * M2[j] + w4 * M2[3 + j] + w5 * M2[6 + j];
            Ja[i * 6 + j] = (w0 * G[j] + w1 * G[3 + j] + w2 * G[6 + j]) + wm;
            Ja[i * 6 + 3 + j] = -wp;
            Jb[i * 6 + j] = -wm;
            Jb[i * 6 + 3 + j] = wp;
        }
    }
}

__global__ __launch_bounds__(64) void k_pg_poses(PgArgs a)
{
    const TrCtrl* ct = a.ctrl;
    if(ct->done || !ct->need_jac)
        return;
    const int k = blockIdx.x, lane = threadIdx.x;
    if(a.ci[k] < 0)
        return;
    double acc[27];
#pragma unroll
    for(int j = 0; j < 27; ++j)
        acc[j] = 0.0;
    for(int pos = a.inc_ptr[k] + lane; pos < a.inc_ptr[k + 1]; pos += 64)
    {
        const int code = a.inc[pos];
        const double* Jp = a.J + (size_t)(code >> 1) * 72 + (code & 1) * 36;
        const double* rp = a.r + (size_t)(code >> 1) * 6;
        double J[36], r[6];
#pragma unroll
        for(int j = 0; j < 36; ++j)
            J[j] = Jp[j];
#pragma unroll
        for(int j = 0; j < 6; ++j)
            r[j] = rp[j];
        int j = 0;
#pragma unroll
        for(int rr = 0; rr < 6; ++rr)
#pragma unroll
            for(int c = rr; c < 6; ++c)
            {
                double s = 0.0;
#pragma unroll
                for(int i = 0; i < 6; ++i)
                    s += J[i * 6 + rr] * J[i * 6 + c];
                acc[j++] += s;
            }
#pragma unroll
        for(int rr = 0; rr < 6; ++rr)
        {
            double s = 0.0;
#pragma unroll
            for(int i = 0; i < 6; ++i)
                s += J[i * 6 + rr] * r[i];
            acc[21 + rr] += s;
        }
    }
#pragma unroll
    for(int j = 0; j < 27; ++j)
        acc[j] = wave_sum(acc[j]);
    if(lane == 0)
    {
#pragma unroll
        for(int j = 0; j < 21; ++j)
            a.U[(size_t)k * 21 + j] = acc[j];
#pragma unroll
        for(int j = 0; j < 6; ++j)
            a.gc[(size_t)k * 6 + j] = acc[21 + j];
        if(ct->first)
        {
            int d = 0;
#pragma unroll
            for(int j = 0; j < 6; ++j)
            {
                a.sc[(size_t)k * 6 + j] = 1.0 / (1.0 + sqrt(acc[d]));
                d += 6 - j;
            }
        }
    }
}

// ---- FinalizeIterationAndCheckIfMinimizerCanContinue: one wave ------------------------------------------------------------

__global__ __launch_bounds__(64) void k_pg_check(PgArgs a)
{
    if(a.ctrl->done)
        return;
    const int lane = threadIdx.x;
    bool ok = true;
    double gmax = 0.0;
    for(int k = lane; k < a.K; k += 64)
        if(a.ci[k] >= 0)
            tr_pose_gradient(a.pose + (size_t)k * 7, a.gc + (size_t)k * 6, a.U + (size_t)k * 21, ok, gmax);
    tr_check(a.ctrl, a.h_done, lane, a.part, a.n_blocks, ok, gmax);
}

// ---- the normal equations: a wave per pair of free poses ------------------------------------------------------------------

// One body for every layout: the pair's lookup, the diagonal with its damping, the sum over the pair's edge list and the
// scaling; SysView (reduced_system.hpp) knows where the entries go.  ci is the block in index order with PaddedLower, the
// position in the chosen order with Envelope, the block in index order again with Pairs (k1 < k2 gives b1 < b2, which SysView's
// Pairs store relies on).  kDamped = false (mslam_hip_pose_graph_covariance): the scaled J^T J itself and a
// right-hand side of zeros.
template <SysLayout kLayout, bool kDamped = true>
__device__ __forceinline__ void pg_assemble_pair(const PgArgs& a)
{
    const TrCtrl* ct = a.ctrl;
    if(ct->done)
        return;
    const int lane = threadIdx.x;
    const int k1 = a.pairs[blockIdx.x * 2], k2 = a.pairs[blockIdx.x * 2 + 1];
    const int b1 = a.ci[k1], b2 = a.ci[k2];
    const SysView<kLayout> sys(a);
    if(k1 == k2)
    {
        if(lane < 36)
        {
            const int r = lane / 6, c = lane % 6;
            const double u = a.sc[(size_t)k1 * 6 + r] * a.U[(size_t)k1 * 21 + (r <= c ? tri6(r, c) : tri6(c, r))] * a.sc[(size_t)k1 * 6 + c];
            if constexpr(kDamped)
                sys.store(b1, b1, true, r, c, r == c ? u + fmin(fmax(u, kTrMinDiagonal), kTrMaxDiagonal) / ct->radius : u);
            else
                sys.store(b1, b1, true, r, c, u);
        }
        else if(lane < 42)
        {
            const int r = lane - 36;
            if constexpr(kDamped)
                sys.store_rhs(b1, r, a.sc[(size_t)k1 * 6 + r] * a.gc[(size_t)k1 * 6 + r]);
            else
                sys.store_rhs(b1, r, 0.0);
        }
        return;
    }
    if(lane >= 36)
        return;
    // entry (r, c) of sum_e J_k1^T J_k2, in the order of the pair's list
    const int r = lane / 6, c = lane % 6;
    double s = 0.0;
    for(int pos = a.pair_ptr[blockIdx.x]; pos < a.pair_ptr[blockIdx.x + 1]; ++pos)
    {
        const int e = a.pair_edge[pos];
        const bool fwd = a.ea[e] == k1;
        const double* J1 = a.J + (size_t)e * 72 + (fwd ? 0 : 36);
        const double* J2 = a.J + (size_t)e * 72 + (fwd ? 36 : 0);
        double t = 0.0;
#pragma unroll
        for(int i = 0; i < 6; ++i)
            t += J1[i * 6 + r] * J2[i * 6 + c];
        s += t;
    }
    sys.store(b1, b2, false, r, c, a.sc[(size_t)k1 * 6 + r] * s * a.sc[(size_t)k2 * 6 + c]);
}

__global__ __launch_bounds__(64) void k_pg_assemble(PgArgs a) { pg_assemble_pair<SysLayout::PaddedLower>(a); }
__global__ __launch_bounds__(64) void k_pg_assemble_env(PgArgs a) { pg_assemble_pair<SysLayout::Envelope>(a); }
__global__ __launch_bounds__(64) void k_pg_assemble_env_undamped(PgArgs a) { pg_assemble_pair<SysLayout::Envelope, false>(a); }
// mslam_hip_set_pose_graph_pcg: the normal equations as their non-zero blocks.  A diagonal wave writes all 36 entries of its
// block and the six of the right-hand side, an off-diagonal wave all 36 of its pair's: nothing is cleared before it.  The
// kernels of k_pcg.hip follow (pcg_solve).  DESIGN.md 4.30.
__global__ __launch_bounds__(64) void k_pg_assemble_pairs(PgArgs a) { pg_assemble_pair<SysLayout::Pairs>(a); }

// delta = step * scaling with step = -y; Plus.  Poses outside the problem are copied.
__global__ __launch_bounds__(256) void k_pg_candidate(PgArgs a)
{
    if(a.ctrl->done)
        return;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if(t >= a.K)
        return;
    const int bk = a.ci[t];
    tr_pose_plus(a.pose + (size_t)t * 7, bk < 0 ? nullptr : a.yc + (size_t)bk * 6, a.sc + (size_t)t * 6, a.cand + (size_t)t * 7);
}

// the step of pose k in its tangent, 0 for a pose outside the problem
__device__ __forceinline__ void pg_step(const PgArgs& a, int k, double s[6])
{
    const int bk = a.ci[k];
#pragma unroll
    for(int j = 0; j < 6; ++j)
        s[j] = 0.0;
    if(bk >= 0)
    {
#pragma unroll
        for(int j = 0; j < 6; ++j)
            s[j] = -a.yc[(size_t)bk * 6 + j] * a.sc[(size_t)k * 6 + j];
    }
}

// at_start: only the cost at the state, for iteration 0
__global__ __launch_bounds__(256) void k_pg_eval(PgArgs a, int at_start)
{
    __shared__ double red[4];
    if(a.ctrl->done)
        return;
    const int e = blockIdx.x * 256 + threadIdx.x;
    double model = 0.0, cost = 0.0;
    if(e < a.E)
    {
        const int ka = a.ea[e], kb = a.eb[e];
        const double* z = a.meas + (size_t)e * 7;
        const double* info = a.info ? a.info + (size_t)e * 36 : nullptr;
        double r[6];
        if(at_start)
            pg_residual(a.pose + (size_t)ka * 7, a.pose + (size_t)kb * 7, z, info, r);
        else
        {
            double sa[6], sb[6];
            pg_step(a, ka, sa);
            pg_step(a, kb, sb);
            const double* Ja = a.J + (size_t)e * 72;
            const double* f = a.r + (size_t)e * 6;
#pragma unroll
            for(int i = 0; i < 6; ++i)
            {
                double js = 0.0;
#pragma unroll
                for(int j = 0; j < 6; ++j)
                    js += Ja[i * 6 + j] * sa[j];
#pragma unroll
                for(int j = 0; j < 6; ++j)
                    js += Ja[36 + i * 6 + j] * sb[j];
                model += js * (f[i] + js / 2.0);
            }
            model = -model;
            pg_residual(a.cand + (size_t)ka * 7, a.cand + (size_t)kb * 7, z, info, r);
        }
        cost = 0.5 * (((r[0] * r[0] + r[1] * r[1]) + (r[2] * r[2] + r[3] * r[3])) + (r[4] * r[4] + r[5] * r[5]));
    }
    const double ms = block_sum(model, red), cs = block_sum(cost, red);
    if(threadIdx.x == 0)
    {
        a.part[blockIdx.x] = ms;
        a.part[a.n_blocks + blockIdx.x] = cs;
    }
}

// ---- the trust-region bookkeeping of one iteration: one wave ----------------------------------------------------------------

__global__ __launch_bounds__(64) void k_pg_control(PgArgs a)
{
    if(a.ctrl->done)
        return;
    const int lane = threadIdx.x;
    bool finite = true;
    double xn = 0.0, sn = 0.0;
    for(int k = lane; k < a.K; k += 64)
        if(a.ci[k] >= 0)
            tr_pose_step(a.pose + (size_t)k * 7, a.cand + (size_t)k * 7, a.yc + (size_t)a.ci[k] * 6, finite, xn, sn);
    if(!tr_control(a.ctrl, a.h_done, lane, a.part, a.n_blocks, finite, xn, sn))
        return;
    for(int k = lane; k < a.K; k += 64)
        if(a.ci[k] >= 0)
            for(int j = 0; j < 7; ++j)
                a.pose[(size_t)k * 7 + j] = a.cand[(size_t)k * 7 + j];
}

// ---- mslam_hip_set_pose_graph_loss: the second forms, launched only with HUBER or CAUCHY -----------------------------------

// Both repeat their NONE twin's text instead of sharing a body with it: k_pg_edges and k_pg_eval read the kernel argument in
// place, and moving their bodies into a function reorders their instructions (k_ba.hip keeps its ba_loss for the same reason:
// the kernels of before the setting keep their machine code).  A change to one of the twins belongs in the other.

// Ceres's corrector as corrector.cc writes it, on the rows: the body of k_pg_edges, then the stored r_e and both stored
// Jacobians times sqrt(w_e), w_e = rho'(|r_e|^2) at the state.  Everything that reads a.r and a.J then runs on the corrected
// blocks.  sqrt(1.0) is 1.0 and a product with 1.0 keeps its bits: an edge of weight 1 stores what k_pg_edges stores
__global__ __launch_bounds__(256) void k_pg_edges_loss(PgArgs a, TrLoss loss)
{
    const TrCtrl* ct = a.ctrl;
    if(ct->done || !ct->need_jac)
        return;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if(e >= a.E)
        return;
    const double* xa = a.pose + (size_t)a.ea[e] * 7;
    const double* xb = a.pose + (size_t)a.eb[e] * 7;
    const double* z = a.meas + (size_t)e * 7;
    const double* info = a.info ? a.info + (size_t)e * 36 : nullptr;
    double r[6];
    pg_residual(xa, xb, z, info, r);
#pragma unroll
    for(int i = 0; i < 6; ++i)
        a.r[(size_t)e * 6 + i] = r[i];
    // P = R_a^T, G = 2 P [v]x, M2 = 2 M
    double qai[4], qbi[4], A[4], P[9], G[9], M2[9];
    quat_inverse(xa, qai);
    quat_inverse(xb, qbi);
    quat_matrix(qai, P);
    const double v[3] = {xb[4] - xa[4], xb[5] - xa[5], xb[6] - xa[6]};
    const double vx[9] = {0.0, -v[2], v[1], v[2], 0.0, -v[0], -v[1], v[0], 0.0};
#pragma unroll
    for(int i = 0; i < 3; ++i)
#pragma unroll
        for(int j = 0; j < 3; ++j)
            G[i * 3 + j] = 2.0 * (P[i * 3] * vx[j] + P[i * 3 + 1] * vx[3 + j] + P[i * 3 + 2] * vx[6 + j]);
    const double qm[4] = {z[0], z[1], z[2], z[3]}, B[4] = {xa[0], xa[1], xa[2], xa[3]};
    quat_product(qm, qbi, A);
#pragma unroll
    for(int j = 0; j < 3; ++j)
    {
        const double ej[4] = {j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0, 0.0};
        double t[4], w[4];
        quat_product(A, ej, t);
        quat_product(t, B, w);
        M2[j] = 2.0 * w[0], M2[3 + j] = 2.0 * w[1], M2[6 + j] = 2.0 * w[2];
    }
    double* Ja = a.J + (size_t)e * 72;
    double* Jb = Ja + 36;
#pragma unroll
    for(int i = 0; i < 6; ++i)
    {
        const double w0 = pg_info(info, i, 0), w1 = pg_info(info, i, 1), w2 = pg_info(info, i, 2);
        const double w3 = pg_info(info, i, 3), w4 = pg_info(info, i, 4), w5 = pg_info(info, i, 5);
#pragma unroll
        for(int j = 0; j < 3; ++j)
        {
            const double wp = w0 * P[j] + w1 * P[3 + j] + w2 * P[6 + j];
            const double wm = w3 * M2[j] + w4 * M2[3 + j] + w5 * M2[6 + j];
            Ja[i * 6 + j] = (w0 * G[j] + w1 * G[3 + j] + w2 * G[6 + j]) + wm;
            Ja[i * 6 + 3 + j] = -wp;
            Jb[i * 6 + j] = -wm;
            Jb[i * 6 + 3 + j] = wp;
        }
    }
    double rho, w;
    tr_loss(loss.kind, loss.scale, pg_sq_norm(r), rho, w);
    const double sw = sqrt(w);
#pragma unroll
    for(int i = 0; i < 6; ++i)
        a.r[(size_t)e * 6 + i] = sw * r[i];
#pragma unroll
    for(int j = 0; j < 72; ++j)
        Ja[j] = sw * Ja[j];
}

// k_pg_eval with cost = 1/2 rho(|r|^2) of the uncorrected residual, at the state (at_start) and at the candidate; the model
// term reads the corrected blocks k_pg_edges_loss stored
__global__ __launch_bounds__(256) void k_pg_eval_loss(PgArgs a, int at_start, TrLoss loss)
{
    __shared__ double red[4];
    if(a.ctrl->done)
        return;
    const int e = blockIdx.x * 256 + threadIdx.x;
    double model = 0.0, cost = 0.0;
    if(e < a.E)
    {
        const int ka = a.ea[e], kb = a.eb[e];
        const double* z = a.meas + (size_t)e * 7;
        const double* info = a.info ? a.info + (size_t)e * 36 : nullptr;
        double r[6];
        if(at_start)
            pg_residual(a.pose + (size_t)ka * 7, a.pose + (size_t)kb * 7, z, info, r);
        else
        {
            double sa[6], sb[6];
            pg_step(a, ka, sa);
            pg_step(a, kb, sb);
            const double* Ja = a.J + (size_t)e * 72;
            const double* f = a.r + (size_t)e * 6;
#pragma unroll
            for(int i = 0; i < 6; ++i)
            {
                double js = 0.0;
#pragma unroll
                for(int j = 0; j < 6; ++j)
                    js += Ja[i * 6 + j] * sa[j];
#pragma unroll
                for(int j = 0; j < 6; ++j)
                    js += Ja[36 + i * 6 + j] * sb[j];
                model += js * (f[i] + js / 2.0);
            }
            model = -model;
            pg_residual(a.cand + (size_t)ka * 7, a.cand + (size_t)kb * 7, z, info, r);
        }
        double rho, w;
        tr_loss(loss.kind, loss.scale, pg_sq_norm(r), rho, w);
        cost = 0.5 * rho;
    }
    const double ms = block_sum(model, red), cs = block_sum(cost, red);
    if(threadIdx.x == 0)
    {
        a.part[blockIdx.x] = ms;
        a.part[a.n_blocks + blockIdx.x] = cs;
    }
}

// mslam_hip_pose_graph_edge_weights: a lane per edge, chi2 = |r_e|^2 at the given poses and weight = rho'(chi2)
struct PgWeightArgs
{
    int E, loss_kind;
    double loss_scale;
    const double* pose;     // [K] x 7
    const int32_t *ea, *eb; // [E]
    const double *meas, *info; // [E] x 7; [E] x 36 or nullptr
    double *chi2, *weight;  // [E] each
};

__global__ __launch_bounds__(256) void k_pg_edge_weights(PgWeightArgs a)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if(e >= a.E)
        return;
    double r[6];
    pg_residual(a.pose + (size_t)a.ea[e] * 7, a.pose + (size_t)a.eb[e] * 7, a.meas + (size_t)e * 7,
                a.info ? a.info + (size_t)e * 36 : nullptr, r);
    const double s = pg_sq_norm(r);
    double rho, w = 1.0;
    if(a.loss_kind != MSLAM_HIP_BA_LOSS_NONE)
        tr_loss(a.loss_kind, a.loss_scale, s, rho, w);
    a.chi2[e] = s;
    a.weight[e] = w;
}

} // namespace mslam

using namespace mslam;

// the argument checks of mslam_hip_pose_graph; k_max: the K cap of the solver in use
static int pg_validate(mslam_hip_ctx* c, int k_max, const double* poses, int K, const int32_t* edge_a, const int32_t* edge_b,
                       const double* edge_meas, const double* sqrt_info, int E, int max_iterations)
{
    if(K < 0 || K > k_max)
        return fail(c, MSLAM_HIP_E_INVALID, "pose_graph: K outside 0.." + std::to_string(k_max));
    if(E < 0 || E > kPgMaxEdges)
        return fail(c, MSLAM_HIP_E_INVALID, "pose_graph: E outside 0.." + std::to_string(kPgMaxEdges));
    if(max_iterations < 0 || (K > 0 && !poses) || (E > 0 && (!edge_a || !edge_b || !edge_meas)))
        return fail(c, MSLAM_HIP_E_INVALID, "pose_graph: bad argument (pointers, max_iterations >= 0)");
    for(int e = 0; e < E; ++e)
    {
        if(edge_a[e] < 0 || edge_a[e] >= K || edge_b[e] < 0 || edge_b[e] >= K)
            return fail(c, MSLAM_HIP_E_INVALID, "pose_graph: edge " + std::to_string(e) + " names a pose out of range");
        if(edge_a[e] == edge_b[e])
            return fail(c, MSLAM_HIP_E_INVALID, "pose_graph: edge " + std::to_string(e) + " joins a pose with itself");
        if(!tr_unit_quaternion(edge_meas + (size_t)e * 7))
            return fail(c, MSLAM_HIP_E_INVALID, "pose_graph: the quaternion of measurement " + std::to_string(e) + " is not unit");
        if(sqrt_info)
            for(int j = 0; j < 36; ++j)
                if(!std::isfinite(sqrt_info[(size_t)e * 36 + j]))
                    return fail(c, MSLAM_HIP_E_INVALID, "pose_graph: sqrt_info of edge " + std::to_string(e) + " is not finite");
    }
    for(int k = 0; k < K; ++k)
        if(!tr_unit_quaternion(poses + (size_t)k * 7))
            return fail(c, MSLAM_HIP_E_INVALID, "pose_graph: the quaternion of pose " + std::to_string(k) + " is not unit");
    return MSLAM_HIP_OK;
}

// the host's view of the edges
struct PgRows
{
    std::vector<int32_t> inc_ptr, inc;               // incidences by pose in edge order
    std::vector<int32_t> ci;                         // [K] the pose's block, -1: constant or without an edge
    std::vector<int32_t> pairs, pair_ptr, pair_edge; // the pairs of free poses, sorted by (k1, k2); every list in edge order
    int n_free = 0;
};

// incidences by pose in edge order (a stable counting sort) and the blocks of the free poses in index order
static void pg_incidences(const uint8_t* fixed, int K, const int32_t* edge_a, const int32_t* edge_b, int E, PgRows& rw)
{
    std::vector<int32_t>&inc_ptr = rw.inc_ptr, &inc = rw.inc;
    inc_ptr.assign((size_t)K + 1, 0), inc.assign((size_t)E * 2, 0);
    for(int e = 0; e < E; ++e)
        ++inc_ptr[(size_t)edge_a[e] + 1], ++inc_ptr[(size_t)edge_b[e] + 1];
    for(int k = 0; k < K; ++k)
        inc_ptr[(size_t)k + 1] += inc_ptr[(size_t)k];
    std::vector<int32_t> at(inc_ptr.begin(), inc_ptr.end() - 1);
    for(int e = 0; e < E; ++e)
        inc[(size_t)at[(size_t)edge_a[e]]++] = 2 * e, inc[(size_t)at[(size_t)edge_b[e]]++] = 2 * e + 1;
    rw.ci.assign((size_t)K, -1);
    rw.n_free = 0;
    for(int k = 0; k < K; ++k)
        if(!(fixed && fixed[k]) && inc_ptr[(size_t)k + 1] > inc_ptr[(size_t)k])
            rw.ci[(size_t)k] = rw.n_free++;
}

// the pairs with their edges; only the sign of ci is read
static void pg_pairs(int K, const int32_t* edge_a, const int32_t* edge_b, int E, PgRows& rw)
{
    const std::vector<int32_t>& ci = rw.ci;
    std::map<std::pair<int, int>, std::vector<int32_t>> by_pair;
    for(int k = 0; k < K; ++k)
        if(ci[(size_t)k] >= 0)
            by_pair[{k, k}];
    for(int e = 0; e < E; ++e)
        if(ci[(size_t)edge_a[e]] >= 0 && ci[(size_t)edge_b[e]] >= 0)
            by_pair[{std::min(edge_a[e], edge_b[e]), std::max(edge_a[e], edge_b[e])}].push_back(e);
    rw.pair_ptr.assign(1, 0);
    for(const auto& kv : by_pair)
    {
        rw.pairs.push_back(kv.first.first), rw.pairs.push_back(kv.first.second);
        rw.pair_edge.insert(rw.pair_edge.end(), kv.second.begin(), kv.second.end());
        rw.pair_ptr.push_back((int32_t)rw.pair_edge.size());
    }
}

extern "C" int mslam_hip_pose_graph(mslam_hip_ctx* c, double* poses, const uint8_t* fixed, int K, const int32_t* edge_a,
                                    const int32_t* edge_b, const double* edge_meas, const double* sqrt_info, int E,
                                    int max_iterations, mslam_hip_ba_summary* summary)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    // mslam_hip_set_pose_graph_pcg stands where the solver's kind stands
    LinearSolve ls(c->pg_solver == MSLAM_HIP_PG_SOLVER_SPARSE, c->pg_pcg != 0, c->pg_pcg_max_iterations, c->pg_pcg_tolerance);
    if(const int rc = pg_validate(c, ls.k_max(), poses, K, edge_a, edge_b, edge_meas, sqrt_info, E, max_iterations); rc != MSLAM_HIP_OK)
        return rc;
    mslam_hip_ba_summary sum{};
    c->pg_pcg_stats = mslam_hip_pcg_stats{};
    if(E == 0)
    {
        // solver.cc Minimize(): no parameter blocks -> CONVERGENCE at cost 0, nothing touched
        if(summary)
            *summary = sum;
        return MSLAM_HIP_OK;
    }
    PgRows rw;
    pg_incidences(fixed, K, edge_a, edge_b, E, rw);
    if(ls.sparse)
        pg_symbolic(fixed, K, edge_a, edge_b, E, ls.sy); // its nodes are the free poses that have an edge: rw.n_free of them
    if(ls.pcg)
    {
        // no order and no envelope: the stored blocks are the pairs themselves
        pg_pairs(K, edge_a, edge_b, E, rw);
        if(const int rc = ls.index_pairs(c, "pose_graph", rw.pairs, rw.ci, rw.n_free); rc != MSLAM_HIP_OK)
            return rc;
    }
    else
    {
        if(const int rc = ls.index(c, "pose_graph", rw.ci, rw.n_free); rc != MSLAM_HIP_OK)
            return rc;
        pg_pairs(K, edge_a, edge_b, E, rw);
    }

    PgArgs a{};
    a.K = K, a.E = E, a.n = ls.n, a.n_pad = ls.n_pad, a.ld = ls.ld;
    a.n_pairs = (int)(rw.pairs.size() / 2), a.n_blocks = (E + 255) / 256;
    // one block: what is uploaded first (the control block at 0), then the working arrays
    TrStaging st(max_iterations);
    const size_t n_info = sqrt_info ? (size_t)E * 288 : 0;
    const size_t o_pose = st.put(poses, (size_t)K * 56), o_meas = st.put(edge_meas, (size_t)E * 56), o_info = st.put(sqrt_info, n_info);
    const size_t o_ea = st.put(edge_a, (size_t)E * 4), o_eb = st.put(edge_b, (size_t)E * 4), o_iptr = st.put(rw.inc_ptr.data(), ((size_t)K + 1) * 4);
    const size_t o_inc = st.put(rw.inc.data(), (size_t)E * 8), o_ci = st.put(rw.ci.data(), (size_t)K * 4);
    const size_t o_pairs = st.put(rw.pairs.data(), rw.pairs.size() * 4), o_pptr = st.put(rw.pair_ptr.data(), rw.pair_ptr.size() * 4);
    const size_t o_pedge = st.put(rw.pair_edge.data(), rw.pair_edge.size() * 4);
    ls.put(st);
    const size_t o_cand = st.carve((size_t)K * 56), o_r = st.carve((size_t)E * 48), o_J = st.carve((size_t)E * 576);
    const size_t o_U = st.carve((size_t)K * 168), o_gc = st.carve((size_t)K * 48), o_sc = st.carve((size_t)K * 48), o_yc = st.carve((size_t)a.n * 8);
    const size_t o_part = st.carve((size_t)a.n_blocks * 16);
    ls.carve(st);
    MSLAM_CHK(c, hipSetDevice(c->p.device));
    MSLAM_CHK(c, grow(c->d_pg, st.size, c->stream));
    MSLAM_CHK(c, ls.grow_S(c));
    if(!c->h_ba)
        MSLAM_CHK(c, c->h_ba.alloc(4));
    uint8_t* d = c->d_pg;
    hipStream_t s = c->stream;
    MSLAM_CHK(c, st.upload(d, s));
    auto dbl = [&](size_t at) { return reinterpret_cast<double*>(d + at); };
    auto i32 = [&](size_t at) { return reinterpret_cast<int32_t*>(d + at); };
    a.ea = i32(o_ea), a.eb = i32(o_eb), a.meas = dbl(o_meas), a.info = sqrt_info ? dbl(o_info) : nullptr;
    a.inc_ptr = i32(o_iptr), a.inc = i32(o_inc), a.ci = i32(o_ci);
    a.pairs = i32(o_pairs), a.pair_ptr = i32(o_pptr), a.pair_edge = i32(o_pedge);
    a.pose = dbl(o_pose), a.cand = dbl(o_cand), a.r = dbl(o_r), a.J = dbl(o_J);
    a.U = dbl(o_U), a.gc = dbl(o_gc), a.sc = dbl(o_sc), a.S = c->d_ba_S.get(), a.yc = dbl(o_yc), a.part = dbl(o_part);
    a.ctrl = reinterpret_cast<TrCtrl*>(d);
    a.h_done = c->h_ba.dev();
    *c->h_ba.get() = 0;
    ls.bind(c, d, a.yc);
    a.env_off = ls.env.row_off, a.env_first = ls.env.first, a.rhs = ls.pcg ? dbl(ls.o_rhs) : ls.env.rhs;
    a.pair_slot = ls.pcg ? i32(ls.o_pslot) : nullptr;
    // NONE: the launches of before the setting existed
    const TrLoss tl{c->pg_loss_kind, c->pg_loss_scale};
    const bool loss = tl.kind != MSLAM_HIP_BA_LOSS_NONE;

    const dim3 g_edge((unsigned)a.n_blocks), g_x((unsigned)((K + 255) / 256)), g_pair((unsigned)a.n_pairs);
    {
        StageScope ts(c, "pg_start_cost");
        if(loss)
            hipLaunchKernelGGL(k_pg_eval_loss, g_edge, dim3(256), 0, s, a, 1, tl);
        else
            hipLaunchKernelGGL(k_pg_eval, g_edge, dim3(256), 0, s, a, 1);
    }
    // one iteration's launches before and after the linear solve
    const auto blocks = [&] {
        StageScope tk(c, "pg_blocks");
        if(loss)
            hipLaunchKernelGGL(k_pg_edges_loss, g_edge, dim3(256), 0, s, a, tl);
        else
            hipLaunchKernelGGL(k_pg_edges, g_edge, dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_pg_poses, dim3((unsigned)K), dim3(64), 0, s, a);
        hipLaunchKernelGGL(k_pg_check, dim3(1), dim3(64), 0, s, a);
    };
    const auto step = [&] {
        StageScope tk(c, "pg_step");
        hipLaunchKernelGGL(k_pg_candidate, g_x, dim3(256), 0, s, a);
        if(loss)
            hipLaunchKernelGGL(k_pg_eval_loss, g_edge, dim3(256), 0, s, a, 0, tl);
        else
            hipLaunchKernelGGL(k_pg_eval, g_edge, dim3(256), 0, s, a, 0);
        hipLaunchKernelGGL(k_pg_control, dim3(1), dim3(64), 0, s, a);
    };
    int rc;
    if(ls.pcg)
    {
        // CG's length is the device's to decide: tr_run_pcg drives one trust-region iteration at a time
        const auto assemble = [&] { hipLaunchKernelGGL(k_pg_assemble_pairs, g_pair, dim3(64), 0, s, a); };
        rc = tr_run_pcg(c, "pg_iterations", "pose_graph", a.ctrl, ls, a.n_pairs > 0, max_iterations, blocks, assemble, step, &c->pg_pcg_stats, sum);
    }
    else
        rc = tr_run(c, "pg_iterations", "pose_graph", a.ctrl, max_iterations, [&] {
            blocks();
            if(a.n_pairs > 0)
                ls.solve(c, s, [&] { hipLaunchKernelGGL(ls.sparse ? k_pg_assemble_env : k_pg_assemble, g_pair, dim3(64), 0, s, a); });
            step();
        }, sum);
    if(rc != MSLAM_HIP_OK)
        return rc;
    const bool usable = sum.termination != kTrFailure;
    std::vector<double> xp((size_t)K * 7);
    if(usable)
    {
        MSLAM_CHK(c, hipMemcpyAsync(xp.data(), a.pose, (size_t)K * 56, hipMemcpyDeviceToHost, s));
        MSLAM_CHK(c, hipStreamSynchronize(s));
    }
    if(summary)
        *summary = sum;
    if(!usable)
        return fail(c, MSLAM_HIP_E_NO_MODEL, "pose_graph: the minimiser ended in FAILURE (non-finite cost or gradient, or 5 invalid "
                                             "steps in a row)");
    std::memcpy(poses, xp.data(), (size_t)K * 56);
    return MSLAM_HIP_OK;
}

extern "C" int mslam_hip_set_pose_graph_solver(mslam_hip_ctx* c, int kind)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    if(kind != MSLAM_HIP_PG_SOLVER_DENSE && kind != MSLAM_HIP_PG_SOLVER_SPARSE)
        return fail(c, MSLAM_HIP_E_INVALID, "set_pose_graph_solver: kind outside 0..1");
    c->pg_solver = kind;
    return MSLAM_HIP_OK;
}

extern "C" int mslam_hip_get_pose_graph_solver(mslam_hip_ctx* c, int* kind)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    if(kind)
        *kind = c->pg_solver;
    return MSLAM_HIP_OK;
}

// PCG for mslam_hip_pose_graph: context state of its own, read when it is called
extern "C" int mslam_hip_set_pose_graph_pcg(mslam_hip_ctx* c, int enable, int max_iterations, double tolerance)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    if(enable < 0 || enable > 1 || max_iterations < 1 || !(tolerance > 0.0 && tolerance < 1.0))
        return fail(c, MSLAM_HIP_E_INVALID, "set_pose_graph_pcg: enable outside 0..1, max_iterations < 1 or a tolerance outside (0, 1)");
    c->pg_pcg = enable, c->pg_pcg_max_iterations = max_iterations, c->pg_pcg_tolerance = tolerance;
    return MSLAM_HIP_OK;
}

extern "C" int mslam_hip_get_pose_graph_pcg(mslam_hip_ctx* c, int* enable, int* max_iterations, double* tolerance)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    if(enable)
        *enable = c->pg_pcg;
    if(max_iterations)
        *max_iterations = c->pg_pcg_max_iterations;
    if(tolerance)
        *tolerance = c->pg_pcg_tolerance;
    return MSLAM_HIP_OK;
}

extern "C" int mslam_hip_get_pose_graph_pcg_stats(mslam_hip_ctx* c, mslam_hip_pcg_stats* stats)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    if(stats)
        *stats = c->pg_pcg_stats;
    return MSLAM_HIP_OK;
}

extern "C" int mslam_hip_set_pose_graph_loss(mslam_hip_ctx* c, int kind, double scale)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    if(kind < MSLAM_HIP_BA_LOSS_NONE || kind > MSLAM_HIP_BA_LOSS_CAUCHY)
        return fail(c, MSLAM_HIP_E_INVALID, "set_pose_graph_loss: kind outside 0..2");
    if(kind != MSLAM_HIP_BA_LOSS_NONE && !(std::isfinite(scale) && scale > 0.0))
        return fail(c, MSLAM_HIP_E_INVALID, "set_pose_graph_loss: the scale of HUBER / CAUCHY must be finite and > 0");
    c->pg_loss_kind = kind;
    c->pg_loss_scale = kind == MSLAM_HIP_BA_LOSS_NONE ? 0.0 : scale;
    return MSLAM_HIP_OK;
}

extern "C" int mslam_hip_get_pose_graph_loss(mslam_hip_ctx* c, int* kind, double* scale)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    if(kind)
        *kind = c->pg_loss_kind;
    if(scale)
        *scale = c->pg_loss_scale;
    return MSLAM_HIP_OK;
}

extern "C" int mslam_hip_pose_graph_edge_weights(mslam_hip_ctx* c, const double* poses, int K, const int32_t* edge_a,
                                                 const int32_t* edge_b, const double* edge_meas, const double* sqrt_info, int E,
                                                 double* chi2, double* weight)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    // no linear system is formed: the cap on K is the SPARSE solver's, whichever solver is set
    if(const int rc = pg_validate(c, MSLAM_HIP_POSE_GRAPH_MAX_KEYFRAMES_SPARSE, poses, K, edge_a, edge_b, edge_meas, sqrt_info, E, 0);
       rc != MSLAM_HIP_OK)
        return rc;
    if(E == 0)
        return MSLAM_HIP_OK;
    // one block: the problem, then chi2 and weight side by side, so the call is one upload, one launch and one download
    TrStaging st(0);
    const size_t o_pose = st.put(poses, (size_t)K * 56), o_meas = st.put(edge_meas, (size_t)E * 56);
    const size_t o_info = st.put(sqrt_info, sqrt_info ? (size_t)E * 288 : 0);
    const size_t o_ea = st.put(edge_a, (size_t)E * 4), o_eb = st.put(edge_b, (size_t)E * 4);
    const size_t o_out = st.carve((size_t)E * 16);
    MSLAM_CHK(c, hipSetDevice(c->p.device));
    MSLAM_CHK(c, grow(c->d_pg, st.size, c->stream));
    uint8_t* d = c->d_pg;
    hipStream_t s = c->stream;
    MSLAM_CHK(c, st.upload(d, s));
    PgWeightArgs a{};
    a.E = E, a.loss_kind = c->pg_loss_kind, a.loss_scale = c->pg_loss_scale;
    a.pose = reinterpret_cast<const double*>(d + o_pose), a.meas = reinterpret_cast<const double*>(d + o_meas);
    a.info = sqrt_info ? reinterpret_cast<const double*>(d + o_info) : nullptr;
    a.ea = reinterpret_cast<const int32_t*>(d + o_ea), a.eb = reinterpret_cast<const int32_t*>(d + o_eb);
    a.chi2 = reinterpret_cast<double*>(d + o_out), a.weight = a.chi2 + E;
    {
        StageScope ts(c, "pg_edge_weights");
        hipLaunchKernelGGL(k_pg_edge_weights, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s, a);
    }
    MSLAM_CHK(c, hipGetLastError());
    std::vector<double> out((size_t)E * 2);
    MSLAM_CHK(c, hipMemcpyAsync(out.data(), a.chi2, (size_t)E * 16, hipMemcpyDeviceToHost, s));
    MSLAM_CHK(c, hipStreamSynchronize(s));
    if(chi2)
        std::memcpy(chi2, out.data(), (size_t)E * 8);
    if(weight)
        std::memcpy(weight, out.data() + E, (size_t)E * 8);
    return MSLAM_HIP_OK;
}

// ---- mslam_hip_pose_graph_covariance ---------------------------------------------------------------------------------------

// The structural rank test: a connected component of the node graph (the free poses that have an edge, joined by the edges
// between them) none of whose members has an edge to a constant pose has a free gauge.  -> the least pose of such a
// component, or -1.
static int pg_free_gauge(const std::vector<int32_t>& ci, const int32_t* edge_a, const int32_t* edge_b, int E)
{
    const int K = (int)ci.size();
    std::vector<int32_t> root((size_t)K);
    for(int k = 0; k < K; ++k)
        root[(size_t)k] = k;
    auto find = [&](int k) {
        while(root[(size_t)k] != k)
            k = root[(size_t)k] = root[(size_t)root[(size_t)k]];
        return k;
    };
    for(int e = 0; e < E; ++e)
        if(ci[(size_t)edge_a[e]] >= 0 && ci[(size_t)edge_b[e]] >= 0)
        {
            const int ra = find(edge_a[e]), rb = find(edge_b[e]);
            root[(size_t)std::max(ra, rb)] = std::min(ra, rb); // the root is the component's least pose
        }
    std::vector<uint8_t> held((size_t)K, 0);
    for(int e = 0; e < E; ++e)
    {
        const bool fa = ci[(size_t)edge_a[e]] >= 0, fb = ci[(size_t)edge_b[e]] >= 0;
        if(fa != fb) // a pose of an edge has an edge: the other end is constant
            held[(size_t)find(fa ? edge_a[e] : edge_b[e])] = 1;
    }
    for(int k = 0; k < K; ++k)
        if(ci[(size_t)k] >= 0 && find(k) == k && !held[(size_t)k])
            return k;
    return -1;
}

extern "C" int mslam_hip_pose_graph_covariance(mslam_hip_ctx* c, const double* poses, const uint8_t* fixed, int K, const int32_t* edge_a,
                                               const int32_t* edge_b, const double* edge_meas, const double* sqrt_info, int E,
                                               const int32_t* pose_idx, int P, double* cov, const int32_t* pair_a,
                                               const int32_t* pair_b, int Q, double* cross)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    LinearSolve ls(true); // the envelope at every K; mslam_hip_set_pose_graph_solver is not read
    if(const int rc = pg_validate(c, ls.k_max(), poses, K, edge_a, edge_b, edge_meas, sqrt_info, E, 0); rc != MSLAM_HIP_OK)
        return rc;
    constexpr int kMaxBlocks = 65536;
    if(P < 0 || P > kMaxBlocks || Q < 0 || Q > kMaxBlocks || (P > 0 && (!pose_idx || !cov)) || (Q > 0 && (!pair_a || !pair_b || !cross)))
        return fail(c, MSLAM_HIP_E_INVALID, "pose_graph_covariance: bad argument (P and Q in 0..65536, pointers)");
    PgRows rw;
    pg_incidences(fixed, K, edge_a, edge_b, E, rw);
    // the requests: a constant pose gives zeros, a free pose must be in the problem
    auto constant = [&](int k) { return fixed && fixed[k]; };
    auto in_problem = [&](int k, const char* what, int at) {
        if(k < 0 || k >= K)
            return fail(c, MSLAM_HIP_E_INVALID, std::string("pose_graph_covariance: ") + what + " " + std::to_string(at) + " names a pose out of range");
        if(!constant(k) && rw.ci[(size_t)k] < 0)
            return fail(c, MSLAM_HIP_E_INVALID, std::string("pose_graph_covariance: ") + what + " " + std::to_string(at) + " names pose " +
                                                    std::to_string(k) + ", which is free and has no edge");
        return (int)MSLAM_HIP_OK;
    };
    for(int p = 0; p < P; ++p)
        if(const int rc = in_problem(pose_idx[p], "pose_idx", p); rc != MSLAM_HIP_OK)
            return rc;
    pg_pairs(K, edge_a, edge_b, E, rw);
    for(int q = 0; q < Q; ++q)
    {
        if(const int rc = in_problem(pair_a[q], "pair_a", q); rc != MSLAM_HIP_OK)
            return rc;
        if(const int rc = in_problem(pair_b[q], "pair_b", q); rc != MSLAM_HIP_OK)
            return rc;
        if(pair_a[q] == pair_b[q])
            return fail(c, MSLAM_HIP_E_INVALID, "pose_graph_covariance: pair " + std::to_string(q) + " names one pose twice (its block is cov's)");
        if(constant(pair_a[q]) || constant(pair_b[q]))
            continue;
        // rw.pairs is sorted by (k1, k2): is the pair among the pairs an edge joins?
        const int32_t lo = std::min(pair_a[q], pair_b[q]), hi = std::max(pair_a[q], pair_b[q]);
        size_t l = 0, r = rw.pairs.size() / 2;
        while(l < r)
        {
            const size_t mid = (l + r) / 2;
            if(std::make_pair(rw.pairs[mid * 2], rw.pairs[mid * 2 + 1]) < std::make_pair(lo, hi))
                l = mid + 1;
            else
                r = mid;
        }
        if(l == rw.pairs.size() / 2 || rw.pairs[l * 2] != lo || rw.pairs[l * 2 + 1] != hi)
            return fail(c, MSLAM_HIP_E_INVALID, "pose_graph_covariance: no edge joins the poses of pair " + std::to_string(q) +
                                                    ": the block may lie outside the envelope");
    }
    if(const int k = pg_free_gauge(rw.ci, edge_a, edge_b, E); k >= 0)
        return fail(c, MSLAM_HIP_E_NO_MODEL, "pose_graph_covariance: the component of pose " + std::to_string(k) +
                                                 " has no edge to a constant pose: its gauge is free and J^T J is singular");
    const int n_req = P + Q;
    if(rw.n_free == 0)
    {
        // every pose of the problem is constant: zeros
        if(P > 0)
            std::memset(cov, 0, (size_t)P * 288);
        if(Q > 0)
            std::memset(cross, 0, (size_t)Q * 288);
        return MSLAM_HIP_OK;
    }
    pg_symbolic(fixed, K, edge_a, edge_b, E, ls.sy);
    if(const int rc = ls.index(c, "pose_graph_covariance", rw.ci, rw.n_free); rc != MSLAM_HIP_OK)
        return rc;
    int longest = 0; // the longest column list: the rows of k_pgs_selinv's scratch
    for(int j = 0; j < ls.n_free; ++j)
        longest = std::max(longest, ls.sy.col_ptr[(size_t)j + 1] - ls.sy.col_ptr[(size_t)j]);
    std::vector<int32_t> req((size_t)n_req * 2);
    for(int p = 0; p < P; ++p)
        req[(size_t)p * 2] = req[(size_t)p * 2 + 1] = pose_idx[p];
    for(int q = 0; q < Q; ++q)
        req[(size_t)(P + q) * 2] = pair_a[q], req[(size_t)(P + q) * 2 + 1] = pair_b[q];

    PgArgs a{};
    a.K = K, a.E = E, a.n = ls.n, a.n_pad = ls.n_pad, a.ld = ls.ld;
    a.n_pairs = (int)(rw.pairs.size() / 2), a.n_blocks = (E + 255) / 256;
    // mslam_hip_pose_graph's block: the control block of a solve at its start (done = 0, need_jac, first), so k_pg_edges and
    // k_pg_poses run as in the first iteration and take the Jacobi scaling at the given poses
    TrStaging st(0);
    const size_t n_info = sqrt_info ? (size_t)E * 288 : 0;
    const size_t o_pose = st.put(poses, (size_t)K * 56), o_meas = st.put(edge_meas, (size_t)E * 56), o_info = st.put(sqrt_info, n_info);
    const size_t o_ea = st.put(edge_a, (size_t)E * 4), o_eb = st.put(edge_b, (size_t)E * 4), o_iptr = st.put(rw.inc_ptr.data(), ((size_t)K + 1) * 4);
    const size_t o_inc = st.put(rw.inc.data(), (size_t)E * 8), o_ci = st.put(rw.ci.data(), (size_t)K * 4);
    const size_t o_pairs = st.put(rw.pairs.data(), rw.pairs.size() * 4), o_pptr = st.put(rw.pair_ptr.data(), rw.pair_ptr.size() * 4);
    const size_t o_pedge = st.put(rw.pair_edge.data(), rw.pair_edge.size() * 4), o_req = st.put(req.data(), req.size() * 4);
    ls.put(st);
    const size_t o_r = st.carve((size_t)E * 48), o_J = st.carve((size_t)E * 576);
    const size_t o_U = st.carve((size_t)K * 168), o_gc = st.carve((size_t)K * 48), o_sc = st.carve((size_t)K * 48), o_yc = st.carve((size_t)a.n * 8);
    const size_t o_scratch = st.carve((size_t)longest * 288), o_out = st.carve((size_t)n_req * 288 + 8);
    ls.carve(st);
    MSLAM_CHK(c, hipSetDevice(c->p.device));
    MSLAM_CHK(c, grow(c->d_pg, st.size, c->stream));
    MSLAM_CHK(c, ls.grow_S(c));
    uint8_t* d = c->d_pg;
    hipStream_t s = c->stream;
    MSLAM_CHK(c, st.upload(d, s));
    auto dbl = [&](size_t at) { return reinterpret_cast<double*>(d + at); };
    auto i32 = [&](size_t at) { return reinterpret_cast<int32_t*>(d + at); };
    a.ea = i32(o_ea), a.eb = i32(o_eb), a.meas = dbl(o_meas), a.info = sqrt_info ? dbl(o_info) : nullptr;
    a.inc_ptr = i32(o_iptr), a.inc = i32(o_inc), a.ci = i32(o_ci);
    a.pairs = i32(o_pairs), a.pair_ptr = i32(o_pptr), a.pair_edge = i32(o_pedge);
    a.pose = dbl(o_pose), a.r = dbl(o_r), a.J = dbl(o_J);
    a.U = dbl(o_U), a.gc = dbl(o_gc), a.sc = dbl(o_sc), a.S = c->d_ba_S.get(), a.yc = dbl(o_yc);
    a.ctrl = reinterpret_cast<TrCtrl*>(d);
    ls.bind(c, d, a.yc);
    a.env_off = ls.env.row_off, a.env_first = ls.env.first, a.rhs = ls.env.rhs;
    const TrLoss tl{c->pg_loss_kind, c->pg_loss_scale};
    const dim3 g_edge((unsigned)a.n_blocks), g_pair((unsigned)a.n_pairs);
    {
        StageScope tk(c, "cov_blocks");
        if(tl.kind != MSLAM_HIP_BA_LOSS_NONE)
            hipLaunchKernelGGL(k_pg_edges_loss, g_edge, dim3(256), 0, s, a, tl);
        else
            hipLaunchKernelGGL(k_pg_edges, g_edge, dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_pg_poses, dim3((unsigned)K), dim3(64), 0, s, a);
    }
    pg_sparse_factor(c, ls.env, s, [&] { hipLaunchKernelGGL(k_pg_assemble_env_undamped, g_pair, dim3(64), 0, s, a); });
    PgCovArgs g{};
    g.n = a.n, g.n_pad = a.n_pad, g.ld = a.ld, g.S = a.S, g.rhs = a.rhs, g.env_off = a.env_off, g.env_first = a.env_first;
    g.ci = a.ci, g.sc = a.sc, g.req = i32(o_req), g.n_req = n_req, g.out = dbl(o_out), g.ctrl = a.ctrl;
    pg_cov_enqueue(c, ls.env, g, dbl(o_scratch), s);
    MSLAM_CHK(c, hipGetLastError());
    // one download: the blocks, then the factor's verdict
    std::vector<double> out((size_t)n_req * 36 + 1);
    MSLAM_CHK(c, hipMemcpyAsync(out.data(), g.out, out.size() * 8, hipMemcpyDeviceToHost, s));
    MSLAM_CHK(c, hipStreamSynchronize(s));
    if(out.back() != 0.0)
        return fail(c, MSLAM_HIP_E_NO_MODEL, "pose_graph_covariance: a pivot of the factor of J^T J is not > 0 or not finite: the "
                                             "problem is rank deficient at these poses");
    if(P > 0)
        std::memcpy(cov, out.data(), (size_t)P * 288);
    if(Q > 0)
        std::memcpy(cross, out.data() + (size_t)P * 36, (size_t)Q * 288);
    return MSLAM_HIP_OK;
}
