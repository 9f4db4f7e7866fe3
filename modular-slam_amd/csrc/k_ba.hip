// k_ba.hip — bundle adjustment: the solve of CeresBackend::bundleAdjustment (reference ceres_backend.cpp:185-240).
//
// Levenberg-Marquardt over keyframe poses (q, p) and landmarks X of cost = 1/2 sum_m |r_m|^2 with
//     r_m = rot(q^-1, X) - rot(q^-1, p) - obs_cam[m]                                  (ReprojectionError::operator(), :31-47)
// The trust-region loop is Ceres 2.2's, with the Solver::Options defaults: function tolerance 1e-6, gradient tolerance 1e-10,
// parameter tolerance 1e-8, initial radius 1e4, monotonic steps, Jacobi scaling.  Its control block, decisions, reductions,
// quaternions and host driver are trust_region.hpp's, shared with k_posegraph.hip; this file holds the blocks of the problem.
// The SAME / DEVIATES table is in include/mslam_hip.h, the walk-through in DESIGN.md 4.14.  PARITY UNPINNED: no Ceres
// build exists here; tests/ba_ref.py restates the same algorithm in numpy with two linear solvers.
//
// A free pose has the tangent (delta, dp): EigenQuaternionManifold's Plus q_delta (x) q and the position.  With R^T the matrix
// of v -> rot(q^-1, v) and d = X - p the derivatives are dr/dX = R^T, dr/dp = -R^T, dr/d(delta) = 2 R^T [d]x.
//
// One trust-region iteration is nine launches on the context's stream; every one reads the control block first and returns
// when the solve has ended, so the host may enqueue iterations ahead and look at a mapped word between batches:
//   k_ba_landmarks  a lane per landmark walks the landmark's row in order: V_l = sum J_l^T J_l, g_l = sum J_l^T r; the
//                   column scaling at the first pass; then (S V_l S + D^2)^-1 for this iteration's radius
//   k_ba_cameras    a workgroup per free keyframe walks the keyframe's row by lane stride: U_k (21 entries), g_k, by a
//                   fixed butterfly and a fixed sum over the four waves; W = J_c^T J_l (6 x 3) stored per observation
//   k_ba_check      one wave: FinalizeIterationAndCheckIfMinimizerCanContinue (iteration cap, gradient, radius)
//   k_ba_schur      a wave per pair k1 <= k2 of free keyframes joins the two rows (both sorted by landmark):
//                   S_k1k2 = delta U_k1 - sum_l W_k1l V_l^-1 W_k2l^T and, on the diagonal, the reduced right-hand side
//   k_ba_solve      one workgroup: Cholesky of the reduced system (at most 384 x 384, in global memory), both substitutions
//   k_ba_backsub    a lane per landmark: y_l = V_l^-1 (g_l - sum W^T y_c), in row order
//   k_ba_candidate  Plus on every pose and landmark
//   k_ba_eval       a lane per observation: the model cost change term -(J_s s) . (f + J_s s / 2) at x and the cost at the
//                   candidate, summed per block by a fixed tree
//   k_ba_control    one wave: sums the block partials in a fixed order, step validity, parameter / function tolerance,
//                   accept or reject, radius
// Jacobians are kept unscaled (U, V, W, g) and scaled where they are used, as k_pnp_mse.hip does; after a rejected step the
// state has not moved, so the block kernels reuse what they stored and only the damping is redone.
// No sum uses an atomic and every sum has one order: two calls on the same input return the same bits.  No kernel waits on
// another workgroup; every device loop is bounded by a count the host validated.  All arithmetic is f64.
//
// mslam_hip_set_ba_loss (an extension: the reference passes lossFunction = nullptr): with HUBER or CAUCHY the cost is
// 1/2 sum_m rho(|r_m|^2) and observation m carries the weight w_m = rho'(|r_m|^2) at the state (ba_loss below; Ceres's
// corrector in its simple branch, since rho'' <= 0 for both).  k_ba_landmarks, k_ba_cameras and k_ba_eval have a second
// instantiation that applies w_m to every product of observation m (V, g_l, U, g_c, W, the model term) and rho to the costs;
// each recomputes w_m from ba_residual, so all three use the same bits.  Everything else reads only what these store.
// With NONE the instantiations of before are launched.  DESIGN.md 4.22.
//
// mslam_hip_set_ba_global_solver (an extension, read by mslam_hip_bundle_adjust_global alone): with SPARSE the reduced camera
// system lives on its block envelope (pg_sparse.hpp).  The host lists the covisible pairs without a K x K table, orders the
// covisibility graph of the free observed keyframes (pg_symbolic with a node mask: a keyframe without a partner is a row of
// degree 0) and makes ci the position in that order; k_bag_schur_env, the third form of ba_schur_pair, writes every pair's
// block into its envelope slot, and k_pgs_clear / k_pgs_factor / k_pgs_backsolve of k_pg_sparse.hip stand where the blocked
// solver stands.  Every other kernel is the one DENSE launches.  With DENSE the launches of before.  DESIGN.md 4.26.
//
// mslam_hip_set_ba_global_pcg (an extension, read by mslam_hip_bundle_adjust_global alone): the reduced camera system is kept as
// its non-zero blocks, the diagonal ones and one per covisible pair (ba_symbolic's list, no order, no envelope), written by
// k_bag_schur_pairs, the fourth form of ba_schur_pair, and solved by the block-Jacobi preconditioned conjugate gradients of
// k_pcg.hip.  CG's length is the device's to decide, so tr_run_pcg (reduced_system.hpp) drives one trust-region iteration at a
// time instead of tr_run's batches.  Every other kernel is the one DENSE launches.  Off: the launches of before.  DESIGN.md 4.29.
//
// ba_schur_pair has one form per layout of the reduced system (SysLayout of reduced_system.hpp: Full for k_ba_schur,
// PaddedLower for k_bag_schur, Envelope for k_bag_schur_env, Pairs for k_bag_schur_pairs) and stores through SysView; on the
// host ba_run decides one BaMode (local, global dense, global sparse, global PCG) and runs in parts: ba_validate, ba_rows, a
// pair lister (ba_pairs_all, ba_pairs_table, ba_symbolic), ba_stage, the iteration, ba_read_back.  The global modes take cap, block index, envelope staging, sizes and
// the solve from LinearSolve (reduced_system.hpp), which mslam_hip_pose_graph uses too.
#include "reduced_system.hpp"

#include <algorithm>

namespace mslam
{

constexpr int kBaMaxKeyframes = 64;
constexpr int kBaSolveThreads = 6 * kBaMaxKeyframes; // one thread per row of the reduced system

struct BaArgs
{
    int K, L, M, n;     // n = 6 x (free keyframes with observations): the reduced system's size
    int n_pairs, n_blocks; // pairs of free keyframes; blocks of k_ba_eval
    int n_pad, ld;         // the blocked solver's padded size and leading dimension (CholArgs)
    // the problem
    const int32_t *obs_kf, *obs_lm;
    const double* obs_cam;
    const int32_t *lm_ptr, *lm_obs;         // observations by landmark (rows in input order)
    const int32_t *kf_ptr, *kf_obs, *kf_lm; // observations by keyframe, every row sorted by landmark; kf_lm = the landmark
    const int32_t* ci;                      // [K] the keyframe's block in the reduced system, -1: constant or unobserved
    const int32_t* pairs;                   // [n_pairs][2] keyframes k1, k2 with ci[k1] <= ci[k2]
    const uint8_t* lm_active;               // [L] the landmark has an observation
    // state and candidate
    double *pose, *lm, *cand_pose, *cand_lm;
    // blocks
    double *V, *gl, *Vinv, *sl; // [L] x 6, 3, 6, 3
    double *U, *gc, *sc, *W;    // [K] x 21, 6, 6; [M] x 18
    double *S, *rhs, *yc, *yl;  // n x n column-major, n, n, [L] x 3
    double* part;               // [2][n_blocks]: model cost change, candidate cost
    TrCtrl* ctrl;
    int32_t* h_done; // mapped
    // mslam_hip_set_ba_loss: MSLAM_HIP_BA_LOSS_*, and a (metres) of HUBER / CAUCHY
    int loss_kind;
    double loss_scale;
    // MSLAM_HIP_BA_GLOBAL_SOLVER_SPARSE: S is the block envelope (pg_sparse.hpp), ci the position in the chosen order; row i's
    // first block and first column.  The right-hand side is rhs
    const int32_t *env_off, *env_first;
    // mslam_hip_set_ba_global_pcg: S holds the pairs' blocks themselves (SysLayout::Pairs), ci the index order; the block of
    // pair i of `pairs`.  The right-hand side is rhs
    const int32_t* pair_slot;
};

__device__ __forceinline__ void ba_residual(const double* __restrict__ pose, const double* __restrict__ X, const double* __restrict__ obs,
                                            double r[3])
{
    double qi[4], a[3], b[3];
    quat_inverse(pose, qi);
    const double x[3] = {X[0], X[1], X[2]}, p[3] = {pose[4], pose[5], pose[6]};
    quat_rotate(qi, x, a);
    quat_rotate(qi, p, b);
    r[0] = a[0] - b[0] - obs[0], r[1] = a[1] - b[1] - obs[1], r[2] = a[2] - b[2] - obs[2];
}
// loss_function.h's HuberLoss / CauchyLoss Evaluate at s = |r|^2 with scale a: rho(s) and w = rho'(s).  b = a^2.
//   Huber:  s > b: rho = 2 a sqrt(s) - b, rho' = max(DBL_MIN, a / sqrt(s)); else rho = s, rho' = 1 (s == b is the inlier branch)
//   Cauchy: rho = b log(1 + s c), rho' = max(DBL_MIN, 1 / (1 + s c)), c = 1 / b
// rho'' <= 0 for both, so corrector.cc takes the branch that scales residual and Jacobians by sqrt(rho') and nothing else.
// s = 0 gives w = 1 in both (no 0 / 0); a NaN s gives a NaN rho, which the cost carries to FAILURE.
__device__ __forceinline__ void ba_loss(int kind, double a, double s, double& rho, double& w)
{
    const double b = a * a;
    if(kind == MSLAM_HIP_BA_LOSS_HUBER)
    {
        if(s > b)
        {
            const double r = sqrt(s);
            rho = 2.0 * a * r - b;
            w = fmax(DBL_MIN, a / r);
        }
        else
            rho = s, w = 1.0;
    }
    else
    {
        const double sum = 1.0 + s * (1.0 / b);
        rho = b * log(sum);
        w = fmax(DBL_MIN, 1.0 / sum);
    }
}
// w_m of observation m from its residual
__device__ __forceinline__ double ba_weight(const BaArgs& a, const double r[3])
{
    double rho, w;
    ba_loss(a.loss_kind, a.loss_scale, r[0] * r[0] + r[1] * r[1] + r[2] * r[2], rho, w);
    return w;
}
// a product of observation m: w x with a loss, x itself (no multiplication by 1) without; w is then not evaluated by the caller
template <bool kLoss>
__device__ __forceinline__ double ba_weighted(double w, double x)
{
    if constexpr(kLoss)
        return w * x;
    else
        return x;
}
// J_c = [2 R^T [d]x | -R^T] (3 x 6), d = X - p
__device__ __forceinline__ void ba_camera_jacobian(const double Rt[9], const double d[3], double Jc[3][6])
{
    const double dx[9] = {0.0, -d[2], d[1], d[2], 0.0, -d[0], -d[1], d[0], 0.0};
    for(int i = 0; i < 3; ++i)
        for(int j = 0; j < 3; ++j)
        {
            Jc[i][j] = 2.0 * (Rt[i * 3] * dx[j] + Rt[i * 3 + 1] * dx[3 + j] + Rt[i * 3 + 2] * dx[6 + j]);
            Jc[i][3 + j] = -Rt[i * 3 + j];
        }
}

// ---- blocks ------------------------------------------------------------------------------------------------------------

// kLoss = false: no loss function, the kernels of mslam_hip_bundle_adjust as the reference states it; kLoss = true: every
// product of observation m takes w_m
template <bool kLoss>
__device__ __forceinline__ void ba_landmarks_rows(const BaArgs& a)
{
    const TrCtrl* ct = a.ctrl;
    if(ct->done)
        return;
    const int l = blockIdx.x * 256 + threadIdx.x;
    if(l >= a.L || !a.lm_active[l])
        return;
    double V[6], g[3];
    if(ct->need_jac)
    {
        for(int k = 0; k < 6; ++k)
            V[k] = 0.0;
        g[0] = g[1] = g[2] = 0.0;
        const double* X = a.lm + (size_t)l * 3;
        for(int i = a.lm_ptr[l]; i < a.lm_ptr[l + 1]; ++i)
        {
            const int m = a.lm_obs[i];
            const double* pose = a.pose + (size_t)a.obs_kf[m] * 7;
            double qi[4], Rt[9], r[3];
            quat_inverse(pose, qi);
            quat_matrix(qi, Rt);
            ba_residual(pose, X, a.obs_cam + (size_t)m * 3, r);
            double w = 1.0; // read only with a loss.  Constant keyframes too: their rows are part of V and g_l
            if constexpr(kLoss)
                w = ba_weight(a, r);
            for(int rr = 0; rr < 3; ++rr)
            {
                for(int c = rr; c < 3; ++c)
                    V[tri3(rr, c)] += ba_weighted<kLoss>(w, Rt[rr] * Rt[c] + Rt[3 + rr] * Rt[3 + c] + Rt[6 + rr] * Rt[6 + c]);
                g[rr] += ba_weighted<kLoss>(w, Rt[rr] * r[0] + Rt[3 + rr] * r[1] + Rt[6 + rr] * r[2]);
            }
        }
        for(int k = 0; k < 6; ++k)
            a.V[(size_t)l * 6 + k] = V[k];
        for(int k = 0; k < 3; ++k)
            a.gl[(size_t)l * 3 + k] = g[k];
    }
    else
        for(int k = 0; k < 6; ++k)
            V[k] = a.V[(size_t)l * 6 + k];
    double s[3];
    for(int k = 0; k < 3; ++k)
    {
        if(ct->first)
            a.sl[(size_t)l * 3 + k] = s[k] = 1.0 / (1.0 + sqrt(V[tri3(k, k)]));
        else
            s[k] = a.sl[(size_t)l * 3 + k];
    }
    // A = S V S + D^2, D^2 = clamp(diag(S V S), 1e-6, 1e32) / radius; its inverse from the cofactors
    const double radius = ct->radius;
    double A[6];
    for(int r = 0; r < 3; ++r)
        for(int c = r; c < 3; ++c)
            A[tri3(r, c)] = s[r] * V[tri3(r, c)] * s[c];
    for(int k = 0; k < 3; ++k)
        A[tri3(k, k)] += fmin(fmax(A[tri3(k, k)], kTrMinDiagonal), kTrMaxDiagonal) / radius;
    const double a00 = A[0], a01 = A[1], a02 = A[2], a11 = A[3], a12 = A[4], a22 = A[5];
    const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
    const double det = a00 * c00 + a01 * c01 + a02 * c02;
    double* I = a.Vinv + (size_t)l * 6;
    I[0] = c00 / det, I[1] = c01 / det, I[2] = c02 / det;
    I[3] = (a00 * a22 - a02 * a02) / det, I[4] = (a01 * a02 - a00 * a12) / det, I[5] = (a00 * a11 - a01 * a01) / det;
}

__global__ __launch_bounds__(256) void k_ba_landmarks(BaArgs a) { ba_landmarks_rows<false>(a); }

template <bool kLoss>
__device__ __forceinline__ void ba_cameras_rows(const BaArgs& a)
{
    __shared__ double red[4][27];
    const TrCtrl* ct = a.ctrl;
    if(ct->done || !ct->need_jac)
        return;
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if(a.ci[k] < 0)
        return;
    const double* pose = a.pose + (size_t)k * 7;
    double qi[4], Rt[9];
    quat_inverse(pose, qi);
    quat_matrix(qi, Rt);
    double acc[27];
    for(int j = 0; j < 27; ++j)
        acc[j] = 0.0;
    for(int pos = a.kf_ptr[k] + tid; pos < a.kf_ptr[k + 1]; pos += 256)
    {
        const int m = a.kf_obs[pos];
        const double* X = a.lm + (size_t)a.obs_lm[m] * 3;
        const double d[3] = {X[0] - pose[4], X[1] - pose[5], X[2] - pose[6]};
        double r[3], Jc[3][6];
        ba_residual(pose, X, a.obs_cam + (size_t)m * 3, r);
        ba_camera_jacobian(Rt, d, Jc);
        int j = 0;
        double w = 1.0; // read only with a loss
        if constexpr(kLoss)
            w = ba_weight(a, r);
        for(int rr = 0; rr < 6; ++rr)
            for(int c = rr; c < 6; ++c)
                acc[j++] += ba_weighted<kLoss>(w, Jc[0][rr] * Jc[0][c] + Jc[1][rr] * Jc[1][c] + Jc[2][rr] * Jc[2][c]);
        for(int rr = 0; rr < 6; ++rr)
            acc[21 + rr] += ba_weighted<kLoss>(w, Jc[0][rr] * r[0] + Jc[1][rr] * r[1] + Jc[2][rr] * r[2]);
        double* W = a.W + (size_t)m * 18; // J_c^T J_l, J_l = R^T
        for(int rr = 0; rr < 6; ++rr)
            for(int c = 0; c < 3; ++c)
                W[rr * 3 + c] = ba_weighted<kLoss>(w, Jc[0][rr] * Rt[c] + Jc[1][rr] * Rt[3 + c] + Jc[2][rr] * Rt[6 + c]);
    }
    for(int j = 0; j < 27; ++j)
    {
        const double v = wave_sum(acc[j]);
        if(lane == 0)
            red[wave][j] = v;
    }
    __syncthreads();
    if(tid < 27)
    {
        const double v = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
        if(tid < 21)
            a.U[(size_t)k * 21 + tid] = v;
        else
            a.gc[(size_t)k * 6 + (tid - 21)] = v;
    }
    if(tid < 6 && ct->first)
    {
        const int j = tri6(tid, tid);
        a.sc[(size_t)k * 6 + tid] = 1.0 / (1.0 + sqrt(((red[0][j] + red[1][j]) + red[2][j]) + red[3][j]));
    }
}

__global__ __launch_bounds__(256) void k_ba_cameras(BaArgs a) { ba_cameras_rows<false>(a); }

// ---- FinalizeIterationAndCheckIfMinimizerCanContinue: one wave ------------------------------------------------------------

__global__ __launch_bounds__(64) void k_ba_check(BaArgs a)
{
    if(a.ctrl->done)
        return;
    const int lane = threadIdx.x;
    bool ok = true;
    double gmax = 0.0;
    for(int k = lane; k < a.K; k += 64)
        if(a.ci[k] >= 0)
            tr_pose_gradient(a.pose + (size_t)k * 7, a.gc + (size_t)k * 6, a.U + (size_t)k * 21, ok, gmax);
    for(int l = lane; l < a.L; l += 64)
    {
        if(!a.lm_active[l])
            continue;
        const double* X = a.lm + (size_t)l * 3;
        const double* g = a.gl + (size_t)l * 3;
        for(int j = 0; j < 3; ++j)
        {
            gmax = fmax(gmax, fabs(X[j] - (X[j] + (-g[j]))));
            ok = ok && isfinite(g[j]) && isfinite(a.V[(size_t)l * 6 + tri3(j, j)]);
        }
    }
    tr_check(a.ctrl, a.h_done, lane, a.part, a.n_blocks, ok, gmax);
}

// ---- the reduced camera system ------------------------------------------------------------------------------------------

// The block of a pair and, on the diagonal, the reduced right-hand side, stored through SysView (reduced_system.hpp): Full for
// k_ba_solve, PaddedLower for the blocked solve, Envelope for the envelope factor, where b1 and b2 are positions in the chosen
// order and of a diagonal block only the lower triangle is written.
template <SysLayout kLayout>
__device__ __forceinline__ void ba_schur_pair(const BaArgs& a)
{
    const TrCtrl* ct = a.ctrl;
    if(ct->done)
        return;
    const int lane = threadIdx.x;
    const int k1 = a.pairs[blockIdx.x * 2], k2 = a.pairs[blockIdx.x * 2 + 1];
    const int b1 = a.ci[k1], b2 = a.ci[k2];
    const bool diag = k1 == k2;
    double s1[6], s2[6];
    for(int j = 0; j < 6; ++j)
        s1[j] = a.sc[(size_t)k1 * 6 + j], s2[j] = a.sc[(size_t)k2 * 6 + j];
    double acc[36], accr[6];
    for(int j = 0; j < 36; ++j)
        acc[j] = 0.0;
    for(int j = 0; j < 6; ++j)
        accr[j] = 0.0;
    const int lo2 = a.kf_ptr[k2], hi2 = a.kf_ptr[k2 + 1];
    for(int pos = a.kf_ptr[k1] + lane; pos < a.kf_ptr[k1 + 1]; pos += 64)
    {
        const int l = a.kf_lm[pos];
        // the first observation of landmark l in row k2
        int lo = lo2, hi = hi2;
        while(lo < hi)
        {
            const int mid = (lo + hi) >> 1;
            if(a.kf_lm[mid] < l)
                lo = mid + 1;
            else
                hi = mid;
        }
        if(!diag && (lo >= hi2 || a.kf_lm[lo] != l))
            continue;
        const double* W1 = a.W + (size_t)a.kf_obs[pos] * 18;
        const double* Vi = a.Vinv + (size_t)l * 6;
        const double* sl = a.sl + (size_t)l * 3;
        // T = W1s V^-1 (6 x 3), W1s = S_c W1 S_l
        double T[6][3];
        for(int r = 0; r < 6; ++r)
        {
            const double w0 = s1[r] * W1[r * 3] * sl[0], w1 = s1[r] * W1[r * 3 + 1] * sl[1], w2 = s1[r] * W1[r * 3 + 2] * sl[2];
            T[r][0] = w0 * Vi[0] + w1 * Vi[1] + w2 * Vi[2];
            T[r][1] = w0 * Vi[1] + w1 * Vi[3] + w2 * Vi[4];
            T[r][2] = w0 * Vi[2] + w1 * Vi[4] + w2 * Vi[5];
        }
        if(diag)
        {
            const double* g = a.gl + (size_t)l * 3;
            const double g0 = sl[0] * g[0], g1 = sl[1] * g[1], g2 = sl[2] * g[2];
            for(int r = 0; r < 6; ++r)
                accr[r] += T[r][0] * g0 + T[r][1] * g1 + T[r][2] * g2;
        }
        for(int p2 = lo; p2 < hi2 && a.kf_lm[p2] == l; ++p2)
        {
            const double* W2 = a.W + (size_t)a.kf_obs[p2] * 18;
            for(int c = 0; c < 6; ++c)
            {
                const double w0 = s2[c] * W2[c * 3] * sl[0], w1 = s2[c] * W2[c * 3 + 1] * sl[1], w2 = s2[c] * W2[c * 3 + 2] * sl[2];
                for(int r = 0; r < 6; ++r)
                    acc[r * 6 + c] += T[r][0] * w0 + T[r][1] * w1 + T[r][2] * w2;
            }
        }
    }
    // lane j keeps entry j of the block (j < 36), lane 36 + r entry r of the right-hand side
    double mine = 0.0;
    for(int j = 0; j < 36; ++j)
    {
        const double v = wave_sum(acc[j]);
        if(lane == j)
            mine = v;
    }
    if(diag)
        for(int j = 0; j < 6; ++j)
        {
            const double v = wave_sum(accr[j]);
            if(lane == 36 + j)
                mine = v;
        }
    const SysView<kLayout> sys(a);
    if(lane < 36)
    {
        const int r = lane / 6, c = lane % 6;
        double v = -mine;
        if(diag)
        {
            const double u = s1[r] * a.U[(size_t)k1 * 21 + (r <= c ? tri6(r, c) : tri6(c, r))] * s1[c];
            v = u - mine;
            if(r == c)
                v = (u + fmin(fmax(u, kTrMinDiagonal), kTrMaxDiagonal) / ct->radius) - mine;
        }
        sys.store(b1, b2, diag, r, c, v, true);
    }
    else if(diag && lane < 42)
    {
        const int r = lane - 36;
        sys.store_rhs(b1, r, s1[r] * a.gc[(size_t)k1 * 6 + r] - mine);
    }
}

__global__ __launch_bounds__(64) void k_ba_schur(BaArgs a) { ba_schur_pair<SysLayout::Full>(a); }

// Cholesky S = L L^T in place (lower triangle, column-major), then L y = rhs and L^T x = y.  Thread i owns row i.
__global__ __launch_bounds__(kBaSolveThreads) void k_ba_solve(BaArgs a)
{
    __shared__ double rowj[kBaSolveThreads], b[kBaSolveThreads];
    __shared__ double sdiag;
    __shared__ int bad;
    TrCtrl* ct = a.ctrl;
    if(ct->done)
        return;
    const int i = threadIdx.x, n = a.n;
    double* S = a.S;
    if(i == 0)
        bad = 0;
    for(int j = 0; j < n; ++j)
    {
        if(i < j)
            rowj[i] = S[(size_t)j + (size_t)i * n];
        __syncthreads();
        double v = 0.0;
        if(i >= j && i < n)
        {
            v = S[(size_t)i + (size_t)j * n];
            for(int k = 0; k < j; ++k)
                v -= S[(size_t)i + (size_t)k * n] * rowj[k];
        }
        if(i == j)
        {
            if(!(v > 0.0))
                bad = 1; // a non-positive pivot: the step is invalid; the factorisation goes on with bounded values
            sdiag = sqrt(fmax(v, DBL_MIN));
        }
        __syncthreads();
        if(i >= j && i < n)
            S[(size_t)i + (size_t)j * n] = i == j ? sdiag : v / sdiag;
        __syncthreads();
    }
    if(i < n)
        b[i] = a.rhs[i];
    __syncthreads();
    for(int k = 0; k < n; ++k)
    {
        if(i == k)
            b[k] = b[k] / S[(size_t)k + (size_t)k * n];
        __syncthreads();
        if(i > k && i < n)
            b[i] -= S[(size_t)i + (size_t)k * n] * b[k];
        __syncthreads();
    }
    for(int k = n - 1; k >= 0; --k)
    {
        if(i == k)
            b[k] = b[k] / S[(size_t)k + (size_t)k * n];
        __syncthreads();
        if(i < k)
            b[i] -= S[(size_t)k + (size_t)i * n] * b[k];
        __syncthreads();
    }
    if(i < n)
        a.yc[i] = b[i];
    if(i == 0 && bad)
        ct->solve_bad = 1;
}

// the reduced system of mslam_hip_bundle_adjust_global for the blocked solve (chol_solver.hpp)
__global__ __launch_bounds__(64) void k_bag_schur(BaArgs a) { ba_schur_pair<SysLayout::PaddedLower>(a); }

__global__ __launch_bounds__(256) void k_ba_backsub(BaArgs a)
{
    if(a.ctrl->done)
        return;
    const int l = blockIdx.x * 256 + threadIdx.x;
    if(l >= a.L || !a.lm_active[l])
        return;
    const double* sl = a.sl + (size_t)l * 3;
    const double* g = a.gl + (size_t)l * 3;
    double t[3] = {sl[0] * g[0], sl[1] * g[1], sl[2] * g[2]};
    for(int i = a.lm_ptr[l]; i < a.lm_ptr[l + 1]; ++i)
    {
        const int m = a.lm_obs[i], k = a.obs_kf[m], bk = a.ci[k];
        if(bk < 0)
            continue;
        const double* W = a.W + (size_t)m * 18;
        const double* sc = a.sc + (size_t)k * 6;
        const double* y = a.yc + (size_t)bk * 6;
        for(int c = 0; c < 3; ++c)
        {
            double s = 0.0;
            for(int r = 0; r < 6; ++r)
                s += sc[r] * W[r * 3 + c] * sl[c] * y[r];
            t[c] -= s;
        }
    }
    const double* Vi = a.Vinv + (size_t)l * 6;
    double* y = a.yl + (size_t)l * 3;
    y[0] = Vi[0] * t[0] + Vi[1] * t[1] + Vi[2] * t[2];
    y[1] = Vi[1] * t[0] + Vi[3] * t[1] + Vi[4] * t[2];
    y[2] = Vi[2] * t[0] + Vi[4] * t[1] + Vi[5] * t[2];
}

// delta = step * scaling with step = -y; Plus.  Blocks outside the problem are copied.
__global__ __launch_bounds__(256) void k_ba_candidate(BaArgs a)
{
    if(a.ctrl->done)
        return;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if(t < a.K)
    {
        const int bk = a.ci[t];
        tr_pose_plus(a.pose + (size_t)t * 7, bk < 0 ? nullptr : a.yc + (size_t)bk * 6, a.sc + (size_t)t * 6, a.cand_pose + (size_t)t * 7);
    }
    else if(t < a.K + a.L)
    {
        const int l = t - a.K;
        const double* x = a.lm + (size_t)l * 3;
        double* c = a.cand_lm + (size_t)l * 3;
        const bool on = a.lm_active[l];
        for(int j = 0; j < 3; ++j)
            c[j] = on ? x[j] + (-a.yl[(size_t)l * 3 + j] * a.sl[(size_t)l * 3 + j]) : x[j];
    }
}

// at_start: only the cost at the state (pose, lm), for iteration 0.  kLoss: the model term takes w_m at the state, the cost
// is rho(|r|^2) / 2
template <bool kLoss>
__device__ __forceinline__ void ba_eval_rows(const BaArgs& a, int at_start)
{
    __shared__ double red[4];
    if(a.ctrl->done)
        return;
    const int m = blockIdx.x * 256 + threadIdx.x;
    double model = 0.0, cost = 0.0;
    if(m < a.M)
    {
        const int k = a.obs_kf[m], l = a.obs_lm[m];
        const double* obs = a.obs_cam + (size_t)m * 3;
        double r[3];
        if(at_start)
            ba_residual(a.pose + (size_t)k * 7, a.lm + (size_t)l * 3, obs, r);
        else
        {
            const double* pose = a.pose + (size_t)k * 7;
            const double* X = a.lm + (size_t)l * 3;
            double f[3], qi[4], Rt[9];
            ba_residual(pose, X, obs, f);
            quat_inverse(pose, qi);
            quat_matrix(qi, Rt);
            // J_s s = R^T (2 d x delta - dp + dX)
            double v[3] = {-a.yl[(size_t)l * 3] * a.sl[(size_t)l * 3], -a.yl[(size_t)l * 3 + 1] * a.sl[(size_t)l * 3 + 1],
                           -a.yl[(size_t)l * 3 + 2] * a.sl[(size_t)l * 3 + 2]};
            const int bk = a.ci[k];
            if(bk >= 0)
            {
                const double* y = a.yc + (size_t)bk * 6;
                const double* sc = a.sc + (size_t)k * 6;
                const double dl[3] = {-y[0] * sc[0], -y[1] * sc[1], -y[2] * sc[2]};
                const double d[3] = {X[0] - pose[4], X[1] - pose[5], X[2] - pose[6]};
                v[0] += 2.0 * (d[1] * dl[2] - d[2] * dl[1]) - (-y[3] * sc[3]);
                v[1] += 2.0 * (d[2] * dl[0] - d[0] * dl[2]) - (-y[4] * sc[4]);
                v[2] += 2.0 * (d[0] * dl[1] - d[1] * dl[0]) - (-y[5] * sc[5]);
            }
            double Js[3];
            for(int j = 0; j < 3; ++j)
                Js[j] = Rt[j * 3] * v[0] + Rt[j * 3 + 1] * v[1] + Rt[j * 3 + 2] * v[2];
            model = -(Js[0] * (f[0] + Js[0] / 2.0) + Js[1] * (f[1] + Js[1] / 2.0) + Js[2] * (f[2] + Js[2] / 2.0));
            if constexpr(kLoss)
                model = ba_weight(a, f) * model;
            ba_residual(a.cand_pose + (size_t)k * 7, a.cand_lm + (size_t)l * 3, obs, r);
        }
        if constexpr(kLoss)
        {
            double rho, w;
            ba_loss(a.loss_kind, a.loss_scale, r[0] * r[0] + r[1] * r[1] + r[2] * r[2], rho, w);
            cost = 0.5 * rho;
        }
        else
            cost = 0.5 * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    }
    const double ms = block_sum(model, red), cs = block_sum(cost, red);
    if(threadIdx.x == 0)
    {
        a.part[blockIdx.x] = ms;
        a.part[a.n_blocks + blockIdx.x] = cs;
    }
}

__global__ __launch_bounds__(256) void k_ba_eval(BaArgs a, int at_start) { ba_eval_rows<false>(a, at_start); }

// ---- the trust-region bookkeeping of one iteration: one wave ----------------------------------------------------------------

__global__ __launch_bounds__(64) void k_ba_control(BaArgs a)
{
    if(a.ctrl->done)
        return;
    const int lane = threadIdx.x;
    bool finite = true;
    double xn = 0.0, sn = 0.0;
    for(int k = lane; k < a.K; k += 64)
        if(a.ci[k] >= 0)
            tr_pose_step(a.pose + (size_t)k * 7, a.cand_pose + (size_t)k * 7, a.yc + (size_t)a.ci[k] * 6, finite, xn, sn);
    for(int l = lane; l < a.L; l += 64)
    {
        if(!a.lm_active[l])
            continue;
        for(int j = 0; j < 3; ++j)
        {
            finite = finite && isfinite(a.yl[(size_t)l * 3 + j]);
            const double x = a.lm[(size_t)l * 3 + j], d = x - a.cand_lm[(size_t)l * 3 + j];
            xn += x * x, sn += d * d;
        }
    }
    if(!tr_control(a.ctrl, a.h_done, lane, a.part, a.n_blocks, finite, xn, sn))
        return;
    for(int k = lane; k < a.K; k += 64)
        if(a.ci[k] >= 0)
            for(int j = 0; j < 7; ++j)
                a.pose[(size_t)k * 7 + j] = a.cand_pose[(size_t)k * 7 + j];
    for(int l = lane; l < a.L; l += 64)
        if(a.lm_active[l])
            for(int j = 0; j < 3; ++j)
                a.lm[(size_t)l * 3 + j] = a.cand_lm[(size_t)l * 3 + j];
}

// createOutput (:212-230): |r_m|^2 > threshold^2 at (pose, lm)
__global__ __launch_bounds__(256) void k_ba_outliers(BaArgs a, const double* __restrict__ pose, const double* __restrict__ lm,
                                                     double threshold2, uint8_t* __restrict__ out)
{
    const int m = blockIdx.x * 256 + threadIdx.x;
    if(m >= a.M)
        return;
    double r[3];
    ba_residual(pose + (size_t)a.obs_kf[m] * 7, lm + (size_t)a.obs_lm[m] * 3, a.obs_cam + (size_t)m * 3, r);
    out[m] = (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) > threshold2 ? 1 : 0;
}

// ---- the kernels of a solve with a loss function --------------------------------------------------------------------------
// Defined after every kernel of before, so that those keep their place in the code object: a solve without a loss runs the
// code it ran, where it was.
__global__ __launch_bounds__(256) void k_ba_landmarks_loss(BaArgs a) { ba_landmarks_rows<true>(a); }
__global__ __launch_bounds__(256) void k_ba_cameras_loss(BaArgs a) { ba_cameras_rows<true>(a); }
__global__ __launch_bounds__(256) void k_ba_eval_loss(BaArgs a, int at_start) { ba_eval_rows<true>(a, at_start); }

// ---- the reduced system of mslam_hip_bundle_adjust_global on its block envelope (MSLAM_HIP_BA_GLOBAL_SOLVER_SPARSE) -----------
// After the kernels above, for the same reason.  One wave per covisible pair; k_pgs_clear has zeroed the blocks no pair
// writes (the fill-in) before it, k_pgs_factor and k_pgs_backsolve follow (pg_sparse_solve).  DESIGN.md 4.26.
__global__ __launch_bounds__(64) void k_bag_schur_env(BaArgs a) { ba_schur_pair<SysLayout::Envelope>(a); }

// ---- the reduced system of mslam_hip_bundle_adjust_global as its non-zero blocks (mslam_hip_set_ba_global_pcg) ----------------
// After the kernels above, for the same reason.  One wave per covisible pair writes all 36 entries of the pair's block and, on
// the diagonal, the right-hand side: nothing is cleared before it.  The kernels of k_pcg.hip follow (pcg_solve).  DESIGN.md 4.29.
__global__ __launch_bounds__(64) void k_bag_schur_pairs(BaArgs a) { ba_schur_pair<SysLayout::Pairs>(a); }

} // namespace mslam

using namespace mslam;

// the first observation that names a keyframe or landmark out of range, -1: none
static int ba_bad_observation(int K, int L, const int32_t* obs_kf, const int32_t* obs_lm, int M)
{
    for(int m = 0; m < M; ++m)
        if(obs_kf[m] < 0 || obs_kf[m] >= K || obs_lm[m] < 0 || obs_lm[m] >= L)
            return m;
    return -1;
}

// the host's view of the observations: both orders, and the free keyframes that have an observation
struct BaRows
{
    std::vector<int32_t> lm_ptr, lm_obs;         // observations by landmark (rows in input order)
    std::vector<int32_t> kf_ptr, kf_obs, kf_lm;  // observations by keyframe, every row sorted by landmark
    std::vector<int32_t> ci;                     // [K] the keyframe's block in index order, -1: constant or unobserved
    int n_free = 0;
};

static void ba_rows(const uint8_t* fixed, int K, int L, const int32_t* obs_kf, const int32_t* obs_lm, int M, BaRows& rw)
{
    std::vector<int32_t>&lm_ptr = rw.lm_ptr, &lm_obs = rw.lm_obs, &kf_ptr = rw.kf_ptr, &kf_obs = rw.kf_obs, &kf_lm = rw.kf_lm;
    // the two orders of the observations, by stable counting sorts: by landmark; by keyframe with rows sorted by landmark
    lm_ptr.assign((size_t)L + 1, 0), lm_obs.assign((size_t)M, 0), kf_ptr.assign((size_t)K + 1, 0), kf_obs.assign((size_t)M, 0);
    kf_lm.assign((size_t)M, 0);
    for(int m = 0; m < M; ++m)
        ++lm_ptr[(size_t)obs_lm[m] + 1], ++kf_ptr[(size_t)obs_kf[m] + 1];
    for(int l = 0; l < L; ++l)
        lm_ptr[(size_t)l + 1] += lm_ptr[(size_t)l];
    for(int k = 0; k < K; ++k)
        kf_ptr[(size_t)k + 1] += kf_ptr[(size_t)k];
    {
        std::vector<int32_t> at(lm_ptr.begin(), lm_ptr.end() - 1);
        for(int m = 0; m < M; ++m)
            lm_obs[(size_t)at[(size_t)obs_lm[m]]++] = m;
        at.assign(kf_ptr.begin(), kf_ptr.end() - 1);
        for(int i = 0; i < M; ++i) // in landmark order: every keyframe's row comes out sorted by landmark
        {
            const int m = lm_obs[(size_t)i];
            const int pos = at[(size_t)obs_kf[m]]++;
            kf_obs[(size_t)pos] = m, kf_lm[(size_t)pos] = obs_lm[m];
        }
    }
    rw.ci.assign((size_t)K, -1);
    rw.n_free = 0;
    for(int k = 0; k < K; ++k)
        if(!(fixed && fixed[k]) && kf_ptr[(size_t)k + 1] > kf_ptr[(size_t)k])
            rw.ci[(size_t)k] = rw.n_free++;
}

// The symbolic phase of MSLAM_HIP_BA_GLOBAL_SOLVER_SPARSE (mslam_hip_bundle_adjust_global_analyze exposes it).  pairs: the
// covisible pairs k1 <= k2 of free observed keyframes, every diagonal pair included, sorted by (k1, k2), each once: the list
// the bit table of the DENSE path reads out, built without a K x K pass.  Keyframe k1 walks its row, and for every landmark of
// it that landmark's row, and notes each later keyframe the first time it meets it (a stamp per keyframe): sum over the
// landmarks of views^2 steps and O(K) memory, then a sort per keyframe.  The nodes are the free observed keyframes, the edges
// the pairs off the diagonal; pg_symbolic gives the two orders and keeps the smaller envelope.  sy = nullptr: the pairs alone
// (mslam_hip_set_ba_global_pcg needs no order and no envelope).
static void ba_symbolic(const uint8_t* fixed, int K, const int32_t* obs_kf, const BaRows& rw, std::vector<int32_t>& pairs, PgSymbolic* sy)
{
    std::vector<int32_t> stamp((size_t)K, -1), later, ea, eb;
    std::vector<uint8_t> node((size_t)K, 0);
    pairs.clear();
    for(int k1 = 0; k1 < K; ++k1)
    {
        if(rw.ci[(size_t)k1] < 0)
            continue;
        node[(size_t)k1] = 1;
        later.clear();
        for(int pos = rw.kf_ptr[(size_t)k1]; pos < rw.kf_ptr[(size_t)k1 + 1]; ++pos)
        {
            const int l = rw.kf_lm[(size_t)pos];
            if(pos > rw.kf_ptr[(size_t)k1] && rw.kf_lm[(size_t)pos - 1] == l)
                continue; // the landmark twice in this keyframe: its row has been walked
            for(int i = rw.lm_ptr[(size_t)l]; i < rw.lm_ptr[(size_t)l + 1]; ++i)
            {
                const int k2 = obs_kf[rw.lm_obs[(size_t)i]];
                if(k2 > k1 && rw.ci[(size_t)k2] >= 0 && stamp[(size_t)k2] != k1)
                    stamp[(size_t)k2] = k1, later.push_back(k2);
            }
        }
        std::sort(later.begin(), later.end());
        pairs.push_back(k1), pairs.push_back(k1);
        for(const int32_t k2 : later)
        {
            pairs.push_back(k1), pairs.push_back(k2);
            if(sy)
                ea.push_back(k1), eb.push_back(k2);
        }
    }
    if(sy)
        pg_symbolic(fixed, K, ea.data(), eb.data(), ea.size(), *sy, node.data());
}

// every pair k1 <= k2 of free observed keyframes (mslam_hip_bundle_adjust)
static void ba_pairs_all(int K, const std::vector<int32_t>& ci, std::vector<int32_t>& pairs)
{
    for(int k1 = 0; k1 < K; ++k1)
        for(int k2 = k1; k2 < K; ++k2)
            if(ci[(size_t)k1] >= 0 && ci[(size_t)k2] >= 0)
                pairs.push_back(k1), pairs.push_back(k2);
}

// The covisible pairs by a K x K bit table (the DENSE solver, K <= 1024): every k1 <= k2 of free keyframes that share a landmark,
// and every diagonal pair.  A row of W words per keyframe: a landmark's row becomes one bit set, which every keyframe of the
// row ORs into its own (views x W word operations per landmark, not views^2), read out in (k1, k2) order: sorted, each pair
// once.  The list ba_symbolic walks out; the host costs differ by shape, so each solver keeps its lister.
static void ba_pairs_table(int K, int L, const int32_t* obs_kf, const BaRows& rw, std::vector<int32_t>& pairs)
{
    const std::vector<int32_t>&lm_ptr = rw.lm_ptr, &lm_obs = rw.lm_obs, &ci = rw.ci;
    const size_t W = ((size_t)K + 63) / 64;
    std::vector<uint64_t> shares((size_t)K * W, 0), seen(W);
    for(int l = 0; l < L; ++l)
    {
        if(lm_ptr[(size_t)l + 1] - lm_ptr[(size_t)l] < 2)
            continue; // one view: only the diagonal pair, which is listed anyway
        std::fill(seen.begin(), seen.end(), 0);
        for(int i = lm_ptr[(size_t)l]; i < lm_ptr[(size_t)l + 1]; ++i)
        {
            const int k = obs_kf[lm_obs[(size_t)i]];
            if(ci[(size_t)k] >= 0)
                seen[(size_t)k >> 6] |= 1ull << (k & 63);
        }
        for(size_t w = 0; w < W; ++w)
            for(uint64_t bits = seen[w]; bits; bits &= bits - 1)
            {
                uint64_t* mine = &shares[(w * 64 + (size_t)__builtin_ctzll(bits)) * W];
                for(size_t v = 0; v < W; ++v)
                    mine[v] |= seen[v];
            }
    }
    for(int k1 = 0; k1 < K; ++k1)
        for(int k2 = k1; k2 < K; ++k2)
            if(ci[(size_t)k1] >= 0 && (k1 == k2 || (shares[(size_t)k1 * W + ((size_t)k2 >> 6)] >> (k2 & 63) & 1)))
                pairs.push_back(k1), pairs.push_back(k2);
}

// Local: mslam_hip_bundle_adjust (every pair of free keyframes, k_ba_schur, k_ba_solve, S inside d_ba).  The other two:
// mslam_hip_bundle_adjust_global (covisible pairs, S in d_ba_S) with its solver DENSE (k_bag_schur, the blocked factor) or
// SPARSE (k_bag_schur_env, the envelope factor) or, after mslam_hip_set_ba_global_pcg, whatever that solver is, PCG
// (k_bag_schur_pairs, k_pcg.hip).  Decided once, at the top of ba_run.
enum class BaMode { Local, GlobalDense, GlobalSparse, GlobalPcg };

// the caller's problem, as the entry points take it
struct BaProblem
{
    double *poses, *landmarks;
    const uint8_t* fixed;
    const int32_t *obs_kf, *obs_lm;
    const double* obs_cam;
    int K, L, M;
};

static int ba_validate(mslam_hip_ctx* c, BaMode mode, const BaProblem& p, int k_max, int max_iterations, double outlier_threshold)
{
    const int K = p.K, L = p.L, M = p.M;
    if(K < 0 || K > k_max)
        return fail(c, MSLAM_HIP_E_INVALID, mode == BaMode::GlobalSparse  ? "bundle_adjust_global: K outside 0..16384 (the SPARSE solver)"
                                            : mode == BaMode::GlobalPcg   ? "bundle_adjust_global: K outside 0..16384 (PCG)"
                                            : mode == BaMode::GlobalDense ? "bundle_adjust_global: K outside 0..1024"
                                                                          : "bundle_adjust: K outside 0..64");
    if(L < 0 || M < 0 || L > (1 << 24) || M > (1 << 24) || max_iterations < 0 || !(outlier_threshold >= 0.0) || (K > 0 && !p.poses) ||
       (L > 0 && !p.landmarks) || (M > 0 && (!p.obs_kf || !p.obs_lm || !p.obs_cam)))
        return fail(c, MSLAM_HIP_E_INVALID, "bundle_adjust: bad argument (counts, pointers, max_iterations >= 0, threshold >= 0)");
    if(const int m = ba_bad_observation(K, L, p.obs_kf, p.obs_lm, M); m >= 0)
        return fail(c, MSLAM_HIP_E_INVALID, "bundle_adjust: observation " + std::to_string(m) + " names a keyframe or landmark out of range");
    for(int k = 0; k < K; ++k)
        if(!tr_unit_quaternion(p.poses + (size_t)k * 7))
            return fail(c, MSLAM_HIP_E_INVALID, "bundle_adjust: the quaternion of pose " + std::to_string(k) + " is not unit");
    return MSLAM_HIP_OK;
}

// what the read-back needs beside BaArgs: the kept inputs and the outlier mask, on the device
struct BaKept
{
    double *pose0, *lm0;
    uint8_t* out;
};

// Staging and argument wiring: one device block (what is uploaded first, the control block at 0, then the working arrays),
// S where the mode keeps it, and a filled in.  st is the caller's: the upload reads its host block
static int ba_stage(mslam_hip_ctx* c, BaMode mode, const BaProblem& p, const BaRows& rw, const std::vector<int32_t>& pairs,
                    LinearSolve& ls, TrStaging& st, BaArgs& a, BaKept& kept)
{
    const int K = p.K, L = p.L, M = p.M;
    const bool local = mode == BaMode::Local;
    std::vector<uint8_t> lm_active((size_t)L, 0);
    for(int l = 0; l < L; ++l)
        lm_active[(size_t)l] = rw.lm_ptr[(size_t)l + 1] > rw.lm_ptr[(size_t)l];
    a.K = K, a.L = L, a.M = M, a.n = 6 * rw.n_free, a.n_pad = ls.n_pad, a.ld = ls.ld;
    a.n_pairs = (int)(pairs.size() / 2), a.n_blocks = (M + 255) / 256;
    const size_t o_pose = st.put(p.poses, (size_t)K * 56), o_lm = st.put(p.landmarks, (size_t)L * 24), o_cam = st.put(p.obs_cam, (size_t)M * 24);
    const size_t o_okf = st.put(p.obs_kf, (size_t)M * 4), o_olm = st.put(p.obs_lm, (size_t)M * 4), o_lptr = st.put(rw.lm_ptr.data(), ((size_t)L + 1) * 4);
    const size_t o_lobs = st.put(rw.lm_obs.data(), (size_t)M * 4), o_kptr = st.put(rw.kf_ptr.data(), ((size_t)K + 1) * 4);
    const size_t o_kobs = st.put(rw.kf_obs.data(), (size_t)M * 4), o_klm = st.put(rw.kf_lm.data(), (size_t)M * 4), o_ci = st.put(rw.ci.data(), (size_t)K * 4);
    const size_t o_pairs = st.put(pairs.data(), pairs.size() * 4), o_act = st.put(lm_active.data(), (size_t)L);
    ls.put(st);
    const size_t o_pose0 = st.carve((size_t)K * 56), o_lm0 = st.carve((size_t)L * 24), o_cpose = st.carve((size_t)K * 56), o_clm = st.carve((size_t)L * 24);
    const size_t o_V = st.carve((size_t)L * 48), o_gl = st.carve((size_t)L * 24), o_Vinv = st.carve((size_t)L * 48), o_sl = st.carve((size_t)L * 24);
    const size_t o_U = st.carve((size_t)K * 168), o_gc = st.carve((size_t)K * 48), o_sc = st.carve((size_t)K * 48), o_W = st.carve((size_t)M * 144);
    const size_t o_S = st.carve(local ? (size_t)a.n * a.n * 8 : 0), o_rhs = st.carve((size_t)a.n * 8), o_yc = st.carve((size_t)a.n * 8);
    const size_t o_yl = st.carve((size_t)L * 24), o_part = st.carve((size_t)a.n_blocks * 16), o_out = st.carve((size_t)M);
    ls.carve(st, &o_rhs);
    MSLAM_CHK(c, hipSetDevice(c->p.device));
    MSLAM_CHK(c, grow(c->d_ba, st.size, c->stream));
    if(!local)
        MSLAM_CHK(c, ls.grow_S(c));
    if(!c->h_ba)
        MSLAM_CHK(c, c->h_ba.alloc(4));
    uint8_t* d = c->d_ba;
    hipStream_t s = c->stream;
    MSLAM_CHK(c, st.upload(d, s));
    // the inputs are kept: a FAILURE judges the outliers there
    MSLAM_CHK(c, hipMemcpyAsync(d + o_pose0, d + o_pose, (size_t)K * 56, hipMemcpyDeviceToDevice, s));
    MSLAM_CHK(c, hipMemcpyAsync(d + o_lm0, d + o_lm, (size_t)L * 24, hipMemcpyDeviceToDevice, s));
    auto dbl = [&](size_t at) { return reinterpret_cast<double*>(d + at); };
    auto i32 = [&](size_t at) { return reinterpret_cast<int32_t*>(d + at); };
    a.obs_kf = i32(o_okf), a.obs_lm = i32(o_olm), a.obs_cam = dbl(o_cam);
    a.lm_ptr = i32(o_lptr), a.lm_obs = i32(o_lobs), a.kf_ptr = i32(o_kptr), a.kf_obs = i32(o_kobs), a.kf_lm = i32(o_klm);
    a.ci = i32(o_ci), a.pairs = i32(o_pairs), a.lm_active = d + o_act;
    a.pose = dbl(o_pose), a.lm = dbl(o_lm), a.cand_pose = dbl(o_cpose), a.cand_lm = dbl(o_clm);
    a.V = dbl(o_V), a.gl = dbl(o_gl), a.Vinv = dbl(o_Vinv), a.sl = dbl(o_sl);
    a.U = dbl(o_U), a.gc = dbl(o_gc), a.sc = dbl(o_sc), a.W = dbl(o_W);
    a.S = local ? dbl(o_S) : c->d_ba_S.get(), a.rhs = dbl(o_rhs), a.yc = dbl(o_yc), a.yl = dbl(o_yl), a.part = dbl(o_part);
    a.ctrl = reinterpret_cast<TrCtrl*>(d);
    a.h_done = c->h_ba.dev();
    a.loss_kind = c->ba_loss_kind, a.loss_scale = c->ba_loss_scale;
    *c->h_ba.get() = 0;
    if(!local)
        ls.bind(c, d, a.yc);
    a.env_off = ls.env.row_off, a.env_first = ls.env.first;
    a.pair_slot = ls.pcg ? reinterpret_cast<const int32_t*>(d + ls.o_pslot) : nullptr;
    kept = {dbl(o_pose0), dbl(o_lm0), d + o_out};
    return MSLAM_HIP_OK;
}

// Read-back: the outliers at the result (after a FAILURE: at the inputs), then poses and landmarks
static int ba_read_back(mslam_hip_ctx* c, const BaProblem& p, const BaArgs& a, const BaKept& kept, double outlier_threshold,
                        uint8_t* outlier, mslam_hip_ba_summary& sum, mslam_hip_ba_summary* summary)
{
    const int K = p.K, L = p.L, M = p.M;
    hipStream_t s = c->stream;
    const bool usable = sum.termination != kTrFailure;
    std::vector<uint8_t> mask((size_t)M);
    hipLaunchKernelGGL(k_ba_outliers, dim3((unsigned)a.n_blocks), dim3(256), 0, s, a, usable ? a.pose : kept.pose0, usable ? a.lm : kept.lm0,
                       outlier_threshold * outlier_threshold, kept.out);
    MSLAM_CHK(c, hipGetLastError());
    MSLAM_CHK(c, hipMemcpyAsync(mask.data(), kept.out, (size_t)M, hipMemcpyDeviceToHost, s));
    std::vector<double> xp((size_t)K * 7), xl((size_t)L * 3);
    if(usable)
    {
        MSLAM_CHK(c, hipMemcpyAsync(xp.data(), a.pose, (size_t)K * 56, hipMemcpyDeviceToHost, s));
        MSLAM_CHK(c, hipMemcpyAsync(xl.data(), a.lm, (size_t)L * 24, hipMemcpyDeviceToHost, s));
    }
    MSLAM_CHK(c, hipStreamSynchronize(s));
    for(int m = 0; m < M; ++m)
        sum.n_outliers += mask[(size_t)m] ? 1 : 0;
    if(outlier)
        std::memcpy(outlier, mask.data(), (size_t)M);
    if(summary)
        *summary = sum;
    if(!usable)
        return fail(c, MSLAM_HIP_E_NO_MODEL, "bundle_adjust: the minimiser ended in FAILURE (non-finite cost or gradient, or 5 "
                                             "invalid steps in a row)");
    std::memcpy(p.poses, xp.data(), (size_t)K * 56);
    std::memcpy(p.landmarks, xl.data(), (size_t)L * 24);
    return MSLAM_HIP_OK;
}

// Both entry points
static int ba_run(mslam_hip_ctx* c, bool global, const BaProblem& p, int max_iterations, double outlier_threshold, uint8_t* outlier,
                  mslam_hip_ba_summary* summary)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    const BaMode mode = !global                                              ? BaMode::Local
                        : c->bag_pcg                                         ? BaMode::GlobalPcg
                        : c->bag_solver == MSLAM_HIP_BA_GLOBAL_SOLVER_SPARSE ? BaMode::GlobalSparse
                                                                             : BaMode::GlobalDense;
    // not used by Local, which stages nothing of it and has its own solve
    LinearSolve ls(mode == BaMode::GlobalSparse, mode == BaMode::GlobalPcg, c->bag_pcg_max_iterations, c->bag_pcg_tolerance);
    if(const int rc = ba_validate(c, mode, p, global ? ls.k_max() : kBaMaxKeyframes, max_iterations, outlier_threshold); rc != MSLAM_HIP_OK)
        return rc;
    mslam_hip_ba_summary sum{};
    if(global)
        c->bag_pcg_stats = mslam_hip_pcg_stats{};
    if(p.M == 0)
    {
        // solver.cc Minimize(): no parameter blocks -> CONVERGENCE at cost 0, nothing touched
        if(summary)
            *summary = sum;
        return MSLAM_HIP_OK;
    }
    BaRows rw;
    ba_rows(p.fixed, p.K, p.L, p.obs_kf, p.obs_lm, p.M, rw);
    std::vector<int32_t> pairs;
    if(mode == BaMode::Local)
        ba_pairs_all(p.K, rw.ci, pairs);
    else if(mode == BaMode::GlobalDense)
        ba_pairs_table(p.K, p.L, p.obs_kf, rw, pairs);
    else
        ba_symbolic(p.fixed, p.K, p.obs_kf, rw, pairs, mode == BaMode::GlobalPcg ? nullptr : &ls.sy);
    if(mode != BaMode::Local)
        if(const int rc = mode == BaMode::GlobalPcg ? ls.index_pairs(c, "bundle_adjust_global", pairs, rw.ci, rw.n_free)
                                                    : ls.index(c, "bundle_adjust_global", rw.ci, rw.n_free);
           rc != MSLAM_HIP_OK)
            return rc;
    BaArgs a{};
    BaKept kept{};
    TrStaging st(max_iterations);
    if(const int rc = ba_stage(c, mode, p, rw, pairs, ls, st, a, kept); rc != MSLAM_HIP_OK)
        return rc;

    hipStream_t s = c->stream;
    const bool loss = a.loss_kind != MSLAM_HIP_BA_LOSS_NONE;
    const dim3 g_lm((unsigned)((p.L + 255) / 256)), g_obs((unsigned)a.n_blocks), g_x((unsigned)((p.K + p.L + 255) / 256)), g_pair((unsigned)a.n_pairs);
    {
        StageScope ts(c, "ba_start_cost");
        hipLaunchKernelGGL(loss ? k_ba_eval_loss : k_ba_eval, g_obs, dim3(256), 0, s, a, 1);
    }
    // one iteration's launches before and after the linear solve
    const auto blocks = [&] {
        hipLaunchKernelGGL(loss ? k_ba_landmarks_loss : k_ba_landmarks, g_lm, dim3(256), 0, s, a);
        hipLaunchKernelGGL(loss ? k_ba_cameras_loss : k_ba_cameras, dim3((unsigned)p.K), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_ba_check, dim3(1), dim3(64), 0, s, a);
    };
    const auto step = [&] {
        hipLaunchKernelGGL(k_ba_backsub, g_lm, dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_ba_candidate, g_x, dim3(256), 0, s, a);
        hipLaunchKernelGGL(loss ? k_ba_eval_loss : k_ba_eval, g_obs, dim3(256), 0, s, a, 0);
        hipLaunchKernelGGL(k_ba_control, dim3(1), dim3(64), 0, s, a);
    };
    if(mode == BaMode::GlobalPcg)
    {
        // CG's length is the device's to decide: tr_run_pcg drives one trust-region iteration at a time
        const auto assemble = [&] { hipLaunchKernelGGL(k_bag_schur_pairs, g_pair, dim3(64), 0, s, a); };
        if(const int rc = tr_run_pcg(c, "ba_iterations", "bundle_adjust", a.ctrl, ls, a.n_pairs > 0, max_iterations, blocks, assemble, step,
                                     &c->bag_pcg_stats, sum);
           rc != MSLAM_HIP_OK)
            return rc;
        return ba_read_back(c, p, a, kept, outlier_threshold, outlier, sum, summary);
    }
    const int rc = tr_run(c, "ba_iterations", "bundle_adjust", a.ctrl, max_iterations, [&] {
        blocks();
        if(a.n_pairs > 0 && mode == BaMode::Local)
        {
            {
                StageScope tk(c, "solver_schur");
                hipLaunchKernelGGL(k_ba_schur, g_pair, dim3(64), 0, s, a);
            }
            StageScope tk(c, "solver_factor_subst");
            hipLaunchKernelGGL(k_ba_solve, dim3(1), dim3(kBaSolveThreads), 0, s, a);
        }
        else if(a.n_pairs > 0)
        {
            // the factor overwrote S and the radius moved: the reduced system is rebuilt in every iteration
            ls.solve(c, s, [&] { hipLaunchKernelGGL(ls.sparse ? k_bag_schur_env : k_bag_schur, g_pair, dim3(64), 0, s, a); });
        }
        step();
    }, sum);
    if(rc != MSLAM_HIP_OK)
        return rc;
    return ba_read_back(c, p, a, kept, outlier_threshold, outlier, sum, summary);
}

extern "C" int mslam_hip_bundle_adjust(mslam_hip_ctx* c, double* poses, const uint8_t* fixed, int K, double* landmarks, int L,
                                       const int32_t* obs_kf, const int32_t* obs_lm, const double* obs_cam, int M,
                                       int max_iterations, double outlier_threshold, uint8_t* outlier,
                                       mslam_hip_ba_summary* summary)
{
    return ba_run(c, false, {poses, landmarks, fixed, obs_kf, obs_lm, obs_cam, K, L, M}, max_iterations, outlier_threshold, outlier, summary);
}

extern "C" int mslam_hip_bundle_adjust_global(mslam_hip_ctx* c, double* poses, const uint8_t* fixed, int K, double* landmarks,
                                              int L, const int32_t* obs_kf, const int32_t* obs_lm, const double* obs_cam, int M,
                                              int max_iterations, double outlier_threshold, uint8_t* outlier,
                                              mslam_hip_ba_summary* summary)
{
    return ba_run(c, true, {poses, landmarks, fixed, obs_kf, obs_lm, obs_cam, K, L, M}, max_iterations, outlier_threshold, outlier, summary);
}

// The symbolic phase of the SPARSE solver without a context or a GPU: the argument checks of the solve, ba_rows, ba_symbolic
extern "C" int mslam_hip_bundle_adjust_global_analyze(const uint8_t* fixed, int K, const int32_t* obs_kf, const int32_t* obs_lm, int M,
                                                      int L, int32_t* order, int32_t* first, int* n_free, int* ordering,
                                                      int64_t* envelope_blocks, int* n_pairs)
{
    if(K < 0 || K > MSLAM_HIP_BA_GLOBAL_MAX_KEYFRAMES_SPARSE || L < 0 || M < 0 || L > (1 << 24) || M > (1 << 24) ||
       (M > 0 && (!obs_kf || !obs_lm)))
        return MSLAM_HIP_E_INVALID;
    if(ba_bad_observation(K, L, obs_kf, obs_lm, M) >= 0)
        return MSLAM_HIP_E_INVALID;
    BaRows rw;
    ba_rows(fixed, K, L, obs_kf, obs_lm, M, rw);
    std::vector<int32_t> pairs;
    PgSymbolic sy;
    ba_symbolic(fixed, K, obs_kf, rw, pairs, &sy);
    if(n_pairs)
        *n_pairs = (int)(pairs.size() / 2);
    return pg_symbolic_out(sy, order, first, n_free, ordering, envelope_blocks);
}

// The linear solver of mslam_hip_bundle_adjust_global: context state, read when it is called
extern "C" int mslam_hip_set_ba_global_solver(mslam_hip_ctx* c, int kind)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    if(kind != MSLAM_HIP_BA_GLOBAL_SOLVER_DENSE && kind != MSLAM_HIP_BA_GLOBAL_SOLVER_SPARSE)
        return fail(c, MSLAM_HIP_E_INVALID, "set_ba_global_solver: kind outside 0..1");
    c->bag_solver = kind;
    return MSLAM_HIP_OK;
}

extern "C" int mslam_hip_get_ba_global_solver(mslam_hip_ctx* c, int* kind)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    if(kind)
        *kind = c->bag_solver;
    return MSLAM_HIP_OK;
}

// PCG for mslam_hip_bundle_adjust_global: context state, read when it is called
extern "C" int mslam_hip_set_ba_global_pcg(mslam_hip_ctx* c, int enable, int max_iterations, double tolerance)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    if(enable < 0 || enable > 1 || max_iterations < 1 || !(tolerance > 0.0 && tolerance < 1.0))
        return fail(c, MSLAM_HIP_E_INVALID, "set_ba_global_pcg: enable outside 0..1, max_iterations < 1 or a tolerance outside (0, 1)");
    c->bag_pcg = enable, c->bag_pcg_max_iterations = max_iterations, c->bag_pcg_tolerance = tolerance;
    return MSLAM_HIP_OK;
}

extern "C" int mslam_hip_get_ba_global_pcg(mslam_hip_ctx* c, int* enable, int* max_iterations, double* tolerance)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    if(enable)
        *enable = c->bag_pcg;
    if(max_iterations)
        *max_iterations = c->bag_pcg_max_iterations;
    if(tolerance)
        *tolerance = c->bag_pcg_tolerance;
    return MSLAM_HIP_OK;
}

extern "C" int mslam_hip_get_ba_global_pcg_stats(mslam_hip_ctx* c, mslam_hip_pcg_stats* stats)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    if(stats)
        *stats = c->bag_pcg_stats;
    return MSLAM_HIP_OK;
}

// The loss of both entry points above: context state, read when they are called
extern "C" int mslam_hip_set_ba_loss(mslam_hip_ctx* c, int kind, double scale)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    if(kind < MSLAM_HIP_BA_LOSS_NONE || kind > MSLAM_HIP_BA_LOSS_CAUCHY)
        return fail(c, MSLAM_HIP_E_INVALID, "set_ba_loss: kind outside 0..2");
    if(kind != MSLAM_HIP_BA_LOSS_NONE && !(std::isfinite(scale) && scale > 0.0))
        return fail(c, MSLAM_HIP_E_INVALID, "set_ba_loss: the scale of HUBER / CAUCHY must be finite and > 0");
    c->ba_loss_kind = kind;
    c->ba_loss_scale = kind == MSLAM_HIP_BA_LOSS_NONE ? 0.0 : scale;
    return MSLAM_HIP_OK;
}

extern "C" int mslam_hip_get_ba_loss(mslam_hip_ctx* c, int* kind, double* scale)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    if(kind)
        *kind = c->ba_loss_kind;
    if(scale)
        *scale = c->ba_loss_scale;
    return MSLAM_HIP_OK;
}
