// ba_solver.hpp — what the solves outside k_ba.hip need of it: the control block every trust-region kernel reads first, the
// argument block the k_bag_* kernels take, and the launch sequence of the blocked f64 Cholesky (defined in k_ba.hip, beside
// the kernels: a kernel is launched from the object that holds it).  mslam_hip_bundle_adjust_global and
// mslam_hip_pose_graph (k_posegraph.hip) both solve their damped normal equations through ba_blocked_solve.
#pragma once
#include "context.hpp"

#include <functional>

namespace mslam
{

constexpr int kBagNB = 48; // panel width of the blocked factor: 8 keyframe blocks, 3 MFMA tiles

struct BaCtrl
{
    int32_t done, termination, iteration, need_jac, first, successful, invalid_run, solve_bad;
    int32_t rejected, invalid_total, max_iterations, pad;
    double radius, decrease_factor, x_cost, initial_cost;
};

struct BaArgs
{
    int K, L, M, n;     // n = 6 x (free keyframes with observations): the reduced system's size
    int n_pairs, n_blocks; // pairs of free keyframes; blocks of k_ba_eval
    int n_pad, ld;         // the blocked solver: n rounded up to kBagNB; leading dimension n_pad + 16 (row n_pad: the right-hand side)
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
    BaCtrl* ctrl;
    int32_t* h_done; // mapped
};

// One solve of S y = b by the blocked solver, enqueued on s.  Reads of `a`: n, n_pad, ld, S (n_pad columns of ld rows), yc
// (the result, n) and ctrl (done: every launch returns at once; solve_bad: set by a non-positive pivot).  k_bag_clear zeroes
// the lower triangle and row n_pad and sets the pad's diagonal; then `assemble` has to enqueue, on s, whatever writes the
// lower triangle of S and the right-hand side into row n_pad; then the factor, panel by panel, and the back-substitution.
// The stages are timed as solver_schur (clear and assembly), solver_factor and solver_subst.
void ba_blocked_solve(mslam_hip_ctx* c, const BaArgs& a, hipStream_t s, const std::function<void()>& assemble);

} // namespace mslam
