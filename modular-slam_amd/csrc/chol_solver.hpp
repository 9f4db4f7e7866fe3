// chol_solver.hpp — the blocked f64 Cholesky solve of k_chol.hip.  mslam_hip_bundle_adjust_global (k_ba.hip) solves its
// reduced camera system through it, mslam_hip_pose_graph (k_posegraph.hip) its damped normal equations, both with their DENSE
// solver and both through LinearSolve of reduced_system.hpp, whose SysView<SysLayout::PaddedLower> is the layout of S below.
#pragma once
#include "trust_region.hpp"

#include <functional>

namespace mslam
{

constexpr int kBagNB = 48; // panel width of the blocked factor: 8 keyframe blocks, 3 MFMA tiles

struct CholArgs
{
    int n, n_pad, ld; // the system's size; n rounded up to kBagNB; leading dimension n_pad + 16 (row n_pad: the right-hand side)
    double* S;        // n_pad columns of ld rows, column-major; only the lower triangle is read
    double* yc;       // the result, n
    TrCtrl* ctrl;     // done: every launch returns at once; solve_bad: set by a non-positive pivot
};

// One solve of S y = b, enqueued on s.  k_bag_clear zeroes the lower triangle and row n_pad and sets the pad's diagonal; then
// `assemble` has to enqueue, on s, whatever writes the lower triangle of S and the right-hand side into row n_pad; then the
// factor, panel by panel, and the back-substitution.  The stages are timed as solver_schur (clear and assembly),
// solver_factor and solver_subst.
void ba_blocked_solve(mslam_hip_ctx* c, const CholArgs& a, hipStream_t s, const std::function<void()>& assemble);

} // namespace mslam
