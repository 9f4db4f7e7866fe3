// pcg.hpp — the block-Jacobi preconditioned conjugate gradients of k_pcg.hip on a symmetric system kept as its non-zero 6 x 6
// blocks (SysLayout::Pairs of reduced_system.hpp): the third linear solver of mslam_hip_bundle_adjust_global
// (mslam_hip_set_ba_global_pcg) and of mslam_hip_pose_graph (mslam_hip_set_pose_graph_pcg).  The caller reaches pcg_solve
// through LinearSolve.  DESIGN.md 4.29, 4.30.
#pragma once
#include "trust_region.hpp"

#include <functional>

namespace mslam
{

constexpr int kPcgChunk = 10; // neighbours a wave of k_pcg_product takes per pass: 10 x 6 of its 64 lanes
constexpr int kPcgRows = 4;   // block rows per workgroup of k_pcg_product, a wave each
constexpr int kPcgBatch = 32; // CG iterations enqueued between two looks at the mapped word

// CG's state on the device.  A launch of CG iteration `it` (the host's count of enqueued iterations, whatever the device has
// decided) reads slot it & 1 and only thread 0 of workgroup 0 of the last launch writes slot (it + 1) & 1: no launch reads a
// word that the same launch writes.
struct PcgCtrl
{
    int32_t done[2], k[2]; // the solve has ended; iterations taken
    int32_t broke, pad;    // p . q was not > 0 or not finite (k_pcg_update of this iteration)
    double rz[2], bb;      // r . z; |b|^2
    mslam_hip_pcg_stats stats;
};

struct PcgArgs
{
    int n_free, n;              // block rows; 6 x n_free
    int n_prod_part, n_vec_part; // workgroups of k_pcg_product; of the vector kernels (256 entries each)
    int max_iterations;
    double tolerance;
    const int32_t *row_ptr, *nb_col, *nb_slot; // row i's neighbours, ascending, the diagonal in its place: column; 2 x block + transposed
    const double *S, *rhs;                     // 36 doubles per block, row-major inside; [n]
    double *minv;                              // [n_free] x 36: the inverses of the diagonal blocks
    double *x, *r, *z, *p, *q;                 // [n] each, r [2][n] (read it & 1, written (it + 1) & 1)
    double *part_pq, *part_rr, *part_rz;       // per-workgroup partial sums
    PcgCtrl* cg;
    TrCtrl* ctrl;    // done: every launch returns at once; solve_bad: a bad pivot of the preconditioner, a breakdown
    int32_t* h_done; // mapped: CG has ended
};

// One solve of S y = b, enqueued on s with looks at the context's mapped words in between: `assemble` has to enqueue whatever
// writes every block of S and rhs (stage solver_schur), then the preconditioner and the start (solver_precond), then CG
// iterations in batches of kPcgBatch until the device has ended it (solver_cg).  The stopping index is the device's; the
// looks only bound the launches that follow it.
int pcg_solve(mslam_hip_ctx* c, const PcgArgs& a, hipStream_t s, const std::function<void()>& assemble);

} // namespace mslam
