// pg_sparse.hpp — the block-envelope (skyline) Cholesky solve of k_pg_sparse.hip: mslam_hip_pose_graph's second linear solver
// (MSLAM_HIP_PG_SOLVER_SPARSE), mslam_hip_bundle_adjust_global's (MSLAM_HIP_BA_GLOBAL_SOLVER_SPARSE), and the symbolic phase the
// two *_analyze entry points expose.  The callers reach pg_sparse_solve through LinearSolve and address the envelope through
// SysView<SysLayout::Envelope> (both reduced_system.hpp).  DESIGN.md 4.25, 4.26.
#pragma once
#include "trust_region.hpp"

#include <functional>

namespace mslam
{

// The symbolic phase of one solve, host only.  Nodes are the free poses that have an edge; position i of the chosen order
// is block row i of the factor.
struct PgSymbolic
{
    int n_free = 0, ordering = 0; // ordering: 0 NATURAL, 1 RCM
    int64_t blocks = 0;           // the envelope of the chosen order in 6 x 6 blocks, diagonal included
    std::vector<int32_t> order;   // [n_free] pose index per position
    std::vector<int32_t> first;   // [n_free] the least position among row i's neighbours and i itself
    // the layout (pg_layout): row i holds the blocks of columns first[i] .. i from block row_off[i] on; column j's rows below
    // the diagonal, ascending, as the block of (row, j) and the row, from col_ptr[j] on
    std::vector<int32_t> row_off, col_ptr, col_blk, col_row;
};

// the orders and the envelope; the caller has checked K, E, the indices and the self-edges.  node_mask (K flags, or nullptr):
// the nodes are the free poses it marks, with or without an edge (mslam_hip_bundle_adjust_global's SPARSE solver: a free
// keyframe that shares no landmark is still a row, of degree 0); without it, the free poses that have an edge.  E is a
// size_t's worth there: a covisibility graph has more edges than a pose graph may
void pg_symbolic(const uint8_t* fixed, int K, const int32_t* edge_a, const int32_t* edge_b, size_t E, PgSymbolic& sy,
                 const uint8_t* node_mask = nullptr);
// row offsets and column lists of an envelope that fits MSLAM_HIP_POSE_GRAPH_MAX_ENVELOPE_BLOCKS
void pg_layout(PgSymbolic& sy);
// the tail of the two *_analyze entry points: copies out through pointers that may be NULL; MSLAM_HIP_E_CAPACITY for an
// envelope above the bound, MSLAM_HIP_OK otherwise
int pg_symbolic_out(const PgSymbolic& sy, int32_t* order, int32_t* first, int* n_free, int* ordering, int64_t* envelope_blocks);

struct PgsArgs
{
    int n;          // block rows
    int64_t blocks; // the envelope
    const int32_t *row_off, *first, *col_ptr, *col_blk, *col_row;
    double* S;    // the envelope, 36 doubles per block, row-major inside a block (the context's d_ba_S)
    double* rhs;  // [6 n] the right-hand side; y = L^-1 b after the factor
    double* dinv; // [6 n] 1 / diagonal of L
    double* yc;   // [6 n] the solution
    TrCtrl* ctrl; // done: every launch returns at once; solve_bad: set by a pivot that is not finite or not > 0
};

// One solve of S y = b, enqueued on s: the clear, then `assemble` has to enqueue whatever writes the envelope and rhs, then
// the factor with the forward substitution (one workgroup), then the back-substitution (one workgroup).  The stages are
// timed under ba_blocked_solve's names: solver_schur, solver_factor, solver_subst.
void pg_sparse_solve(mslam_hip_ctx* c, const PgsArgs& a, hipStream_t s, const std::function<void()>& assemble);

// ---- k_pg_cov.hip: the blocks of the inverse inside the envelope (mslam_hip_pose_graph_covariance) ----------

// the clear, `assemble` and the factor of pg_sparse_solve without the back-substitution: the envelope then holds L
void pg_sparse_factor(mslam_hip_ctx* c, const PgsArgs& a, hipStream_t s, const std::function<void()>& assemble);

// what k_pg_cov_gather reads; the members SysView<SysLayout::Envelope> takes have PgArgs's names
struct PgCovArgs
{
    int n, n_pad, ld; // SysView's; only the envelope's members are read
    double *S, *rhs;
    const int32_t *env_off, *env_first;
    const int32_t* ci;  // [K] position in the chosen order, -1: constant (the host rejects a free pose without an edge)
    const double* sc;   // [K] x 6 the Jacobi scaling of the factor
    const int32_t* req; // [n_req][2] poses (a, b) per output block; a == b for a marginal
    int n_req;
    double* out;        // [n_req] x 36 row-major, then one word: solve_bad as 0.0 / 1.0
    const TrCtrl* ctrl;
};

// After the factor, enqueued on s: k_pgs_selinv (one workgroup; the envelope then holds the blocks of the inverse; scratch
// takes 36 doubles per row of the longest column list), then k_pg_cov_gather.  Stages cov_selinv, cov_gather.
void pg_cov_enqueue(mslam_hip_ctx* c, const PgsArgs& env, const PgCovArgs& cov, double* scratch, hipStream_t s);

} // namespace mslam
