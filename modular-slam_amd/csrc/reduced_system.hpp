// reduced_system.hpp — what lies between the trust-region loop (trust_region.hpp) and the two factorisations of a symmetric
// system in 6 x 6 blocks (ba_blocked_solve of chol_solver.hpp, pg_sparse_solve of pg_sparse.hpp), shared by k_ba.hip and
// k_posegraph.hip:
//   SysView      device: where entry (r, c) of the block of a pair and entry r of the right-hand side live, per layout
//   LinearSolve  host: the choice DENSE / SPARSE of one solve and what follows from it (cap, block index, staging, sizes, solve)
// DESIGN.md 4.17, 4.25, 4.26.
#pragma once
#include "chol_solver.hpp"
#include "pg_sparse.hpp"

namespace mslam
{

enum class SysLayout
{
    Full,        // n x n column-major, both halves written; the right-hand side in its own array (k_ba_solve)
    PaddedLower, // CholArgs: leading dimension ld, only the lower half written; the right-hand side is row n_pad
    Envelope,    // PgsArgs: blocks are positions in the chosen order; the right-hand side in its own array
};

// The stores of an assembly kernel.  Args: BaArgs or PgArgs (S, rhs, n, n_pad, ld, env_off, env_first).
template <SysLayout kLayout>
struct SysView
{
    double *S, *rhs;
    size_t ld, n_pad;
    const int32_t *env_off, *env_first;

    template <class Args>
    __device__ __forceinline__ explicit SysView(const Args& a)
        : S(a.S), rhs(a.rhs), ld(kLayout == SysLayout::Full ? (size_t)a.n : (size_t)a.ld), n_pad((size_t)a.n_pad), env_off(a.env_off),
          env_first(a.env_first)
    {
    }
    // the envelope's block of (row, col), row >= col: row-major inside
    __device__ __forceinline__ double* env_block(int row, int col) const { return S + (size_t)(env_off[row] + col - env_first[row]) * 36; }

    // entry (r, c) of the block of the pair (b1, b2); diag: b1 == b2.  The dense layouts keep an off-diagonal block in the lower
    // half as its transpose (Full in both halves); the envelope holds the block of (row, col) with row >= col, so a pair whose
    // first member comes later in the order is written transposed.  diag_lower: of a diagonal envelope block only c <= r.
    __device__ __forceinline__ void store(int b1, int b2, bool diag, int r, int c, double v, bool diag_lower = false) const
    {
        if constexpr(kLayout == SysLayout::Envelope)
        {
            if(diag)
            {
                if(!diag_lower || c <= r)
                    env_block(b1, b1)[r * 6 + c] = v;
            }
            else if(b2 > b1)
                env_block(b2, b1)[c * 6 + r] = v;
            else
                env_block(b1, b2)[r * 6 + c] = v;
        }
        else
        {
            const size_t row = (size_t)b1 * 6 + r, col = (size_t)b2 * 6 + c;
            if(kLayout == SysLayout::Full || diag)
                S[row + col * ld] = v;
            if(!diag)
                S[col + row * ld] = v;
        }
    }
    // entry r of the right-hand side of block b
    __device__ __forceinline__ void store_rhs(int b, int r, double v) const
    {
        if constexpr(kLayout == SysLayout::PaddedLower)
            S[n_pad + ((size_t)b * 6 + r) * ld] = v;
        else
            rhs[(size_t)b * 6 + r] = v;
    }
};

static_assert(MSLAM_HIP_BA_GLOBAL_MAX_KEYFRAMES_SPARSE == MSLAM_HIP_POSE_GRAPH_MAX_KEYFRAMES_SPARSE, "one K cap per solver");

// One solve's linear solver.  The calls, in this order: the K cap; the caller's symbolic phase into sy (SPARSE); index; put
// after the caller's own puts, carve after its carves; grow_S; bind once the block is uploaded; solve in every iteration.
// With DENSE nothing is staged and sy stays empty.
struct LinearSolve
{
    const bool sparse;
    PgSymbolic sy;
    int n_free = 0, n = 0, n_pad = 0, ld = 0; // blocks; 6 x blocks; CholArgs's padded size and leading dimension
    size_t o_roff = 0, o_first = 0, o_cptr = 0, o_cblk = 0, o_crow = 0, o_rhs = 0, o_dinv = 0;
    CholArgs chol{}; // bind fills the one in use
    PgsArgs env{};

    explicit LinearSolve(bool sparse_) : sparse(sparse_) {}
    // DENSE: (6 x 1024)^2 doubles = 302 MB of d_ba_S
    int k_max() const { return sparse ? MSLAM_HIP_POSE_GRAPH_MAX_KEYFRAMES_SPARSE : MSLAM_HIP_BA_GLOBAL_MAX_KEYFRAMES; }

    // ci: the blocks in index order, n_free of them, -1 outside the system; with SPARSE it becomes the position in sy.order
    int index(mslam_hip_ctx* c, const char* who, std::vector<int32_t>& ci, int n_free_)
    {
        n_free = n_free_, n = 6 * n_free;
        n_pad = (n + kBagNB - 1) / kBagNB * kBagNB, ld = n_pad + 16;
        if(!sparse)
            return MSLAM_HIP_OK;
        if(sy.blocks > MSLAM_HIP_POSE_GRAPH_MAX_ENVELOPE_BLOCKS)
            return fail(c, MSLAM_HIP_E_CAPACITY, std::string(who) + ": the envelope needs " + std::to_string(sy.blocks) + " blocks, at most " +
                                                     std::to_string(MSLAM_HIP_POSE_GRAPH_MAX_ENVELOPE_BLOCKS) + " per solve");
        pg_layout(sy);
        for(int i = 0; i < n_free; ++i)
            ci[(size_t)sy.order[(size_t)i]] = i;
        return MSLAM_HIP_OK;
    }
    void put(TrStaging& st)
    {
        o_roff = st.put(sy.row_off.data(), sy.row_off.size() * 4), o_first = st.put(sy.first.data(), sy.first.size() * 4);
        o_cptr = st.put(sy.col_ptr.data(), sy.col_ptr.size() * 4), o_cblk = st.put(sy.col_blk.data(), sy.col_blk.size() * 4);
        o_crow = st.put(sy.col_row.data(), sy.col_row.size() * 4);
    }
    // the factor's right-hand side, unless the caller has carved one (own_rhs: its offset), and 1 / diagonal
    void carve(TrStaging& st, const size_t* own_rhs = nullptr)
    {
        o_rhs = own_rhs ? *own_rhs : st.carve(sparse ? (size_t)n * 8 : 0);
        o_dinv = st.carve(sparse ? (size_t)n * 8 : 0);
    }
    hipError_t grow_S(mslam_hip_ctx* c) { return grow(c->d_ba_S, sparse ? (size_t)sy.blocks * 36 : (size_t)ld * n_pad, c->stream); }
    // d: the uploaded block (the control block at 0); S is the context's d_ba_S; yc: the solution, n
    void bind(mslam_hip_ctx* c, uint8_t* d, double* yc)
    {
        auto dbl = [&](size_t at) { return reinterpret_cast<double*>(d + at); };
        auto i32 = [&](size_t at) { return reinterpret_cast<const int32_t*>(d + at); };
        TrCtrl* ctrl = reinterpret_cast<TrCtrl*>(d);
        if(sparse)
            env = PgsArgs{n_free, sy.blocks, i32(o_roff), i32(o_first), i32(o_cptr), i32(o_cblk), i32(o_crow), c->d_ba_S.get(), dbl(o_rhs), dbl(o_dinv), yc, ctrl};
        else
            chol = CholArgs{n, n_pad, ld, c->d_ba_S.get(), yc, ctrl};
    }
    // assemble: enqueues the caller's assembly kernel for the layout in use (Envelope with SPARSE, PaddedLower with DENSE)
    void solve(mslam_hip_ctx* c, hipStream_t s, const std::function<void()>& assemble) const
    {
        if(sparse)
            pg_sparse_solve(c, env, s, assemble);
        else
            ba_blocked_solve(c, chol, s, assemble);
    }
};

} // namespace mslam
