// reduced_system.hpp — what lies between the trust-region loop (trust_region.hpp) and the linear solvers of a symmetric
// system in 6 x 6 blocks (ba_blocked_solve of chol_solver.hpp, pg_sparse_solve of pg_sparse.hpp, pcg_solve of pcg.hpp), shared
// by k_ba.hip and k_posegraph.hip:
//   SysView      device: where entry (r, c) of the block of a pair and entry r of the right-hand side live, per layout
//   LinearSolve  host: the choice DENSE / SPARSE / PCG of one solve and what follows from it (cap, block index, staging, sizes,
//                solve)
//   tr_run_pcg   host: the trust-region loop of a solve with PCG, one iteration at a time
// DESIGN.md 4.17, 4.25, 4.26, 4.29, 4.30.
#pragma once
#include "chol_solver.hpp"
#include "pcg.hpp"
#include "pg_sparse.hpp"

namespace mslam
{

enum class SysLayout
{
    Full,        // n x n column-major, both halves written; the right-hand side in its own array (k_ba_solve)
    PaddedLower, // CholArgs: leading dimension ld, only the lower half written; the right-hand side is row n_pad
    Envelope,    // PgsArgs: blocks are positions in the chosen order; the right-hand side in its own array
    Pairs,       // PcgArgs: the pairs themselves, 36 doubles each, row-major inside: the diagonal block of block b is block b, a
                 // pair b1 < b2 is stored once, as the block of (b1, b2), where pair_slot says; the right-hand side in its own
                 // array.  Every entry of a diagonal block is written, both triangles
};

// The stores of an assembly kernel.  Args: BaArgs or PgArgs (S, rhs, n, n_pad, ld, env_off, env_first).
template <SysLayout kLayout>
struct SysView
{
    double *S, *rhs;
    size_t ld, n_pad;
    const int32_t *env_off, *env_first;
    size_t slot = 0; // Pairs: the block of this workgroup's pair

    // Pairs: a workgroup assembles pair blockIdx.x of the caller's list, and Args::pair_slot [n_pairs] names its block
    template <class Args>
    __device__ __forceinline__ explicit SysView(const Args& a)
        : S(a.S), rhs(a.rhs), ld(kLayout == SysLayout::Full ? (size_t)a.n : (size_t)a.ld), n_pad((size_t)a.n_pad), env_off(a.env_off),
          env_first(a.env_first)
    {
        if constexpr(kLayout == SysLayout::Pairs)
            slot = (size_t)a.pair_slot[blockIdx.x];
    }
    // the envelope's block of (row, col), row >= col: row-major inside
    __device__ __forceinline__ double* env_block(int row, int col) const { return S + (size_t)(env_off[row] + col - env_first[row]) * 36; }

    // entry (r, c) of the block of the pair (b1, b2); diag: b1 == b2.  The dense layouts keep an off-diagonal block in the lower
    // half as its transpose (Full in both halves); the envelope holds the block of (row, col) with row >= col, so a pair whose
    // first member comes later in the order is written transposed.  diag_lower: of a diagonal envelope block only c <= r.
    __device__ __forceinline__ void store(int b1, int b2, bool diag, int r, int c, double v, bool diag_lower = false) const
    {
        if constexpr(kLayout == SysLayout::Pairs)
            S[slot * 36 + r * 6 + c] = v; // b1 < b2 off the diagonal: the caller's pairs come in index order
        else if constexpr(kLayout == SysLayout::Envelope)
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

// One solve's linear solver.  The calls, in this order: the K cap; the caller's symbolic phase into sy (SPARSE); index (PCG:
// index_pairs); put after the caller's own puts, carve after its carves; grow_S; bind once the block is uploaded; solve in
// every iteration (PCG: solve_pcg, which synchronises and so is not called from tr_run).  With DENSE nothing is staged and sy
// stays empty.  PCG (pcg.hpp): sparse is false with it; the cap on CG's iterations and its tolerance are the caller's
// (mslam_hip_set_ba_global_pcg for the bundle adjustment, mslam_hip_set_pose_graph_pcg for the pose graph).
struct LinearSolve
{
    const bool sparse, pcg;
    const int cg_max_iterations; // PCG: CG iterations per solve at most; |r| <= cg_tolerance |b| ends it
    const double cg_tolerance;
    PgSymbolic sy;
    int n_free = 0, n = 0, n_pad = 0, ld = 0; // blocks; 6 x blocks; CholArgs's padded size and leading dimension
    size_t o_roff = 0, o_first = 0, o_cptr = 0, o_cblk = 0, o_crow = 0, o_rhs = 0, o_dinv = 0;
    CholArgs chol{}; // bind fills the one in use
    PgsArgs env{};
    // PCG: the stored blocks; per block row its neighbours in ascending order, the diagonal in its place, as column and
    // 2 x block + transposed; per pair of the caller's list its block
    int64_t blocks = 0;
    std::vector<int32_t> row_ptr, nb_col, nb_slot, pair_slot;
    PcgCtrl cg_ctrl{};
    PcgArgs cg{};
    size_t o_rptr = 0, o_ncol = 0, o_nslot = 0, o_pslot = 0, o_cg = 0, o_minv = 0, o_vec = 0, o_part = 0;

    explicit LinearSolve(bool sparse_, bool pcg_ = false, int cg_max_iterations_ = 0, double cg_tolerance_ = 0.0)
        : sparse(sparse_ && !pcg_), pcg(pcg_), cg_max_iterations(cg_max_iterations_), cg_tolerance(cg_tolerance_)
    {
    }
    // DENSE: (6 x 1024)^2 doubles = 302 MB of d_ba_S
    int k_max() const { return sparse || pcg ? MSLAM_HIP_POSE_GRAPH_MAX_KEYFRAMES_SPARSE : MSLAM_HIP_BA_GLOBAL_MAX_KEYFRAMES; }

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
    // PCG.  pairs: [.][2] members k1 <= k2 sorted by (k1, k2), each once, every diagonal pair of a block included; ci keeps the
    // index order.  The blocks: the n_free diagonal ones first, then the other pairs in list order.  No order, no envelope
    int index_pairs(mslam_hip_ctx* c, const char* who, const std::vector<int32_t>& pairs, const std::vector<int32_t>& ci, int n_free_)
    {
        n_free = n_free_, n = 6 * n_free;
        blocks = (int64_t)(pairs.size() / 2);
        if(blocks > MSLAM_HIP_POSE_GRAPH_MAX_ENVELOPE_BLOCKS)
            return fail(c, MSLAM_HIP_E_CAPACITY, std::string(who) + ": the reduced system has " + std::to_string(blocks) + " blocks, at most " +
                                                     std::to_string(MSLAM_HIP_POSE_GRAPH_MAX_ENVELOPE_BLOCKS) + " per solve");
        const size_t np = pairs.size() / 2;
        pair_slot.assign(np, 0);
        row_ptr.assign((size_t)n_free + 1, 0);
        for(size_t i = 0; i < np; ++i)
        {
            const int b1 = ci[(size_t)pairs[2 * i]], b2 = ci[(size_t)pairs[2 * i + 1]];
            ++row_ptr[(size_t)b1 + 1];
            if(b1 != b2)
                ++row_ptr[(size_t)b2 + 1];
        }
        for(int i = 0; i < n_free; ++i)
            row_ptr[(size_t)i + 1] += row_ptr[(size_t)i];
        nb_col.assign((size_t)row_ptr[(size_t)n_free], 0), nb_slot.assign((size_t)row_ptr[(size_t)n_free], 0);
        std::vector<int32_t> fill(row_ptr.begin(), row_ptr.end() - 1);
        int32_t off = n_free;
        // the list is sorted by (b1, b2): row b receives its earlier neighbours (as the second member, b1 ascending), then
        // its own pairs (b2 ascending from the diagonal on), so every row comes out ascending
        for(size_t i = 0; i < np; ++i)
        {
            const int b1 = ci[(size_t)pairs[2 * i]], b2 = ci[(size_t)pairs[2 * i + 1]];
            const int32_t slot = b1 == b2 ? b1 : off++;
            pair_slot[i] = slot;
            int32_t at = fill[(size_t)b1]++;
            nb_col[(size_t)at] = b2, nb_slot[(size_t)at] = 2 * slot;
            if(b1 != b2)
            {
                at = fill[(size_t)b2]++;
                nb_col[(size_t)at] = b1, nb_slot[(size_t)at] = 2 * slot + 1;
            }
        }
        return MSLAM_HIP_OK;
    }
    void put(TrStaging& st)
    {
        if(pcg)
        {
            o_rptr = st.put(row_ptr.data(), row_ptr.size() * 4), o_ncol = st.put(nb_col.data(), nb_col.size() * 4);
            o_nslot = st.put(nb_slot.data(), nb_slot.size() * 4), o_pslot = st.put(pair_slot.data(), pair_slot.size() * 4);
            o_cg = st.put(&cg_ctrl, sizeof(cg_ctrl)); // zeros: the statistics start there
            return;
        }
        o_roff = st.put(sy.row_off.data(), sy.row_off.size() * 4), o_first = st.put(sy.first.data(), sy.first.size() * 4);
        o_cptr = st.put(sy.col_ptr.data(), sy.col_ptr.size() * 4), o_cblk = st.put(sy.col_blk.data(), sy.col_blk.size() * 4);
        o_crow = st.put(sy.col_row.data(), sy.col_row.size() * 4);
    }
    // the factor's right-hand side, unless the caller has carved one (own_rhs: its offset), and 1 / diagonal; PCG: the inverses
    // of the diagonal blocks, r (twice), z, p, q, and the three rows of partial sums
    void carve(TrStaging& st, const size_t* own_rhs = nullptr)
    {
        o_rhs = own_rhs ? *own_rhs : st.carve(sparse || pcg ? (size_t)n * 8 : 0);
        o_dinv = st.carve(sparse ? (size_t)n * 8 : 0);
        if(!pcg)
            return;
        o_minv = st.carve((size_t)n_free * 288), o_vec = st.carve((size_t)n * 8 * 5);
        o_part = st.carve(((size_t)pcg_prod_parts() + 2 * (size_t)pcg_vec_parts()) * 8);
    }
    int pcg_prod_parts() const { return (n_free + kPcgRows - 1) / kPcgRows; }
    int pcg_vec_parts() const { return (n + 255) / 256; }
    hipError_t grow_S(mslam_hip_ctx* c)
    {
        return grow(c->d_ba_S, pcg ? (size_t)blocks * 36 : sparse ? (size_t)sy.blocks * 36 : (size_t)ld * n_pad, c->stream);
    }
    // d: the uploaded block (the control block at 0); S is the context's d_ba_S; yc: the solution, n
    void bind(mslam_hip_ctx* c, uint8_t* d, double* yc)
    {
        auto dbl = [&](size_t at) { return reinterpret_cast<double*>(d + at); };
        auto i32 = [&](size_t at) { return reinterpret_cast<const int32_t*>(d + at); };
        TrCtrl* ctrl = reinterpret_cast<TrCtrl*>(d);
        if(pcg)
        {
            double *v = dbl(o_vec), *part = dbl(o_part);
            const size_t nn = (size_t)n;
            cg = PcgArgs{n_free, n, pcg_prod_parts(), pcg_vec_parts(), cg_max_iterations, cg_tolerance, i32(o_rptr), i32(o_ncol),
                         i32(o_nslot), c->d_ba_S.get(), dbl(o_rhs), dbl(o_minv), yc, v, v + 2 * nn, v + 3 * nn, v + 4 * nn, part,
                         part + pcg_prod_parts(), part + pcg_prod_parts() + pcg_vec_parts(), reinterpret_cast<PcgCtrl*>(d + o_cg), ctrl,
                         c->h_ba.dev() + 1};
        }
        else if(sparse)
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
    // PCG: assemble enqueues the caller's assembly kernel for Pairs.  Synchronises the stream; a MSLAM_HIP_* status
    int solve_pcg(mslam_hip_ctx* c, hipStream_t s, const std::function<void()>& assemble) const { return pcg_solve(c, cg, s, assemble); }
};

// tr_run for a solve with PCG.  tr_run enqueues kTrBatch iterations blind; with a CG of unknown length inside that is
// thousands of launches that do nothing, so one trust-region iteration is driven at a time: `before` (the launches up to the
// check kernel), pcg_solve with `assemble` where the factor stands (it looks at the mapped words between batches of CG
// iterations; skipped when the problem has no system: !has_system), `after` (the step's launches), then a look at the
// termination word.  Every decision is the device's; the looks only bound the launches that follow it.  At the end the
// control block fills `sum` and, where a system was formed, CG's statistics come back into *stats.  `stage` names the timed
// stage of an iteration, `who` the entry point in the error
inline int tr_run_pcg(mslam_hip_ctx* c, const char* stage, const char* who, const TrCtrl* d_ctrl, const LinearSolve& ls, bool has_system,
                      int max_iterations, const std::function<void()>& before, const std::function<void()>& assemble,
                      const std::function<void()>& after, mslam_hip_pcg_stats* stats, mslam_hip_ba_summary& sum)
{
    hipStream_t s = c->stream;
    // iteration max_iterations + 1 only reaches the check kernel, which ends the solve with NO_CONVERGENCE
    for(long long it = 0; it <= max_iterations; ++it)
    {
        StageScope ts(c, stage);
        before();
        if(has_system)
            if(const int rc = ls.solve_pcg(c, s, assemble); rc != MSLAM_HIP_OK)
                return rc;
        after();
        MSLAM_CHK(c, hipGetLastError());
        MSLAM_CHK(c, hipStreamSynchronize(s));
        if(*static_cast<volatile int32_t*>(c->h_ba.get()))
            break;
    }
    TrCtrl ctrl;
    MSLAM_CHK(c, hipMemcpyAsync(&ctrl, d_ctrl, sizeof(ctrl), hipMemcpyDeviceToHost, s));
    if(has_system)
        MSLAM_CHK(c, hipMemcpyAsync(stats, &ls.cg.cg->stats, sizeof(*stats), hipMemcpyDeviceToHost, s));
    MSLAM_CHK(c, hipStreamSynchronize(s));
    if(!ctrl.done)
        return fail(c, MSLAM_HIP_E_RUNTIME, std::string(who) + ": the kernels left no termination");
    sum.termination = ctrl.termination, sum.iterations = ctrl.iteration;
    sum.rejected_steps = ctrl.rejected, sum.invalid_steps = ctrl.invalid_total;
    sum.initial_cost = ctrl.initial_cost, sum.final_cost = ctrl.x_cost;
    return MSLAM_HIP_OK;
}

} // namespace mslam
