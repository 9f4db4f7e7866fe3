// k_pcg.hip — block-Jacobi preconditioned conjugate gradients on a symmetric positive definite system in 6 x 6 blocks, kept as
// its non-zero blocks (SysLayout::Pairs of reduced_system.hpp: diagonal blocks first, every off-diagonal pair once) with a
// list of neighbours per block row.  mslam_hip_bundle_adjust_global runs it on its reduced camera system after
// mslam_hip_set_ba_global_pcg, mslam_hip_pose_graph on its normal equations after mslam_hip_set_pose_graph_pcg; pcg.hpp has the
// arguments and the control block.  DESIGN.md 4.29, 4.30.
//
//   x = 0, r = b, z = M^-1 r, p = z;  per iteration  q = S p, alpha = r.z / p.q, x += alpha p, r -= alpha q, z = M^-1 r,
//   stop at |r| <= tol |b| or at the cap, else beta = r.z / (r.z)_old, p = z + beta p
//
// with M the block diagonal of S.  Launches of one solve, every one returning at once when the trust-region loop has ended:
//   k_pcg_precond    a lane per block row: Cholesky and inverse of the 6 x 6 diagonal block
//   k_pcg_start      a lane per entry: x, r, z, p and the partials of |b|^2 and r.z
//   k_pcg_begin      one workgroup: sums them, fills the control block; b = 0 ends the solve with x = 0
// and three per CG iteration, every one returning at once when CG has ended:
//   k_pcg_product    a wave per block row: q_i = sum_j S_ij p_j over the row's list in passes of kPcgChunk neighbours, lane
//                    (g, r) keeping row r of every kPcgChunk-th neighbour from the g-th on, then the ten lanes of a row in
//                    order; the partial of p.q per workgroup
//   k_pcg_update     a lane per entry: alpha from the partials, x, r, z; the partials of |r|^2 and r.z
//   k_pcg_direction  a lane per entry: the decision from the partials, then p; thread 0 of workgroup 0 writes the next
//                    control slot
// Every workgroup that needs a scalar sums the partials itself, in one order (pcg_sum), so all of them hold the same bits.
// No atomics; no kernel waits on another workgroup; every loop is bounded by a count the host computed.  All arithmetic f64.
#include "pcg.hpp"

namespace mslam
{

// the sum of `count` partials in every thread of a workgroup of 256: thread t takes t, t + 256, ... in order, then block_sum's
// fixed tree, whose result every thread computes from the same four words
__device__ __forceinline__ double pcg_sum(const double* __restrict__ part, int count, double* red)
{
    double s = 0.0;
    for(int i = threadIdx.x; i < count; i += 256)
        s += part[i];
    return block_sum(s, red);
}

__global__ __launch_bounds__(256) void k_pcg_precond(PcgArgs a)
{
    TrCtrl* ct = a.ctrl;
    if(ct->done)
        return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if(i >= a.n_free)
        return;
    // block i is the diagonal block of row i; its lower triangle is read
    const double* B = a.S + (size_t)i * 36;
    double L[6][6], Li[6][6];
    bool bad = false;
    for(int j = 0; j < 6; ++j)
    {
        double v = B[j * 6 + j];
        for(int k = 0; k < j; ++k)
            v -= L[j][k] * L[j][k];
        if(!(v > 0.0) || !isfinite(v))
            bad = true; // the step is invalid; the factor goes on with bounded values
        const double d = sqrt(fmax(v, DBL_MIN));
        L[j][j] = d;
        for(int r = j + 1; r < 6; ++r)
        {
            double w = B[r * 6 + j];
            for(int k = 0; k < j; ++k)
                w -= L[r][k] * L[j][k];
            L[r][j] = w / d;
        }
    }
    // Li = L^-1 (lower), column by column
    for(int c = 0; c < 6; ++c)
        for(int r = 0; r < 6; ++r)
        {
            if(r < c)
            {
                Li[r][c] = 0.0;
                continue;
            }
            double w = r == c ? 1.0 : 0.0;
            for(int k = c; k < r; ++k)
                w -= L[r][k] * Li[k][c];
            Li[r][c] = w / L[r][r];
        }
    // M^-1 = L^-T L^-1, one triangle computed and mirrored
    double* Mi = a.minv + (size_t)i * 36;
    for(int r = 0; r < 6; ++r)
        for(int c = r; c < 6; ++c)
        {
            double w = 0.0;
            for(int k = c; k < 6; ++k)
                w += Li[k][r] * Li[k][c];
            Mi[r * 6 + c] = w;
            Mi[c * 6 + r] = w;
        }
    if(bad)
        ct->solve_bad = 1;
}

// z_e = row (e mod 6) of the block's M^-1 times the block's six entries of v
__device__ __forceinline__ double pcg_precondition(const double* __restrict__ Mi, int c, const double v[6])
{
    double z = 0.0;
    for(int j = 0; j < 6; ++j)
        z += Mi[c * 6 + j] * v[j];
    return z;
}

__global__ __launch_bounds__(256) void k_pcg_start(PcgArgs a)
{
    __shared__ double red[4];
    if(a.ctrl->done)
        return;
    const int e = blockIdx.x * 256 + threadIdx.x;
    double bb = 0.0, rz = 0.0;
    if(e < a.n)
    {
        const int row = e / 6, c = e % 6;
        double v[6];
        for(int j = 0; j < 6; ++j)
            v[j] = a.rhs[(size_t)row * 6 + j];
        const double z = pcg_precondition(a.minv + (size_t)row * 36, c, v);
        a.x[e] = 0.0, a.r[e] = v[c], a.z[e] = z, a.p[e] = z;
        bb = v[c] * v[c], rz = v[c] * z;
    }
    bb = block_sum(bb, red), rz = block_sum(rz, red);
    if(threadIdx.x == 0)
        a.part_rr[blockIdx.x] = bb, a.part_rz[blockIdx.x] = rz;
}

__global__ __launch_bounds__(256) void k_pcg_begin(PcgArgs a)
{
    __shared__ double red[4];
    const TrCtrl* ct = a.ctrl;
    if(ct->done)
        return;
    const double bb = pcg_sum(a.part_rr, a.n_vec_part, red), rz = pcg_sum(a.part_rz, a.n_vec_part, red);
    if(threadIdx.x != 0)
        return;
    PcgCtrl* cg = a.cg;
    // b = 0: x = 0 is the solution.  A bad pivot of the preconditioner has made the step invalid already
    const int32_t end = bb == 0.0 || ct->solve_bad ? 1 : 0;
    cg->done[0] = end, cg->done[1] = end, cg->k[0] = 0, cg->k[1] = 0, cg->broke = 0;
    cg->rz[0] = rz, cg->rz[1] = rz, cg->bb = bb;
    cg->stats.solves += 1;
    if(end)
        *a.h_done = 1;
}

__global__ __launch_bounds__(64 * kPcgRows) void k_pcg_product(PcgArgs a, int it)
{
    __shared__ double red[kPcgRows];
    if(a.ctrl->done || a.cg->done[it & 1])
        return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * kPcgRows + wave;
    const bool row = i < a.n_free;
    const int g = lane / 6, r = lane % 6;
    double acc = 0.0;
    if(row && g < kPcgChunk)
        for(int at = a.row_ptr[i] + g; at < a.row_ptr[i + 1]; at += kPcgChunk)
        {
            const int slot2 = a.nb_slot[at];
            const double* B = a.S + (size_t)(slot2 >> 1) * 36;
            const double* pj = a.p + (size_t)a.nb_col[at] * 6;
            double s = 0.0;
            if(slot2 & 1) // the stored block is the pair's (column's row, this row): its transpose is read
                for(int c = 0; c < 6; ++c)
                    s += B[c * 6 + r] * pj[c];
            else
                for(int c = 0; c < 6; ++c)
                    s += B[r * 6 + c] * pj[c];
            acc += s;
        }
    // lanes 0..5: q_r, the ten lanes of row r in order
    double q = 0.0;
    for(int k = 0; k < kPcgChunk; ++k)
        q += __shfl(acc, k * 6 + r, 64);
    const bool mine = row && lane < 6;
    const double d = mine ? a.p[(size_t)i * 6 + r] * q : 0.0;
    double pq = 0.0;
    for(int k = 0; k < 6; ++k)
        pq += __shfl(d, k, 64);
    if(mine)
        a.q[(size_t)i * 6 + r] = q;
    if(lane == 0)
        red[wave] = pq; // 0 for a wave past the last row
    __syncthreads();
    if(threadIdx.x == 0)
        a.part_pq[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}
static_assert(kPcgRows == 4 && kPcgChunk * 6 <= 64, "k_pcg_product's lane layout and its sum over the waves");

__global__ __launch_bounds__(256) void k_pcg_update(PcgArgs a, int it)
{
    __shared__ double red[4];
    PcgCtrl* cg = a.cg;
    if(a.ctrl->done || cg->done[it & 1])
        return;
    const double pq = pcg_sum(a.part_pq, a.n_prod_part, red);
    if(!(pq > 0.0) || !isfinite(pq))
    {
        // a breakdown: every workgroup sees the same bits and leaves; k_pcg_direction ends the solve
        if(blockIdx.x == 0 && threadIdx.x == 0)
            cg->broke = 1;
        return;
    }
    const double alpha = cg->rz[it & 1] / pq;
    const double* r_in = a.r + (size_t)(it & 1) * a.n;
    double* r_out = a.r + (size_t)((it + 1) & 1) * a.n;
    const int e = blockIdx.x * 256 + threadIdx.x;
    double rr = 0.0, rz = 0.0;
    if(e < a.n)
    {
        const int row = e / 6, c = e % 6;
        double v[6]; // the block's six entries of the new r: every lane of the block computes the same six
        for(int j = 0; j < 6; ++j)
            v[j] = r_in[(size_t)row * 6 + j] - alpha * a.q[(size_t)row * 6 + j];
        const double z = pcg_precondition(a.minv + (size_t)row * 36, c, v);
        a.x[e] = a.x[e] + alpha * a.p[e];
        r_out[e] = v[c], a.z[e] = z;
        rr = v[c] * v[c], rz = v[c] * z;
    }
    rr = block_sum(rr, red), rz = block_sum(rz, red);
    if(threadIdx.x == 0)
        a.part_rr[blockIdx.x] = rr, a.part_rz[blockIdx.x] = rz;
}

__global__ __launch_bounds__(256) void k_pcg_direction(PcgArgs a, int it)
{
    __shared__ double red[4];
    PcgCtrl* cg = a.cg;
    TrCtrl* ct = a.ctrl;
    if(ct->done)
        return;
    const int cur = it & 1, next = (it + 1) & 1;
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if(cg->done[cur])
    {
        if(first)
            cg->done[next] = 1;
        return;
    }
    const int k = cg->k[cur];
    if(cg->broke)
    {
        if(first)
        {
            cg->done[next] = 1, cg->k[next] = k;
            ct->solve_bad = 1;
            cg->stats.breakdowns += 1, cg->stats.iterations += k;
            cg->stats.longest = cg->stats.longest > k ? cg->stats.longest : k;
            *a.h_done = 1;
        }
        return;
    }
    const double rr = pcg_sum(a.part_rr, a.n_vec_part, red), rz = pcg_sum(a.part_rz, a.n_vec_part, red);
    const int k1 = k + 1;
    const bool converged = sqrt(rr) <= a.tolerance * sqrt(cg->bb);
    const bool at_cap = !converged && k1 >= a.max_iterations; // the iterate is taken
    const bool end = converged || at_cap;
    if(first)
    {
        cg->done[next] = end ? 1 : 0, cg->k[next] = k1, cg->rz[next] = rz;
        if(end)
        {
            cg->stats.iterations += k1, cg->stats.at_cap += at_cap ? 1 : 0;
            cg->stats.longest = cg->stats.longest > k1 ? cg->stats.longest : k1;
            *a.h_done = 1;
        }
    }
    if(end)
        return;
    const double beta = rz / cg->rz[cur];
    const int e = blockIdx.x * 256 + threadIdx.x;
    if(e < a.n)
        a.p[e] = a.z[e] + beta * a.p[e];
}

int pcg_solve(mslam_hip_ctx* c, const PcgArgs& a, hipStream_t s, const std::function<void()>& assemble)
{
    volatile int32_t* h = c->h_ba.get(); // [0] the trust-region loop has ended, [1] CG has
    h[1] = 0;
    {
        // every stored block and every entry of rhs has one writer, which writes all of it: nothing is cleared
        StageScope ts(c, "solver_schur");
        assemble();
    }
    const dim3 g_vec((unsigned)a.n_vec_part), g_prod((unsigned)a.n_prod_part);
    {
        StageScope ts(c, "solver_precond");
        hipLaunchKernelGGL(k_pcg_precond, dim3((unsigned)((a.n_free + 255) / 256)), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_pcg_start, g_vec, dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_pcg_begin, dim3(1), dim3(256), 0, s, a);
    }
    for(int it = 0; it < a.max_iterations;)
    {
        StageScope ts(c, "solver_cg");
        for(int b = 0; b < kPcgBatch && it < a.max_iterations; ++b, ++it)
        {
            hipLaunchKernelGGL(k_pcg_product, g_prod, dim3(64 * kPcgRows), 0, s, a, it);
            hipLaunchKernelGGL(k_pcg_update, g_vec, dim3(256), 0, s, a, it);
            hipLaunchKernelGGL(k_pcg_direction, g_vec, dim3(256), 0, s, a, it);
        }
        MSLAM_CHK(c, hipGetLastError());
        MSLAM_CHK(c, hipStreamSynchronize(s));
        if(h[0] || h[1])
            break;
    }
    return MSLAM_HIP_OK;
}

} // namespace mslam
