// k_pg_cov.hip — marginal covariances of the pose graph: the blocks of Z = A^-1 inside the block envelope of A = L L^T
// (k_pg_sparse.hip's factor), by the Takahashi / Erisman-Tinney recursion, and their read-out.  mslam_hip_pose_graph_covariance
// (k_posegraph.hip) enqueues the undamped assembly and the factor in front.  DESIGN.md 4.28; include/mslam_hip.h has the
// semantics.
//
// A Cholesky pattern is closed under the recursion: with R the rows below the diagonal of column i (its list col_row), every
// pair (j, k) of R lies inside the envelope (first[max] <= i < min), so column i of Z follows from blocks of later columns:
//     G_k  = L_ki L_ii^-1                                   k in R
//     Z_ji = - sum_{k in R} Z_jk G_k                        j in R
//     Z_ii = L_ii^-T L_ii^-1 - sum_{k in R} G_k^T Z_ki
// The pairs (j, k) are the pairs of the factor's trailing update of column i.
//
//   k_pgs_selinv     ONE workgroup of 256 walks the block columns from the last to the first (the chain of dependencies is the
//                    factor's, backwards).  For column i:
//                      1. every thread inverts L_ii in registers (W, the same bits everywhere); G_k = L_ki W, a thread per row
//                         of a block, in place over L_ki;  barrier
//                      2. Z_ji into the column scratch, a thread per entry, k ascending; Z_jk is read from the envelope at
//                         (j, k), or as the transpose of (k, j);  barrier
//                      3. Z_ii, a thread per entry of the lower triangle, k ascending, into a register;  barrier (these
//                         threads read the G_k the copy below writes over)
//                      4. Z_ii stored with its mirror; the scratch copied over the column;  barrier
//   k_pg_cov_gather  a thread per output entry: the block of (a, b) from the envelope (transposed when a comes first in the
//                    order), the Jacobi scaling undone, zeros for a constant pose; thread 0 copies solve_bad behind the blocks,
//                    so the call has one download.
// No atomics, one order of every sum, all arithmetic f64; no kernel waits on another workgroup; every loop is bounded by a
// count the host computed (n, the lists' lengths).
#include "reduced_system.hpp"

namespace mslam
{

__device__ __forceinline__ int pgc_tri(int r, int c) { return r * (r + 1) / 2 + c; } // c <= r < 6

__global__ __launch_bounds__(256) void k_pgs_selinv(PgsArgs a, double* __restrict__ scratch)
{
    const TrCtrl* ct = a.ctrl;
    if(ct->done || ct->solve_bad)
        return; // a pivot was not > 0 or not finite: the call reports it, nothing is read out
    const int t = threadIdx.x;
    for(int i = a.n - 1; i >= 0; --i)
    {
        // 1. W = L_ii^-1, lower triangular: column c by forward substitution on e_c
        double* D = a.S + (size_t)(a.row_off[i] + i - a.first[i]) * 36;
        double Ld[21], W[21];
#pragma unroll
        for(int r = 0; r < 6; ++r)
#pragma unroll
            for(int c = 0; c <= r; ++c)
                Ld[pgc_tri(r, c)] = D[r * 6 + c];
#pragma unroll
        for(int c = 0; c < 6; ++c)
#pragma unroll
            for(int r = c; r < 6; ++r)
            {
                double s = r == c ? 1.0 : 0.0;
#pragma unroll
                for(int k = c; k < r; ++k)
                    s -= Ld[pgc_tri(r, k)] * W[pgc_tri(k, c)];
                W[pgc_tri(r, c)] = s * a.dinv[(size_t)i * 6 + r];
            }
        const int cp = a.col_ptr[i], m = a.col_ptr[i + 1] - cp;
        for(int w = t; w < 6 * m; w += 256)
        {
            double* P = a.S + (size_t)a.col_blk[cp + w / 6] * 36 + (w % 6) * 6;
            double x[6];
#pragma unroll
            for(int c = 0; c < 6; ++c)
                x[c] = P[c];
#pragma unroll
            for(int c = 0; c < 6; ++c)
            {
                double s = 0.0;
#pragma unroll
                for(int k = c; k < 6; ++k)
                    s += x[k] * W[pgc_tri(k, c)];
                P[c] = s;
            }
        }
        __syncthreads();
        // 2. Z_ji = - sum_k Z_jk G_k: entry (r, c) of the j-th row of the list
        for(int w = t; w < 36 * m; w += 256)
        {
            const int j = w / 36, e = w % 36, r = e / 6, c = e % 6;
            const int bj = a.col_blk[cp + j], rj = a.col_row[cp + j];
            double s = 0.0;
            for(int k = 0; k < m; ++k)
            {
                const int bk = a.col_blk[cp + k], rk = a.col_row[cp + k];
                const double* G = a.S + (size_t)bk * 36 + c;
                // block (j, k) of the envelope lies (rk - i) blocks after (j, i); for k > j it is (k, j), read transposed
                const double* Z = k <= j ? a.S + (size_t)(bj + (rk - i)) * 36 + r * 6 : a.S + (size_t)(bk + (rj - i)) * 36 + r;
                const int zs = k <= j ? 1 : 6;
                double u = 0.0;
#pragma unroll
                for(int p = 0; p < 6; ++p)
                    u += Z[p * zs] * G[p * 6];
                s += u;
            }
            scratch[(size_t)w] = -s;
        }
        __syncthreads();
        // 3. Z_ii = W^T W - sum_k G_k^T Z_ki, entry (r, c) with c <= r
        double zii = 0.0;
        int zr = 0, zc = 0;
        if(t < 21)
        {
            // the thread's entry of W^T W; the indices of W stay compile-time constants, so W stays in registers
            double ww = 0.0;
#pragma unroll
            for(int r = 0; r < 6; ++r)
#pragma unroll
                for(int c = 0; c <= r; ++c)
                    if(t == pgc_tri(r, c))
                    {
                        zr = r, zc = c;
#pragma unroll
                        for(int p = r; p < 6; ++p)
                            ww += W[pgc_tri(p, r)] * W[pgc_tri(p, c)];
                    }
            double s = 0.0;
            for(int k = 0; k < m; ++k)
            {
                const double* G = a.S + (size_t)a.col_blk[cp + k] * 36 + zr;
                const double* Z = scratch + (size_t)k * 36 + zc;
                double u = 0.0;
#pragma unroll
                for(int p = 0; p < 6; ++p)
                    u += G[p * 6] * Z[p * 6];
                s += u;
            }
            zii = ww - s;
        }
        __syncthreads();
        // 4. the column takes its blocks of Z
        if(t < 21)
        {
            D[zr * 6 + zc] = zii;
            D[zc * 6 + zr] = zii;
        }
        for(int w = t; w < 36 * m; w += 256)
            a.S[(size_t)a.col_blk[cp + w / 36] * 36 + w % 36] = scratch[(size_t)w];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_pg_cov_gather(PgCovArgs a)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if(t == 0)
        a.out[(size_t)a.n_req * 36] = a.ctrl->solve_bad ? 1.0 : 0.0;
    if(t >= a.n_req * 36)
        return;
    const int q = t / 36, r = (t % 36) / 6, c = t % 6;
    const int ka = a.req[q * 2], kb = a.req[q * 2 + 1];
    const int pa = a.ci[ka], pb = a.ci[kb];
    double v = 0.0;
    if(pa >= 0 && pb >= 0)
    {
        const SysView<SysLayout::Envelope> sys(a);
        const double z = pa >= pb ? sys.env_block(pa, pb)[r * 6 + c] : sys.env_block(pb, pa)[c * 6 + r];
        v = (a.sc[(size_t)ka * 6 + r] * a.sc[(size_t)kb * 6 + c]) * z; // the product of the scales first: (a, b) and (b, a) agree bit for bit
    }
    a.out[(size_t)t] = v;
}

void pg_cov_enqueue(mslam_hip_ctx* c, const PgsArgs& env, const PgCovArgs& cov, double* scratch, hipStream_t s)
{
    {
        StageScope tk(c, "cov_selinv");
        hipLaunchKernelGGL(k_pgs_selinv, dim3(1), dim3(256), 0, s, env, scratch);
    }
    StageScope tk(c, "cov_gather");
    hipLaunchKernelGGL(k_pg_cov_gather, dim3((unsigned)(((size_t)cov.n_req * 36 + 256) / 256)), dim3(256), 0, s, cov);
}

} // namespace mslam
