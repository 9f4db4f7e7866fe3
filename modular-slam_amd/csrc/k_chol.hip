// k_chol.hip — the blocked f64 Cholesky solve of chol_solver.hpp: the kernels and, beside them, their launch sequence (a
// kernel is launched from the object that holds it).
//
// S is dense, column-major, n_pad = n rounded up to kBagNB columns, leading dimension ld = n_pad + 16: row n_pad carries the
// right-hand side, so the factorisation of [S b; b^T .] leaves y = L^-1 b there (the forward solve costs one more 16-row
// tile per panel and no launch).  Right-looking, three launches per panel j on one stream: k_bag_potrf (the diagonal block, one
// workgroup, in LDS), k_bag_trsm (the rows below it), k_bag_update (every lower tile right of it, on the matrix cores); then
// k_bag_backsolve per panel from the last to the first.  Only the lower triangle is read.  Every tile's sums have one order.
// Every launch reads the solve's control block first and returns when the solve has ended.  No kernel waits on another
// workgroup; every loop is bounded by n_pad and ld, which the host computed.
#include "chol_solver.hpp"

namespace mslam
{

typedef double bag_d4 __attribute__((ext_vector_type(4)));

// zero below (and in) the diagonal kBagNB-block of every column, 1 on the pad's diagonal; a block per column
__global__ __launch_bounds__(256) void k_bag_clear(CholArgs a)
{
    if(a.ctrl->done)
        return;
    const int c = blockIdx.x;
    double* col = a.S + (size_t)c * a.ld;
    for(int r = (c / kBagNB) * kBagNB + threadIdx.x; r < a.ld; r += 256)
        col[r] = (r == c && c >= a.n) ? 1.0 : 0.0;
}

// the diagonal block of panel j into LDS (lower triangle, the rest 0)
__device__ __forceinline__ void bag_load_diag(const CholArgs& a, int j, double (*A)[kBagNB + 1])
{
    const double* D = a.S + (size_t)j * kBagNB * ((size_t)a.ld + 1);
    const int i = threadIdx.x;
    if(i < kBagNB)
        for(int c = 0; c < kBagNB; ++c)
            A[i][c] = c <= i ? D[(size_t)i + (size_t)c * a.ld] : 0.0;
    __syncthreads();
}

// Cholesky of the diagonal block of panel j; thread i owns row i, k_ba_solve's pivot rule
__global__ __launch_bounds__(64) void k_bag_potrf(CholArgs a, int j)
{
    __shared__ double A[kBagNB][kBagNB + 1];
    __shared__ double sdiag;
    TrCtrl* ct = a.ctrl;
    if(ct->done)
        return;
    const int i = threadIdx.x;
    bag_load_diag(a, j, A);
    bool bad = false;
    for(int jj = 0; jj < kBagNB; ++jj)
    {
        double v = 0.0;
        if(i >= jj && i < kBagNB)
        {
            v = A[i][jj];
            for(int k = 0; k < jj; ++k)
                v -= A[i][k] * A[jj][k];
        }
        if(i == jj)
        {
            if(!(v > 0.0))
                bad = true; // a non-positive pivot: the step is invalid; the factorisation goes on with bounded values
            sdiag = sqrt(fmax(v, DBL_MIN));
        }
        __syncthreads();
        if(i >= jj && i < kBagNB)
            A[i][jj] = i == jj ? sdiag : v / sdiag;
        __syncthreads();
    }
    double* D = a.S + (size_t)j * kBagNB * ((size_t)a.ld + 1);
    if(i < kBagNB)
        for(int c = 0; c <= i; ++c)
            D[(size_t)i + (size_t)c * a.ld] = A[i][c];
    if(bad)
        ct->solve_bad = 1;
}

// X L_jj^T = A for the rows below the diagonal block of panel j (the right-hand side's row included): a thread per row
__global__ __launch_bounds__(64) void k_bag_trsm(CholArgs a, int j)
{
    __shared__ double Lj[kBagNB][kBagNB + 1];
    if(a.ctrl->done)
        return;
    bag_load_diag(a, j, Lj);
    const int row = (j + 1) * kBagNB + blockIdx.x * 64 + threadIdx.x;
    if(row >= a.ld)
        return;
    double* P = a.S + (size_t)row + (size_t)j * kBagNB * a.ld;
    double x[kBagNB];
#pragma unroll
    for(int c = 0; c < kBagNB; ++c)
        x[c] = P[(size_t)c * a.ld];
#pragma unroll
    for(int c = 0; c < kBagNB; ++c)
    {
        double v = x[c];
#pragma unroll
        for(int k = 0; k < c; ++k)
            v -= x[k] * Lj[c][k];
        x[c] = v / Lj[c][c];
    }
#pragma unroll
    for(int c = 0; c < kBagNB; ++c)
        P[(size_t)c * a.ld] = x[c];
}

// A_rc -= L_rj L_cj^T for the tile (row block r, column block c), j < c <= r; r = n_pad / kBagNB is the right-hand side's
// 16 rows.  One wave per tile: 3 x 3 accumulators of v_mfma_f64_16x16x4_f64, 12 steps over the panel's 48 columns.  The wave
// computes the transposed product (A operand from the column block, B from the row block): a result register then holds 16
// consecutive rows of one column of S (D: column = lane & 15, row = (lane >> 4) + 4 reg).
__global__ __launch_bounds__(64) void k_bag_update(CholArgs a, int j)
{
    if(a.ctrl->done)
        return;
    const int np = a.n_pad / kBagNB;
    // the grid is the tiles themselves: with nt = np - j - 1 column blocks right of the panel, the lower triangle of nt x nt
    // blocks row by row (x (x + 1) / 2 + y, y <= x), then the nt tiles of the right-hand side's row
    const int nt = np - j - 1, tri = nt * (nt + 1) / 2, b = (int)blockIdx.x;
    int x, y;
    if(b < tri)
    {
        x = (int)((sqrt(8.0 * b + 1.0) - 1.0) / 2.0);
        if(x * (x + 1) / 2 > b) // the root rounded up or down by one: at most one step either way
            --x;
        else if((x + 1) * (x + 2) / 2 <= b)
            ++x;
        y = b - x * (x + 1) / 2;
    }
    else
        x = nt, y = b - tri;
    if(x > nt || y < 0 || y >= nt || y > x)
        return; // cannot happen for a grid of tri + t blocks: no tile outside S is ever written
    const int rb = j + 1 + x, cb = j + 1 + y;
    const int lane = threadIdx.x, lo = lane & 15, hi = lane >> 4;
    const int mt = rb == np ? 1 : 3; // 16-row tiles of the row block
    const size_t ld = (size_t)a.ld;
    const double* Lr = a.S + (size_t)rb * kBagNB + lo + ((size_t)j * kBagNB + hi) * ld;
    const double* Lc = a.S + (size_t)cb * kBagNB + lo + ((size_t)j * kBagNB + hi) * ld;
    bag_d4 acc[3][3];
#pragma unroll
    for(int ti = 0; ti < 3; ++ti)
#pragma unroll
        for(int tj = 0; tj < 3; ++tj)
            acc[ti][tj] = bag_d4{0.0, 0.0, 0.0, 0.0};
    for(int ks = 0; ks < kBagNB / 4; ++ks)
    {
        double cv[3], rv[3];
#pragma unroll
        for(int t = 0; t < 3; ++t)
        {
            cv[t] = Lc[t * 16 + (size_t)ks * 4 * ld];
            rv[t] = t < mt ? Lr[t * 16 + (size_t)ks * 4 * ld] : 0.0;
        }
#pragma unroll
        for(int ti = 0; ti < 3; ++ti)
#pragma unroll
            for(int tj = 0; tj < 3; ++tj)
                acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(cv[tj], rv[ti], acc[ti][tj], 0, 0, 0);
    }
#pragma unroll
    for(int ti = 0; ti < 3; ++ti)
    {
        if(ti >= mt) // wave-uniform
            break;
#pragma unroll
        for(int tj = 0; tj < 3; ++tj)
#pragma unroll
            for(int reg = 0; reg < 4; ++reg)
            {
                double* C = a.S + ((size_t)rb * kBagNB + ti * 16 + lo) + ((size_t)cb * kBagNB + tj * 16 + hi + 4 * reg) * ld;
                *C -= acc[ti][tj][reg];
            }
    }
}

// Panel j of L^T x = y, from the last panel to the first.  Every workgroup solves the diagonal block for x_j (the same
// arithmetic, so the same bits); workgroup j writes it to yc, workgroup b < j takes L_jb^T x_j off y_b.
__global__ __launch_bounds__(64) void k_bag_backsolve(CholArgs a, int j)
{
    __shared__ double Lj[kBagNB][kBagNB + 1];
    __shared__ double x[kBagNB];
    if(a.ctrl->done)
        return;
    const int i = threadIdx.x, b = blockIdx.x;
    const size_t ld = (size_t)a.ld, np_ = (size_t)a.n_pad;
    bag_load_diag(a, j, Lj);
    if(i < kBagNB)
        x[i] = a.S[np_ + ((size_t)j * kBagNB + i) * ld];
    __syncthreads();
    for(int k = kBagNB - 1; k >= 0; --k)
    {
        if(i == k)
            x[k] = x[k] / Lj[k][k];
        __syncthreads();
        if(i < k)
            x[i] -= Lj[k][i] * x[k];
        __syncthreads();
    }
    if(i >= kBagNB)
        return;
    if(b == j)
    {
        if(j * kBagNB + i < a.n)
            a.yc[j * kBagNB + i] = x[i];
        return;
    }
    const size_t col = (size_t)b * kBagNB + i;
    double s = a.S[np_ + col * ld];
    for(int r = 0; r < kBagNB; ++r)
        s -= a.S[(size_t)j * kBagNB + r + col * ld] * x[r];
    a.S[np_ + col * ld] = s;
}

void ba_blocked_solve(mslam_hip_ctx* c, const CholArgs& a, hipStream_t s, const std::function<void()>& assemble)
{
    const int np = a.n_pad / kBagNB;
    {
        StageScope tk(c, "solver_schur");
        hipLaunchKernelGGL(k_bag_clear, dim3((unsigned)a.n_pad), dim3(256), 0, s, a);
        assemble();
    }
    {
        StageScope tk(c, "solver_factor");
        for(int j = 0; j < np; ++j)
        {
            hipLaunchKernelGGL(k_bag_potrf, dim3(1), dim3(64), 0, s, a, j);
            hipLaunchKernelGGL(k_bag_trsm, dim3((unsigned)((a.ld - (j + 1) * kBagNB + 63) / 64)), dim3(64), 0, s, a, j);
            if(j + 1 < np)
            {
                const unsigned t = (unsigned)(np - j - 1); // column blocks right of the panel
                hipLaunchKernelGGL(k_bag_update, dim3(t * (t + 1) / 2 + t), dim3(64), 0, s, a, j);
            }
        }
    }
    StageScope tk(c, "solver_subst");
    for(int j = np - 1; j >= 0; --j)
        hipLaunchKernelGGL(k_bag_backsolve, dim3((unsigned)(j + 1)), dim3(64), 0, s, a, j);
}

} // namespace mslam
