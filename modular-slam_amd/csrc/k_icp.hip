// k_icp.hip — frame-to-model alignment: point-to-plane ICP of a depth frame against a rendered model, mslam_hip_icp_* and
// mslam_hip_tsdf_icp* (include/mslam_hip.h has the rule, operation by operation; DESIGN.md 4.34 the structure).  Everything is
// f64, one separately rounded operation after the other, and every sum has one order, so a solve has one result, bit for bit.
//   k_icp_frame       once per call, one thread per pixel: depth -> vertex and frame normal (six f64 planes and a flag); its
//                     first thread turns the guess into the start state.
//   k_icp_linearize   one thread per pixel of the level, 256 per workgroup: the pair, its 28 terms and the count, the
//                     butterfly of trust_region.hpp's wave_sum per wave, the four waves in order: one row of partials.
//   k_icp_finish      one workgroup: the partials in ascending order (staged through LDS, 64 rows at a time), the LDL^T, the
//                     Cayley update, the step test, the control block (pose, done flag, level cursor, record row).
// The host enqueues the frame kernel and two launches per scheduled iteration, reads nothing in between and waits once.
#include "context.hpp"
#include "icp.hpp"
#include "trust_region.hpp"
#include "tsdf.hpp"
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

namespace mslam
{

void icp_destroy(IcpState* s) { delete s; }

constexpr int kIcpThreads = 256;
constexpr int kIcpSums = 28;  // A21, g6, r r
constexpr int kIcpRow = 32;   // doubles per row of partials: the sums, the count, padding
constexpr long long kIcpMaxPixels = 1ll << 24;
constexpr int kIcpTile = 64;  // rows of partials the finish kernel holds in LDS at a time
static_assert(kIcpSums + 1 <= kIcpRow, "the count follows the sums");

struct IcpFrameArgs
{
    const uint16_t* depth;
    int width, height;
    float factor;
    double fx, fy, cx, cy, max_depth;
    double R0[9], t0[3];
    double* frame; // six planes
    uint8_t* has;
    IcpCtrl* ctrl;
};

struct IcpVertex
{
    double x, y, z;
    bool valid;
};
__device__ __forceinline__ IcpVertex icp_vertex(const IcpFrameArgs& a, int px, int py)
{
    const float d = (float)a.depth[(size_t)py * (size_t)a.width + (size_t)px] * a.factor;
    IcpVertex v;
    v.valid = d > FLT_EPSILON && (double)d <= a.max_depth;
    v.z = (double)d;
    v.x = ((double)px - a.cx) / a.fx * v.z;
    v.y = ((double)py - a.cy) / a.fy * v.z;
    return v;
}

__global__ __launch_bounds__(kIcpThreads) void k_icp_frame(const IcpFrameArgs a)
{
    const size_t n_px = (size_t)a.width * (size_t)a.height;
    const size_t i = (size_t)blockIdx.x * kIcpThreads + threadIdx.x;
    if(i == 0) // the control block was zeroed on the stream before this launch
    {
        for(int r = 0; r < 3; ++r)
        {
            for(int col = 0; col < 3; ++col)
                a.ctrl->Q[3 * r + col] = a.R0[3 * col + r];
            a.ctrl->s[r] = -((a.R0[r] * a.t0[0] + a.R0[3 + r] * a.t0[1]) + a.R0[6 + r] * a.t0[2]);
        }
    }
    if(i >= n_px)
        return;
    const int px = (int)(i % (size_t)a.width), py = (int)(i / (size_t)a.width);
    const IcpVertex v = icp_vertex(a, px, py);
    double n[3] = {0.0, 0.0, 0.0};
    bool has = false;
    if(v.valid && px >= 1 && px <= a.width - 2 && py >= 1 && py <= a.height - 2)
    {
        const IcpVertex xp = icp_vertex(a, px + 1, py), xm = icp_vertex(a, px - 1, py);
        const IcpVertex yp = icp_vertex(a, px, py + 1), ym = icp_vertex(a, px, py - 1);
        if(xp.valid && xm.valid && yp.valid && ym.valid)
        {
            const double a0 = xp.x - xm.x, a1 = xp.y - xm.y, a2 = xp.z - xm.z;
            const double b0 = yp.x - ym.x, b1 = yp.y - ym.y, b2 = yp.z - ym.z;
            const double c0 = b1 * a2 - b2 * a1, c1 = b2 * a0 - b0 * a2, c2 = b0 * a1 - b1 * a0;
            const double len = sqrt((c0 * c0 + c1 * c1) + c2 * c2);
            if(len > 0.0)
                has = true, n[0] = c0 / len, n[1] = c1 / len, n[2] = c2 / len;
        }
    }
    a.frame[i] = v.x, a.frame[n_px + i] = v.y, a.frame[2 * n_px + i] = v.z;
    a.frame[3 * n_px + i] = n[0], a.frame[4 * n_px + i] = n[1], a.frame[5 * n_px + i] = n[2];
    a.has[i] = has ? 1 : 0;
}

struct IcpLinArgs
{
    const IcpCtrl* ctrl;
    int level;        // the launch returns unless the control block's cursor is here
    int stride, lw;   // the level's pixels: (py / stride, px / stride), lw per row
    unsigned M;       // lw x lh
    int width, height;
    const double* frame;
    const uint8_t* has;
    const float* mxyz;
    const float* mnrm;
    int mw, mh;
    double mfx, mfy, mcx, mcy;
    double Rm[9], tm[3];
    double dist2, cos_min; // dist_max * dist_max, rounded once
    double* part;          // [gridDim.x][kIcpRow]
};

__global__ __launch_bounds__(kIcpThreads) void k_icp_linearize(const IcpLinArgs a)
{
    __shared__ double s_red[kIcpThreads / 64][kIcpRow];
    const IcpCtrl* ct = a.ctrl;
    if(ct->done || ct->level != a.level) // the same in every thread of the grid
        return;
    const unsigned i = blockIdx.x * kIcpThreads + threadIdx.x;
    double T[kIcpSums];
#pragma unroll
    for(int k = 0; k < kIcpSums; ++k)
        T[k] = 0.0;
    bool ok = false;
    if(i < a.M)
    {
        const int px = (int)(i % (unsigned)a.lw) * a.stride, py = (int)(i / (unsigned)a.lw) * a.stride; // inside the frame
        const size_t n_px = (size_t)a.width * (size_t)a.height, pix = (size_t)py * (size_t)a.width + (size_t)px;
        if(a.has[pix])
        {
            const double* Q = ct->Q;
            const double V0 = a.frame[pix], V1 = a.frame[n_px + pix], V2 = a.frame[2 * n_px + pix];
            const double n0 = a.frame[3 * n_px + pix], n1 = a.frame[4 * n_px + pix], n2 = a.frame[5 * n_px + pix];
            double X[3], N[3], c[3];
            for(int r = 0; r < 3; ++r)
            {
                X[r] = ((Q[3 * r] * V0 + Q[3 * r + 1] * V1) + Q[3 * r + 2] * V2) + ct->s[r];
                N[r] = (Q[3 * r] * n0 + Q[3 * r + 1] * n1) + Q[3 * r + 2] * n2;
            }
            for(int r = 0; r < 3; ++r)
                c[r] = ((a.Rm[3 * r] * X[0] + a.Rm[3 * r + 1] * X[1]) + a.Rm[3 * r + 2] * X[2]) + a.tm[r];
            if(c[2] > 0.0)
            {
                const double u = (c[0] / c[2]) * a.mfx + a.mcx, v = (c[1] / c[2]) * a.mfy + a.mcy;
                const double uh = u + 0.5, vh = v + 0.5;
                if(uh >= 0.0 && uh < (double)a.mw && vh >= 0.0 && vh < (double)a.mh) // false for NaN
                {
                    // 0 <= floor(uh) < mw and 0 <= floor(vh) < mh: a pixel of the model
                    const size_t mp = ((size_t)(int)floor(vh) * (size_t)a.mw + (size_t)(int)floor(uh)) * 3;
                    const double q0 = (double)a.mxyz[mp], q1 = (double)a.mxyz[mp + 1], q2 = (double)a.mxyz[mp + 2];
                    const double m0 = (double)a.mnrm[mp], m1 = (double)a.mnrm[mp + 1], m2 = (double)a.mnrm[mp + 2];
                    if(!(m0 == 0.0 && m1 == 0.0 && m2 == 0.0))
                    {
                        const double e0 = X[0] - q0, e1 = X[1] - q1, e2 = X[2] - q2;
                        if((e0 * e0 + e1 * e1) + e2 * e2 <= a.dist2 && (N[0] * m0 + N[1] * m1) + N[2] * m2 >= a.cos_min)
                        {
                            ok = true;
                            const double r = (m0 * e0 + m1 * e1) + m2 * e2;
                            const double J[6] = {X[1] * m2 - X[2] * m1, X[2] * m0 - X[0] * m2, X[0] * m1 - X[1] * m0, m0, m1, m2};
                            int k = 0;
#pragma unroll
                            for(int p = 0; p < 6; ++p)
#pragma unroll
                                for(int q = p; q < 6; ++q)
                                    T[k++] = J[p] * J[q];
#pragma unroll
                            for(int p = 0; p < 6; ++p)
                                T[21 + p] = J[p] * r;
                            T[27] = r * r;
                        }
                    }
                }
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for(int k = 0; k < kIcpSums; ++k)
    {
        const double v = wave_sum(T[k]);
        if(lane == 0)
            s_red[wave][k] = v;
    }
    const int cnt = __popcll(__ballot(ok));
    if(lane == 0)
        s_red[wave][kIcpSums] = (double)cnt;
    __syncthreads();
    if(threadIdx.x <= kIcpSums) // block_sum's order for the four waves; the counts are small integers: exact
        a.part[(size_t)blockIdx.x * kIcpRow + threadIdx.x] =
            ((s_red[0][threadIdx.x] + s_red[1][threadIdx.x]) + s_red[2][threadIdx.x]) + s_red[3][threadIdx.x];
}

struct IcpFinishArgs
{
    IcpCtrl* ctrl;
    mslam_hip_icp_record* record; // [MSLAM_HIP_ICP_MAX_ITERATIONS]
    const double* part;
    unsigned n_chunks;
    int level, last_iteration, last_level; // this launch is the level's last scheduled one; the level is the last one
    int min_pairs;
    double rot_tol2, trans_tol2;
    int sums_only; // mslam_hip_icp_linearize: the sums and nothing else
};

// A x = -g by the header's LDL^T; false: a pivot that is not > 0.  D holds the pivots computed so far, the rest stay 0.0.
__device__ bool icp_ldl_solve(const double* __restrict__ S, double D[6], double x[6])
{
    double L[6][6];
    for(int j = 0; j < 6; ++j)
    {
        double v[6];
        for(int k = 0; k < j; ++k)
            v[k] = L[j][k] * D[k];
        double d = S[tri6(j, j)];
        for(int k = 0; k < j; ++k)
            d = d - L[j][k] * v[k];
        D[j] = d;
        if(!(d > 0.0))
            return false;
        for(int i = j + 1; i < 6; ++i)
        {
            double e = S[tri6(j, i)];
            for(int k = 0; k < j; ++k)
                e = e - L[i][k] * v[k];
            L[i][j] = e / d;
        }
    }
    double y[6];
    for(int i = 0; i < 6; ++i)
    {
        double b = -S[21 + i];
        for(int k = 0; k < i; ++k)
            b = b - L[i][k] * y[k];
        y[i] = b;
    }
    for(int i = 5; i >= 0; --i)
    {
        double b = y[i] / D[i];
        for(int k = i + 1; k < 6; ++k)
            b = b - L[k][i] * x[k];
        x[i] = b;
    }
    return true;
}

__global__ __launch_bounds__(kIcpThreads) void k_icp_finish(const IcpFinishArgs a)
{
    __shared__ double s_tile[kIcpTile * kIcpRow];
    __shared__ double s_sum[kIcpRow];
    IcpCtrl* ct = a.ctrl;
    if(ct->done || ct->level != a.level)
        return;
    // The rows come in through LDS, kIcpTile at a time and all threads loading, so that the one chain of additions per sum
    // waits for LDS and not for memory; the order stays the ascending chunk index.
    double acc = 0.0;
    for(unsigned c0 = 0; c0 < a.n_chunks; c0 += kIcpTile)
    {
        const unsigned rows = min((unsigned)kIcpTile, a.n_chunks - c0);
        for(unsigned k = threadIdx.x; k < rows * kIcpRow; k += kIcpThreads) // inside the n_chunks rows
            s_tile[k] = a.part[(size_t)c0 * kIcpRow + k];
        __syncthreads();
        if(threadIdx.x <= kIcpSums)
            for(unsigned c = 0; c < rows; ++c)
                acc = acc + s_tile[c * kIcpRow + threadIdx.x];
        __syncthreads();
    }
    if(threadIdx.x <= kIcpSums)
        s_sum[threadIdx.x] = acc;
    __syncthreads();
    if(threadIdx.x != 0)
        return;
    for(int k = 0; k <= kIcpSums; ++k)
        ct->sums[k] = s_sum[k];
    if(a.sums_only)
        return;
    const int count = (int)s_sum[kIcpSums];
    const double cost = s_sum[27];
    mslam_hip_icp_record row{a.level, count, cost, 0.0, 0.0};
    double D[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, x[6];
    const bool solved = count >= a.min_pairs && icp_ldl_solve(s_sum, D, x);
    ct->count = count, ct->cost = cost, ct->last_level = a.level;
    for(int k = 0; k < 6; ++k)
        ct->pivots[k] = D[k];
    const int n_lin = ct->n_lin; // < MSLAM_HIP_ICP_MAX_ITERATIONS: one row per scheduled iteration at most
    ct->n_lin = n_lin + 1;
    if(!solved)
    {
        a.record[n_lin] = row;
        ct->status = MSLAM_HIP_ICP_DEGENERATE;
        ct->done = 1;
        return;
    }
    const double a0 = x[0] * 0.5, a1 = x[1] * 0.5, a2 = x[2] * 0.5;
    const double aa = (a0 * a0 + a1 * a1) + a2 * a2;
    const double den = 1.0 + aa, one = 1.0 - aa;
    const double dR[9] = {(one + 2.0 * (a0 * a0)) / den,        (2.0 * (a0 * a1) - 2.0 * a2) / den, (2.0 * (a0 * a2) + 2.0 * a1) / den,
                          (2.0 * (a0 * a1) + 2.0 * a2) / den, (one + 2.0 * (a1 * a1)) / den,        (2.0 * (a1 * a2) - 2.0 * a0) / den,
                          (2.0 * (a0 * a2) - 2.0 * a1) / den, (2.0 * (a1 * a2) + 2.0 * a0) / den, (one + 2.0 * (a2 * a2)) / den};
    double Q[9], s[3];
    for(int i = 0; i < 3; ++i)
    {
        for(int j = 0; j < 3; ++j)
            Q[3 * i + j] = (dR[3 * i] * ct->Q[j] + dR[3 * i + 1] * ct->Q[3 + j]) + dR[3 * i + 2] * ct->Q[6 + j];
        s[i] = ((dR[3 * i] * ct->s[0] + dR[3 * i + 1] * ct->s[1]) + dR[3 * i + 2] * ct->s[2]) + x[3 + i];
    }
    for(int k = 0; k < 9; ++k)
        ct->Q[k] = Q[k];
    for(int k = 0; k < 3; ++k)
        ct->s[k] = s[k];
    row.rot2 = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
    row.trans2 = (x[3] * x[3] + x[4] * x[4]) + x[5] * x[5];
    a.record[n_lin] = row;
    const bool small = row.rot2 <= a.rot_tol2 && row.trans2 <= a.trans_tol2;
    if(!small && !a.last_iteration)
        return;
    if(!a.last_level)
    {
        ct->level = a.level + 1;
        return;
    }
    for(int r = 0; r < 3; ++r)
    {
        for(int col = 0; col < 3; ++col)
            ct->R[3 * r + col] = Q[3 * col + r];
        ct->t[r] = -((Q[r] * s[0] + Q[3 + r] * s[1]) + Q[6 + r] * s[2]);
    }
    ct->status = small ? MSLAM_HIP_ICP_CONVERGED : MSLAM_HIP_ICP_ITERATIONS;
    ct->done = 1;
}

// ---- host -------------------------------------------------------------------------------------------------------------------
static bool icp_finite(const double* v, int n)
{
    for(int i = 0; i < n; ++i)
        if(!std::isfinite(v[i]))
            return false;
    return true;
}

// the argument errors of the parameters; *total = the scheduled iterations
static int icp_check_params(mslam_hip_ctx* c, const mslam_hip_icp_params* p, const std::string& who, int* total)
{
    if(p->width < 1 || p->height < 1 || (long long)p->width * p->height > kIcpMaxPixels)
        return fail(c, MSLAM_HIP_E_INVALID, who + ": width, height must be >= 1 with at most 2^24 pixels");
    if(p->model_width < 1 || p->model_height < 1 || (long long)p->model_width * p->model_height > (1 << 30))
        return fail(c, MSLAM_HIP_E_INVALID, who + ": model_width, model_height must be >= 1 with at most 2^30 pixels");
    const double k[8] = {p->fx, p->fy, p->cx, p->cy, p->mfx, p->mfy, p->mcx, p->mcy};
    if(!icp_finite(k, 8) || !std::isfinite(p->factor) || p->fx == 0 || p->fy == 0 || p->mfx == 0 || p->mfy == 0)
        return fail(c, MSLAM_HIP_E_INVALID, who + ": a non-finite intrinsic or factor, or a focal length of zero");
    if(!(p->max_depth > 0))
        return fail(c, MSLAM_HIP_E_INVALID, who + ": max_depth must be > 0");
    if(p->n_levels < 1 || p->n_levels > MSLAM_HIP_ICP_MAX_LEVELS)
        return fail(c, MSLAM_HIP_E_INVALID, who + ": n_levels must be 1..4");
    long long sum = 0;
    for(int l = 0; l < p->n_levels; ++l)
    {
        if(p->stride[l] < 1 || p->iterations[l] < 1)
            return fail(c, MSLAM_HIP_E_INVALID, who + ": a stride or an iteration count below 1");
        sum += p->iterations[l];
    }
    if(sum > MSLAM_HIP_ICP_MAX_ITERATIONS)
        return fail(c, MSLAM_HIP_E_INVALID, who + ": more than 256 iterations in all");
    if(!std::isfinite(p->dist_max) || !(p->dist_max > 0) || !(p->cos_min >= -1.0 && p->cos_min <= 1.0))
        return fail(c, MSLAM_HIP_E_INVALID, who + ": dist_max must be finite and > 0, cos_min in [-1, 1]");
    if(p->min_pairs < 6)
        return fail(c, MSLAM_HIP_E_INVALID, who + ": min_pairs must be >= 6");
    if(!std::isfinite(p->rot_tol) || p->rot_tol < 0 || !std::isfinite(p->trans_tol) || p->trans_tol < 0)
        return fail(c, MSLAM_HIP_E_INVALID, who + ": rot_tol, trans_tol must be finite and >= 0");
    *total = (int)sum;
    return MSLAM_HIP_OK;
}

struct IcpImages
{
    const uint16_t* depth;
    const float* mxyz;
    const float* mnrm;
    bool depth_on_device, model_on_device;
};

static unsigned icp_level_pixels(const mslam_hip_icp_params* p, int stride, int* lw)
{
    *lw = (p->width + stride - 1) / stride; // the px with px % stride == 0: 0, stride, .. < width
    const int lh = (p->height + stride - 1) / stride;
    return (unsigned)*lw * (unsigned)lh;
}

// Uploads what is on the host, enqueues the frame kernel and fills the launch arguments both solve and linearize use.
// (R0, t0): the pose the state starts from.
static hipError_t icp_prepare(mslam_hip_ctx* c, const mslam_hip_icp_params* p, const IcpImages& im, const double* Rm, const double* tm,
                              const double* R0, const double* t0, IcpLinArgs& lin, IcpFinishArgs& fin)
{
    if(!c->icp)
        c->icp = new IcpState();
    IcpState* s = c->icp;
    hipStream_t st = c->stream;
    const size_t px = (size_t)p->width * (size_t)p->height, mpx = (size_t)p->model_width * (size_t)p->model_height;
    const size_t max_chunks = (px + kIcpThreads - 1) / kIcpThreads; // stride 1 has the most pixels
    hipError_t e = grow(s->d_frame, px * 6, st);
    if(e == hipSuccess)
        e = grow(s->d_has, px, st);
    if(e == hipSuccess)
        e = grow(s->d_part, max_chunks * kIcpRow, st);
    if(e == hipSuccess)
        e = grow(s->d_ctrl, sizeof(IcpCtrl) + sizeof(mslam_hip_icp_record) * MSLAM_HIP_ICP_MAX_ITERATIONS, st);
    if(e == hipSuccess && !im.depth_on_device)
        e = grow(s->d_depth, px, st);
    if(e == hipSuccess && !im.model_on_device)
    {
        e = grow(s->d_mxyz, mpx * 3, st);
        if(e == hipSuccess)
            e = grow(s->d_mnrm, mpx * 3, st);
    }
    if(e != hipSuccess)
        return e;
    IcpFrameArgs f{};
    f.depth = im.depth, lin.mxyz = im.mxyz, lin.mnrm = im.mnrm;
    if(!im.depth_on_device)
    {
        if((e = hipMemcpyAsync(s->d_depth, im.depth, px * sizeof(uint16_t), hipMemcpyHostToDevice, st)) != hipSuccess)
            return e;
        f.depth = s->d_depth;
    }
    if(!im.model_on_device)
    {
        if((e = hipMemcpyAsync(s->d_mxyz, im.mxyz, mpx * 3 * sizeof(float), hipMemcpyHostToDevice, st)) != hipSuccess)
            return e;
        if((e = hipMemcpyAsync(s->d_mnrm, im.mnrm, mpx * 3 * sizeof(float), hipMemcpyHostToDevice, st)) != hipSuccess)
            return e;
        lin.mxyz = s->d_mxyz, lin.mnrm = s->d_mnrm;
    }
    IcpCtrl* ctrl = reinterpret_cast<IcpCtrl*>(s->d_ctrl.get());
    if((e = hipMemsetAsync(ctrl, 0, sizeof(IcpCtrl), st)) != hipSuccess)
        return e;
    f.width = p->width, f.height = p->height, f.factor = p->factor;
    f.fx = p->fx, f.fy = p->fy, f.cx = p->cx, f.cy = p->cy, f.max_depth = p->max_depth;
    std::memcpy(f.R0, R0, sizeof(f.R0));
    std::memcpy(f.t0, t0, sizeof(f.t0));
    f.frame = s->d_frame, f.has = s->d_has, f.ctrl = ctrl;
    {
        StageScope ts(c, "icp_frame");
        hipLaunchKernelGGL(k_icp_frame, dim3((unsigned)max_chunks), dim3(kIcpThreads), 0, st, f);
        if((e = hipGetLastError()) != hipSuccess)
            return e;
    }
    lin.ctrl = ctrl;
    lin.width = p->width, lin.height = p->height;
    lin.frame = s->d_frame, lin.has = s->d_has;
    lin.mw = p->model_width, lin.mh = p->model_height;
    lin.mfx = p->mfx, lin.mfy = p->mfy, lin.mcx = p->mcx, lin.mcy = p->mcy;
    std::memcpy(lin.Rm, Rm, sizeof(lin.Rm));
    std::memcpy(lin.tm, tm, sizeof(lin.tm));
    lin.dist2 = p->dist_max * p->dist_max, lin.cos_min = p->cos_min;
    lin.part = s->d_part;
    fin.ctrl = ctrl;
    fin.record = reinterpret_cast<mslam_hip_icp_record*>(s->d_ctrl.get() + sizeof(IcpCtrl));
    fin.part = s->d_part;
    fin.min_pairs = p->min_pairs;
    fin.rot_tol2 = p->rot_tol * p->rot_tol, fin.trans_tol2 = p->trans_tol * p->trans_tol;
    return hipSuccess;
}

// one scheduled iteration: two launches
static hipError_t icp_enqueue(mslam_hip_ctx* c, const mslam_hip_icp_params* p, IcpLinArgs& lin, IcpFinishArgs& fin, int level, int stride)
{
    lin.level = fin.level = level;
    lin.stride = stride;
    lin.M = icp_level_pixels(p, stride, &lin.lw);
    fin.n_chunks = (lin.M + kIcpThreads - 1) / kIcpThreads;
    {
        StageScope ts(c, "icp_linearize");
        hipLaunchKernelGGL(k_icp_linearize, dim3(fin.n_chunks), dim3(kIcpThreads), 0, c->stream, lin);
    }
    {
        StageScope ts(c, "icp_finish");
        hipLaunchKernelGGL(k_icp_finish, dim3(1), dim3(kIcpThreads), 0, c->stream, fin);
    }
    return hipGetLastError();
}

static int icp_solve(mslam_hip_ctx* c, const mslam_hip_icp_params* p, const IcpImages& im, const double* Rm, const double* tm,
                     const double* R0, const double* t0, double* R, double* t, mslam_hip_icp_result* result,
                     mslam_hip_icp_record* record, int total, const std::string& who)
{
    IcpLinArgs lin{};
    IcpFinishArgs fin{};
    hipError_t e = icp_prepare(c, p, im, Rm, tm, R0, t0, lin, fin);
    for(int l = 0; l < p->n_levels && e == hipSuccess; ++l)
        for(int k = 0; k < p->iterations[l] && e == hipSuccess; ++k)
        {
            fin.last_iteration = k == p->iterations[l] - 1, fin.last_level = l == p->n_levels - 1;
            e = icp_enqueue(c, p, lin, fin, l, p->stride[l]);
        }
    std::vector<uint8_t> back(sizeof(IcpCtrl) + sizeof(mslam_hip_icp_record) * (size_t)total);
    if(e == hipSuccess)
        e = hipMemcpyAsync(back.data(), c->icp->d_ctrl, back.size(), hipMemcpyDeviceToHost, c->stream);
    if(e == hipSuccess)
        e = hipStreamSynchronize(c->stream);
    if(e != hipSuccess)
        return fail(c, MSLAM_HIP_E_RUNTIME, who + ": " + hipGetErrorString(e));
    IcpCtrl ct;
    std::memcpy(&ct, back.data(), sizeof(ct));
    if(!ct.done || ct.n_lin < 1 || ct.n_lin > total)
        return fail(c, MSLAM_HIP_E_RUNTIME, who + ": the kernels left no termination");
    const bool degenerate = ct.status == MSLAM_HIP_ICP_DEGENERATE;
    std::memcpy(R, degenerate ? R0 : ct.R, 9 * sizeof(double));
    std::memcpy(t, degenerate ? t0 : ct.t, 3 * sizeof(double));
    std::memset(result, 0, sizeof(*result));
    result->status = ct.status, result->iterations = ct.n_lin, result->count = ct.count, result->level = ct.last_level;
    result->cost = ct.cost;
    std::memcpy(result->pivots, ct.pivots, sizeof(ct.pivots));
    if(record)
        std::memcpy(record, back.data() + sizeof(IcpCtrl), sizeof(mslam_hip_icp_record) * (size_t)ct.n_lin);
    return MSLAM_HIP_OK;
}

static int icp_point_plane(mslam_hip_ctx* c, const mslam_hip_icp_params* p, const IcpImages& im, const double* Rm, const double* tm,
                           const double* R0, const double* t0, double* R, double* t, mslam_hip_icp_result* result,
                           mslam_hip_icp_record* record, int record_capacity, const char* name)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    const std::string who(name);
    if(!p || !im.depth || !im.mxyz || !im.mnrm || !Rm || !tm || !R0 || !t0 || !R || !t || !result)
        return fail(c, MSLAM_HIP_E_INVALID, who + ": a NULL argument");
    int total = 0;
    if(const int rc = icp_check_params(c, p, who, &total))
        return rc;
    if(!icp_finite(Rm, 9) || !icp_finite(tm, 3) || !icp_finite(R0, 9) || !icp_finite(t0, 3))
        return fail(c, MSLAM_HIP_E_INVALID, who + ": a non-finite pose entry");
    if(record && record_capacity < total)
        return fail(c, MSLAM_HIP_E_INVALID, who + ": record_capacity is below the scheduled iterations");
    if(hipSetDevice(c->p.device) != hipSuccess)
        return fail(c, MSLAM_HIP_E_RUNTIME, who + ": hipSetDevice");
    return icp_solve(c, p, im, Rm, tm, R0, t0, R, t, result, record, total, who);
}

static int tsdf_icp(mslam_hip_ctx* c, const mslam_hip_icp_params* p, const mslam_hip_tsdf_raycast_params* q, const uint16_t* depth,
                    bool depth_on_device, const double* R0, const double* t0, double* R, double* t, mslam_hip_icp_result* result,
                    mslam_hip_icp_record* record, int record_capacity, const char* name)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    const std::string who(name);
    TsdfState* s = c->tsdf;
    if(!s)
        return fail(c, MSLAM_HIP_E_INVALID, who + ": no volume (mslam_hip_tsdf_create)");
    if(!p || !q || !depth || !R0 || !t0 || !R || !t || !result)
        return fail(c, MSLAM_HIP_E_INVALID, who + ": a NULL argument");
    const mslam_hip_tsdf_params& v = s->p;
    if(p->width != v.width || p->height != v.height || !(p->factor == v.factor) || !(p->fx == v.fx) || !(p->fy == v.fy) ||
       !(p->cx == v.cx) || !(p->cy == v.cy) || !(p->max_depth == v.max_depth))
        return fail(c, MSLAM_HIP_E_INVALID, who + ": the frame camera of params is not the volume's");
    mslam_hip_icp_params pm = *p; // the model is the render
    pm.model_width = q->width, pm.model_height = q->height;
    pm.mfx = q->fx, pm.mfy = q->fy, pm.mcx = q->cx, pm.mcy = q->cy;
    int total = 0;
    if(const int rc = icp_check_params(c, &pm, who, &total))
        return rc;
    if(!icp_finite(R0, 9) || !icp_finite(t0, 3))
        return fail(c, MSLAM_HIP_E_INVALID, who + ": a non-finite pose entry");
    if(record && record_capacity < total)
        return fail(c, MSLAM_HIP_E_INVALID, who + ": record_capacity is below the scheduled iterations");
    if(hipSetDevice(c->p.device) != hipSuccess)
        return fail(c, MSLAM_HIP_E_RUNTIME, who + ": hipSetDevice");
    const size_t mpx = (size_t)q->width * (size_t)q->height;
    hipError_t e = grow(s->d_ray_depth, mpx, c->stream);
    if(e == hipSuccess)
        e = grow(s->d_xyz, mpx * 3, c->stream);
    if(e == hipSuccess)
        e = grow(s->d_normal, mpx * 3, c->stream);
    if(e != hipSuccess)
        return fail(c, MSLAM_HIP_E_RUNTIME, who + ": " + hipGetErrorString(e));
    // the ray-cast refuses its own argument errors before it enqueues anything
    if(const int rc = mslam_hip_tsdf_raycast_dev(c, q, R0, t0, s->d_ray_depth, s->d_xyz, s->d_normal, nullptr))
        return rc;
    const IcpImages im{depth, s->d_xyz, s->d_normal, depth_on_device, true};
    return icp_solve(c, &pm, im, R0, t0, R0, t0, R, t, result, record, total, who);
}

} // namespace mslam

using namespace mslam;

extern "C" int mslam_hip_icp_point_plane(mslam_hip_ctx* c, const mslam_hip_icp_params* p, const uint16_t* depth, const float* model_xyz,
                                         const float* model_normal, const double* Rm, const double* tm, const double* R0,
                                         const double* t0, double* R, double* t, mslam_hip_icp_result* result,
                                         mslam_hip_icp_record* record, int record_capacity)
{
    return icp_point_plane(c, p, IcpImages{depth, model_xyz, model_normal, false, false}, Rm, tm, R0, t0, R, t, result, record,
                           record_capacity, "icp_point_plane");
}

extern "C" int mslam_hip_icp_point_plane_dev(mslam_hip_ctx* c, const mslam_hip_icp_params* p, const uint16_t* d_depth,
                                             const float* d_model_xyz, const float* d_model_normal, const double* Rm, const double* tm,
                                             const double* R0, const double* t0, double* R, double* t, mslam_hip_icp_result* result,
                                             mslam_hip_icp_record* record, int record_capacity)
{
    return icp_point_plane(c, p, IcpImages{d_depth, d_model_xyz, d_model_normal, true, true}, Rm, tm, R0, t0, R, t, result, record,
                           record_capacity, "icp_point_plane_dev");
}

extern "C" int mslam_hip_icp_linearize(mslam_hip_ctx* c, const mslam_hip_icp_params* p, const uint16_t* depth, const float* model_xyz,
                                       const float* model_normal, const double* Rm, const double* tm, const double* R, const double* t,
                                       int stride, double* A21, double* g6, int* count, double* cost)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    const std::string who("icp_linearize");
    if(!p || !depth || !model_xyz || !model_normal || !Rm || !tm || !R || !t || !A21 || !g6 || !count || !cost)
        return fail(c, MSLAM_HIP_E_INVALID, who + ": a NULL argument");
    int total = 0;
    if(const int rc = icp_check_params(c, p, who, &total))
        return rc;
    if(stride < 1)
        return fail(c, MSLAM_HIP_E_INVALID, who + ": stride must be >= 1");
    if(!icp_finite(Rm, 9) || !icp_finite(tm, 3) || !icp_finite(R, 9) || !icp_finite(t, 3))
        return fail(c, MSLAM_HIP_E_INVALID, who + ": a non-finite pose entry");
    if(hipSetDevice(c->p.device) != hipSuccess)
        return fail(c, MSLAM_HIP_E_RUNTIME, who + ": hipSetDevice");
    IcpLinArgs lin{};
    IcpFinishArgs fin{};
    hipError_t e = icp_prepare(c, p, IcpImages{depth, model_xyz, model_normal, false, false}, Rm, tm, R, t, lin, fin);
    fin.sums_only = 1;
    if(e == hipSuccess)
        e = icp_enqueue(c, p, lin, fin, 0, stride);
    IcpCtrl ct;
    if(e == hipSuccess)
        e = hipMemcpyAsync(&ct, c->icp->d_ctrl, sizeof(ct), hipMemcpyDeviceToHost, c->stream);
    if(e == hipSuccess)
        e = hipStreamSynchronize(c->stream);
    if(e != hipSuccess)
        return fail(c, MSLAM_HIP_E_RUNTIME, who + ": " + hipGetErrorString(e));
    std::memcpy(A21, ct.sums, 21 * sizeof(double));
    std::memcpy(g6, ct.sums + 21, 6 * sizeof(double));
    *cost = ct.sums[27];
    *count = (int)ct.sums[kIcpSums];
    return MSLAM_HIP_OK;
}

extern "C" int mslam_hip_tsdf_icp(mslam_hip_ctx* c, const mslam_hip_icp_params* p, const mslam_hip_tsdf_raycast_params* q,
                                  const uint16_t* depth, const double* R0, const double* t0, double* R, double* t,
                                  mslam_hip_icp_result* result, mslam_hip_icp_record* record, int record_capacity)
{
    return tsdf_icp(c, p, q, depth, false, R0, t0, R, t, result, record, record_capacity, "tsdf_icp");
}

extern "C" int mslam_hip_tsdf_icp_dev(mslam_hip_ctx* c, const mslam_hip_icp_params* p, const mslam_hip_tsdf_raycast_params* q,
                                      const uint16_t* d_depth, const double* R0, const double* t0, double* R, double* t,
                                      mslam_hip_icp_result* result, mslam_hip_icp_record* record, int record_capacity)
{
    return tsdf_icp(c, p, q, d_depth, true, R0, t0, R, t, result, record, record_capacity, "tsdf_icp_dev");
}
