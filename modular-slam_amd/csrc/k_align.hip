// k_align.hip — RANSAC rigid alignment of two 3-D point sets: dst_i ~ R src_i + t.
//
// No reference counterpart (the reference estimates a tracked pose by PnP only): an extension, modelled on the fixed-scale
// Sim3Solver of ORB-SLAM's RGB-D tracking.  It estimates the metric the back end minimises (k_ba.hip: the 3-D difference in
// the camera frame) where k_pnp.hip estimates the reprojection error.  The loop is k_pnp.hip's, piece by piece: the same
// sampler with three draws, hypotheses looked at in order, a new best one needs MORE inliers and more than 3 (the sample's
// own points prove nothing), RANSACUpdateNumIters with 3 model points after every new best one.  What differs is the model:
// the closed-form least-squares rigid transform (centroids, then Horn's unit quaternion — the eigenvector of the largest
// eigenvalue of the 4 x 4 symmetric matrix of the cross-covariance, by cyclic Jacobi sweeps), for the three pairs of a sample
// and again for the consensus set.  No iterations, no start, never a reflection, safe at 180 degrees.
//
// One workgroup solves one problem: hypotheses are generated one per thread, every wave scores one hypothesis per round
// against the points staged in LDS (6 floats each), thread 0 walks each round in order, and the refit's sums (centroids
// first, then the centred products) are reduced in a fixed order (bit-reproducible).  All arithmetic is f64: + - * / sqrt.
#include "context.hpp"
#include "ransac_common.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace mslam
{

struct AlignArgs
{
    const float* src; // [n][3]
    const float* dst; // [n][3]
    int n;
    int iterations;
    double confidence; // as PnpArgs: outside (0, 1) never early
    double thr2;       // max_distance^2
    unsigned long long seed;
    double* hyp;     // [iterations][12] R (row major), t — used beyond kAlignLdsHyp hypotheses
    int32_t* counts; // [iterations]
    uint8_t* mask;   // [n]
    double* out;     // R[9], t[3], n_inliers, best hypothesis, status, 0
};

constexpr int kAlignModelPoints = 3;
constexpr int kAlignThreads = kRansacThreads;
// LDS of a workgroup: wg_sum's block (1.1 KB) + hypotheses (12.5 KB) + points (24 KB) + their mask (1 KB) = 38.6 KB, so four
// workgroups share a CU's 160 KB (a tracking window is one workgroup per frame) and no launch needs the > 64 KB attribute
constexpr int kAlignLdsPts = 1024; // points staged in LDS for the scoring loop and the refit
constexpr int kAlignLdsHyp = 128;  // hypotheses (12 doubles + a count) kept in LDS up to this many
constexpr size_t kAlignLdsBytes = (size_t)kRansacRed * 8 + (size_t)kAlignLdsHyp * (96 + 4) + (size_t)kAlignLdsPts * 25;
constexpr int kAlignSweeps = 8; // cyclic Jacobi sweeps of the 4 x 4 matrix: converged to rounding after 5 or 6

// a usable triple: |a x b|^2 > 1e-6 |a|^2 |b|^2 (false for collinear points, coincident points and NaN)
__device__ __forceinline__ bool triple_ok(V3 p0, V3 p1, V3 p2)
{
    const V3 a = p1 - p0, b = p2 - p0, c = cross(a, b);
    return dot(c, c) > 1e-6 * (dot(a, a) * dot(b, b));
}

// one Jacobi rotation of the symmetric 4 x 4 matrix A in the (P, Q) plane, accumulated into V (columns = eigenvectors)
template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double (&A)[4][4], double (&V)[4][4])
{
    const double apq = A[P][Q];
    // a vanishing entry has nothing to annihilate, and theta^2 below would overflow (or be 0 / 0)
    if(!(fabs(apq) > 1e-300))
        return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    double t;
    if(fabs(theta) > 1e150)
        t = 0.5 / theta;
    else
    {
        t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
        if(theta < 0.0)
            t = -t;
    }
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for(int k = 0; k < 4; ++k)
    {
        const double akp = A[k][P], akq = A[k][Q];
        A[k][P] = c * akp - s * akq;
        A[k][Q] = s * akp + c * akq;
    }
#pragma unroll
    for(int k = 0; k < 4; ++k)
    {
        const double apk = A[P][k], aqk = A[Q][k];
        A[P][k] = c * apk - s * aqk;
        A[Q][k] = s * apk + c * aqk;
    }
#pragma unroll
    for(int k = 0; k < 4; ++k)
    {
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - s * vkq;
        V[k][Q] = s * vkp + c * vkq;
    }
}

// R = argmax over SO(3) of sum (d_i - dbar) . R (s_i - sbar) from the cross-covariance S[a][b] = sum (s_i - sbar)_a (d_i - dbar)_b
// (Horn 1987), t = dbar - R sbar
__device__ __forceinline__ void rigid_from_covariance(const double* S, V3 sbar, V3 dbar, double* R, double* t)
{
    const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
    double A[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for(int sweep = 0; sweep < kAlignSweeps; ++sweep)
    {
        jacobi_rotate<0, 1>(A, V);
        jacobi_rotate<0, 2>(A, V);
        jacobi_rotate<0, 3>(A, V);
        jacobi_rotate<1, 2>(A, V);
        jacobi_rotate<1, 3>(A, V);
        jacobi_rotate<2, 3>(A, V);
    }
    // the eigenvector of the largest eigenvalue (the first one on ties)
    double lam = A[0][0], qw = V[0][0], qx = V[1][0], qy = V[2][0], qz = V[3][0];
#pragma unroll
    for(int k = 1; k < 4; ++k)
    {
        const bool up = A[k][k] > lam;
        lam = up ? A[k][k] : lam;
        qw = up ? V[0][k] : qw, qx = up ? V[1][k] : qx, qy = up ? V[2][k] : qy, qz = up ? V[3][k] : qz;
    }
    const double inv = 1.0 / sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
    qw *= inv, qx *= inv, qy *= inv, qz *= inv;
    R[0] = 1.0 - 2.0 * (qy * qy + qz * qz), R[1] = 2.0 * (qx * qy - qw * qz), R[2] = 2.0 * (qx * qz + qw * qy);
    R[3] = 2.0 * (qx * qy + qw * qz), R[4] = 1.0 - 2.0 * (qx * qx + qz * qz), R[5] = 2.0 * (qy * qz - qw * qx);
    R[6] = 2.0 * (qx * qz - qw * qy), R[7] = 2.0 * (qy * qz + qw * qx), R[8] = 1.0 - 2.0 * (qx * qx + qy * qy);
    const V3 Rs = mulR(R, sbar);
    t[0] = dbar.x - Rs.x, t[1] = dbar.y - Rs.y, t[2] = dbar.z - Rs.z;
}

// |R s + t - d|^2 <= thr2; false for a non-finite value
__device__ __forceinline__ bool align_inlier(const double* R, const double* t, V3 s, V3 d, double thr2)
{
    const V3 r = mulR(R, s) + v3(t[0], t[1], t[2]) - d;
    return dot(r, r) <= thr2;
}

__device__ __forceinline__ V3 load3(const float* p) { return v3((double)p[0], (double)p[1], (double)p[2]); }

// one problem, one workgroup (shared by the single-problem kernel and the batched one)
__device__ __forceinline__ void align_problem(const AlignArgs& a, double* red /* LDS, kAlignLdsBytes */)
{
    __shared__ int s_best, s_cnt, s_niters;
    const int tid = threadIdx.x;
    const int n = a.n;
    double* l_hyp = red + kRansacRed;
    int32_t* l_cnt = reinterpret_cast<int32_t*>(l_hyp + kAlignLdsHyp * 12);
    float* pts = reinterpret_cast<float*>(l_cnt + kAlignLdsHyp);
    uint8_t* l_mask = reinterpret_cast<uint8_t*>(pts + 6 * kAlignLdsPts);
    double* hyp = a.iterations <= kAlignLdsHyp ? l_hyp : a.hyp;
    int32_t* counts = a.iterations <= kAlignLdsHyp ? l_cnt : a.counts;

    // ---- 1. hypotheses: thread h draws 3 distinct pairs and aligns them
    for(int h = tid; h < a.iterations; h += kAlignThreads)
    {
        unsigned long long x = a.seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(h + 1);
        int idx[3];
        bool ok = n >= 3;
        for(int k = 0; k < 3 && ok; ++k)
        {
            int tries = 0;
            for(;;)
            {
                idx[k] = (int)(splitmix(x) % (unsigned long long)n);
                bool dup = false;
                for(int j = 0; j < k; ++j)
                    dup = dup || idx[j] == idx[k];
                if(!dup)
                    break;
                if(++tries > 64)
                {
                    ok = false;
                    break;
                }
            }
        }
        double R[9], t[3];
        if(ok)
        {
            const V3 s0 = load3(a.src + 3 * idx[0]), s1 = load3(a.src + 3 * idx[1]), s2 = load3(a.src + 3 * idx[2]);
            const V3 d0 = load3(a.dst + 3 * idx[0]), d1 = load3(a.dst + 3 * idx[1]), d2 = load3(a.dst + 3 * idx[2]);
            ok = triple_ok(s0, s1, s2) && triple_ok(d0, d1, d2);
            if(ok)
            {
                const V3 sbar = (1.0 / 3.0) * (s0 + s1 + s2), dbar = (1.0 / 3.0) * (d0 + d1 + d2);
                const V3 sc[3] = {s0 - sbar, s1 - sbar, s2 - sbar}, dc[3] = {d0 - dbar, d1 - dbar, d2 - dbar};
                double S[9];
#pragma unroll
                for(int j = 0; j < 9; ++j)
                    S[j] = 0.0;
#pragma unroll
                for(int k = 0; k < 3; ++k)
                {
                    S[0] += sc[k].x * dc[k].x, S[1] += sc[k].x * dc[k].y, S[2] += sc[k].x * dc[k].z;
                    S[3] += sc[k].y * dc[k].x, S[4] += sc[k].y * dc[k].y, S[5] += sc[k].y * dc[k].z;
                    S[6] += sc[k].z * dc[k].x, S[7] += sc[k].z * dc[k].y, S[8] += sc[k].z * dc[k].z;
                }
                rigid_from_covariance(S, sbar, dbar, R, t);
            }
        }
        double* hp = hyp + (size_t)h * 12;
        for(int j = 0; j < 9; ++j)
            hp[j] = ok ? R[j] : 0.0;
        for(int j = 0; j < 3; ++j)
            hp[9 + j] = ok ? t[j] : 0.0;
        counts[h] = ok ? 0 : -1;
    }

    // ---- 2. score every hypothesis against every point: wave w takes hypotheses w, w+4, ...
    const int n_lds = min(n, kAlignLdsPts);
    for(int i = tid; i < n_lds; i += kAlignThreads)
    {
        pts[6 * i] = a.src[3 * i], pts[6 * i + 1] = a.src[3 * i + 1], pts[6 * i + 2] = a.src[3 * i + 2];
        pts[6 * i + 3] = a.dst[3 * i], pts[6 * i + 4] = a.dst[3 * i + 1], pts[6 * i + 5] = a.dst[3 * i + 2];
    }
    if(tid == 0)
        s_best = -1, s_cnt = -1, s_niters = a.iterations;
    __syncthreads();
    const bool in_lds = n <= n_lds; // workgroup-uniform
    // Rounds of one hypothesis per wave; after every round thread 0 walks the round's hypotheses in order, exactly as the
    // sequential RANSAC loop would (a new best hypothesis lowers s_niters; a hypothesis at or beyond s_niters is never
    // looked at)
    {
        const int lane = tid & 63, wave = tid >> 6;
        constexpr int W = kAlignThreads / 64;
        for(int h0 = 0; h0 < s_niters; h0 += W)
        {
            const int h = h0 + wave;
            if(h < a.iterations && counts[h] >= 0)
            {
                double hp[12];
                for(int j = 0; j < 12; ++j)
                    hp[j] = hyp[(size_t)h * 12 + j];
                int c = 0;
                if(in_lds)
                {
                    auto one = [&](int i) -> int {
                        if(i >= n)
                            return 0;
                        const float* po = pts + 6 * i;
                        return align_inlier(hp, hp + 9, load3(po), load3(po + 3), a.thr2) ? 1 : 0;
                    };
                    for(int i = lane; i < n; i += 256)
                        c += one(i) + one(i + 64) + one(i + 128) + one(i + 192);
                }
                else
                {
                    // (not unrolled: the compiler's own unrolling of this loop hoists every load and takes the kernel from
                    // 146 VGPRs to 256 + 44 AGPRs)
#pragma unroll 1
                    for(int i = lane; i < n; i += 64)
                        c += align_inlier(hp, hp + 9, load3(a.src + 3 * (size_t)i), load3(a.dst + 3 * (size_t)i), a.thr2) ? 1 : 0;
                }
                for(int o = 32; o > 0; o >>= 1)
                    c += __shfl_xor(c, o);
                if(lane == 0)
                    counts[h] = c;
            }
            __syncthreads();
            if(tid == 0)
            {
                int best = s_best, bc = s_cnt, niters = s_niters;
                for(int k = 0; k < W && h0 + k < niters; ++k)
                {
                    const int hh = h0 + k;
                    if(counts[hh] > max(bc, kAlignModelPoints))
                    {
                        bc = counts[hh], best = hh;
                        niters = ransac_update_iters(a.confidence, (double)(n - bc) / (double)n, kAlignModelPoints, niters);
                    }
                }
                s_best = best, s_cnt = bc, s_niters = niters;
            }
            __syncthreads();
        }
    }
    const int best = s_best;
    if(best < 0)
    {
        if(tid == 0)
        {
            for(int j = 0; j < 12; ++j)
                a.out[j] = 0.0;
            a.out[12] = 0.0, a.out[13] = -1.0, a.out[14] = 0.0, a.out[15] = 0.0; // status 0: no model
        }
        for(int i = tid; i < n; i += kAlignThreads)
            a.mask[i] = 0;
        return;
    }
    // ---- 3. consensus set of the best hypothesis
    {
        const double* hp = hyp + (size_t)best * 12;
        for(int i = tid; i < n; i += kAlignThreads)
        {
            const bool in = align_inlier(hp, hp + 9, load3(a.src + 3 * (size_t)i), load3(a.dst + 3 * (size_t)i), a.thr2);
            a.mask[i] = in ? 1 : 0;
            if(i < n_lds)
                l_mask[i] = in ? 1 : 0;
        }
    }
    __syncthreads();
    // ---- 4. the closed form over the consensus set: centroids first, then the centred products
    auto fetch = [&](int i, V3& s, V3& d) -> bool {
        if(in_lds)
        {
            if(!l_mask[i])
                return false;
            s = load3(pts + 6 * i), d = load3(pts + 6 * i + 3);
            return true;
        }
        if(!a.mask[i])
            return false;
        s = load3(a.src + 3 * (size_t)i), d = load3(a.dst + 3 * (size_t)i);
        return true;
    };
    const double inv_cnt = 1.0 / (double)s_cnt;
    double acc[9];
#pragma unroll
    for(int j = 0; j < 9; ++j)
        acc[j] = 0.0;
    for(int i = tid; i < n; i += kAlignThreads)
    {
        V3 s, d;
        if(!fetch(i, s, d))
            continue;
        acc[0] += s.x, acc[1] += s.y, acc[2] += s.z, acc[3] += d.x, acc[4] += d.y, acc[5] += d.z;
    }
    wg_sum<6>(acc, red, tid);
    const V3 sbar = v3(red[0] * inv_cnt, red[1] * inv_cnt, red[2] * inv_cnt);
    const V3 dbar = v3(red[3] * inv_cnt, red[4] * inv_cnt, red[5] * inv_cnt);
    __syncthreads(); // red[] is read before wg_sum writes it again
#pragma unroll
    for(int j = 0; j < 9; ++j)
        acc[j] = 0.0;
    for(int i = tid; i < n; i += kAlignThreads)
    {
        V3 s, d;
        if(!fetch(i, s, d))
            continue;
        const V3 sc = s - sbar, dc = d - dbar;
        acc[0] += sc.x * dc.x, acc[1] += sc.x * dc.y, acc[2] += sc.x * dc.z;
        acc[3] += sc.y * dc.x, acc[4] += sc.y * dc.y, acc[5] += sc.y * dc.z;
        acc[6] += sc.z * dc.x, acc[7] += sc.z * dc.y, acc[8] += sc.z * dc.z;
    }
    wg_sum<9>(acc, red, tid);
    if(tid == 0)
    {
        double S[9], R[9], t[3];
#pragma unroll
        for(int j = 0; j < 9; ++j)
            S[j] = red[j];
        rigid_from_covariance(S, sbar, dbar, R, t);
        for(int j = 0; j < 9; ++j)
            a.out[j] = R[j];
        a.out[9] = t[0], a.out[10] = t[1], a.out[11] = t[2];
        a.out[12] = (double)s_cnt;
        a.out[13] = (double)best;
        a.out[14] = 1.0;
        a.out[15] = 0.0;
    }
}

__global__ __launch_bounds__(kAlignThreads) void k_align_ransac(AlignArgs a)
{
    extern __shared__ double red[];
    align_problem(a, red);
}

struct AlignBatchArgs
{
    AlignArgs proto;  // iterations, threshold, seed; pointers = problem 0's slices
    const int32_t* n; // [B] correspondences per problem
    int cap;          // per-problem stride (points)
};

__global__ __launch_bounds__(kAlignThreads) void k_align_ransac_batch(AlignBatchArgs b)
{
    extern __shared__ double red[];
    const int t = blockIdx.x;
    AlignArgs a = b.proto;
    a.n = min(b.n[t], b.cap);
    a.src += (size_t)t * b.cap * 3;
    a.dst += (size_t)t * b.cap * 3;
    a.mask += (size_t)t * b.cap;
    a.hyp += (size_t)t * a.iterations * 12;
    a.counts += (size_t)t * a.iterations;
    a.out += (size_t)t * 16;
    a.seed += (unsigned long long)t;
    if(a.n < 3)
    {
        if(threadIdx.x < 16)
            a.out[threadIdx.x] = threadIdx.x == 13 ? -1.0 : 0.0; // status 0: no model
        if(threadIdx.x < max(a.n, 0))
            a.mask[threadIdx.x] = 0;
        return;
    }
    align_problem(a, red);
}

// frame t: matches (from = keypoint of t, to = keypoint of t-1) with a valid 3-D point at both ends, in match order
__global__ __launch_bounds__(256) void k_align_gather(const int32_t* __restrict__ mfrom, const int32_t* __restrict__ mto,
                                                      const int32_t* __restrict__ mcount, const double* __restrict__ xyz,
                                                      const uint8_t* __restrict__ valid, int cap, float* __restrict__ src,
                                                      float* __restrict__ dst, int32_t* __restrict__ n_out)
{
    __shared__ uint32_t wsum[4];
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = t >= 1 ? min(max(mcount[t], 0), cap) : 0;
    const size_t ft = (size_t)t * cap, fp = t >= 1 ? (size_t)(t - 1) * cap : 0;
    uint32_t running = 0;
    for(int base = 0; base < m; base += 256)
    {
        const int i = base + tid;
        int from = 0, to = 0;
        bool ok = false;
        if(i < m)
        {
            from = mfrom[ft + i], to = mto[ft + i];
            ok = (unsigned)from < (unsigned)cap && (unsigned)to < (unsigned)cap && valid[fp + to] != 0 && valid[ft + from] != 0;
        }
        const unsigned long long b = __ballot(ok);
        if(lane == 0)
            wsum[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t pre = 0, tot = 0;
        for(int k = 0; k < 4; ++k)
        {
            pre += k < wave ? wsum[k] : 0;
            tot += wsum[k];
        }
        if(ok)
        {
            const size_t o = ft + running + pre + (uint32_t)__popcll(b & ((1ull << lane) - 1ull)); // < ft + m <= ft + cap
            const double* P = xyz + (fp + to) * 3;
            const double* Q = xyz + (ft + from) * 3;
            src[o * 3] = (float)P[0], src[o * 3 + 1] = (float)P[1], src[o * 3 + 2] = (float)P[2];
            dst[o * 3] = (float)Q[0], dst[o * 3 + 1] = (float)Q[1], dst[o * 3 + 2] = (float)Q[2];
        }
        running += tot;
        __syncthreads();
    }
    if(tid == 0)
        n_out[t] = (int32_t)running;
}

} // namespace mslam

using namespace mslam;

// Rodrigues vector of a rotation through its unit quaternion (the largest of the four candidates is the pivot), so that a
// rotation by 180 degrees keeps every digit: the record's R comes from a quaternion and is orthonormal to rounding
static void rotation_to_rvec(const double R[9], double r[3])
{
    const double tr = R[0] + R[4] + R[8];
    double w, x, y, z;
    if(tr >= R[0] && tr >= R[4] && tr >= R[8])
    {
        w = 1.0 + tr, x = R[7] - R[5], y = R[2] - R[6], z = R[3] - R[1];
    }
    else if(R[0] >= R[4] && R[0] >= R[8])
    {
        w = R[7] - R[5], x = 1.0 + R[0] - R[4] - R[8], y = R[1] + R[3], z = R[2] + R[6];
    }
    else if(R[4] >= R[8])
    {
        w = R[2] - R[6], x = R[1] + R[3], y = 1.0 - R[0] + R[4] - R[8], z = R[5] + R[7];
    }
    else
    {
        w = R[3] - R[1], x = R[2] + R[6], y = R[5] + R[7], z = 1.0 - R[0] - R[4] + R[8];
    }
    if(w < 0.0)
        w = -w, x = -x, y = -y, z = -z;
    const double vn = std::sqrt(x * x + y * y + z * z);
    if(!(vn > 0.0))
    {
        r[0] = r[1] = r[2] = 0.0;
        return;
    }
    const double k = 2.0 * std::atan2(vn, w) / vn;
    r[0] = k * x, r[1] = k * y, r[2] = k * z;
}

static void align_fill(AlignArgs& a, mslam_hip_ctx* c, int iterations, double max_distance, unsigned long long seed)
{
    a.iterations = iterations;
    a.confidence = c->pnp_confidence;
    a.thr2 = max_distance * max_distance;
    a.seed = seed;
}

extern "C" int mslam_hip_align_ransac(mslam_hip_ctx* c, const float* src, const float* dst, int n, int iterations,
                                      double max_distance, uint64_t seed, double* rvec, double* tvec, uint8_t* inliers,
                                      int* n_inliers)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    if(!src || !dst || !rvec || !tvec || n < 3 || iterations < 1 || iterations > 4096 || !(max_distance > 0))
        return fail(c, MSLAM_HIP_E_INVALID, "align_ransac: bad argument (at least 3 points, 1..4096 iterations, max_distance > 0; a model needs 4 inliers)");
    if(n_inliers)
        *n_inliers = 0;
    hipError_t e = hipSetDevice(c->p.device);
#define ACHK(call)                                                                                                     \
    if(e == hipSuccess)                                                                                                \
    e = (call)
    // scratch of the single-problem call lives in the context and only grows, as mslam_hip_pnp_ransac's does
    if(n > c->align1_n_cap || iterations > c->align1_it_cap)
    {
        ACHK(hipStreamSynchronize(c->stream)); // what reads the old blocks has finished before they are freed
        const size_t n_cap = std::max({n, 1024, c->align1_n_cap}), it_cap = std::max({iterations, 128, c->align1_it_cap});
        c->align1_n_cap = c->align1_it_cap = 0;
        ACHK(c->d_align1_src.alloc(n_cap * 3));
        ACHK(c->d_align1_dst.alloc(n_cap * 3));
        ACHK(c->d_align1_hyp.alloc(it_cap * 12));
        if(!c->d_align1_out)
            ACHK(c->d_align1_out.alloc(16));
        ACHK(c->d_align1_counts.alloc(it_cap));
        ACHK(c->d_align1_mask.alloc(n_cap));
        if(e == hipSuccess)
            c->align1_n_cap = (int)n_cap, c->align1_it_cap = (int)it_cap;
    }
    ACHK(hipMemcpyAsync(c->d_align1_src, src, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
    ACHK(hipMemcpyAsync(c->d_align1_dst, dst, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
    AlignArgs a{};
    a.src = c->d_align1_src, a.dst = c->d_align1_dst, a.n = n;
    align_fill(a, c, iterations, max_distance, seed);
    a.hyp = c->d_align1_hyp, a.counts = c->d_align1_counts, a.mask = c->d_align1_mask, a.out = c->d_align1_out;
    if(e == hipSuccess)
        hipLaunchKernelGGL(k_align_ransac, dim3(1), dim3(kAlignThreads), kAlignLdsBytes, c->stream, a);
    ACHK(hipGetLastError());
    double out[16] = {0};
    std::vector<uint8_t> mask((size_t)n);
    ACHK(hipMemcpyAsync(out, c->d_align1_out, sizeof(out), hipMemcpyDeviceToHost, c->stream));
    ACHK(hipMemcpyAsync(mask.data(), c->d_align1_mask, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    ACHK(hipStreamSynchronize(c->stream));
#undef ACHK
    if(e != hipSuccess)
        return fail(c, MSLAM_HIP_E_RUNTIME, std::string("align_ransac: ") + hipGetErrorString(e));
    if(out[14] != 1.0)
        return fail(c, MSLAM_HIP_E_NO_MODEL, "align_ransac: no hypothesis reached 4 inliers");
    rotation_to_rvec(out, rvec);
    tvec[0] = out[9], tvec[1] = out[10], tvec[2] = out[11];
    if(inliers)
        std::memcpy(inliers, mask.data(), (size_t)n);
    if(n_inliers)
        *n_inliers = (int)out[12];
    return MSLAM_HIP_OK;
}

static int align_batch_buffers(mslam_hip_ctx* c, int iterations)
{
    const size_t B = (size_t)c->p.max_batch, K = (size_t)c->p.max_keypoints;
    if(c->d_align_src && c->align_iterations >= iterations)
        return MSLAM_HIP_OK;
    const size_t it = (size_t)iterations;
    c->align_iterations = 0; // until every block is there
    hipError_t e = hipStreamSynchronize(c->stream); // a launch that reads the old blocks has finished
    if(e == hipSuccess) e = c->d_align_src.alloc(B * K * 3);
    if(e == hipSuccess) e = c->d_align_dst.alloc(B * K * 3);
    if(e == hipSuccess) e = c->d_align_n.alloc(B);
    if(e == hipSuccess) e = c->d_align_counts.alloc(B * it);
    if(e == hipSuccess) e = c->d_align_hyp.alloc(B * it * 12);
    if(e == hipSuccess) e = c->d_align_out.alloc(B * 16);
    if(e == hipSuccess) e = c->d_align_mask.alloc(B * K);
    if(e == hipSuccess) e = hipMemset(c->d_align_n, 0, B * 4);
    if(e == hipSuccess) e = hipMemset(c->d_align_out, 0, B * 16 * 8);
    if(e != hipSuccess)
        return fail(c, MSLAM_HIP_E_RUNTIME, std::string("align_batch_dev: ") + hipGetErrorString(e));
    c->align_iterations = iterations;
    return MSLAM_HIP_OK;
}

extern "C" int mslam_hip_align_batch_dev(mslam_hip_ctx* c, int iterations, double max_distance, uint64_t seed)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    if(iterations < 1 || iterations > 4096 || !(max_distance > 0))
        return fail(c, MSLAM_HIP_E_INVALID, "align_batch_dev: bad argument (1..4096 iterations, max_distance > 0)");
    if(c->n_last < 1 || !c->d_xyz)
        return fail(c, MSLAM_HIP_E_INVALID, "align_batch_dev: needs a detect batch, its matches and its back-projection");
    if(hipSetDevice(c->p.device) != hipSuccess)
        return fail(c, MSLAM_HIP_E_RUNTIME, "align_batch_dev: hipSetDevice");
    int rc = align_batch_buffers(c, iterations);
    if(rc)
        return rc;
    rc = mslam_hip_join_matcher(c); // the matches come from the matcher's stream
    if(rc)
        return rc;
    const int K = c->p.max_keypoints, n = c->n_last;
    {
        StageScope t(c, "align_gather");
        // (the points of the batch's frame 0 sit one slot into the output set's arrays, as in mslam_hip_pnp_batch_dev the
        // coordinates do; d_xyz / d_valid hold the batch's frames only)
        hipLaunchKernelGGL(k_align_gather, dim3(n), dim3(256), 0, c->stream, cur_out(c).mfrom, cur_out(c).mto, cur_out(c).mcount,
                           c->d_xyz, c->d_valid, K, c->d_align_src, c->d_align_dst, c->d_align_n);
    }
    AlignBatchLaunch l{};
    l.src = c->d_align_src, l.dst = c->d_align_dst, l.n = c->d_align_n;
    l.n_problems = n, l.cap = K;
    l.iterations = iterations, l.max_distance = max_distance, l.seed = seed;
    l.hyp = c->d_align_hyp, l.counts = c->d_align_counts, l.mask = c->d_align_mask, l.out = c->d_align_out;
    return align_launch_batch(c, l);
}

namespace mslam
{
int align_launch_batch(mslam_hip_ctx* c, const AlignBatchLaunch& l)
{
    AlignBatchArgs b{};
    AlignArgs& a = b.proto;
    a.src = l.src, a.dst = l.dst, a.n = 0;
    align_fill(a, c, l.iterations, l.max_distance, l.seed);
    a.hyp = l.hyp, a.counts = l.counts, a.mask = l.mask, a.out = l.out;
    b.n = l.n;
    b.cap = l.cap;
    {
        StageScope t(c, "align_ransac");
        hipLaunchKernelGGL(k_align_ransac_batch, dim3(l.n_problems), dim3(kAlignThreads), kAlignLdsBytes, c->stream, b);
    }
    if(hipGetLastError() != hipSuccess)
        return fail(c, MSLAM_HIP_E_RUNTIME, "align: launch failed");
    return MSLAM_HIP_OK;
}
} // namespace mslam

extern "C" int mslam_hip_get_align_view(mslam_hip_ctx* c, mslam_hip_align_view* v)
{
    if(!c || !v)
        return MSLAM_HIP_E_INVALID;
    if(!c->d_align_src && !c->d_align1_out)
        return fail(c, MSLAM_HIP_E_INVALID, "get_align_view: neither mslam_hip_align_batch_dev nor mslam_hip_align_ransac has run");
    v->capacity = c->p.max_keypoints;
    v->pose = c->d_align_out;
    v->n_points = c->d_align_n;
    v->src_points = c->d_align_src;
    v->dst_points = c->d_align_dst;
    v->inliers = c->d_align_mask;
    v->single_pose = c->d_align1_out;
    return MSLAM_HIP_OK;
}

extern "C" int mslam_hip_set_track_pose(mslam_hip_ctx* c, int kind, double max_distance)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    if(kind != MSLAM_HIP_TRACK_POSE_PNP && kind != MSLAM_HIP_TRACK_POSE_ALIGN)
        return fail(c, MSLAM_HIP_E_INVALID, "set_track_pose: unknown kind");
    if(kind == MSLAM_HIP_TRACK_POSE_ALIGN && !(max_distance > 0))
        return fail(c, MSLAM_HIP_E_INVALID, "set_track_pose: ALIGN needs max_distance > 0");
    c->track_pose_kind = kind;
    c->track_align_distance = kind == MSLAM_HIP_TRACK_POSE_ALIGN ? max_distance : 0.0;
    return MSLAM_HIP_OK;
}

extern "C" int mslam_hip_get_track_pose(mslam_hip_ctx* c, int* kind, double* max_distance)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    if(kind)
        *kind = c->track_pose_kind;
    if(max_distance)
        *max_distance = c->track_align_distance;
    return MSLAM_HIP_OK;
}
