// ransac_common.hpp — what the two RANSAC kernels share (k_pnp.hip: 3-D / 2-D, P3P; k_align.hip: 3-D / 3-D, rigid
// alignment): the counter-based sampler, the small f64 vector helpers, OpenCV's iteration-count rule and the fixed-order
// workgroup sum of the final refit.  Device code only; both files launch workgroups of kRansacThreads threads.
#pragma once
#include "common.hpp"

namespace mslam
{

__device__ __forceinline__ unsigned long long splitmix(unsigned long long& x)
{
    x += 0x9E3779B97F4A7C15ull;
    unsigned long long z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct V3
{
    double x, y, z;
};
__device__ __forceinline__ V3 v3(double x, double y, double z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 operator*(double s, V3 a) { return v3(s * a.x, s * a.y, s * a.z); }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
__device__ __forceinline__ V3 mulR(const double* R, V3 p)
{
    return v3(R[0] * p.x + R[1] * p.y + R[2] * p.z, R[3] * p.x + R[4] * p.y + R[5] * p.z, R[6] * p.x + R[7] * p.y + R[8] * p.z);
}

// OpenCV's RANSACUpdateNumIters(p, ep, modelPoints, maxIters) (calib3d/src/ptsetreg.cpp): the number of samples after which
// an all-inlier sample has been drawn with probability p when a share ep of the points are outliers
__device__ __forceinline__ int ransac_update_iters(double p, double ep, int model_points, int max_iters)
{
    if(!(p > 0.0) || !(p < 1.0))
        return max_iters; // no early exit asked for
    ep = fmax(ep, 0.0);
    ep = fmin(ep, 1.0);
    double num = fmax(1.0 - p, 2.2250738585072014e-308);
    double w = 1.0 - ep, wm = 1.0;
    for(int i = 0; i < model_points; ++i)
        wm *= w; // pow(1 - ep, modelPoints) for a small integer exponent, in a fixed order
    double denom = 1.0 - wm;
    if(denom < 2.2250738585072014e-308)
        return 0;
    num = log(num);
    denom = log(denom);
    if(denom >= 0 || -num >= max_iters * (-denom))
        return max_iters;
    return (int)rint(num / denom); // cvRound
}

constexpr int kRansacThreads = 256;

// fixed-order workgroup sum of `cnt` doubles per thread (acc[cnt]); the totals land in red[0..cnt).  Butterfly inside
// each wave (cross-lane moves, no memory), then the four wave totals are added in wave order: one barrier pair instead
// of a nine-barrier LDS tree, and 1.2 KB of LDS instead of 57 KB (which held the batched kernel to 2 workgroups per CU).
constexpr int kRansacRed = 32 + 28 * (kRansacThreads / 64); // doubles of LDS: totals [32] + per-wave partials [28][waves]
template <int CNT>
__device__ __forceinline__ void wg_sum(double* acc, double* red, int tid)
{
    const int lane = tid & 63, wave = tid >> 6;
    constexpr int W = kRansacThreads / 64;
    // CNT independent butterflies, fully unrolled: the cross-lane moves of different sums overlap
#pragma unroll
    for(int o = 32; o > 0; o >>= 1)
    {
#pragma unroll
        for(int j = 0; j < CNT; ++j)
            acc[j] += __shfl_xor(acc[j], o);
    }
    if(lane == 0)
    {
#pragma unroll
        for(int j = 0; j < CNT; ++j)
            red[32 + j * W + wave] = acc[j];
    }
    __syncthreads();
    if(tid < CNT)
    {
        double t = red[32 + tid * W];
#pragma unroll
        for(int w = 1; w < W; ++w)
            t += red[32 + tid * W + w];
        red[tid] = t;
    }
    __syncthreads();
}

} // namespace mslam
