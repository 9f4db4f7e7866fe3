// distinct.hpp — the per-lane pieces of the union's DISTINCTIVE descriptor mode (k_localmap.hip: k_lm_distinct), callable on
// the host as well: tests/test_distinct_union.py compiles them into a small host program and holds tests/distinct_ref.py's
// restatement to them, as tests/test_lm_table_edges.py does with lm_hash.
//
// The rule (ORB-SLAM's MapPoint::ComputeDistinctiveDescriptors): among the N observations of a landmark, the descriptor
// whose median Hamming distance to all N of them (itself included, distance 0) is the least; median = the
// (N - 1) / 2-th smallest, counted from 0.  Ties go to the observation of the largest rank.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mslam
{

// popcount of the xor over the 256 bits: 0 .. 256 (256 needs nine bits)
__host__ __device__ __forceinline__ uint32_t distinct_distance(const uint32_t* a, const uint32_t* b)
{
    uint32_t d = 0;
    for(int w = 0; w < 8; ++w)
    {
#if defined(__HIP_DEVICE_COMPILE__)
        d += (uint32_t)__popc(a[w] ^ b[w]);
#else
        d += (uint32_t)__builtin_popcount(a[w] ^ b[w]);
#endif
    }
    return d;
}

// the m-th smallest (from 0) of the n values row[0], row[stride], .. row[(n - 1) * stride], each in 0 .. 256, 0 <= m < n:
// the least v with at least m + 1 values <= v, by bisection on 0 .. 256 — nine rounds halve 257 candidates to one
__host__ __device__ __forceinline__ uint32_t distinct_mth_smallest(const uint16_t* row, int stride, int n, int m)
{
    uint32_t lo = 0, hi = 256;
    for(int round = 0; round < 9; ++round)
    {
        const uint32_t mid = (lo + hi) >> 1;
        int below = 0;
        for(int c = 0; c < n; ++c)
            below += row[c * stride] <= mid ? 1 : 0;
        if(below > m)
            hi = mid;
        else
            lo = mid + 1;
    }
    return hi;
}

// what the wave reduces to its minimum: the least median first, then the largest rank (0 .. 63; ranks are unique, so the
// winner is).  The median takes nine bits: (256 << 6) | 63 = 16447.
__host__ __device__ __forceinline__ uint32_t distinct_key(uint32_t median, int rank) { return (median << 6) | (uint32_t)(63 - rank); }

constexpr uint32_t kDistinctAbsent = 0xFFFFFFFFu; // the key of a lane that holds no observation: above every key

} // namespace mslam
