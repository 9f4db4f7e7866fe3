// lm_table.hpp — the open-addressing table on landmark ids that k_localmap.hip (union, covisibility, the list rewrite),
// k_fuse.hip (eligibility), k_cull.hip (observer counts) and k_lmcull.hip (judged landmarks, the ids to remove) share: {u64 key, u64 val} buckets, a power of two of them and at
// least twice the keys that can be inserted, cleared to all-ones (a landmark id is never all-ones: ids are below 2^63),
// linear probing.  A key is claimed with one compare-and-swap; what the value holds is the caller's.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace mslam
{

struct LmBucket
{
    unsigned long long key, val;
};

constexpr unsigned long long kLmEmpty = ~0ull;

// splitmix64's finaliser (callable on the host as well: tests/test_lm_table_edges.py holds its restatement to this one)
__host__ __device__ __forceinline__ unsigned long long lm_hash(unsigned long long x)
{
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

// a table as kernels take it, by value: its buckets and their number less one
struct LmTable
{
    LmBucket* b;
    unsigned long long mask;
};

// the bucket of `key`, claimed if no thread has claimed one for it yet.  The table has at least twice as many buckets as
// keys are ever inserted, so the walk ends; it is bounded by the table's size all the same (-1: cannot happen).
__device__ __forceinline__ long long lm_claim(LmTable t, unsigned long long key)
{
    unsigned long long h = lm_hash(key) & t.mask;
    for(unsigned long long step = 0; step <= t.mask; ++step)
    {
        const unsigned long long prev = atomicCAS(&t.b[h].key, kLmEmpty, key);
        if(prev == kLmEmpty || prev == key)
            return (long long)h;
        h = (h + 1) & t.mask;
    }
    return -1;
}

// the bucket of `key`, -1 when the table does not hold it (read-only: every insert is in an earlier launch)
__device__ __forceinline__ long long lm_find(LmTable t, unsigned long long key)
{
    unsigned long long h = lm_hash(key) & t.mask;
    for(unsigned long long step = 0; step <= t.mask; ++step)
    {
        const unsigned long long k = t.b[h].key;
        if(k == key)
            return (long long)h;
        if(k == kLmEmpty)
            return -1;
        h = (h + 1) & t.mask;
    }
    return -1;
}

inline size_t lm_bucket_count(size_t keys)
{
    size_t b = 64;
    while(b < 2 * keys)
        b <<= 1;
    return b;
}

inline size_t lm_bytes(LmTable t) // what a clear of the table covers
{
    return (size_t)(t.mask + 1) * sizeof(LmBucket);
}

} // namespace mslam
