// compact.hpp — the in-place compaction of one keyframe-store entry by one workgroup, which k_prune.hip (the named
// observations leave) and k_lmcull.hip (the culled or listed landmarks leave) share; what differs is the drop test.
//
// The workgroup walks its entry in chunks of kCompactChunk positions: a thread loads its landmark (id, descriptor, world
// point: 8 + 32 + 24 bytes) into registers, asks `drop(id)`, and a workgroup scan of the keep flags (a ballot per wave, one
// LDS word per wave) gives the landmark's destination.  The scan's barrier separates the chunk's loads from its stores; a
// destination never lies above its source (dst <= i) and a chunk's stores end below the next chunk's loads, so the
// compaction needs no second buffer.  A landmark that stays where it is issues no store: an entry that loses nothing is
// not written at all.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace mslam
{

constexpr int kCompactChunk = 256; // positions per chunk = threads per workgroup (tests/prune_ref.py: T)

// Called by every thread of a workgroup of kCompactChunk threads.  base = slot * K, n = the entry's count; drop(id) is
// called once per live position (it may count its hits: an integer atomicAdd, whose value does not depend on the order)
// -> the number of landmarks kept, the same in every thread.  store_* are read and written through the same pointers: no
// __restrict__ on them.
template <class Drop>
__device__ __forceinline__ int compact_entry(uint8_t* store_desc, double* store_world, int64_t* store_lid, size_t base, int n, Drop drop)
{
    constexpr int kWaves = kCompactChunk / 64;
    __shared__ int s_wave[2][kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int running = 0; // landmarks kept below this chunk: the same in every thread
    for(int start = 0, chunk = 0; start < n; start += kCompactChunk, ++chunk)
    {
        const int i = start + tid;
        const bool live = i < n;
        bool keep = false;
        int64_t lid = 0;
        uint4 d0{}, d1{};
        double w0 = 0.0, w1 = 0.0, w2 = 0.0;
        if(live)
        {
            const size_t at = base + i;
            lid = store_lid[at];
            const uint4* d = reinterpret_cast<const uint4*>(store_desc + at * 32);
            d0 = d[0], d1 = d[1];
            w0 = store_world[at * 3], w1 = store_world[at * 3 + 1], w2 = store_world[at * 3 + 2];
            keep = !drop(lid);
        }
        const unsigned long long bal = __ballot(keep);
        if(lane == 0)
            s_wave[chunk & 1][wave] = (int)__popcll(bal);
        // every load of the chunk has returned before any of its stores is issued.  (The two halves of s_wave alternate:
        // a thread that writes half h again has passed the barrier of the chunk in between, which every thread reaches
        // only after its reads of h.)
        __syncthreads();
        int before = 0, total = 0;
        for(int w = 0; w < kWaves; ++w)
        {
            const int cnt = s_wave[chunk & 1][w];
            before += w < wave ? cnt : 0;
            total += cnt;
        }
        const int dst = running + before + (int)__popcll(bal & ((1ull << lane) - 1ull));
        if(keep && dst != i) // dst <= i always
        {
            const size_t to = base + dst;
            store_lid[to] = lid;
            uint4* d = reinterpret_cast<uint4*>(store_desc + to * 32);
            d[0] = d0, d[1] = d1;
            store_world[to * 3] = w0, store_world[to * 3 + 1] = w1, store_world[to * 3 + 2] = w2;
        }
        running += total;
    }
    return running;
}

} // namespace mslam
