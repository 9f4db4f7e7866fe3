// guided_walk.hpp — the device side of "match inside a window round a projection", stated once for guided matching
// (k_match_guided.hip) and landmark fusion (k_fuse.hip, k_fuse_multi.hip): the f64 pinhole projection, the in-frame test
// and cell of a keypoint, the counting sort of a row's keypoints into cells, the cells a window overlaps, the 256-bit
// Hamming distance and the knn-2 walk over the listed keypoints.  Every result is a function of the keys
// dist << 16 | index alone: it depends neither on the cell size nor on the order inside a cell.
#pragma once
#include "reloc.hpp"

namespace mslam
{

// camera = R * world + t, (u, v) = the pinhole image of it.  All f64, every operation rounded on its own
// (-ffp-contract=off), in the order written; c2 <= 0 is behind the camera, and u, v are then whatever the division gives.
struct GuidedUV
{
    double u, v, c2;
};
__device__ __forceinline__ GuidedUV guided_project(const double* R, const double* t, double fx, double fy, double cx, double cy,
                                                   const double* __restrict__ P)
{
    const double X = P[0], Y = P[1], Z = P[2];
    const double c0 = ((R[0] * X + R[1] * Y) + R[2] * Z) + t[0];
    const double c1 = ((R[3] * X + R[4] * Y) + R[5] * Z) + t[1];
    const double c2 = ((R[6] * X + R[7] * Y) + R[8] * Z) + t[2];
    return GuidedUV{(c0 / c2) * fx + cx, (c1 / c2) * fy + cy, c2};
}

__device__ __forceinline__ uint32_t guided_hamming(const uint4& da, const uint4& db, const uint4& qa, const uint4& qb)
{
    return (uint32_t)(((__popc(da.x ^ qa.x) + __popc(da.y ^ qa.y)) + (__popc(da.z ^ qa.z) + __popc(da.w ^ qa.w))) +
                      ((__popc(db.x ^ qb.x) + __popc(db.y ^ qb.y)) + (__popc(db.z ^ qb.z) + __popc(db.w ^ qb.w))));
}

// the cell of a keypoint, or -1 when it is not in the frame (NaN and infinities fail the comparisons)
__device__ __forceinline__ int guided_cell(float x, float y, int width, int height, const GuidedGrid& g)
{
    const double dx = (double)x, dy = (double)y;
    if(!(dx >= 0.0 && dx < (double)width && dy >= 0.0 && dy < (double)height))
        return -1;
    return ((int)y >> g.shift) * g.nx + ((int)x >> g.shift); // (int) of [0, extent): 0 .. extent - 1
}

// the cells [lo, hi] (inclusive) a window [u - radius, u + radius] can hold keypoints of, along one axis of `extent` pixels;
// false: none.  Conservative: the window is widened by a pixel and by a bound of the roundings of u - radius, of the
// membership test's x - u and of this sum, and everything is clamped in f64 before the conversion (u can be +-1e300, an
// infinity or a NaN).  A NaN bound selects every cell; the exact membership test decides.
__device__ __forceinline__ bool guided_span(double u, double radius, int extent, int shift, int* lo, int* hi)
{
    const double m = 1.0 + (fabs(u) + radius) * 0x1p-50;
    const double a = (u - radius) - m, b = (u + radius) + m, last = (double)(extent - 1);
    if(a > last || b < 0.0)
        return false;
    *lo = (a > 0.0 ? (int)a : 0) >> shift;        // 0 < a <= last
    *hi = (b < last ? (int)b : extent - 1) >> shift; // 0 <= b < last
    return true;
}

// one row of the binning: n keypoints (coordinates and descriptors) in, the row's cell offsets and list out
struct GuidedBinRow
{
    const float* xy;     // [n][2]
    const uint8_t* desc; // [n][32]
    int n;
    int32_t* cell_off;  // [kGuidedMaxCells + 1]
    float4* list;       // [n]
    uint8_t* list_desc; // [n][32]
};

// (1024 threads: the two walks over the row's keypoints are a chain of dependent fetches per thread; more threads, shorter chains)
constexpr int kGuidedBinThreads = 1024;

// A workgroup of kGuidedBinThreads threads: counting sort of the row's in-frame keypoints into square cells (LDS histogram,
// scan, scatter) -> cell offsets + a list that holds, cell by cell, each keypoint's coordinates, index and a copy of its
// descriptor.  The order inside a cell is the scatter's and not deterministic.
__device__ __forceinline__ void guided_bin_row(const GuidedBinRow& r, int width, int height, const GuidedGrid& grid)
{
    __shared__ uint32_t cell[kGuidedMaxCells]; // counts, then running offsets
    __shared__ uint32_t wtot[kGuidedBinThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_cells = grid.nx * grid.ny; // <= kGuidedMaxCells (guided_grid)
    for(int c = tid; c < n_cells; c += kGuidedBinThreads)
        cell[c] = 0;
    __syncthreads();
    for(int i = tid; i < r.n; i += kGuidedBinThreads)
    {
        const int c = guided_cell(r.xy[2 * (size_t)i], r.xy[2 * (size_t)i + 1], width, height, grid);
        if(c >= 0)
            atomicAdd(&cell[c], 1u);
    }
    __syncthreads();
    // exclusive scan: thread t owns the cells [t * per, t * per + per)
    const int per = (n_cells + kGuidedBinThreads - 1) / kGuidedBinThreads, c0 = tid * per, c1 = min(c0 + per, n_cells);
    uint32_t mine = 0;
    for(int c = c0; c < c1; ++c)
        mine += cell[c];
    uint32_t incl = mine;
    for(int o = 1; o < 64; o <<= 1)
    {
        const uint32_t up = __shfl_up(incl, o);
        if(lane >= o)
            incl += up;
    }
    if(lane == 63)
        wtot[wave] = incl;
    __syncthreads();
    uint32_t run = incl - mine;
    for(int w = 0; w < wave; ++w)
        run += wtot[w];
    for(int c = c0; c < c1; ++c)
    {
        const uint32_t k = cell[c];
        cell[c] = run;
        r.cell_off[c] = (int32_t)run;
        run += k;
    }
    if(tid == kGuidedBinThreads - 1)
        r.cell_off[n_cells] = (int32_t)run; // the in-frame keypoints of the row: <= n
    __syncthreads();
    for(int i = tid; i < r.n; i += kGuidedBinThreads)
    {
        const float x = r.xy[2 * (size_t)i], y = r.xy[2 * (size_t)i + 1];
        const int c = guided_cell(x, y, width, height, grid);
        if(c >= 0)
        {
            const size_t pos = atomicAdd(&cell[c], 1u); // < the row's in-frame count <= n
            r.list[pos] = make_float4(x, y, __int_as_float(i), 0.f);
            copy_desc(r.desc + (size_t)i * 32, r.list_desc + pos * 32);
        }
    }
}

// The knn-2 of one query among a row's listed keypoints, by the eight lanes g = 0 .. 7 of the query: visit the cell rows
// the window round (u, v) overlaps (the cells of one cell row are one contiguous span of the list), each lane tests one
// listed keypoint at a time — exact window membership, then cand(index), then xor / popcount over its 32 bytes against
// the query descriptor q[0 .. 1] — and keeps two minima of dist << 16 | index (index <= 65534); a butterfly merges the
// eight lanes' minima.  -> (k0 <= k1) in all eight lanes, ~0u = absent.  Every lane of the wave calls this, the eight
// lanes of a query with the same arguments; active == false: nothing to search (nothing is read), the lanes only take
// part in the merge.
// kFetchFirst: the listed keypoint's descriptor is fetched together with the keypoint, ahead of both tests (guided
// matching: the gather is latency-bound), or only once cand() has accepted the keypoint (fusion: the gate reads the
// candidate's world point first).  No result shows which; each caller keeps the order it was measured with.
template <bool kFetchFirst, class Cand>
__device__ __forceinline__ uint2 guided_walk(bool active, double u, double v, double radius, int width, int height, const GuidedGrid& grid,
                                             const int32_t* __restrict__ cell_off, const float4* __restrict__ list,
                                             const uint8_t* __restrict__ list_desc_bytes, const uint8_t* __restrict__ q_bytes, int g, Cand&& cand)
{
    uint32_t k0 = ~0u, k1 = ~0u;
    int cx0, cx1, cy0, cy1;
    if(active && guided_span(u, radius, width, grid.shift, &cx0, &cx1) && guided_span(v, radius, height, grid.shift, &cy0, &cy1))
    {
        const uint4* q = reinterpret_cast<const uint4*>(q_bytes);
        const uint4 qa = q[0], qb = q[1];
        const uint4* list_desc = reinterpret_cast<const uint4*>(list_desc_bytes);
        // cells cx0 .. cx1 of a cell row lie side by side in the list; the next cell row's span is fetched while this
        // one is walked
        int b = cell_off[cy0 * grid.nx + cx0], e = cell_off[cy0 * grid.nx + cx1 + 1];
        for(int cy = cy0; cy <= cy1; ++cy)
        {
            int nb = 0, ne = 0;
            if(cy < cy1)
                nb = cell_off[(cy + 1) * grid.nx + cx0], ne = cell_off[(cy + 1) * grid.nx + cx1 + 1];
            for(int p = b + g; p < e; p += 8)
            {
                const float4 pt = list[p];
                uint4 da, db;
                if constexpr(kFetchFirst)
                    da = list_desc[2 * (size_t)p], db = list_desc[2 * (size_t)p + 1];
                if(fabs((double)pt.x - u) <= radius && fabs((double)pt.y - v) <= radius && cand(__float_as_int(pt.z)))
                {
                    if constexpr(!kFetchFirst)
                        da = list_desc[2 * (size_t)p], db = list_desc[2 * (size_t)p + 1];
                    const uint32_t key = (guided_hamming(da, db, qa, qb) << 16) | (uint32_t)__float_as_int(pt.z);
                    k1 = min(k1, max(k0, key));
                    k0 = min(k0, key);
                }
            }
            b = nb, e = ne;
        }
    }
    // the eight lanes' (k0 <= k1) pairs: keys are distinct (one per listed keypoint) apart from the absent key
    for(int o = 1; o < 8; o <<= 1)
    {
        const uint32_t o0 = __shfl_xor(k0, o), o1 = __shfl_xor(k1, o);
        k1 = min(max(k0, o0), min(k1, o1));
        k0 = min(k0, o0);
    }
    return make_uint2(k0, k1);
}

} // namespace mslam
