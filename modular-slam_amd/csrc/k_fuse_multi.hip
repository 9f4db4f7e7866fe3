// k_fuse_multi.hip — landmark fusion into many target entries in one call: mslam_hip_kf_fuse_search_multi projects the
// landmarks of one entry ("keep") into up to 64 others ("drop" targets), each under its own pose, runs k_fuse.hip's search
// per target, and resolves what the targets found on landmark ids, so that the result is one to one on ids;
// mslam_hip_kf_fuse_multi then rewrites the store through the list rewrite of k_localmap.hip (rewrite_enqueue, reloc.hpp)
// without the pair list leaving the device (the semantics are stated once, at mslam_hip_kf_fuse_search_multi in
// include/mslam_hip.h).  The model is ORB-SLAM's SearchAndFuse over the keyframes connected to the current one; the
// reference has no code for it (closeLoop is an empty body, rgbd_feature_frontend.cpp:577-580).
//
// The target is a grid dimension, so the number of launches does not grow with n_drop:
//
//   k_fusem_ids      the keep entry's ids into one table, every target's ids into another (lm_table.hpp): the second one is
//                    global eligibility for the keep side and, later, the claim board of step A
//   k_fusem_project  one thread per (target, landmark of either side): eligibility and the f64 projection, as k_fuse_project
//   k_fusem_bin      k_guided_bin's counting sort, one workgroup per target, on that target's slice of the drop arrays
//   k_fusem_search   k_fuse_search's walk per (target, keep landmark); the accepted key claims its drop position with
//                    atomicMin of d0 << 16 | keep position (the per-target resolution)
//   k_fusem_claim_a  a keep landmark that holds its drop position is a row; it claims its drop landmark id with
//                    atomicMin of dist << 22 | target << 16 | keep position on the id's bucket of the drop table
//   k_fusem_claim_b  a row that holds its drop id claims its keep landmark id with dist << 22 | target << 16 | drop position
//                    on the keep table
//   k_fusem_count    a row that holds both is a pair; per (target, block of 256 keep positions), the number of them
//   k_fusem_compact  one workgroup per target: its base from the counts of the targets before it, then the ordered
//                    compaction (ballot + scan) of its pairs, which are in keep-position order already
//
// dist <= 256, target < 64 and position < 65536 fit 31 bits, and (target, keep position) as well as (target, drop position)
// name a row, so each claim's key is a total order and no tie is left to arrival order.  Every result is a function of the
// keys alone.  All projection arithmetic is f64, every operation rounded on its own (-ffp-contract=off).
#include "lm_table.hpp"
#include "reloc.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace mslam
{

constexpr int kFuseMaxTargets = 64;

struct FuseMultiHead // the mapped result block's first 16 bytes
{
    int32_t n_pairs, pad[3];
};

// one target, as uploaded
struct FuseTarget
{
    double R[9], t[3];
    int32_t slot, cap, off, pad; // cap: what the host knows the entry's count not to exceed; off: its place in the drop arrays
};

struct FuseMultiPairs
{
    int32_t *target, *keep_pos, *drop_pos, *dist;
    int64_t *keep_lid, *drop_lid;
};

struct FuseMultiArgs
{
    const uint8_t* desc; // the store
    const double* world;
    const int64_t* lid;
    const int32_t* n;
    int K, keep_slot, nk_cap, n_drop;
    const FuseTarget* tgt; // [n_drop], device
    LmTable tab_keep, tab_drop;
    double fx, fy, cx, cy, radius, gate2, ratio;
    int max_distance, width, height;
    GuidedGrid grid;
    float* drop_xy;    // [ND][2], ND = the sum of the targets' caps
    double* keep_uv;   // [n_drop][nk][2]
    uint8_t* keep_ok;  // [n_drop][nk] eligible and in front of the target's camera
    int32_t* cell_off; // [n_drop][kGuidedMaxCells + 1]
    float4* list;      // [ND]
    uint8_t* list_desc; // [ND][32]
    uint32_t* acc;     // [n_drop][nk] the accepted key, or ~0u
    uint32_t* best;    // [ND] cleared to ~0u
    uint8_t* row;      // [n_drop][nk] 0: no row, 1: a row, 2: holds its drop id, 3: a pair
    uint32_t* cnt;     // [n_drop][ceil(nk / 256)] pairs per block of k_fusem_count
    FuseMultiPairs dev, host;
    double* pair_world; // [P][3] the keep landmark's world point
    int32_t* n_pairs;   // device
    FuseMultiHead* head; // mapped
};

__device__ __forceinline__ int fusem_keep_count(const FuseMultiArgs& a)
{
    return min(max(a.n[a.keep_slot], 0), a.nk_cap);
}
__device__ __forceinline__ int fusem_drop_count(const FuseMultiArgs& a, const FuseTarget& t)
{
    return min(max(a.n[t.slot], 0), t.cap);
}
__device__ __forceinline__ uint32_t fusem_key(uint32_t dist, int target, int pos)
{
    return (dist << 22) | ((uint32_t)target << 16) | (uint32_t)pos;
}

// grid (blocks, 1 + n_drop): y = 0 is the keep entry
__global__ __launch_bounds__(256) void k_fusem_ids(FuseMultiArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if(blockIdx.y == 0)
    {
        if(i < fusem_keep_count(a))
            (void)lm_claim(a.tab_keep, (unsigned long long)a.lid[(size_t)a.keep_slot * a.K + i]);
        return;
    }
    const FuseTarget& t = a.tgt[blockIdx.y - 1];
    if(i < fusem_drop_count(a, t))
        (void)lm_claim(a.tab_drop, (unsigned long long)a.lid[(size_t)t.slot * a.K + i]);
}

// grid (blocks, n_drop, 2): z = 0 the keep landmarks under target y's pose, z = 1 target y's own landmarks
__global__ __launch_bounds__(256) void k_fusem_project(FuseMultiArgs a)
{
    const int m = blockIdx.y, side = blockIdx.z, i = blockIdx.x * 256 + threadIdx.x;
    const FuseTarget& t = a.tgt[m];
    if(i >= (side ? fusem_drop_count(a, t) : fusem_keep_count(a)))
        return;
    const size_t at = (size_t)(side ? t.slot : a.keep_slot) * a.K + i;
    const bool eligible = lm_find(side ? a.tab_keep : a.tab_drop, (unsigned long long)a.lid[at]) < 0;
    const double X = a.world[at * 3], Y = a.world[at * 3 + 1], Z = a.world[at * 3 + 2];
    const double c0 = ((t.R[0] * X + t.R[1] * Y) + t.R[2] * Z) + t.t[0];
    const double c1 = ((t.R[3] * X + t.R[4] * Y) + t.R[5] * Z) + t.t[1];
    const double c2 = ((t.R[6] * X + t.R[7] * Y) + t.R[8] * Z) + t.t[2];
    const double u = (c0 / c2) * a.fx + a.cx, v = (c1 / c2) * a.fy + a.cy;
    const bool ok = eligible && c2 > 0.0;
    if(side)
    {
        const float nan = __int_as_float(0x7fc00000);
        const size_t o = (size_t)t.off + i;
        a.drop_xy[2 * o] = ok ? (float)u : nan; // (the in-frame test is the binning's)
        a.drop_xy[2 * o + 1] = ok ? (float)v : nan;
    }
    else
    {
        const size_t o = (size_t)m * a.nk_cap + i;
        a.keep_uv[2 * o] = u, a.keep_uv[2 * o + 1] = v;
        a.keep_ok[o] = ok ? 1 : 0;
    }
}

// the cell of a "keypoint", or -1 when it is not in the frame (NaN and infinities fail the comparisons): k_guided_bin's test
__device__ __forceinline__ int fusem_cell(float x, float y, int width, int height, const GuidedGrid& g)
{
    const double dx = (double)x, dy = (double)y;
    if(!(dx >= 0.0 && dx < (double)width && dy >= 0.0 && dy < (double)height))
        return -1;
    return ((int)y >> g.shift) * g.nx + ((int)x >> g.shift);
}

constexpr int kFusemBinThreads = 1024;

// grid (n_drop): the counting sort of k_guided_bin (LDS histogram, scan, scatter) on target blockIdx.x's slice
__global__ __launch_bounds__(kFusemBinThreads) void k_fusem_bin(FuseMultiArgs a)
{
    __shared__ uint32_t cell[kGuidedMaxCells]; // counts, then running offsets
    __shared__ uint32_t wtot[kFusemBinThreads / 64];
    const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const FuseTarget& t = a.tgt[m];
    const int n = fusem_drop_count(a, t);
    const int n_cells = a.grid.nx * a.grid.ny; // <= kGuidedMaxCells (guided_grid)
    const float* xy = a.drop_xy + (size_t)t.off * 2;
    int32_t* off = a.cell_off + (size_t)m * (kGuidedMaxCells + 1);
    float4* list = a.list + t.off;
    uint8_t* list_desc = a.list_desc + (size_t)t.off * 32;
    const uint8_t* kd = a.desc + (size_t)t.slot * a.K * 32;
    for(int c = tid; c < n_cells; c += kFusemBinThreads)
        cell[c] = 0;
    __syncthreads();
    for(int i = tid; i < n; i += kFusemBinThreads)
    {
        const int c = fusem_cell(xy[2 * (size_t)i], xy[2 * (size_t)i + 1], a.width, a.height, a.grid);
        if(c >= 0)
            atomicAdd(&cell[c], 1u);
    }
    __syncthreads();
    // exclusive scan: thread t owns the cells [t * per, t * per + per)
    const int per = (n_cells + kFusemBinThreads - 1) / kFusemBinThreads, c0 = min(tid * per, n_cells), c1 = min(c0 + per, n_cells);
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
        off[c] = (int32_t)run;
        run += k;
    }
    if(tid == kFusemBinThreads - 1)
        off[n_cells] = (int32_t)run; // the in-frame landmarks of the target: <= n <= its cap
    __syncthreads();
    for(int i = tid; i < n; i += kFusemBinThreads)
    {
        const float x = xy[2 * (size_t)i], y = xy[2 * (size_t)i + 1];
        const int c = fusem_cell(x, y, a.width, a.height, a.grid);
        if(c >= 0)
        {
            const size_t pos = atomicAdd(&cell[c], 1u); // < the target's in-frame count <= its cap
            list[pos] = make_float4(x, y, __int_as_float(i), 0.f);
            copy_desc(kd + (size_t)i * 32, list_desc + pos * 32);
        }
    }
}

// grid (blocks, n_drop), 64 or 256 threads: 8 or 32 keep landmarks per workgroup
__global__ __launch_bounds__(256) void k_fusem_search(FuseMultiArgs a)
{
    const int m = blockIdx.y, g = threadIdx.x & 7;
    const int j = blockIdx.x * (blockDim.x >> 3) + (threadIdx.x >> 3);
    const bool live = j < fusem_keep_count(a); // (the eight lanes of a landmark agree)
    const FuseTarget& t = a.tgt[m];
    const size_t row = (size_t)m * a.nk_cap + (live ? j : 0);
    uint32_t k0 = ~0u, k1 = ~0u;
    if(live && a.keep_ok[row])
    {
        const double u = a.keep_uv[2 * row], v = a.keep_uv[2 * row + 1];
        int cx0, cx1, cy0, cy1;
        if(guided_span(u, a.radius, a.width, a.grid.shift, &cx0, &cx1) && guided_span(v, a.radius, a.height, a.grid.shift, &cy0, &cy1))
        {
            const size_t at = (size_t)a.keep_slot * a.K + j;
            const uint4* q = reinterpret_cast<const uint4*>(a.desc + at * 32);
            const uint4 qa = q[0], qb = q[1];
            const double X = a.world[at * 3], Y = a.world[at * 3 + 1], Z = a.world[at * 3 + 2];
            const double* dw = a.world + (size_t)t.slot * a.K * 3;
            const int32_t* cell_off = a.cell_off + (size_t)m * (kGuidedMaxCells + 1);
            const float4* list = a.list + t.off;
            const uint4* list_desc = reinterpret_cast<const uint4*>(a.list_desc + (size_t)t.off * 32);
            int b = cell_off[cy0 * a.grid.nx + cx0], e = cell_off[cy0 * a.grid.nx + cx1 + 1];
            for(int cy = cy0; cy <= cy1; ++cy)
            {
                int nb = 0, ne = 0;
                if(cy < cy1)
                    nb = cell_off[(cy + 1) * a.grid.nx + cx0], ne = cell_off[(cy + 1) * a.grid.nx + cx1 + 1];
                for(int p = b + g; p < e; p += 8)
                {
                    const float4 pt = list[p];
                    if(fabs((double)pt.x - u) <= a.radius && fabs((double)pt.y - v) <= a.radius)
                    {
                        const size_t i = (size_t)__float_as_int(pt.z); // a drop position: < the target's count
                        const double dx = dw[i * 3] - X, dy = dw[i * 3 + 1] - Y, dz = dw[i * 3 + 2] - Z;
                        if(((dx * dx + dy * dy) + dz * dz) <= a.gate2) // (a NaN fails)
                        {
                            const uint4 da = list_desc[2 * (size_t)p], db = list_desc[2 * (size_t)p + 1];
                            const uint32_t dist = (uint32_t)(((__popc(da.x ^ qa.x) + __popc(da.y ^ qa.y)) + (__popc(da.z ^ qa.z) + __popc(da.w ^ qa.w))) +
                                                             ((__popc(db.x ^ qb.x) + __popc(db.y ^ qb.y)) + (__popc(db.z ^ qb.z) + __popc(db.w ^ qb.w))));
                            const uint32_t key = (dist << 16) | (uint32_t)i; // position <= 65534
                            k1 = min(k1, max(k0, key));
                            k0 = min(k0, key);
                        }
                    }
                }
                b = nb, e = ne;
            }
        }
    }
    // the eight lanes' (k0 <= k1) pairs: keys are distinct (one per drop landmark) apart from the absent key
    for(int o = 1; o < 8; o <<= 1)
    {
        const uint32_t o0 = __shfl_xor(k0, o), o1 = __shfl_xor(k1, o);
        k1 = min(max(k0, o0), min(k1, o1));
        k0 = min(k0, o0);
    }
    if(live && g == 0)
    {
        const int d0 = (int)(k0 >> 16), d1 = (int)(k1 >> 16);
        const bool ok = k0 != ~0u && d0 <= a.max_distance && (k1 == ~0u || (double)d0 < a.ratio * (double)d1);
        a.acc[row] = ok ? k0 : ~0u;
        if(ok) // the per-target resolution: the least (d0, keep position) holds the drop position
            atomicMin(&a.best[(size_t)t.off + (k0 & 0xFFFFu)], (k0 & 0xFFFF0000u) | (uint32_t)j);
    }
}

// grid (blocks, n_drop).  The claims of one launch are read in the next one.
__global__ __launch_bounds__(256) void k_fusem_claim_a(FuseMultiArgs a)
{
    const int m = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if(j >= fusem_keep_count(a))
        return;
    const FuseTarget& t = a.tgt[m];
    const size_t row = (size_t)m * a.nk_cap + j;
    const uint32_t k = a.acc[row];
    const bool is_row = k != ~0u && a.best[(size_t)t.off + (k & 0xFFFFu)] == ((k & 0xFFFF0000u) | (uint32_t)j);
    a.row[row] = is_row ? 1 : 0;
    if(is_row)
    {
        const long long b = lm_find(a.tab_drop, (unsigned long long)a.lid[(size_t)t.slot * a.K + (k & 0xFFFFu)]);
        if(b >= 0) // (every id of a target is in the table)
            atomicMin(&a.tab_drop.b[b].val, (unsigned long long)fusem_key(k >> 16, m, j));
    }
}

__global__ __launch_bounds__(256) void k_fusem_claim_b(FuseMultiArgs a)
{
    const int m = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if(j >= fusem_keep_count(a))
        return;
    const size_t row = (size_t)m * a.nk_cap + j;
    if(!a.row[row])
        return;
    const FuseTarget& t = a.tgt[m];
    const uint32_t k = a.acc[row], i = k & 0xFFFFu;
    const long long b = lm_find(a.tab_drop, (unsigned long long)a.lid[(size_t)t.slot * a.K + i]);
    if(b < 0 || a.tab_drop.b[b].val != (unsigned long long)fusem_key(k >> 16, m, j))
        return;
    a.row[row] = 2;
    const long long bk = lm_find(a.tab_keep, (unsigned long long)a.lid[(size_t)a.keep_slot * a.K + j]);
    if(bk >= 0)
        atomicMin(&a.tab_keep.b[bk].val, (unsigned long long)fusem_key(k >> 16, m, (int)i));
}

// grid (blocks, n_drop): every block leaves its own count, so nothing is cleared beforehand and nothing is added atomically
__global__ __launch_bounds__(256) void k_fusem_count(FuseMultiArgs a)
{
    __shared__ uint32_t wcnt[4];
    const int m = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    bool pair = false;
    if(j < fusem_keep_count(a))
    {
        const size_t row = (size_t)m * a.nk_cap + j;
        if(a.row[row] == 2)
        {
            const uint32_t k = a.acc[row];
            const long long bk = lm_find(a.tab_keep, (unsigned long long)a.lid[(size_t)a.keep_slot * a.K + j]);
            pair = bk >= 0 && a.tab_keep.b[bk].val == (unsigned long long)fusem_key(k >> 16, m, (int)(k & 0xFFFFu));
            if(pair)
                a.row[row] = 3;
        }
    }
    const unsigned long long bal = __ballot(pair);
    if((threadIdx.x & 63) == 0)
        wcnt[threadIdx.x >> 6] = (uint32_t)__popcll(bal);
    __syncthreads();
    if(threadIdx.x == 0)
        a.cnt[(size_t)m * gridDim.x + blockIdx.x] = (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
}

constexpr int kFusemCompactThreads = 1024;

// grid (n_drop): one workgroup per target
__global__ __launch_bounds__(kFusemCompactThreads) void k_fusem_compact(FuseMultiArgs a)
{
    __shared__ uint32_t wcnt[kFusemCompactThreads / 64];
    const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nk = fusem_keep_count(a);
    const FuseTarget& t = a.tgt[m];
    // the pairs of the targets before this one: the sum of their blocks' counts
    const int before = m * ((a.nk_cap + 255) / 256);
    uint32_t part = 0;
    for(int w = tid; w < before; w += kFusemCompactThreads)
        part += a.cnt[w];
    for(int o = 32; o > 0; o >>= 1)
        part += __shfl_xor(part, o);
    if(lane == 0)
        wcnt[wave] = part;
    __syncthreads();
    uint32_t base = 0;
    for(int w = 0; w < kFusemCompactThreads / 64; ++w)
        base += wcnt[w];
    __syncthreads();
    for(int j0 = 0; j0 < nk; j0 += kFusemCompactThreads)
    {
        const int j = j0 + tid;
        const bool win = j < nk && a.row[(size_t)m * a.nk_cap + j] == 3;
        const unsigned long long bal = __ballot(win);
        if(lane == 0)
            wcnt[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t pre = 0, tot = 0;
        for(int w = 0; w < kFusemCompactThreads / 64; ++w)
        {
            if(w < wave)
                pre += wcnt[w];
            tot += wcnt[w];
        }
        if(win)
        {
            // one pair per keep id and per drop id: fewer than min(nk, ND) + 1 rows over all targets
            const size_t p = base + pre + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
            const uint32_t k = a.acc[(size_t)m * a.nk_cap + j];
            const int i = (int)(k & 0xFFFFu), d = (int)(k >> 16);
            const size_t ka = (size_t)a.keep_slot * a.K + j, da = (size_t)t.slot * a.K + i;
            const int64_t kl = a.lid[ka], dl = a.lid[da];
            a.dev.target[p] = a.host.target[p] = m;
            a.dev.keep_pos[p] = a.host.keep_pos[p] = j;
            a.dev.drop_pos[p] = a.host.drop_pos[p] = i;
            a.dev.dist[p] = a.host.dist[p] = d;
            a.dev.keep_lid[p] = a.host.keep_lid[p] = kl;
            a.dev.drop_lid[p] = a.host.drop_lid[p] = dl;
            a.pair_world[p * 3] = a.world[ka * 3], a.pair_world[p * 3 + 1] = a.world[ka * 3 + 1], a.pair_world[p * 3 + 2] = a.world[ka * 3 + 2];
        }
        base += tot;
        __syncthreads();
    }
    if(m == a.n_drop - 1 && tid == 0)
    {
        *a.n_pairs = (int32_t)base;
        a.head->n_pairs = (int32_t)base;
    }
}

} // namespace mslam

using namespace mslam;

namespace
{
struct MultiParams
{
    int keep_id;
    const int32_t* drop_ids;
    int n_drop;
    const double *R, *t;
    double fx, fy, cx, cy;
    int width, height;
    double radius;
    int max_distance;
    double ratio, max_world_distance;
};

// what one search leaves behind for the caller
struct MultiPlan
{
    FuseMultiArgs a{};
    int P = 0;          // rows of the pair arrays: min(keep landmarks, all targets' landmarks), by the hosts' upper bounds
    LmTable tab_rep{};  // the replacement table inside d_lm_table (kf_fuse_multi)
    bool empty = false; // the keep entry or every target holds nothing: no launch, no pairs
    size_t up = 0;      // bytes of the search's own part of the upload, in front of the caller's
};

int multi_check(mslam_hip_ctx* c, const std::string& me, const MultiParams& p, int* keep_slot, std::vector<int>* drop_slots)
{
    RelocState* r = c->reloc;
    if(!p.R || !p.t || !p.drop_ids)
        return fail(c, MSLAM_HIP_E_INVALID, me + ": bad argument");
    if(p.n_drop < 1 || p.n_drop > kFuseMaxTargets)
        return fail(c, MSLAM_HIP_E_INVALID, me + ": n_drop lies outside 1..64");
    for(int m = 0; m < p.n_drop; ++m)
    {
        if(p.drop_ids[m] == p.keep_id)
            return fail(c, MSLAM_HIP_E_INVALID, me + ": keep_id is listed as a drop id");
        for(int o = 0; o < m; ++o)
            if(p.drop_ids[o] == p.drop_ids[m])
                return fail(c, MSLAM_HIP_E_INVALID, me + ": drop id " + std::to_string(p.drop_ids[m]) + " is listed twice");
    }
    int rc = store_slot(c, me, "id", p.keep_id, keep_slot);
    drop_slots->assign((size_t)p.n_drop, -1);
    for(int m = 0; !rc && m < p.n_drop; ++m)
        rc = store_slot(c, me, "id", p.drop_ids[m], &(*drop_slots)[(size_t)m]);
    if(rc)
        return rc;
    if(!(p.radius > 0.0))
        return fail(c, MSLAM_HIP_E_INVALID, me + ": the radius is not a positive number");
    if(p.max_distance < 0 || p.max_distance > 256)
        return fail(c, MSLAM_HIP_E_INVALID, me + ": max_distance lies outside 0..256");
    if(p.width < 1 || p.width > 8192 || p.height < 1 || p.height > 8192)
        return fail(c, MSLAM_HIP_E_INVALID, me + ": the frame extent lies outside 1..8192");
    if(!(p.fx != 0.0) || !(p.fy != 0.0) || p.fx != p.fx || p.fy != p.fy)
        return fail(c, MSLAM_HIP_E_INVALID, me + ": fx or fy is zero or NaN");
    if(!(p.max_world_distance > 0.0))
        return fail(c, MSLAM_HIP_E_INVALID, me + ": max_world_distance is not a positive number");
    bool large = r->n_upper[(size_t)*keep_slot] > 65535;
    for(const int s : *drop_slots)
        large = large || r->n_upper[(size_t)s] > 65535;
    if(large)
        return fail(c, MSLAM_HIP_E_INVALID, me + ": entries of more than 65535 landmarks are not supported");
    return MSLAM_HIP_OK;
}

// Scratch, the call's one upload and the launches of one search on c->stream.  The upload is
// [targets n_drop x FuseTarget | the caller's `extra` bytes]; *extra_at = where the
// caller's part begins in d_up.  with_rep: room for kf_fuse_multi's replacement table.  The mapped result block is
// [FuseMultiHead | target P | keep_pos P | drop_pos P | dist P | keep_lid P | drop_lid P].
int multi_enqueue(mslam_hip_ctx* c, const MultiParams& p, int keep_slot, const std::vector<int>& drop_slots, const void* extra,
                  size_t extra_bytes, bool with_rep, MultiPlan* plan, size_t* extra_at)
{
    RelocState* r = c->reloc;
    const int nk = r->n_upper[(size_t)keep_slot], M = p.n_drop;
    size_t ND = 0;
    int nd_max = 0;
    for(const int s : drop_slots)
        ND += (size_t)r->n_upper[(size_t)s], nd_max = std::max(nd_max, r->n_upper[(size_t)s]);
    plan->P = (int)std::min((size_t)nk, ND);
    plan->empty = plan->P == 0;
    if(plan->empty)
        return MSLAM_HIP_OK;
    const size_t K = (size_t)c->p.max_keypoints, P = (size_t)plan->P, rows = (size_t)M * (size_t)nk;
    const size_t bk = lm_bucket_count((size_t)nk), bd = lm_bucket_count(ND), bp = with_rep ? lm_bucket_count(P) : 0;
    // one block, one clear: [keep table | drop table | replacement table | best ND x u32]
    const size_t o_best = (bk + bd + bp) * sizeof(LmBucket), tab_bytes = o_best + ND * 4;
    // the upload
    const size_t u_extra = al256((size_t)M * sizeof(FuseTarget));
    plan->up = u_extra + extra_bytes;
    *extra_at = u_extra;
    // the arena
    size_t o = 0;
    auto carve = [&o](size_t bytes) {
        const size_t at = o;
        o += al256(bytes);
        return at;
    };
    const size_t a_xy = carve(ND * 8), a_uv = carve(rows * 16), a_ok = carve(rows), a_off = carve((size_t)M * (kGuidedMaxCells + 1) * 4);
    const size_t a_list = carve(ND * 16), a_ldesc = carve(ND * 32), a_acc = carve(rows * 4), a_row = carve(rows);
    const size_t a_tgt = carve(P * 4), a_kpos = carve(P * 4), a_dpos = carve(P * 4), a_dist = carve(P * 4), a_klid = carve(P * 8), a_dlid = carve(P * 8);
    const size_t a_world = carve(P * 24), a_n = carve(4), a_cnt = carve((size_t)M * (size_t)((nk + 255) / 256) * 4);
    const size_t h_tgt = al256(sizeof(FuseMultiHead)), h_kpos = h_tgt + al256(P * 4), h_dpos = h_kpos + al256(P * 4), h_dist = h_dpos + al256(P * 4);
    const size_t h_klid = h_dist + al256(P * 4), h_dlid = h_klid + al256(P * 8), h_bytes = h_dlid + al256(P * 8);
    int rc = reloc_scratch(c, plan->up, o, h_bytes);
    if(rc)
        return rc;
    FuseMultiArgs& a = plan->a;
    a.tab_keep = lm_table_grow(c, (size_t)nk, tab_bytes);
    if(!a.tab_keep.b)
        return MSLAM_HIP_E_RUNTIME;
    a.tab_drop = lm_table_grow(c, ND, tab_bytes, bk * sizeof(LmBucket)); // (the block has its size: no growth, no failure)
    if(with_rep)
        plan->tab_rep = lm_table_grow(c, P, tab_bytes, (bk + bd) * sizeof(LmBucket));
    uint8_t *A = r->d_arena, *T = r->d_lm_table, *H = r->h_res.dev(), *hu = r->h_up, *du = r->d_up;
    // the upload's contents
    std::memset(hu, 0, u_extra);
    FuseTarget* ht = reinterpret_cast<FuseTarget*>(hu);
    int off = 0;
    for(int m = 0; m < M; ++m)
    {
        std::memcpy(ht[m].R, p.R + 9 * (size_t)m, sizeof(ht[m].R));
        std::memcpy(ht[m].t, p.t + 3 * (size_t)m, sizeof(ht[m].t));
        ht[m].slot = drop_slots[(size_t)m], ht[m].cap = r->n_upper[(size_t)drop_slots[(size_t)m]], ht[m].off = off;
        off += ht[m].cap;
    }
    if(extra_bytes)
        std::memcpy(hu + u_extra, extra, extra_bytes);
    a.desc = r->d_desc, a.world = r->d_world, a.lid = r->d_lid, a.n = r->d_n;
    a.K = (int)K, a.keep_slot = keep_slot, a.nk_cap = nk, a.n_drop = M;
    a.tgt = reinterpret_cast<const FuseTarget*>(du);
    a.fx = p.fx, a.fy = p.fy, a.cx = p.cx, a.cy = p.cy, a.radius = p.radius, a.ratio = p.ratio;
    a.gate2 = p.max_world_distance * p.max_world_distance;
    a.max_distance = p.max_distance, a.width = p.width, a.height = p.height, a.grid = guided_grid(p.width, p.height);
    a.drop_xy = reinterpret_cast<float*>(A + a_xy), a.keep_uv = reinterpret_cast<double*>(A + a_uv), a.keep_ok = A + a_ok;
    a.cell_off = reinterpret_cast<int32_t*>(A + a_off), a.list = reinterpret_cast<float4*>(A + a_list), a.list_desc = A + a_ldesc;
    a.acc = reinterpret_cast<uint32_t*>(A + a_acc), a.row = A + a_row, a.best = reinterpret_cast<uint32_t*>(T + o_best);
    a.cnt = reinterpret_cast<uint32_t*>(A + a_cnt);
    a.dev = FuseMultiPairs{reinterpret_cast<int32_t*>(A + a_tgt),  reinterpret_cast<int32_t*>(A + a_kpos), reinterpret_cast<int32_t*>(A + a_dpos),
                           reinterpret_cast<int32_t*>(A + a_dist), reinterpret_cast<int64_t*>(A + a_klid), reinterpret_cast<int64_t*>(A + a_dlid)};
    a.host = FuseMultiPairs{reinterpret_cast<int32_t*>(H + h_tgt),  reinterpret_cast<int32_t*>(H + h_kpos), reinterpret_cast<int32_t*>(H + h_dpos),
                            reinterpret_cast<int32_t*>(H + h_dist), reinterpret_cast<int64_t*>(H + h_klid), reinterpret_cast<int64_t*>(H + h_dlid)};
    a.pair_world = reinterpret_cast<double*>(A + a_world), a.n_pairs = reinterpret_cast<int32_t*>(A + a_n);
    a.head = reinterpret_cast<FuseMultiHead*>(H);
    reinterpret_cast<FuseMultiHead*>(r->h_res.get())->n_pairs = -1; // (overwritten by k_fusem_compact; checked after the synchronisation)
    hipStream_t s = c->stream;
    const unsigned bk256 = (unsigned)((nk + 255) / 256), both = (unsigned)((std::max(nk, nd_max) + 255) / 256);
    MSLAM_CHK(c, hipMemcpyAsync(du, hu, plan->up, hipMemcpyHostToDevice, s));
    {
        StageScope ts(c, "fusem_clear");
        MSLAM_CHK(c, hipMemsetAsync(T, 0xFF, tab_bytes, s));
    }
    {
        StageScope ts(c, "fusem_ids");
        hipLaunchKernelGGL(k_fusem_ids, dim3(both, (unsigned)M + 1), dim3(256), 0, s, a);
    }
    {
        StageScope ts(c, "fusem_project");
        hipLaunchKernelGGL(k_fusem_project, dim3(both, (unsigned)M, 2), dim3(256), 0, s, a);
    }
    {
        StageScope ts(c, "fusem_bin");
        hipLaunchKernelGGL(k_fusem_bin, dim3((unsigned)M), dim3(kFusemBinThreads), 0, s, a);
    }
    {
        StageScope ts(c, "fusem_search");
        const int block = nk > 4096 ? 256 : 64, per = block / 8;
        hipLaunchKernelGGL(k_fusem_search, dim3((unsigned)((nk + per - 1) / per), (unsigned)M), dim3(block), 0, s, a);
    }
    {
        StageScope ts(c, "fusem_claim_a");
        hipLaunchKernelGGL(k_fusem_claim_a, dim3(bk256, (unsigned)M), dim3(256), 0, s, a);
    }
    {
        StageScope ts(c, "fusem_claim_b");
        hipLaunchKernelGGL(k_fusem_claim_b, dim3(bk256, (unsigned)M), dim3(256), 0, s, a);
    }
    {
        StageScope ts(c, "fusem_count");
        hipLaunchKernelGGL(k_fusem_count, dim3(bk256, (unsigned)M), dim3(256), 0, s, a);
    }
    {
        StageScope ts(c, "fusem_compact");
        hipLaunchKernelGGL(k_fusem_compact, dim3((unsigned)M), dim3(kFusemCompactThreads), 0, s, a);
    }
    MSLAM_CHK(c, hipGetLastError());
    return MSLAM_HIP_OK;
}

// after the synchronisation: the count, and the pairs when they fit
int multi_collect(mslam_hip_ctx* c, const std::string& me, const MultiPlan& plan, int32_t* target, int32_t* keep_pos, int32_t* drop_pos,
                  int64_t* keep_lid, int64_t* drop_lid, int32_t* dist, int capacity, int* n_pairs)
{
    if(plan.empty)
        return MSLAM_HIP_OK;
    RelocState* r = c->reloc;
    const int32_t n = reinterpret_cast<const FuseMultiHead*>(r->h_res.get())->n_pairs;
    if(n < 0 || n > plan.P)
        return fail(c, MSLAM_HIP_E_RUNTIME, me + ": the kernels left no result");
    *n_pairs = n;
    if(n > capacity)
        return fail(c, MSLAM_HIP_E_CAPACITY, me + ": " + std::to_string(n) + " pairs, more than `capacity`");
    const uint8_t* H = r->h_res.get();
    const size_t dev = reinterpret_cast<size_t>(r->h_res.dev());
    auto copy = [&](void* dst, const void* dev_ptr, size_t each) {
        if(dst)
            std::memcpy(dst, H + (reinterpret_cast<size_t>(dev_ptr) - dev), (size_t)n * each);
    };
    copy(target, plan.a.host.target, 4), copy(keep_pos, plan.a.host.keep_pos, 4), copy(drop_pos, plan.a.host.drop_pos, 4);
    copy(dist, plan.a.host.dist, 4), copy(keep_lid, plan.a.host.keep_lid, 8), copy(drop_lid, plan.a.host.drop_lid, 8);
    return MSLAM_HIP_OK;
}
} // namespace

extern "C" {

int mslam_hip_kf_fuse_search_multi(mslam_hip_ctx* c, int keep_id, const int32_t* drop_ids, int n_drop, const double* R, const double* t,
                                   double fx, double fy, double cx, double cy, int width, int height, double radius, int max_distance,
                                   double ratio, double max_world_distance, int32_t* target, int32_t* keep_pos, int32_t* drop_pos,
                                   int64_t* keep_lid, int64_t* drop_lid, int32_t* dist, int capacity, int* n_pairs)
{
    if(n_pairs)
        *n_pairs = 0;
    int rc = reloc_enter(c);
    if(rc)
        return rc;
    const std::string me = "kf_fuse_search_multi";
    if(!n_pairs || capacity < 0 || (capacity > 0 && (!target || !keep_pos || !drop_pos || !keep_lid || !drop_lid || !dist)))
        return fail(c, MSLAM_HIP_E_INVALID, me + ": bad argument");
    const MultiParams p{keep_id, drop_ids, n_drop, R, t, fx, fy, cx, cy, width, height, radius, max_distance, ratio, max_world_distance};
    int ks = -1;
    std::vector<int> ds;
    rc = multi_check(c, me, p, &ks, &ds);
    if(rc)
        return rc;
    MultiPlan plan;
    size_t extra_at = 0;
    rc = multi_enqueue(c, p, ks, ds, nullptr, 0, false, &plan, &extra_at);
    if(rc)
        return rc;
    if(!plan.empty)
        MSLAM_CHK(c, hipStreamSynchronize(c->stream));
    return multi_collect(c, me, plan, target, keep_pos, drop_pos, keep_lid, drop_lid, dist, capacity, n_pairs);
}

int mslam_hip_kf_fuse_multi(mslam_hip_ctx* c, int keep_id, const int32_t* drop_ids, int n_drop, const double* R, const double* t, double fx,
                            double fy, double cx, double cy, int width, int height, double radius, int max_distance, double ratio,
                            double max_world_distance, int32_t* target, int32_t* keep_pos, int32_t* drop_pos, int64_t* keep_lid,
                            int64_t* drop_lid, int32_t* dist, int capacity, int* n_pairs, int* n_rewritten)
{
    if(n_pairs)
        *n_pairs = 0;
    if(n_rewritten)
        *n_rewritten = 0;
    int rc = reloc_enter(c);
    if(rc)
        return rc;
    const std::string me = "kf_fuse_multi";
    if(!n_pairs || capacity < 0)
        return fail(c, MSLAM_HIP_E_INVALID, me + ": bad argument");
    const MultiParams p{keep_id, drop_ids, n_drop, R, t, fx, fy, cx, cy, width, height, radius, max_distance, ratio, max_world_distance};
    int ks = -1;
    std::vector<int> ds;
    rc = multi_check(c, me, p, &ks, &ds);
    if(rc)
        return rc;
    RelocState* r = c->reloc;
    std::vector<int32_t> slots;
    const int n_max = live_slots(r, &slots);
    // the caller's part of the one upload: [live slots | the count, zero]
    const size_t o_cnt = slots.size() * 4;
    slots.push_back(0);
    MultiPlan plan;
    size_t extra_at = 0;
    rc = multi_enqueue(c, p, ks, ds, slots.data(), slots.size() * 4, true, &plan, &extra_at);
    if(rc || plan.empty)
        return rc;
    uint8_t* d = r->d_up + extra_at;
    // drop_lid -> keep_lid with the keep landmark's world point, straight from the device list (at most P places); nothing
    // when the pairs exceed `capacity`
    const ReplaceList l{plan.a.dev.drop_lid, plan.a.dev.keep_lid, plan.a.pair_world, plan.a.n_pairs, plan.P, std::min(capacity, plan.P)};
    rc = rewrite_enqueue(c, l, plan.tab_rep, reinterpret_cast<const int32_t*>(d), (int)slots.size() - 1, n_max,
                         reinterpret_cast<uint32_t*>(d + o_cnt), "fusem_table", "fusem_replace");
    if(!rc)
        rc = rewrite_count(c, reinterpret_cast<const uint32_t*>(d + o_cnt), n_rewritten);
    return rc ? rc : multi_collect(c, me, plan, target, keep_pos, drop_pos, keep_lid, drop_lid, dist, capacity, n_pairs);
}

} // extern "C"
