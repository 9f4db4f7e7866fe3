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
//   k_fusem_project  one thread per (target, landmark of either side): fuse_project (fuse.hpp)
//   k_fusem_bin      one workgroup per target: guided_bin_row (guided_walk.hpp) on that target's slice of the drop arrays
//   k_fusem_search   fuse_search_one (fuse.hpp) per (target, keep landmark); the accepted key claims its drop position with
//                    atomicMin of d0 << 16 | keep position (the per-target resolution)
//   k_fusem_claim_a  a keep landmark that holds its drop position is a row; it claims its drop landmark id with
//                    atomicMin of dist << 22 | target << 16 | keep position on the id's bucket of the drop table
//   k_fusem_claim_b  a row that holds its drop id claims its keep landmark id with dist << 22 | target << 16 | drop position
//                    on the keep table
//   k_fusem_count    a row that holds both is a pair; per (target, block of 256 keep positions), the number of them
//   k_fusem_compact  one workgroup per target: its base from the counts of the targets before it, then fuse_emit
//                    (fuse.hpp) of its pairs, which are in keep-position order already
//
// dist <= 256, target < 64 and position < 65536 fit 31 bits, and (target, keep position) as well as (target, drop position)
// name a row, so each claim's key is a total order and no tie is left to arrival order.  Every result is a function of the
// keys alone.  All projection arithmetic is f64, every operation rounded on its own (-ffp-contract=off).
#include "fuse.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace mslam
{

constexpr int kFuseMaxTargets = 64;

// one target, as uploaded
struct FuseTarget
{
    double R[9], t[3];
    int32_t slot, cap, off, pad; // cap: what the host knows the entry's count not to exceed; off: its place in the drop arrays
};

struct FuseMultiArgs : FuseCore
{
    int n_drop;
    const FuseTarget* tgt; // [n_drop], device
    uint8_t* row;          // [n_drop][nk] 0: no row, 1: a row, 2: holds its drop id, 3: a pair
    uint32_t* cnt;         // [n_drop][ceil(nk / 256)] pairs per block of k_fusem_count
};

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
        if(i < fuse_keep_count(a))
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
    if(i < (side ? fusem_drop_count(a, t) : fuse_keep_count(a)))
        fuse_project(a, t.R, t.t, side, side ? t.slot : a.keep_slot, i, side ? (size_t)t.off + i : (size_t)m * a.nk_cap + i);
}

// grid (n_drop): target blockIdx.x's slice
__global__ __launch_bounds__(kGuidedBinThreads) void k_fusem_bin(FuseMultiArgs a)
{
    const int m = blockIdx.x;
    const FuseTarget& t = a.tgt[m];
    guided_bin_row(GuidedBinRow{a.drop_xy + (size_t)t.off * 2, a.desc + (size_t)t.slot * a.K * 32, fusem_drop_count(a, t),
                                a.cell_off + (size_t)m * (kGuidedMaxCells + 1), a.list + t.off, a.list_desc + (size_t)t.off * 32},
                   a.width, a.height, a.grid);
}

// grid (blocks, n_drop), 64 or 256 threads: 8 or 32 keep landmarks per workgroup
__global__ __launch_bounds__(256) void k_fusem_search(FuseMultiArgs a)
{
    const int m = blockIdx.y, g = threadIdx.x & 7;
    const int j = blockIdx.x * (blockDim.x >> 3) + (threadIdx.x >> 3);
    const bool live = j < fuse_keep_count(a); // (the eight lanes of a landmark agree)
    const FuseTarget& t = a.tgt[m];
    const size_t row = (size_t)m * a.nk_cap + (live ? j : 0);
    const uint32_t key = fuse_search_one(a, live, j, row, t.slot, a.cell_off + (size_t)m * (kGuidedMaxCells + 1), a.list + t.off,
                                         a.list_desc + (size_t)t.off * 32, g);
    if(live && g == 0)
    {
        a.acc[row] = key;
        if(key != ~0u) // the per-target resolution: the least (d0, keep position) holds the drop position
            atomicMin(&a.best[(size_t)t.off + (key & 0xFFFFu)], (key & 0xFFFF0000u) | (uint32_t)j);
    }
}

// grid (blocks, n_drop).  The claims of one launch are read in the next one.
__global__ __launch_bounds__(256) void k_fusem_claim_a(FuseMultiArgs a)
{
    const int m = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if(j >= fuse_keep_count(a))
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
    if(j >= fuse_keep_count(a))
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
    if(j < fuse_keep_count(a))
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

// grid (n_drop): one workgroup per target
__global__ __launch_bounds__(kFuseEmitThreads) void k_fusem_compact(FuseMultiArgs a)
{
    __shared__ uint32_t wcnt[kFuseEmitThreads / 64];
    const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nk = fuse_keep_count(a);
    // the pairs of the targets before this one: the sum of their blocks' counts
    const int before = m * ((a.nk_cap + 255) / 256);
    uint32_t part = 0;
    for(int w = tid; w < before; w += kFuseEmitThreads)
        part += a.cnt[w];
    for(int o = 32; o > 0; o >>= 1)
        part += __shfl_xor(part, o);
    if(lane == 0)
        wcnt[wave] = part;
    __syncthreads();
    uint32_t base = 0;
    for(int w = 0; w < kFuseEmitThreads / 64; ++w)
        base += wcnt[w];
    __syncthreads();
    // one pair per keep id and per drop id: fewer than min(nk, ND) + 1 rows over all targets
    const uint8_t* row = a.row + (size_t)m * a.nk_cap;
    const uint32_t* acc = a.acc + (size_t)m * a.nk_cap;
    base = fuse_emit(a, nk, m, a.tgt[m].slot, base, wcnt, [row, acc](int j) { return row[j] == 3 ? acc[j] : ~0u; });
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
// mslam_hip_kf_fuse_search_multi (rewrite == false: the caller's arrays are required, the call ends in its own
// synchronisation) and mslam_hip_kf_fuse_multi (the rewrite's launches follow the search's, and its count is the
// synchronisation).  The call's one upload is [targets n_drop x FuseTarget | kf_fuse_multi: live slots | the count, zero].
int fuse_multi_call(mslam_hip_ctx* c, const std::string& me, bool rewrite, const int32_t* drop_ids, int n_drop, const FuseParams& p,
                    const FusePairs& out, int capacity, int* n_pairs, int* n_rewritten)
{
    if(n_pairs)
        *n_pairs = 0;
    if(n_rewritten)
        *n_rewritten = 0;
    int rc = reloc_enter(c);
    if(rc)
        return rc;
    if(!n_pairs || capacity < 0 ||
       (!rewrite && capacity > 0 && (!out.target || !out.keep_pos || !out.drop_pos || !out.keep_lid || !out.drop_lid || !out.dist)))
        return fail(c, MSLAM_HIP_E_INVALID, me + ": bad argument");
    if(!p.R || !p.t || !drop_ids)
        return fail(c, MSLAM_HIP_E_INVALID, me + ": bad argument");
    if(n_drop < 1 || n_drop > kFuseMaxTargets)
        return fail(c, MSLAM_HIP_E_INVALID, me + ": n_drop lies outside 1..64");
    for(int m = 0; m < n_drop; ++m)
    {
        if(drop_ids[m] == p.keep_id)
            return fail(c, MSLAM_HIP_E_INVALID, me + ": keep_id is listed as a drop id");
        for(int o = 0; o < m; ++o)
            if(drop_ids[o] == drop_ids[m])
                return fail(c, MSLAM_HIP_E_INVALID, me + ": drop id " + std::to_string(drop_ids[m]) + " is listed twice");
    }
    int ks = -1;
    std::vector<int> ds;
    rc = fuse_check(c, me, p, drop_ids, n_drop, &ks, &ds);
    if(rc)
        return rc;
    RelocState* r = c->reloc;
    std::vector<int32_t> slots;
    const int n_max = rewrite ? fuse_rewrite_upload(r, &slots) : 0;
    const int nk = r->n_upper[(size_t)ks], M = n_drop;
    const size_t u_slots = al256((size_t)M * sizeof(FuseTarget)), up = u_slots + slots.size() * 4;
    const size_t rows = (size_t)M * (size_t)nk, a_cnt = al256(rows); // the caller's part of the arena: [row | cnt]
    FuseMultiArgs a{};
    FusePlan plan;
    rc = fuse_setup(c, p, ks, ds, true, up, a_cnt + (size_t)M * (size_t)((nk + 255) / 256) * 4, rewrite, &a, &plan);
    if(rc || plan.empty)
        return rc;
    uint8_t *hu = r->h_up, *du = r->d_up;
    // the upload's contents
    std::memset(hu, 0, u_slots);
    FuseTarget* ht = reinterpret_cast<FuseTarget*>(hu);
    int off = 0, nd_max = 0;
    for(int m = 0; m < M; ++m)
    {
        std::memcpy(ht[m].R, p.R + 9 * (size_t)m, sizeof(ht[m].R));
        std::memcpy(ht[m].t, p.t + 3 * (size_t)m, sizeof(ht[m].t));
        ht[m].slot = ds[(size_t)m], ht[m].cap = r->n_upper[(size_t)ds[(size_t)m]], ht[m].off = off;
        off += ht[m].cap;
        nd_max = std::max(nd_max, ht[m].cap);
    }
    if(!slots.empty())
        std::memcpy(hu + u_slots, slots.data(), slots.size() * 4);
    a.n_drop = M, a.tgt = reinterpret_cast<const FuseTarget*>(du);
    a.row = r->d_arena + plan.extra_at, a.cnt = reinterpret_cast<uint32_t*>(r->d_arena + plan.extra_at + a_cnt);
    hipStream_t s = c->stream;
    const unsigned bk256 = (unsigned)((nk + 255) / 256), both = (unsigned)((std::max(nk, nd_max) + 255) / 256);
    MSLAM_CHK(c, hipMemcpyAsync(du, hu, up, hipMemcpyHostToDevice, s));
    {
        StageScope ts(c, "fusem_clear");
        MSLAM_CHK(c, hipMemsetAsync(r->d_lm_table, 0xFF, plan.tab_bytes, s));
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
        hipLaunchKernelGGL(k_fusem_bin, dim3((unsigned)M), dim3(kGuidedBinThreads), 0, s, a);
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
        hipLaunchKernelGGL(k_fusem_compact, dim3((unsigned)M), dim3(kFuseEmitThreads), 0, s, a);
    }
    MSLAM_CHK(c, hipGetLastError());
    if(rewrite)
    {
        rc = fuse_rewrite(c, a, plan, du + u_slots, (int)slots.size() - 1, n_max, capacity, "fusem_table", "fusem_replace", n_rewritten);
        if(rc)
            return rc;
    }
    else
        MSLAM_CHK(c, hipStreamSynchronize(s));
    return fuse_collect(c, me, a, plan, out, capacity, n_pairs);
}
} // namespace

extern "C" {

int mslam_hip_kf_fuse_search_multi(mslam_hip_ctx* c, int keep_id, const int32_t* drop_ids, int n_drop, const double* R, const double* t,
                                   double fx, double fy, double cx, double cy, int width, int height, double radius, int max_distance,
                                   double ratio, double max_world_distance, int32_t* target, int32_t* keep_pos, int32_t* drop_pos,
                                   int64_t* keep_lid, int64_t* drop_lid, int32_t* dist, int capacity, int* n_pairs)
{
    const FuseParams p{keep_id, R, t, fx, fy, cx, cy, width, height, radius, max_distance, ratio, max_world_distance};
    return fuse_multi_call(c, "kf_fuse_search_multi", false, drop_ids, n_drop, p, FusePairs{target, keep_pos, drop_pos, dist, keep_lid, drop_lid},
                           capacity, n_pairs, nullptr);
}

int mslam_hip_kf_fuse_multi(mslam_hip_ctx* c, int keep_id, const int32_t* drop_ids, int n_drop, const double* R, const double* t, double fx,
                            double fy, double cx, double cy, int width, int height, double radius, int max_distance, double ratio,
                            double max_world_distance, int32_t* target, int32_t* keep_pos, int32_t* drop_pos, int64_t* keep_lid,
                            int64_t* drop_lid, int32_t* dist, int capacity, int* n_pairs, int* n_rewritten)
{
    const FuseParams p{keep_id, R, t, fx, fy, cx, cy, width, height, radius, max_distance, ratio, max_world_distance};
    return fuse_multi_call(c, "kf_fuse_multi", true, drop_ids, n_drop, p, FusePairs{target, keep_pos, drop_pos, dist, keep_lid, drop_lid}, capacity,
                           n_pairs, n_rewritten);
}

} // extern "C"
