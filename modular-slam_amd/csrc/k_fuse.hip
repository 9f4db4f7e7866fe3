// k_fuse.hip — landmark fusion on the keyframe store: mslam_hip_kf_fuse_search finds the landmarks of one entry ("drop")
// that duplicate landmarks of another ("keep") by projecting both under one pose and matching inside a window,
// mslam_hip_kf_replace_ids rewrites landmark ids (and world points) across the whole store, and mslam_hip_kf_fuse runs the
// two back to back without the pair list leaving the device (the semantics are stated once, at mslam_hip_kf_fuse_search in
// include/mslam_hip.h).  The rewrite itself is the list rewrite of k_localmap.hip (rewrite_enqueue, reloc.hpp), which
// mslam_hip_kf_update_world shares: stages fuse_table and fuse_replace here.
//
// The reference has no code for this: closeLoop is an empty body (rgbd_feature_frontend.cpp:577-580).  The model is
// ORB-SLAM's SearchAndFuse; this is an extension, not a restatement.
//
//   k_fuse_ids       both entries' landmark ids into one id table each (lm_table.hpp)
//   k_fuse_project   one thread per landmark of either entry: fuse_project (fuse.hpp), so that k_guided_bin
//                    (k_match_guided.hip) bins exactly the drop landmarks that may be candidates
//   k_fuse_search    eight lanes per keep landmark: fuse_search_one (fuse.hpp), per keep landmark the accepted key
//                    d0 << 16 | drop position, or none
//   k_fuse_resolve   one workgroup: atomicMin of d0 << 16 | keep position per claimed drop position, then fuse_emit
//                    (fuse.hpp) of the keep landmarks that hold their claim
//
// Every result is a function of the keys alone (distance, position), never of the order in which the binning scatter or
// the atomics ran.  All projection arithmetic is f64, every operation rounded on its own (-ffp-contract=off).
//
// The host side that k_fuse_multi.hip shares (fuse.hpp) is defined here as well.
#include "fuse.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace mslam
{

struct FuseArgs : FuseCore
{
    int drop_slot, nd_cap; // nd_cap: what the host knows the drop entry's count not to exceed
    double R[9], t[3];
};

__device__ __forceinline__ int fuse_count(const FuseArgs& a, int side) // side 0 = keep, 1 = drop
{
    return side ? min(max(a.n[a.drop_slot], 0), a.nd_cap) : fuse_keep_count(a);
}

// grid (blocks, 2)
__global__ __launch_bounds__(256) void k_fuse_ids(FuseArgs a)
{
    const int side = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if(i >= fuse_count(a, side))
        return;
    const size_t at = (size_t)(side ? a.drop_slot : a.keep_slot) * a.K + i;
    (void)lm_claim(side ? a.tab_drop : a.tab_keep, (unsigned long long)a.lid[at]);
}

// grid (blocks, 2)
__global__ __launch_bounds__(256) void k_fuse_project(FuseArgs a)
{
    const int side = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if(i < fuse_count(a, side))
        fuse_project(a, a.R, a.t, side, side ? a.drop_slot : a.keep_slot, i, (size_t)i);
}

// 64 or 256 threads: 8 or 32 keep landmarks per workgroup
__global__ __launch_bounds__(256) void k_fuse_search(FuseArgs a)
{
    const int g = threadIdx.x & 7;
    const int j = blockIdx.x * (blockDim.x >> 3) + (threadIdx.x >> 3);
    const bool live = j < fuse_keep_count(a); // (the eight lanes of a landmark agree)
    const uint32_t key = fuse_search_one(a, live, j, (size_t)j, a.drop_slot, a.cell_off, a.list, a.list_desc, g);
    if(live && g == 0)
        a.acc[j] = key;
}

// one workgroup.  The claims go through atomicMin and are read back through it as well (an atomic that changes nothing),
// so the second phase sees what the first one left whatever the caches hold.
__global__ __launch_bounds__(kFuseEmitThreads) void k_fuse_resolve(FuseArgs a)
{
    __shared__ uint32_t wcnt[kFuseEmitThreads / 64];
    const int nk = fuse_keep_count(a);
    for(int j = threadIdx.x; j < nk; j += kFuseEmitThreads)
    {
        const uint32_t k = a.acc[j];
        if(k != ~0u)
            atomicMin(&a.best[k & 0xFFFFu], (k & 0xFFFF0000u) | (uint32_t)j);
    }
    __syncthreads();
    // one pair per drop position and per keep position: fewer than min(nk, nd) + 1 rows
    const uint32_t n = fuse_emit(a, nk, 0, a.drop_slot, 0, wcnt, [&a](int j) {
        const uint32_t k = a.acc[j];
        return (k != ~0u && atomicMin(&a.best[k & 0xFFFFu], ~0u) == ((k & 0xFFFF0000u) | (uint32_t)j)) ? k : ~0u;
    });
    if(threadIdx.x == 0)
    {
        *a.n_pairs = (int32_t)n;
        a.head->n_pairs = (int32_t)n;
    }
}

// ---- the host side both fusion files share (fuse.hpp) ------------------------------------------------------------------

int fuse_check(mslam_hip_ctx* c, const std::string& me, const FuseParams& p, const int32_t* drop_ids, int n_drop, int* keep_slot,
               std::vector<int>* drop_slots)
{
    RelocState* r = c->reloc;
    int rc = store_slot(c, me, "id", p.keep_id, keep_slot);
    drop_slots->assign((size_t)n_drop, -1);
    for(int m = 0; !rc && m < n_drop; ++m)
        rc = store_slot(c, me, "id", drop_ids[m], &(*drop_slots)[(size_t)m]);
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

int fuse_setup(mslam_hip_ctx* c, const FuseParams& p, int keep_slot, const std::vector<int>& drop_slots, bool with_target, size_t up,
               size_t extra_arena, bool with_rep, FuseCore* core, FusePlan* plan)
{
    RelocState* r = c->reloc;
    const int nk = r->n_upper[(size_t)keep_slot];
    size_t ND = 0;
    for(const int s : drop_slots)
        ND += (size_t)r->n_upper[(size_t)s];
    plan->P = (int)std::min((size_t)nk, ND);
    plan->empty = plan->P == 0;
    if(plan->empty)
        return MSLAM_HIP_OK;
    const size_t K = (size_t)c->p.max_keypoints, P = (size_t)plan->P, M = drop_slots.size(), rows = M * (size_t)nk;
    const size_t bk = lm_bucket_count((size_t)nk), bd = lm_bucket_count(ND), bp = with_rep ? lm_bucket_count(P) : 0;
    const size_t o_best = (bk + bd + bp) * sizeof(LmBucket);
    plan->tab_bytes = o_best + ND * 4;
    // the arena and the mapped result block
    const auto carve = [](size_t* o, size_t bytes) {
        const size_t at = *o;
        *o += al256(bytes);
        return at;
    };
    struct PairsAt
    {
        size_t target, keep_pos, drop_pos, dist, keep_lid, drop_lid;
    };
    const auto carve_pairs = [&](size_t* o) {
        PairsAt at{};
        if(with_target)
            at.target = carve(o, P * 4);
        at.keep_pos = carve(o, P * 4), at.drop_pos = carve(o, P * 4), at.dist = carve(o, P * 4);
        at.keep_lid = carve(o, P * 8), at.drop_lid = carve(o, P * 8);
        return at;
    };
    const auto pairs = [&](uint8_t* base, const PairsAt& at) {
        return FusePairs{with_target ? reinterpret_cast<int32_t*>(base + at.target) : nullptr,
                         reinterpret_cast<int32_t*>(base + at.keep_pos),
                         reinterpret_cast<int32_t*>(base + at.drop_pos),
                         reinterpret_cast<int32_t*>(base + at.dist),
                         reinterpret_cast<int64_t*>(base + at.keep_lid),
                         reinterpret_cast<int64_t*>(base + at.drop_lid)};
    };
    size_t o = 0, h = al256(sizeof(FuseHead));
    const size_t a_xy = carve(&o, ND * 8), a_uv = carve(&o, rows * 16), a_ok = carve(&o, rows), a_off = carve(&o, M * (kGuidedMaxCells + 1) * 4);
    const size_t a_list = carve(&o, ND * 16), a_ldesc = carve(&o, ND * 32), a_acc = carve(&o, rows * 4);
    const PairsAt a_pairs = carve_pairs(&o), h_pairs = carve_pairs(&h);
    const size_t a_world = carve(&o, P * 24), a_n = carve(&o, 4);
    plan->extra_at = carve(&o, extra_arena);
    int rc = reloc_scratch(c, up, o, h);
    if(rc)
        return rc;
    FuseCore& a = *core;
    a.tab_keep = lm_table_grow(c, (size_t)nk, plan->tab_bytes);
    if(!a.tab_keep.b)
        return MSLAM_HIP_E_RUNTIME;
    a.tab_drop = lm_table_grow(c, ND, plan->tab_bytes, bk * sizeof(LmBucket)); // (the block has its size: no growth, no failure)
    if(with_rep)
        plan->tab_rep = lm_table_grow(c, P, plan->tab_bytes, (bk + bd) * sizeof(LmBucket));
    uint8_t *A = r->d_arena, *T = r->d_lm_table, *H = r->h_res.dev();
    a.desc = r->d_desc, a.world = r->d_world, a.lid = r->d_lid, a.n = r->d_n;
    a.K = (int)K, a.keep_slot = keep_slot, a.nk_cap = nk;
    a.fx = p.fx, a.fy = p.fy, a.cx = p.cx, a.cy = p.cy, a.radius = p.radius, a.ratio = p.ratio;
    a.gate2 = p.max_world_distance * p.max_world_distance;
    a.max_distance = p.max_distance, a.width = p.width, a.height = p.height, a.grid = guided_grid(p.width, p.height);
    a.drop_xy = reinterpret_cast<float*>(A + a_xy), a.keep_uv = reinterpret_cast<double*>(A + a_uv), a.keep_ok = A + a_ok;
    a.cell_off = reinterpret_cast<int32_t*>(A + a_off), a.list = reinterpret_cast<float4*>(A + a_list), a.list_desc = A + a_ldesc;
    a.acc = reinterpret_cast<uint32_t*>(A + a_acc), a.best = reinterpret_cast<uint32_t*>(T + o_best);
    a.dev = pairs(A, a_pairs), a.host = pairs(H, h_pairs);
    a.pair_world = reinterpret_cast<double*>(A + a_world), a.n_pairs = reinterpret_cast<int32_t*>(A + a_n);
    a.head = reinterpret_cast<FuseHead*>(H);
    reinterpret_cast<FuseHead*>(r->h_res.get())->n_pairs = -1; // (overwritten by the last kernel; checked after the synchronisation)
    return MSLAM_HIP_OK;
}

int fuse_rewrite_upload(const RelocState* r, std::vector<int32_t>* slots)
{
    const int n_max = live_slots(r, slots);
    slots->push_back(0);
    return n_max;
}

int fuse_rewrite(mslam_hip_ctx* c, const FuseCore& a, const FusePlan& plan, uint8_t* d, int n_slots, int n_max, int capacity,
                 const char* stage_table, const char* stage_write, int* n_rewritten)
{
    const ReplaceList l{a.dev.drop_lid, a.dev.keep_lid, a.pair_world, a.n_pairs, plan.P, std::min(capacity, plan.P)};
    uint32_t* count = reinterpret_cast<uint32_t*>(d) + n_slots;
    const int rc = rewrite_enqueue(c, l, plan.tab_rep, reinterpret_cast<const int32_t*>(d), n_slots, n_max, count, stage_table, stage_write);
    return rc ? rc : rewrite_count(c, count, n_rewritten);
}

int fuse_collect(mslam_hip_ctx* c, const std::string& me, const FuseCore& a, const FusePlan& plan, const FusePairs& out, int capacity,
                 int* n_pairs)
{
    RelocState* r = c->reloc;
    const int32_t n = reinterpret_cast<const FuseHead*>(r->h_res.get())->n_pairs;
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
    copy(out.target, a.host.target, 4), copy(out.keep_pos, a.host.keep_pos, 4), copy(out.drop_pos, a.host.drop_pos, 4);
    copy(out.dist, a.host.dist, 4), copy(out.keep_lid, a.host.keep_lid, 8), copy(out.drop_lid, a.host.drop_lid, 8);
    return MSLAM_HIP_OK;
}

} // namespace mslam

using namespace mslam;

namespace
{
// mslam_hip_kf_fuse_search (rewrite == false: the caller's arrays are required, the call ends in its own synchronisation)
// and mslam_hip_kf_fuse (the rewrite's upload and launches follow the search's, and its count is the synchronisation)
int fuse_call(mslam_hip_ctx* c, const std::string& me, bool rewrite, int drop_id, const FuseParams& p, const FusePairs& out, int capacity,
              int* n_pairs, int* n_rewritten)
{
    if(n_pairs)
        *n_pairs = 0;
    if(n_rewritten)
        *n_rewritten = 0;
    int rc = reloc_enter(c);
    if(rc)
        return rc;
    if(!n_pairs || capacity < 0 ||
       (!rewrite && capacity > 0 && (!out.keep_pos || !out.drop_pos || !out.keep_lid || !out.drop_lid || !out.dist)))
        return fail(c, MSLAM_HIP_E_INVALID, me + ": bad argument");
    if(!p.R || !p.t)
        return fail(c, MSLAM_HIP_E_INVALID, me + ": bad argument");
    if(p.keep_id == drop_id)
        return fail(c, MSLAM_HIP_E_INVALID, me + ": keep_id and drop_id name one entry");
    int ks = -1;
    std::vector<int> ds;
    rc = fuse_check(c, me, p, &drop_id, 1, &ks, &ds);
    if(rc)
        return rc;
    RelocState* r = c->reloc;
    // kf_fuse's one upload: [live slots | the count, zero]
    std::vector<int32_t> slots;
    const int n_max = rewrite ? fuse_rewrite_upload(r, &slots) : 0;
    const size_t up = slots.size() * 4;
    FuseArgs a{};
    FusePlan plan;
    rc = fuse_setup(c, p, ks, ds, false, up, 0, rewrite, &a, &plan);
    if(rc || plan.empty)
        return rc;
    const int nk = a.nk_cap, nd = r->n_upper[(size_t)ds[0]];
    a.drop_slot = ds[0], a.nd_cap = nd;
    std::memcpy(a.R, p.R, sizeof(a.R));
    std::memcpy(a.t, p.t, sizeof(a.t));
    // the bin kernel's view: the drop entry's projections are the keypoints
    GuidedArgs g{};
    g.kp_desc = r->d_desc + (size_t)a.drop_slot * a.K * 32, g.kp_xy = a.drop_xy;
    g.kp_cnt = r->d_n + a.drop_slot, g.kp_cap = nd;
    g.width = p.width, g.height = p.height, g.grid = a.grid;
    g.cell_off = a.cell_off, g.list = a.list, g.list_desc = a.list_desc;
    hipStream_t s = c->stream;
    const dim3 both((unsigned)((std::max(nk, nd) + 255) / 256), 2);
    {
        StageScope ts(c, "fuse_clear");
        MSLAM_CHK(c, hipMemsetAsync(r->d_lm_table, 0xFF, plan.tab_bytes, s));
    }
    {
        StageScope ts(c, "fuse_ids");
        hipLaunchKernelGGL(k_fuse_ids, both, dim3(256), 0, s, a);
    }
    {
        StageScope ts(c, "fuse_project");
        hipLaunchKernelGGL(k_fuse_project, both, dim3(256), 0, s, a);
    }
    {
        StageScope ts(c, "fuse_bin");
        launch_guided_bin(g, 1, s);
    }
    {
        StageScope ts(c, "fuse_search");
        const int block = nk > 4096 ? 256 : 64, per = block / 8;
        hipLaunchKernelGGL(k_fuse_search, dim3((unsigned)((nk + per - 1) / per)), dim3(block), 0, s, a);
    }
    {
        StageScope ts(c, "fuse_resolve");
        hipLaunchKernelGGL(k_fuse_resolve, dim3(1), dim3(kFuseEmitThreads), 0, s, a);
    }
    MSLAM_CHK(c, hipGetLastError());
    if(rewrite)
    {
        std::memcpy(r->h_up, slots.data(), up);
        MSLAM_CHK(c, hipMemcpyAsync(r->d_up, r->h_up, up, hipMemcpyHostToDevice, s));
        rc = fuse_rewrite(c, a, plan, r->d_up, (int)slots.size() - 1, n_max, capacity, "fuse_table", "fuse_replace", n_rewritten);
        if(rc)
            return rc;
    }
    else
        MSLAM_CHK(c, hipStreamSynchronize(s));
    return fuse_collect(c, me, a, plan, out, capacity, n_pairs);
}
} // namespace

extern "C" {

int mslam_hip_kf_fuse_search(mslam_hip_ctx* c, int keep_id, int drop_id, const double* R, const double* t, double fx, double fy, double cx,
                             double cy, int width, int height, double radius, int max_distance, double ratio, double max_world_distance,
                             int32_t* keep_pos, int32_t* drop_pos, int64_t* keep_lid, int64_t* drop_lid, int32_t* dist, int capacity,
                             int* n_pairs)
{
    const FuseParams p{keep_id, R, t, fx, fy, cx, cy, width, height, radius, max_distance, ratio, max_world_distance};
    return fuse_call(c, "kf_fuse_search", false, drop_id, p, FusePairs{nullptr, keep_pos, drop_pos, dist, keep_lid, drop_lid}, capacity, n_pairs,
                     nullptr);
}

int mslam_hip_kf_replace_ids(mslam_hip_ctx* c, const int64_t* from_ids, const int64_t* to_ids, const double* world_xyz, int n,
                             int* n_rewritten)
{
    if(n_rewritten)
        *n_rewritten = 0;
    int rc = reloc_enter(c);
    if(rc)
        return rc;
    rc = lid_list_check(c, "kf_replace_ids", n, from_ids && to_ids, from_ids, to_ids);
    if(rc)
        return rc;
    return rewrite_host_list(c, from_ids, to_ids, world_xyz, n, "fuse_table", "fuse_replace", n_rewritten);
}

int mslam_hip_kf_fuse(mslam_hip_ctx* c, int keep_id, int drop_id, const double* R, const double* t, double fx, double fy, double cx, double cy,
                      int width, int height, double radius, int max_distance, double ratio, double max_world_distance, int32_t* keep_pos,
                      int32_t* drop_pos, int64_t* keep_lid, int64_t* drop_lid, int32_t* dist, int capacity, int* n_pairs, int* n_rewritten)
{
    const FuseParams p{keep_id, R, t, fx, fy, cx, cy, width, height, radius, max_distance, ratio, max_world_distance};
    return fuse_call(c, "kf_fuse", true, drop_id, p, FusePairs{nullptr, keep_pos, drop_pos, dist, keep_lid, drop_lid}, capacity, n_pairs,
                     n_rewritten);
}

} // extern "C"
