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
//   k_fuse_project   one thread per landmark of either entry: eligibility (its id is absent from the other entry's table)
//                    and the f64 projection.  A keep landmark leaves (u, v) and a flag; a drop landmark leaves the f32
//                    "keypoint" ((float)u, (float)v), or NaNs when it is ineligible or behind the camera, so that
//                    k_guided_bin (k_match_guided.hip, unchanged) bins exactly the drop landmarks that may be candidates
//   k_fuse_search    k_match_guided's walk, eight lanes per keep landmark, with the 3-D gate in front of the knn-2 and the
//                    acceptance test at the end: per keep landmark the accepted key d0 << 16 | drop position, or none
//   k_fuse_resolve   one workgroup: atomicMin of d0 << 16 | keep position per claimed drop position, then the ordered
//                    compaction (ballot + scan) of the keep landmarks that hold their claim
//
// Every result is a function of the keys alone (distance, position), never of the order in which the binning scatter or
// the atomics ran.  All projection arithmetic is f64, every operation rounded on its own (-ffp-contract=off).
#include "lm_table.hpp"
#include "reloc.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace mslam
{

struct FuseHead // the mapped result block's first 16 bytes
{
    int32_t n_pairs, pad[3];
};

// the pair list, on the device (what the replacement reads) and in the mapped result block (what the host reads)
struct FusePairs
{
    int32_t *keep_pos, *drop_pos, *dist;
    int64_t *keep_lid, *drop_lid;
};

struct FuseArgs
{
    const uint8_t* desc; // the store
    const double* world;
    const int64_t* lid;
    const int32_t* n;
    int K, keep_slot, drop_slot, nk_cap, nd_cap; // n*_cap: what the host knows the entries' counts not to exceed
    LmTable tab_keep, tab_drop;
    double R[9], t[3], fx, fy, cx, cy, radius, gate2, ratio;
    int max_distance, width, height;
    GuidedGrid grid;
    float* drop_xy;   // [nd][2]
    double* keep_uv;  // [nk][2]
    uint8_t* keep_ok; // [nk] eligible and in front of the camera
    const int32_t* cell_off;
    const float4* list;
    const uint8_t* list_desc;
    uint32_t* acc;  // [nk] the accepted key, or ~0u
    uint32_t* best; // [nd] cleared to ~0u
    FusePairs dev, host;
    double* pair_world; // [P][3] the keep landmark's world point
    int32_t* n_pairs;   // device
    FuseHead* head;     // mapped
};

__device__ __forceinline__ int fuse_count(const FuseArgs& a, int side) // side 0 = keep, 1 = drop
{
    return min(max(a.n[side ? a.drop_slot : a.keep_slot], 0), side ? a.nd_cap : a.nk_cap);
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
    if(i >= fuse_count(a, side))
        return;
    const size_t at = (size_t)(side ? a.drop_slot : a.keep_slot) * a.K + i;
    const bool eligible = lm_find(side ? a.tab_keep : a.tab_drop, (unsigned long long)a.lid[at]) < 0;
    const double X = a.world[at * 3], Y = a.world[at * 3 + 1], Z = a.world[at * 3 + 2];
    const double c0 = ((a.R[0] * X + a.R[1] * Y) + a.R[2] * Z) + a.t[0];
    const double c1 = ((a.R[3] * X + a.R[4] * Y) + a.R[5] * Z) + a.t[1];
    const double c2 = ((a.R[6] * X + a.R[7] * Y) + a.R[8] * Z) + a.t[2];
    const double u = (c0 / c2) * a.fx + a.cx, v = (c1 / c2) * a.fy + a.cy;
    const bool ok = eligible && c2 > 0.0;
    if(side)
    {
        const float nan = __int_as_float(0x7fc00000);
        a.drop_xy[2 * (size_t)i] = ok ? (float)u : nan; // (the in-frame test is k_guided_bin's)
        a.drop_xy[2 * (size_t)i + 1] = ok ? (float)v : nan;
    }
    else
    {
        a.keep_uv[2 * (size_t)i] = u, a.keep_uv[2 * (size_t)i + 1] = v;
        a.keep_ok[i] = ok ? 1 : 0;
    }
}

// 64 or 256 threads: 8 or 32 keep landmarks per workgroup
__global__ __launch_bounds__(256) void k_fuse_search(FuseArgs a)
{
    const int g = threadIdx.x & 7;
    const int j = blockIdx.x * (blockDim.x >> 3) + (threadIdx.x >> 3);
    const bool live = j < fuse_count(a, 0); // (the eight lanes of a landmark agree)
    uint32_t k0 = ~0u, k1 = ~0u;
    if(live && a.keep_ok[j])
    {
        const double u = a.keep_uv[2 * (size_t)j], v = a.keep_uv[2 * (size_t)j + 1];
        int cx0, cx1, cy0, cy1;
        if(guided_span(u, a.radius, a.width, a.grid.shift, &cx0, &cx1) && guided_span(v, a.radius, a.height, a.grid.shift, &cy0, &cy1))
        {
            const size_t at = (size_t)a.keep_slot * a.K + j;
            const uint4* q = reinterpret_cast<const uint4*>(a.desc + at * 32);
            const uint4 qa = q[0], qb = q[1];
            const double X = a.world[at * 3], Y = a.world[at * 3 + 1], Z = a.world[at * 3 + 2];
            const double* dw = a.world + (size_t)a.drop_slot * a.K * 3;
            const uint4* list_desc = reinterpret_cast<const uint4*>(a.list_desc);
            int b = a.cell_off[cy0 * a.grid.nx + cx0], e = a.cell_off[cy0 * a.grid.nx + cx1 + 1];
            for(int cy = cy0; cy <= cy1; ++cy)
            {
                int nb = 0, ne = 0;
                if(cy < cy1)
                    nb = a.cell_off[(cy + 1) * a.grid.nx + cx0], ne = a.cell_off[(cy + 1) * a.grid.nx + cx1 + 1];
                for(int p = b + g; p < e; p += 8)
                {
                    const float4 pt = a.list[p];
                    if(fabs((double)pt.x - u) <= a.radius && fabs((double)pt.y - v) <= a.radius)
                    {
                        const size_t i = (size_t)__float_as_int(pt.z); // a drop position: < the drop entry's count
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
        a.acc[j] = ok ? k0 : ~0u;
    }
}

constexpr int kResolveThreads = 1024;

// one workgroup.  The claims go through atomicMin and are read back through it as well (an atomic that changes nothing),
// so the second phase sees what the first one left whatever the caches hold.
__global__ __launch_bounds__(kResolveThreads) void k_fuse_resolve(FuseArgs a)
{
    __shared__ uint32_t wcnt[kResolveThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nk = fuse_count(a, 0);
    for(int j = tid; j < nk; j += kResolveThreads)
    {
        const uint32_t k = a.acc[j];
        if(k != ~0u)
            atomicMin(&a.best[k & 0xFFFFu], (k & 0xFFFF0000u) | (uint32_t)j);
    }
    __syncthreads();
    uint32_t base = 0;
    for(int j0 = 0; j0 < nk; j0 += kResolveThreads)
    {
        const int j = j0 + tid;
        uint32_t k = ~0u;
        bool win = false;
        if(j < nk)
        {
            k = a.acc[j];
            win = k != ~0u && atomicMin(&a.best[k & 0xFFFFu], ~0u) == ((k & 0xFFFF0000u) | (uint32_t)j);
        }
        const unsigned long long bal = __ballot(win);
        if(lane == 0)
            wcnt[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t pre = 0, tot = 0;
        for(int w = 0; w < kResolveThreads / 64; ++w)
        {
            if(w < wave)
                pre += wcnt[w];
            tot += wcnt[w];
        }
        if(win)
        {
            // one pair per drop position and per keep position: fewer than min(nk, nd) + 1 rows
            const size_t p = base + pre + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
            const int i = (int)(k & 0xFFFFu), d = (int)(k >> 16);
            const size_t ka = (size_t)a.keep_slot * a.K + j, da = (size_t)a.drop_slot * a.K + i;
            const int64_t kl = a.lid[ka], dl = a.lid[da];
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
    if(tid == 0)
    {
        *a.n_pairs = (int32_t)base;
        a.head->n_pairs = (int32_t)base;
    }
}

} // namespace mslam

using namespace mslam;

namespace
{
struct SearchParams
{
    int keep_id, drop_id;
    const double *R, *t;
    double fx, fy, cx, cy;
    int width, height;
    double radius;
    int max_distance;
    double ratio, max_world_distance;
};

// what one search leaves behind for the caller
struct SearchPlan
{
    FuseArgs a{};
    int P = 0;                       // rows of the pair arrays: min of the two entries' upper bounds
    LmTable tab_rep{};               // the replacement table inside d_lm_table (kf_fuse)
    bool empty = false;              // an entry holds nothing: no launch, no pairs
};

int search_check(mslam_hip_ctx* c, const std::string& me, const SearchParams& p, int* keep_slot, int* drop_slot)
{
    RelocState* r = c->reloc;
    if(!p.R || !p.t)
        return fail(c, MSLAM_HIP_E_INVALID, me + ": bad argument");
    if(p.keep_id == p.drop_id)
        return fail(c, MSLAM_HIP_E_INVALID, me + ": keep_id and drop_id name one entry");
    int rc = store_slot(c, me, "id", p.keep_id, keep_slot);
    if(!rc)
        rc = store_slot(c, me, "id", p.drop_id, drop_slot);
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
    if(r->n_upper[(size_t)*keep_slot] > 65535 || r->n_upper[(size_t)*drop_slot] > 65535)
        return fail(c, MSLAM_HIP_E_INVALID, me + ": entries of more than 65535 landmarks are not supported");
    return MSLAM_HIP_OK;
}

// scratch and launches of one search on c->stream.  up: the bytes of the caller's own upload (the search uploads
// nothing); with_rep: room for kf_fuse's replacement table.  The mapped result block is
// [FuseHead | keep_pos P | drop_pos P | dist P | keep_lid P | drop_lid P].
int search_enqueue(mslam_hip_ctx* c, const SearchParams& p, int keep_slot, int drop_slot, size_t up, bool with_rep, SearchPlan* plan)
{
    RelocState* r = c->reloc;
    const int nk = r->n_upper[(size_t)keep_slot], nd = r->n_upper[(size_t)drop_slot];
    plan->P = std::min(nk, nd);
    plan->empty = plan->P == 0;
    if(plan->empty)
        return MSLAM_HIP_OK;
    const size_t K = (size_t)c->p.max_keypoints, P = (size_t)plan->P;
    const size_t bk = lm_bucket_count((size_t)nk), bd = lm_bucket_count((size_t)nd), bp = with_rep ? lm_bucket_count(P) : 0;
    // one block, one clear: [keep table | drop table | replacement table | best nd x u32]
    const size_t o_best = (bk + bd + bp) * sizeof(LmBucket), tab_bytes = o_best + (size_t)nd * 4;
    // the arena
    size_t o = 0;
    auto carve = [&o](size_t bytes) {
        const size_t at = o;
        o += al256(bytes);
        return at;
    };
    const size_t a_xy = carve((size_t)nd * 8), a_uv = carve((size_t)nk * 16), a_ok = carve((size_t)nk), a_off = carve((size_t)(kGuidedMaxCells + 1) * 4);
    const size_t a_list = carve((size_t)nd * 16), a_ldesc = carve((size_t)nd * 32), a_acc = carve((size_t)nk * 4);
    const size_t a_kpos = carve(P * 4), a_dpos = carve(P * 4), a_dist = carve(P * 4), a_klid = carve(P * 8), a_dlid = carve(P * 8);
    const size_t a_world = carve(P * 24), a_n = carve(4);
    const size_t h_kpos = al256(sizeof(FuseHead)), h_dpos = h_kpos + al256(P * 4), h_dist = h_dpos + al256(P * 4);
    const size_t h_klid = h_dist + al256(P * 4), h_dlid = h_klid + al256(P * 8), h_bytes = h_dlid + al256(P * 8);
    int rc = reloc_scratch(c, up, o, h_bytes);
    if(rc)
        return rc;
    FuseArgs& a = plan->a;
    a.tab_keep = lm_table_grow(c, (size_t)nk, tab_bytes);
    if(!a.tab_keep.b)
        return MSLAM_HIP_E_RUNTIME;
    a.tab_drop = lm_table_grow(c, (size_t)nd, tab_bytes, bk * sizeof(LmBucket)); // (the block has its size: no growth, no failure)
    if(with_rep)
        plan->tab_rep = lm_table_grow(c, P, tab_bytes, (bk + bd) * sizeof(LmBucket));
    uint8_t *A = r->d_arena, *T = r->d_lm_table, *H = r->h_res.dev();
    a.desc = r->d_desc, a.world = r->d_world, a.lid = r->d_lid, a.n = r->d_n;
    a.K = (int)K, a.keep_slot = keep_slot, a.drop_slot = drop_slot, a.nk_cap = nk, a.nd_cap = nd;
    std::memcpy(a.R, p.R, sizeof(a.R));
    std::memcpy(a.t, p.t, sizeof(a.t));
    a.fx = p.fx, a.fy = p.fy, a.cx = p.cx, a.cy = p.cy, a.radius = p.radius, a.ratio = p.ratio;
    a.gate2 = p.max_world_distance * p.max_world_distance;
    a.max_distance = p.max_distance, a.width = p.width, a.height = p.height, a.grid = guided_grid(p.width, p.height);
    a.drop_xy = reinterpret_cast<float*>(A + a_xy), a.keep_uv = reinterpret_cast<double*>(A + a_uv), a.keep_ok = A + a_ok;
    a.cell_off = reinterpret_cast<const int32_t*>(A + a_off), a.list = reinterpret_cast<const float4*>(A + a_list), a.list_desc = A + a_ldesc;
    a.acc = reinterpret_cast<uint32_t*>(A + a_acc), a.best = reinterpret_cast<uint32_t*>(T + o_best);
    a.dev = FusePairs{reinterpret_cast<int32_t*>(A + a_kpos), reinterpret_cast<int32_t*>(A + a_dpos), reinterpret_cast<int32_t*>(A + a_dist),
                      reinterpret_cast<int64_t*>(A + a_klid), reinterpret_cast<int64_t*>(A + a_dlid)};
    a.host = FusePairs{reinterpret_cast<int32_t*>(H + h_kpos), reinterpret_cast<int32_t*>(H + h_dpos), reinterpret_cast<int32_t*>(H + h_dist),
                       reinterpret_cast<int64_t*>(H + h_klid), reinterpret_cast<int64_t*>(H + h_dlid)};
    a.pair_world = reinterpret_cast<double*>(A + a_world), a.n_pairs = reinterpret_cast<int32_t*>(A + a_n);
    a.head = reinterpret_cast<FuseHead*>(H);
    reinterpret_cast<FuseHead*>(r->h_res.get())->n_pairs = -1; // (overwritten by k_fuse_resolve; checked after the synchronisation)
    // the bin kernel's view: the drop entry's projections are the keypoints
    GuidedArgs g{};
    g.kp_desc = r->d_desc + (size_t)drop_slot * K * 32, g.kp_xy = a.drop_xy;
    g.kp_cnt = r->d_n + drop_slot, g.kp_cap = nd;
    g.width = p.width, g.height = p.height, g.grid = a.grid;
    g.cell_off = reinterpret_cast<int32_t*>(A + a_off), g.list = reinterpret_cast<float4*>(A + a_list), g.list_desc = A + a_ldesc;
    hipStream_t s = c->stream;
    const dim3 both((unsigned)((std::max(nk, nd) + 255) / 256), 2);
    {
        StageScope ts(c, "fuse_clear");
        MSLAM_CHK(c, hipMemsetAsync(T, 0xFF, tab_bytes, s));
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
        hipLaunchKernelGGL(k_fuse_resolve, dim3(1), dim3(kResolveThreads), 0, s, a);
    }
    MSLAM_CHK(c, hipGetLastError());
    return MSLAM_HIP_OK;
}

// after the synchronisation: the count, and the pairs when they fit
int search_collect(mslam_hip_ctx* c, const std::string& me, const SearchPlan& plan, int32_t* keep_pos, int32_t* drop_pos, int64_t* keep_lid,
                   int64_t* drop_lid, int32_t* dist, int capacity, int* n_pairs)
{
    if(plan.empty)
        return MSLAM_HIP_OK;
    RelocState* r = c->reloc;
    const int32_t n = reinterpret_cast<const FuseHead*>(r->h_res.get())->n_pairs;
    if(n < 0 || n > plan.P)
        return fail(c, MSLAM_HIP_E_RUNTIME, me + ": the kernels left no result");
    *n_pairs = n;
    if(n > capacity)
        return fail(c, MSLAM_HIP_E_CAPACITY, me + ": " + std::to_string(n) + " pairs, more than `capacity`");
    const uint8_t* H = r->h_res.get();
    const size_t dev = reinterpret_cast<size_t>(r->h_res.dev());
    auto at = [&](const void* dev_ptr) { return H + (reinterpret_cast<size_t>(dev_ptr) - dev); };
    if(keep_pos)
        std::memcpy(keep_pos, at(plan.a.host.keep_pos), (size_t)n * 4);
    if(drop_pos)
        std::memcpy(drop_pos, at(plan.a.host.drop_pos), (size_t)n * 4);
    if(dist)
        std::memcpy(dist, at(plan.a.host.dist), (size_t)n * 4);
    if(keep_lid)
        std::memcpy(keep_lid, at(plan.a.host.keep_lid), (size_t)n * 8);
    if(drop_lid)
        std::memcpy(drop_lid, at(plan.a.host.drop_lid), (size_t)n * 8);
    return MSLAM_HIP_OK;
}
} // namespace

extern "C" {

int mslam_hip_kf_fuse_search(mslam_hip_ctx* c, int keep_id, int drop_id, const double* R, const double* t, double fx, double fy, double cx,
                             double cy, int width, int height, double radius, int max_distance, double ratio, double max_world_distance,
                             int32_t* keep_pos, int32_t* drop_pos, int64_t* keep_lid, int64_t* drop_lid, int32_t* dist, int capacity,
                             int* n_pairs)
{
    if(n_pairs)
        *n_pairs = 0;
    int rc = reloc_enter(c);
    if(rc)
        return rc;
    const std::string me = "kf_fuse_search";
    if(!n_pairs || capacity < 0 || (capacity > 0 && (!keep_pos || !drop_pos || !keep_lid || !drop_lid || !dist)))
        return fail(c, MSLAM_HIP_E_INVALID, me + ": bad argument");
    const SearchParams p{keep_id, drop_id, R, t, fx, fy, cx, cy, width, height, radius, max_distance, ratio, max_world_distance};
    int ks = -1, ds = -1;
    rc = search_check(c, me, p, &ks, &ds);
    if(rc)
        return rc;
    SearchPlan plan;
    rc = search_enqueue(c, p, ks, ds, 0, false, &plan);
    if(rc)
        return rc;
    if(!plan.empty)
        MSLAM_CHK(c, hipStreamSynchronize(c->stream));
    return search_collect(c, me, plan, keep_pos, drop_pos, keep_lid, drop_lid, dist, capacity, n_pairs);
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
    if(n_pairs)
        *n_pairs = 0;
    if(n_rewritten)
        *n_rewritten = 0;
    int rc = reloc_enter(c);
    if(rc)
        return rc;
    const std::string me = "kf_fuse";
    if(!n_pairs || capacity < 0)
        return fail(c, MSLAM_HIP_E_INVALID, me + ": bad argument");
    const SearchParams p{keep_id, drop_id, R, t, fx, fy, cx, cy, width, height, radius, max_distance, ratio, max_world_distance};
    int ks = -1, ds = -1;
    rc = search_check(c, me, p, &ks, &ds);
    if(rc)
        return rc;
    RelocState* r = c->reloc;
    std::vector<int32_t> slots;
    const int n_max = live_slots(r, &slots);
    // one upload: [live slots | the count, zero]
    const size_t o_cnt = slots.size() * 4, up = o_cnt + 4;
    SearchPlan plan;
    rc = search_enqueue(c, p, ks, ds, up, true, &plan);
    if(rc || plan.empty)
        return rc;
    uint8_t *h = r->h_up, *d = r->d_up;
    std::memcpy(h, slots.data(), slots.size() * 4);
    std::memset(h + o_cnt, 0, 4);
    MSLAM_CHK(c, hipMemcpyAsync(d, h, up, hipMemcpyHostToDevice, c->stream));
    // drop_lid -> keep_lid with the keep landmark's world point, straight from the device list (at most P places); nothing
    // when the pairs exceed `capacity`
    const ReplaceList l{plan.a.dev.drop_lid, plan.a.dev.keep_lid, plan.a.pair_world, plan.a.n_pairs, plan.P, std::min(capacity, plan.P)};
    rc = rewrite_enqueue(c, l, plan.tab_rep, reinterpret_cast<const int32_t*>(d), (int)slots.size(), n_max,
                         reinterpret_cast<uint32_t*>(d + o_cnt), "fuse_table", "fuse_replace");
    if(!rc)
        rc = rewrite_count(c, reinterpret_cast<const uint32_t*>(d + o_cnt), n_rewritten);
    return rc ? rc : search_collect(c, me, plan, keep_pos, drop_pos, keep_lid, drop_lid, dist, capacity, n_pairs);
}

} // extern "C"
