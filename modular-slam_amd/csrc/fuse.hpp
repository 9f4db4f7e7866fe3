// fuse.hpp — what landmark fusion into one target (k_fuse.hip) and into many (k_fuse_multi.hip) share: the arguments both
// kernel sets carry, the projection of a landmark of either side, the search of one keep landmark against one target's
// lists (the walk of guided_walk.hpp behind the 3-D gate, then the acceptance test), the ordered emission of the pair
// rows, and on the host the argument checks, the scratch layout, the rewrite tail and the read-back.  The host functions
// are defined in k_fuse.hip.
#pragma once
#include "guided_walk.hpp"

#include <string>
#include <vector>

namespace mslam
{

struct FuseHead // the mapped result block's first 16 bytes
{
    int32_t n_pairs, pad[3];
};

// the pair list, on the device (what the replacement reads), in the mapped result block (what the host reads) and as the
// caller's arrays; target: nullptr in the single-target calls
struct FusePairs
{
    int32_t *target, *keep_pos, *drop_pos, *dist;
    int64_t *keep_lid, *drop_lid;
};

// ND: the sum of the targets' upper bounds, nk: the keep entry's, M: the number of targets (1 in the single-target calls)
struct FuseCore
{
    const uint8_t* desc; // the store
    const double* world;
    const int64_t* lid;
    const int32_t* n;
    int K, keep_slot, nk_cap; // nk_cap: what the host knows the keep entry's count not to exceed
    LmTable tab_keep, tab_drop;
    double fx, fy, cx, cy, radius, gate2, ratio;
    int max_distance, width, height;
    GuidedGrid grid;
    float* drop_xy;     // [ND][2]
    double* keep_uv;    // [M][nk][2]
    uint8_t* keep_ok;   // [M][nk] eligible and in front of the target's camera
    int32_t* cell_off;  // [M][kGuidedMaxCells + 1]
    float4* list;       // [ND]
    uint8_t* list_desc; // [ND][32]
    uint32_t* acc;      // [M][nk] the accepted key, or ~0u
    uint32_t* best;     // [ND] cleared to ~0u
    FusePairs dev, host;
    double* pair_world; // [P][3] the keep landmark's world point
    int32_t* n_pairs;   // device
    FuseHead* head;     // mapped
};

__device__ __forceinline__ int fuse_keep_count(const FuseCore& a) { return min(max(a.n[a.keep_slot], 0), a.nk_cap); }

// Landmark i of entry `slot` under the pose (R, t): eligibility (its id is absent from the other side's table) and the
// projection.  side 0, a keep landmark, leaves (u, v) and a flag at `out`; side 1, a drop landmark, leaves the f32
// "keypoint" ((float)u, (float)v) at `out`, or NaNs when it is ineligible or behind the camera, so that the binning lists
// exactly the drop landmarks that may be candidates (the in-frame test is the binning's).
__device__ __forceinline__ void fuse_project(const FuseCore& a, const double* R, const double* t, int side, int slot, int i, size_t out)
{
    const size_t at = (size_t)slot * a.K + i;
    const bool eligible = lm_find(side ? a.tab_keep : a.tab_drop, (unsigned long long)a.lid[at]) < 0;
    const GuidedUV p = guided_project(R, t, a.fx, a.fy, a.cx, a.cy, a.world + at * 3);
    const bool ok = eligible && p.c2 > 0.0;
    if(side)
    {
        const float nan = __int_as_float(0x7fc00000);
        a.drop_xy[2 * out] = ok ? (float)p.u : nan;
        a.drop_xy[2 * out + 1] = ok ? (float)p.v : nan;
    }
    else
    {
        a.keep_uv[2 * out] = p.u, a.keep_uv[2 * out + 1] = p.v;
        a.keep_ok[out] = ok ? 1 : 0;
    }
}

// Keep landmark j (live: j is one; the eight lanes g of a landmark agree) against the lists of the target in `drop_slot`:
// guided_walk among the listed drop landmarks within gate2 of it in the world, then the acceptance test -> the accepted key
// d0 << 16 | drop position, or ~0u.  row: where j's projection under the target's pose lies in keep_uv / keep_ok.
__device__ __forceinline__ uint32_t fuse_search_one(const FuseCore& a, bool live, int j, size_t row, int drop_slot, const int32_t* cell_off,
                                                    const float4* list, const uint8_t* list_desc, int g)
{
    const bool active = live && a.keep_ok[row];
    const size_t at = (size_t)a.keep_slot * a.K + j;
    double u = 0.0, v = 0.0, X = 0.0, Y = 0.0, Z = 0.0;
    if(active)
    {
        u = a.keep_uv[2 * row], v = a.keep_uv[2 * row + 1];
        X = a.world[at * 3], Y = a.world[at * 3 + 1], Z = a.world[at * 3 + 2];
    }
    const double* dw = a.world + (size_t)drop_slot * a.K * 3;
    const uint2 k = guided_walk<false>(active, u, v, a.radius, a.width, a.height, a.grid, cell_off, list, list_desc, a.desc + at * 32, g, [&](int i) {
        // i: a drop position, < the target's count
        const double dx = dw[(size_t)i * 3] - X, dy = dw[(size_t)i * 3 + 1] - Y, dz = dw[(size_t)i * 3 + 2] - Z;
        return ((dx * dx + dy * dy) + dz * dz) <= a.gate2; // (a NaN fails)
    });
    const int d0 = (int)(k.x >> 16), d1 = (int)(k.y >> 16);
    const bool ok = k.x != ~0u && d0 <= a.max_distance && (k.y == ~0u || (double)d0 < a.ratio * (double)d1);
    return ok ? k.x : ~0u;
}

constexpr int kFuseEmitThreads = 1024;

// One workgroup of kFuseEmitThreads threads: the ordered compaction (ballot + scan) of the keep positions j in [0, nk)
// that won(j) gives an accepted key for (~0u: j is no pair), as pair rows from row `base` on -> the row after the last
// one.  target, drop_slot: whom the keys were accepted against; wcnt: kFuseEmitThreads / 64 words of LDS.
template <class Won>
__device__ __forceinline__ uint32_t fuse_emit(const FuseCore& a, int nk, int target, int drop_slot, uint32_t base, uint32_t* wcnt, Won&& won)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for(int j0 = 0; j0 < nk; j0 += kFuseEmitThreads)
    {
        const int j = j0 + tid;
        const uint32_t k = j < nk ? won(j) : ~0u;
        const unsigned long long bal = __ballot(k != ~0u);
        if(lane == 0)
            wcnt[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t pre = 0, tot = 0;
        for(int o = 0; o < kFuseEmitThreads / 64; ++o)
        {
            if(o < wave)
                pre += wcnt[o];
            tot += wcnt[o];
        }
        if(k != ~0u)
        {
            const size_t p = base + pre + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
            const int i = (int)(k & 0xFFFFu), d = (int)(k >> 16);
            const size_t ka = (size_t)a.keep_slot * a.K + j, da = (size_t)drop_slot * a.K + i;
            const int64_t kl = a.lid[ka], dl = a.lid[da];
            const double x = a.world[ka * 3], y = a.world[ka * 3 + 1], z = a.world[ka * 3 + 2];
            a.dev.keep_pos[p] = a.host.keep_pos[p] = j;
            a.dev.drop_pos[p] = a.host.drop_pos[p] = i;
            a.dev.dist[p] = a.host.dist[p] = d;
            a.dev.keep_lid[p] = a.host.keep_lid[p] = kl;
            a.dev.drop_lid[p] = a.host.drop_lid[p] = dl;
            a.pair_world[p * 3] = x, a.pair_world[p * 3 + 1] = y, a.pair_world[p * 3 + 2] = z;
            if(a.dev.target)
                a.dev.target[p] = a.host.target[p] = target;
        }
        base += tot;
        __syncthreads();
    }
    return base;
}

// ---- host side (k_fuse.hip) -------------------------------------------------------------------------------------------

struct FuseParams // R, t: one pose per target
{
    int keep_id;
    const double *R, *t;
    double fx, fy, cx, cy;
    int width, height;
    double radius;
    int max_distance;
    double ratio, max_world_distance;
};

// what one search leaves behind for the caller
struct FusePlan
{
    int P = 0;            // rows of the pair arrays: min(keep landmarks, all targets' landmarks), by the host's upper bounds
    bool empty = false;   // the keep entry or every target holds nothing: no launch, no pairs
    LmTable tab_rep{};    // the replacement table inside d_lm_table (kf_fuse, kf_fuse_multi)
    size_t tab_bytes = 0; // of d_lm_table, [keep table | drop table | replacement table | best ND x u32]: one block, one clear
    size_t extra_at = 0;  // where the caller's own arrays begin in the arena
};

// The checks after the call's own id rules: the ids' slots (keep first, then the targets in order), the knobs, the sizes.
int fuse_check(mslam_hip_ctx* c, const std::string& me, const FuseParams& p, const int32_t* drop_ids, int n_drop, int* keep_slot,
               std::vector<int>* drop_slots);
// Scratch of one search over the targets in drop_slots — `up` bytes of upload, the arena with `extra_arena` bytes of the
// caller's own at plan->extra_at, the mapped result block
// [FuseHead | target P (with_target) | keep_pos P | drop_pos P | dist P | keep_lid P | drop_lid P] — the id tables
// (with_rep: room for the replacement table) and everything *a holds.  Nothing when plan->empty.
int fuse_setup(mslam_hip_ctx* c, const FuseParams& p, int keep_slot, const std::vector<int>& drop_slots, bool with_target, size_t up,
               size_t extra_arena, bool with_rep, FuseCore* a, FusePlan* plan);
// The live slots and a zero behind them, the count of the rewrite: what kf_fuse and kf_fuse_multi upload -> n_max
int fuse_rewrite_upload(const RelocState* r, std::vector<int32_t>* slots);
// The rewrite behind a search's launches and the call's one synchronisation: every store landmark with a pair's drop id
// takes the keep id and the keep landmark's world point, straight from the device list (at most P places); nothing when
// the pairs exceed `capacity`.  d: fuse_rewrite_upload's words on the device, n_slots of them slots.
int fuse_rewrite(mslam_hip_ctx* c, const FuseCore& a, const FusePlan& plan, uint8_t* d, int n_slots, int n_max, int capacity,
                 const char* stage_table, const char* stage_write, int* n_rewritten);
// after the synchronisation: the count, and the pairs when they fit (a null array of `out` is not asked for)
int fuse_collect(mslam_hip_ctx* c, const std::string& me, const FuseCore& a, const FusePlan& plan, const FusePairs& out, int capacity,
                 int* n_pairs);

} // namespace mslam
