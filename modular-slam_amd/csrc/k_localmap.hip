// k_localmap.hip — the local map on the keyframe store: the union of up to 64 entries as an ordinary entry
// (mslam_hip_kf_union[_dev]) and covisibility counts (mslam_hip_kf_covisible), both on the landmark ids the store keeps
// next to every landmark; and the list rewrite: mslam_hip_kf_update_world writes a list of refined world points into every
// entry that holds their ids (the way back from bundle adjustment, k_ba.hip), and mslam_hip_kf_replace_ids / mslam_hip_kf_fuse
// (k_fuse.hip) rewrite ids, and points, through the same two kernels (rewrite_enqueue, declared in reloc.hpp).
//
// What getLandmarksWithKeypoints builds for track() (reference rgbd_feature_frontend.cpp:256-277): the most recent
// observation of every landmark seen from a set of keyframes (RecentObservationsVisitor, :57-80: the observation whose
// keyframe id is the largest), and the edge test of BasicMap::updateCovisibility (basic_map.cpp:141-164: two keyframes are
// neighbours when they observe a landmark in common).
//
// All run on one open-addressing hash table in device scratch (lm_table.hpp).  A key is claimed with one compare-and-swap;
// what the value holds differs:
//   union        ~pack, pack = (rank + 1) << 32 | list position << 16 | landmark position, lowered with atomicMin: the
//                smallest ~pack is the largest pack, i.e. the listed entry with the largest keyframe id (rank = the rank
//                of its id among the listed ids), and inside one entry the highest position.  The cleared value (all
//                ones) is above every ~pack;
//   covisible    a 64-bit mask, bit k = "entry ids[k] holds this landmark id", so a repeat inside an entry counts once;
//   rewrite      ~(place in the caller's list), lowered with atomicMin: of an id listed twice the later place wins.
// The union's result order is by list position, then landmark position: the grid is laid out that way (blockIdx.y = list
// position), winners are counted per block, one workgroup scans the block counts, and the scatter places every winner
// at its block's offset plus its ballot / popcount prefix, as k_kf_lift does inside one block.
//
// mslam_hip_set_union_descriptor(DISTINCTIVE) (an extension: the reference matches against the most recent observation)
// enqueues three more launches behind the scatter, which leave rows, order, points and ids alone and may replace a row's 32
// descriptor bytes by those of another observation of its landmark — the one with the least median Hamming distance to all
// of them (ORB-SLAM's MapPoint::ComputeDistinctiveDescriptors; distinct.hpp has the rule):
//   k_lm_place     every winner writes its output row into its bucket (one writer per bucket; ~pack is dead after the select);
//   k_lm_observe   the insert's grid: thread (k, i) raises obs[row][k] to i + 1 with atomicMax — one observation per listed
//                  entry, its highest position, whatever the order;
//   k_lm_distinct  one wave per row, lane k = the observation of list position k: all-pairs distances through a per-wave
//                  LDS block, each lane's median by bisection, the wave's minimum of (median, 63 - rank), and the winning
//                  lane overwrites the row's descriptor.  Rows of one or two observations keep the scatter's bytes.
#include "distinct.hpp"
#include "lm_table.hpp"
#include "reloc.hpp"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace mslam
{

// the listed entries of one call, passed by value: nothing is uploaded
struct LmList
{
    int32_t slot[kRelocMaxCand];
    int32_t rank[kRelocMaxCand];
};

struct LmHead // the mapped result block's first 16 bytes, then counts[64]
{
    int32_t needed, pad[3];
};

__device__ __forceinline__ unsigned long long lm_pack(int rank, int k, int i)
{
    return ((unsigned long long)(rank + 1) << 32) | ((unsigned long long)k << 16) | (unsigned long long)i;
}

// One thread per (list position k = blockIdx.y, landmark position i).  as_mask = 0: the union's insert (atomicMin of
// ~pack); as_mask = 1: covisible's insert, every value becomes the empty mask 0.
__global__ __launch_bounds__(256) void k_lm_insert(const int64_t* __restrict__ store_lid, const int32_t* __restrict__ store_n, LmList list,
                                                   int K, LmTable t, int as_mask)
{
    const int k = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int slot = list.slot[k];
    if(i >= entry_count(store_n, slot, K))
        return;
    const long long b = lm_claim(t, (unsigned long long)store_lid[(size_t)slot * K + i]);
    if(b < 0)
        return;
    if(as_mask)
        atomicAnd(&t.b[b].val, 0ull);
    else
        atomicMin(&t.b[b].val, ~lm_pack(list.rank[k], k, i));
}

// Same grid: a thread wins when the bucket of its landmark id holds its own pack.  Per wave the ballot of the winners,
// per block their count.
__global__ __launch_bounds__(256) void k_lm_select(const int64_t* __restrict__ store_lid, const int32_t* __restrict__ store_n, LmList list,
                                                   int K, LmTable t, unsigned long long* __restrict__ win, uint32_t* __restrict__ cnt)
{
    __shared__ uint32_t wsum[4];
    const int k = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = blockIdx.x * 256 + tid;
    const size_t blk = (size_t)k * gridDim.x + blockIdx.x;
    const int slot = list.slot[k];
    bool w = false;
    if(i < entry_count(store_n, slot, K))
    {
        const long long b = lm_find(t, (unsigned long long)store_lid[(size_t)slot * K + i]);
        w = b >= 0 && t.b[b].val == ~lm_pack(list.rank[k], k, i);
    }
    const unsigned long long bal = __ballot(w);
    if(lane == 0)
    {
        win[blk * 4 + wave] = bal;
        wsum[wave] = (uint32_t)__popcll(bal);
    }
    __syncthreads();
    if(tid == 0)
        cnt[blk] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// One workgroup: the exclusive scan of the block counts (ofs[nb] = the total), the new entry's count — 0 when the total
// exceeds the capacity, with the overflow flag when the caller reads no result of its own — and the total for the host.
__global__ __launch_bounds__(256) void k_lm_scan(const uint32_t* __restrict__ cnt, uint32_t* __restrict__ ofs, int nb, int cap,
                                                 int32_t* __restrict__ out_n, uint32_t* __restrict__ flags, int set_flag,
                                                 LmHead* __restrict__ h_res)
{
    __shared__ uint32_t wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t running = 0;
    for(int base = 0; base < nb; base += 256)
    {
        const int b = base + tid;
        const uint32_t v = b < nb ? cnt[b] : 0u;
        uint32_t inc = v; // inclusive scan inside the wave
        for(int o = 1; o < 64; o <<= 1)
        {
            const uint32_t up = __shfl_up(inc, o);
            if(lane >= o)
                inc += up;
        }
        if(lane == 63)
            wsum[wave] = inc;
        __syncthreads();
        uint32_t pre = 0, tot = 0;
        for(int w = 0; w < 4; ++w)
        {
            pre += w < wave ? wsum[w] : 0;
            tot += wsum[w];
        }
        if(b < nb)
            ofs[b] = running + pre + (inc - v);
        running += tot;
        __syncthreads();
    }
    if(tid == 0)
    {
        ofs[nb] = running;
        const bool fits = running <= (uint32_t)cap;
        *out_n = fits ? (int32_t)running : 0;
        if(!fits && set_flag)
            atomicOr(flags, kFlagUnionOverflow);
        h_res->needed = (int32_t)running;
    }
}

// Same grid as k_lm_select: every winner copies its descriptor, world point and landmark id, bit for bit, to position
// ofs[block] + (winners before it in the block) of the new entry.  Nothing is written when the union does not fit.
__global__ __launch_bounds__(256) void k_lm_scatter(const uint8_t* __restrict__ store_desc, const double* __restrict__ store_world,
                                                    const int64_t* __restrict__ store_lid, LmList list, int K,
                                                    const unsigned long long* __restrict__ win, const uint32_t* __restrict__ ofs, int nb,
                                                    uint8_t* __restrict__ out_desc, double* __restrict__ out_world,
                                                    int64_t* __restrict__ out_lid)
{
    if(ofs[nb] > (uint32_t)K)
        return;
    const int k = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = blockIdx.x * 256 + tid;
    const size_t blk = (size_t)k * gridDim.x + blockIdx.x;
    const unsigned long long mine = win[blk * 4 + wave];
    if(!((mine >> lane) & 1ull))
        return;
    uint32_t pre = 0;
    for(int w = 0; w < wave; ++w)
        pre += (uint32_t)__popcll(win[blk * 4 + w]);
    const size_t o = (size_t)ofs[blk] + pre + (uint32_t)__popcll(mine & ((1ull << lane) - 1ull)); // < ofs[nb] <= K
    const size_t src = (size_t)list.slot[k] * K + i; // a winner has i < n <= K
    copy_desc(store_desc + src * 32, out_desc + o * 32);
    out_world[o * 3] = store_world[src * 3], out_world[o * 3 + 1] = store_world[src * 3 + 1], out_world[o * 3 + 2] = store_world[src * 3 + 2];
    out_lid[o] = store_lid[src];
}

// ---- the DISTINCTIVE descriptor mode: three launches behind k_lm_scatter

// k_lm_scatter's grid and row arithmetic: every winner leaves its output row o in the bucket of its landmark id.  `cap` is
// the number of rows the observation table has (<= K): nothing is written when the union does not fit.
__global__ __launch_bounds__(256) void k_lm_place(const int64_t* __restrict__ store_lid, LmList list, int K, LmTable t,
                                                  const unsigned long long* __restrict__ win, const uint32_t* __restrict__ ofs, int nb,
                                                  int cap)
{
    if(ofs[nb] > (uint32_t)cap)
        return;
    const int k = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = blockIdx.x * 256 + tid;
    const size_t blk = (size_t)k * gridDim.x + blockIdx.x;
    const unsigned long long mine = win[blk * 4 + wave];
    if(!((mine >> lane) & 1ull))
        return;
    uint32_t pre = 0;
    for(int w = 0; w < wave; ++w)
        pre += (uint32_t)__popcll(win[blk * 4 + w]);
    const uint32_t o = ofs[blk] + pre + (uint32_t)__popcll(mine & ((1ull << lane) - 1ull));
    const long long b = lm_find(t, (unsigned long long)store_lid[(size_t)list.slot[k] * K + i]);
    if(b >= 0)
        t.b[b].val = (unsigned long long)o; // the one winner of this id: a plain store
}

// k_lm_insert's grid: obs[o][k] = 1 + the highest position at which entry k holds the landmark of row o (0: it does not)
__global__ __launch_bounds__(256) void k_lm_observe(const int64_t* __restrict__ store_lid, const int32_t* __restrict__ store_n, LmList list,
                                                    int K, LmTable t, const uint32_t* __restrict__ ofs, int nb, int cap,
                                                    uint32_t* __restrict__ obs)
{
    if(ofs[nb] > (uint32_t)cap)
        return;
    const int k = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int slot = list.slot[k];
    if(i >= entry_count(store_n, slot, K))
        return;
    const long long b = lm_find(t, (unsigned long long)store_lid[(size_t)slot * K + i]);
    if(b < 0)
        return;
    const unsigned long long o = t.b[b].val;
    if(o < (unsigned long long)ofs[nb]) // (every key has a winner, which placed its row: always)
        atomicMax(&obs[o * kRelocMaxCand + k], (uint32_t)i + 1u);
}

// One wave per union row, four rows per block.  The list's slots and ranks are wanted per lane: thread 0 stages them in LDS
// from the by-value argument with uniform indices (a lane-indexed read of the argument would go through scratch).
__global__ __launch_bounds__(256) void k_lm_distinct(const uint8_t* __restrict__ store_desc, LmList list, int n_ids, int K,
                                                     const uint32_t* __restrict__ ofs, int nb, int cap,
                                                     const uint32_t* __restrict__ obs, uint8_t* __restrict__ out_desc)
{
    __shared__ int32_t s_slot[kRelocMaxCand], s_rank[kRelocMaxCand];
    __shared__ uint16_t s_dist[4][kRelocMaxCand][64]; // [wave][column c][lane]: lane-contiguous, no bank conflicts
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if(tid == 0)
    {
#pragma unroll
        for(int k = 0; k < kRelocMaxCand; ++k)
            s_slot[k] = list.slot[k], s_rank[k] = list.rank[k];
    }
    __syncthreads();
    const uint32_t total = ofs[nb];
    const uint32_t o = blockIdx.x * 4u + (uint32_t)wave;
    if(total > (uint32_t)cap || o >= total)
        return;
    const uint32_t p = lane < n_ids ? obs[(size_t)o * kRelocMaxCand + lane] : 0u;
    const bool present = p > 0u && p <= (uint32_t)K;
    const unsigned long long bal = __ballot(present);
    const int N = __popcll(bal);
    if(N <= 2)
        return; // the most recent observation is the choice, and the scatter wrote it
    uint32_t d[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if(present)
    {
        const uint4* src = reinterpret_cast<const uint4*>(store_desc + ((size_t)s_slot[lane] * K + (p - 1u)) * 32);
        const uint4 a = src[0], b = src[1];
        d[0] = a.x, d[1] = a.y, d[2] = a.z, d[3] = a.w, d[4] = b.x, d[5] = b.y, d[6] = b.z, d[7] = b.w;
    }
    // column c of every lane's row: the distance to the c-th present lane (wave-uniform loop)
    int c = 0;
    for(unsigned long long rest = bal; rest; rest &= rest - 1ull, ++c)
    {
        const int j = __ffsll((long long)rest) - 1;
        uint32_t e[8];
#pragma unroll
        for(int w = 0; w < 8; ++w)
            e[w] = (uint32_t)__builtin_amdgcn_readlane((int)d[w], j);
        s_dist[wave][c][lane] = (uint16_t)distinct_distance(d, e);
    }
    // (each lane reads back what it wrote itself: no barrier)
    uint32_t key = kDistinctAbsent;
    if(present)
        key = distinct_key(distinct_mth_smallest(&s_dist[wave][0][lane], 64, N, (N - 1) / 2), s_rank[lane]);
    uint32_t best = key;
#pragma unroll
    for(int s = 32; s > 0; s >>= 1)
        best = min(best, (uint32_t)__shfl_xor((int)best, s));
    if(present && key == best)
    {
        uint4* dst = reinterpret_cast<uint4*>(out_desc + (size_t)o * 32);
        dst[0] = make_uint4(d[0], d[1], d[2], d[3]);
        dst[1] = make_uint4(d[4], d[5], d[6], d[7]);
    }
}

// One workgroup per listed entry k, over a table built from entry `id` with empty masks: a landmark id the table holds
// sets bit k of its mask, and counts when the bit was clear (a repeat inside entry k counts once).
__global__ __launch_bounds__(256) void k_lm_covisible(const int64_t* __restrict__ store_lid, const int32_t* __restrict__ store_n, LmList list,
                                                      int K, LmTable t, int32_t* __restrict__ h_counts)
{
    __shared__ uint32_t wsum[4];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slot = list.slot[k];
    const int n = entry_count(store_n, slot, K);
    const unsigned long long bit = 1ull << k;
    uint32_t mine = 0; // (wave-uniform: every lane adds the same popcount)
    for(int base = 0; base < n; base += 256)
    {
        const int i = base + tid;
        bool hit = false;
        if(i < n)
        {
            const long long b = lm_find(t, (unsigned long long)store_lid[(size_t)slot * K + i]);
            hit = b >= 0 && !(atomicOr(&t.b[b].val, bit) & bit);
        }
        mine += (uint32_t)__popcll(__ballot(hit));
    }
    if(lane == 0)
        wsum[wave] = mine;
    __syncthreads();
    if(tid == 0)
        h_counts[k] = (int32_t)(((wsum[0] + wsum[1]) + wsum[2]) + wsum[3]);
}

__device__ __forceinline__ int replace_count(const ReplaceList& l)
{
    if(!l.n_dev)
        return l.n;
    const int n = *l.n_dev;
    return n >= 0 && n <= l.cap ? n : 0;
}

// the table of a rewrite's list: value = ~(place), lowered with atomicMin
__global__ __launch_bounds__(256) void k_fuse_table(ReplaceList l, LmTable t)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if(i >= replace_count(l))
        return;
    const long long b = lm_claim(t, (unsigned long long)l.from[i]);
    if(b >= 0)
        atomicMin(&t.b[b].val, ~(unsigned long long)i);
}

// grid (landmark blocks, live slots): a landmark whose id the table holds takes the listed id and the listed world point,
// whichever the list gives.  Every thread reads and writes its own landmark only, so the substitution is simultaneous.
// *rewritten counts the matches (an integer count: its value does not depend on the order of the additions).
__global__ __launch_bounds__(256) void k_fuse_replace(int64_t* __restrict__ store_lid, double* __restrict__ store_world,
                                                      const int32_t* __restrict__ store_n, const int32_t* __restrict__ slots, int K,
                                                      LmTable t, ReplaceList l, uint32_t* __restrict__ rewritten)
{
    const int slot = slots[blockIdx.y], i = blockIdx.x * 256 + threadIdx.x;
    const int n = entry_count(store_n, slot, K), n_list = replace_count(l);
    bool hit = false;
    if(i < n && n_list > 0)
    {
        const size_t at = (size_t)slot * K + i;
        const long long b = lm_find(t, (unsigned long long)store_lid[at]);
        if(b >= 0)
        {
            const unsigned long long src = ~t.b[b].val;
            if(src < (unsigned long long)n_list)
            {
                hit = true;
                if(l.to)
                    store_lid[at] = l.to[src];
                if(l.xyz)
                    store_world[at * 3] = l.xyz[src * 3], store_world[at * 3 + 1] = l.xyz[src * 3 + 1], store_world[at * 3 + 2] = l.xyz[src * 3 + 2];
            }
        }
    }
    const unsigned long long bal = __ballot(hit);
    if((threadIdx.x & 63) == 0 && bal)
        atomicAdd(rewritten, (uint32_t)__popcll(bal));
}

} // namespace mslam

using namespace mslam;

// ---- the list rewrite (declared in reloc.hpp: k_fuse.hip calls it too)
int mslam::live_slots(const RelocState* r, std::vector<int32_t>* slots)
{
    int n_max = 0;
    for(const auto& e : r->slot_of)
    {
        slots->push_back(e.second);
        n_max = std::max(n_max, r->n_upper[(size_t)e.second]);
    }
    std::sort(slots->begin(), slots->end());
    return n_max;
}

int mslam::rewrite_enqueue(mslam_hip_ctx* c, const ReplaceList& l, LmTable t, const int32_t* d_slots, int n_slots, int n_max,
                           uint32_t* d_count, const char* stage_table, const char* stage_write)
{
    RelocState* r = c->reloc;
    {
        StageScope ts(c, stage_table);
        hipLaunchKernelGGL(k_fuse_table, dim3((unsigned)((l.n + 255) / 256)), dim3(256), 0, c->stream, l, t);
    }
    {
        StageScope ts(c, stage_write);
        hipLaunchKernelGGL(k_fuse_replace, dim3((unsigned)std::max((n_max + 255) / 256, 1), (unsigned)n_slots), dim3(256), 0, c->stream,
                           r->d_lid.get(), r->d_world.get(), r->d_n.get(), d_slots, c->p.max_keypoints, t, l, d_count);
    }
    MSLAM_CHK(c, hipGetLastError());
    return MSLAM_HIP_OK;
}

int mslam::rewrite_count(mslam_hip_ctx* c, const uint32_t* d_count, int* n_out)
{
    uint32_t n = 0;
    MSLAM_CHK(c, hipMemcpyAsync(&n, d_count, 4, hipMemcpyDeviceToHost, c->stream));
    MSLAM_CHK(c, hipStreamSynchronize(c->stream));
    if(n_out)
        *n_out = (int)n;
    return MSLAM_HIP_OK;
}

int mslam::rewrite_host_list(mslam_hip_ctx* c, const int64_t* from, const int64_t* to, const double* xyz, int n, const char* stage_table,
                             const char* stage_write, int* n_out)
{
    RelocState* r = c->reloc;
    if(n == 0 || r->slot_of.empty())
        return MSLAM_HIP_OK;
    std::vector<int32_t> slots;
    const int n_max = live_slots(r, &slots);
    // one upload: [from n x i64 | to n x i64 | points n x 3 f64 | live slots | the count, zero], `to` and the points when given
    const size_t o_to = (size_t)n * 8, o_xyz = o_to + (to ? (size_t)n * 8 : 0), o_slots = o_xyz + (xyz ? (size_t)n * 24 : 0);
    const size_t o_cnt = o_slots + slots.size() * 4, up = o_cnt + 4;
    int rc = reloc_scratch(c, up, 0, 0);
    if(rc)
        return rc;
    const LmTable table = lm_table_grow(c, (size_t)n);
    if(!table.b)
        return MSLAM_HIP_E_RUNTIME;
    uint8_t *h = r->h_up, *d = r->d_up;
    std::memcpy(h, from, (size_t)n * 8);
    if(to)
        std::memcpy(h + o_to, to, (size_t)n * 8);
    if(xyz)
        std::memcpy(h + o_xyz, xyz, (size_t)n * 24);
    std::memcpy(h + o_slots, slots.data(), slots.size() * 4);
    std::memset(h + o_cnt, 0, 4);
    const ReplaceList l{reinterpret_cast<const int64_t*>(d), to ? reinterpret_cast<const int64_t*>(d + o_to) : nullptr,
                        xyz ? reinterpret_cast<const double*>(d + o_xyz) : nullptr, nullptr, n, n};
    MSLAM_CHK(c, hipMemcpyAsync(d, h, up, hipMemcpyHostToDevice, c->stream));
    MSLAM_CHK(c, hipMemsetAsync(table.b, 0xFF, lm_bytes(table), c->stream));
    rc = rewrite_enqueue(c, l, table, reinterpret_cast<const int32_t*>(d + o_slots), (int)slots.size(), n_max,
                         reinterpret_cast<uint32_t*>(d + o_cnt), stage_table, stage_write);
    return rc ? rc : rewrite_count(c, reinterpret_cast<const uint32_t*>(d + o_cnt), n_out);
}

// the per-block arrays of nb blocks, in bytes: [win nb x 4 u64 | cnt nb | ofs nb + 1]; and nb of a block of `bytes`
static size_t lm_blocks_bytes(size_t nb) { return nb * 32 + nb * 4 + (nb + 1) * 4; }
static size_t lm_blocks_cap(size_t bytes) { return (bytes - 4) / 40; }

// the scratch union and covisible share: a table for `keys` keys, per-block arrays for `blocks` blocks, the mapped result
static int lm_scratch(mslam_hip_ctx* c, size_t keys, size_t blocks, LmTable* t)
{
    RelocState* r = c->reloc;
    *t = lm_table_grow(c, keys);
    if(!t->b)
        return MSLAM_HIP_E_RUNTIME;
    MSLAM_CHK(c, grow(r->d_lm_blocks, lm_blocks_bytes(std::max(blocks, (size_t)256)), c->stream));
    if(!r->h_lm)
        MSLAM_CHK(c, r->h_lm.alloc(sizeof(LmHead) + kRelocMaxCand * 4));
    return MSLAM_HIP_OK;
}

// the launches of both union forms; *dst_slot receives the new entry's slot
static int union_enqueue(mslam_hip_ctx* c, const char* who, int dst_id, const int32_t* ids, int n_ids, int set_flag, int* dst_slot)
{
    int rc = reloc_enter(c);
    if(rc)
        return rc;
    if(!ids || n_ids < 1 || n_ids > kRelocMaxCand)
        return fail(c, MSLAM_HIP_E_INVALID, std::string(who) + ": bad argument (1 to 64 ids)");
    RelocState* r = c->reloc;
    const int K = c->p.max_keypoints;
    hipStream_t s = c->stream;
    LmList list{};
    size_t keys = 0;
    int n_max = 0;
    for(int k = 0; k < n_ids; ++k)
    {
        rc = store_slot(c, who, "id", ids[k], &list.slot[k]);
        if(rc)
            return rc;
        if(ids[k] == dst_id)
            return fail(c, MSLAM_HIP_E_INVALID, std::string(who) + ": dst_id is one of the listed ids");
        int rank = 0;
        for(int j = 0; j < n_ids; ++j)
        {
            if(j != k && ids[j] == ids[k])
                return fail(c, MSLAM_HIP_E_INVALID, std::string(who) + ": id " + std::to_string(ids[k]) + " is listed twice");
            rank += ids[j] < ids[k] ? 1 : 0;
        }
        list.rank[k] = rank;
        keys += (size_t)r->n_upper[(size_t)list.slot[k]];
        n_max = std::max(n_max, r->n_upper[(size_t)list.slot[k]]);
    }
    const unsigned bx = (unsigned)std::max((n_max + 255) / 256, 1);
    const size_t nb = (size_t)bx * (size_t)n_ids;
    LmTable table{};
    rc = lm_scratch(c, keys, nb, &table);
    if(rc)
        return rc;
    // DISTINCTIVE: the observation table, one row of 64 words per union row there can be.  A landmark has at most one
    // observation per listed entry, so with one or two entries every choice is the most recent one: nothing more runs.
    const size_t obs_rows = std::min(keys, (size_t)K);
    const bool distinct = c->union_descriptor == MSLAM_HIP_UNION_DESC_DISTINCTIVE && n_ids > 2 && obs_rows > 0;
    if(distinct)
        MSLAM_CHK(c, grow(r->d_lm_obs, obs_rows * kRelocMaxCand, s));
    // the store grows here, on the host, before anything is enqueued (slots keep their numbers)
    rc = store_slot_for(c, dst_id, dst_slot);
    if(rc)
        return rc;
    (void)store_next_lid_base(c); // a new serial for the entry; its landmarks keep the ids they have
    const size_t slot = (size_t)*dst_slot;
    unsigned long long* win = reinterpret_cast<unsigned long long*>(r->d_lm_blocks.get());
    const size_t cap_blocks = lm_blocks_cap(r->d_lm_blocks.size());
    uint32_t* cnt = reinterpret_cast<uint32_t*>(r->d_lm_blocks + cap_blocks * 32);
    uint32_t* ofs = cnt + cap_blocks;
    const dim3 grid(bx, (unsigned)n_ids);
    {
        StageScope ts(c, "union_clear");
        MSLAM_CHK(c, hipMemsetAsync(table.b, 0xFF, lm_bytes(table), s));
    }
    {
        StageScope ts(c, "union_insert");
        hipLaunchKernelGGL(k_lm_insert, grid, dim3(256), 0, s, r->d_lid, r->d_n, list, K, table, 0);
    }
    {
        StageScope ts(c, "union_select");
        hipLaunchKernelGGL(k_lm_select, grid, dim3(256), 0, s, r->d_lid, r->d_n, list, K, table, win, cnt);
    }
    {
        StageScope ts(c, "union_scan");
        hipLaunchKernelGGL(k_lm_scan, dim3(1), dim3(256), 0, s, cnt, ofs, (int)nb, K, r->d_n + slot, c->d_flags, set_flag,
                           reinterpret_cast<LmHead*>(r->h_lm.dev()));
    }
    {
        StageScope ts(c, "union_scatter");
        hipLaunchKernelGGL(k_lm_scatter, grid, dim3(256), 0, s, r->d_desc, r->d_world, r->d_lid, list, K, win, ofs, (int)nb,
                           r->d_desc + slot * K * 32, r->d_world + slot * K * 3, r->d_lid + slot * K);
    }
    if(distinct)
    {
        uint32_t* obs = r->d_lm_obs.get();
        {
            StageScope ts(c, "union_obs_clear");
            MSLAM_CHK(c, hipMemsetAsync(obs, 0, obs_rows * kRelocMaxCand * sizeof(uint32_t), s));
        }
        {
            StageScope ts(c, "union_place");
            hipLaunchKernelGGL(k_lm_place, grid, dim3(256), 0, s, r->d_lid, list, K, table, win, ofs, (int)nb, (int)obs_rows);
        }
        {
            StageScope ts(c, "union_observe");
            hipLaunchKernelGGL(k_lm_observe, grid, dim3(256), 0, s, r->d_lid, r->d_n, list, K, table, ofs, (int)nb, (int)obs_rows, obs);
        }
        {
            StageScope ts(c, "union_distinct");
            hipLaunchKernelGGL(k_lm_distinct, dim3((unsigned)((obs_rows + 3) / 4)), dim3(256), 0, s, r->d_desc, list, n_ids, K, ofs, (int)nb,
                               (int)obs_rows, obs, r->d_desc + slot * K * 32);
        }
    }
    MSLAM_CHK(c, hipGetLastError());
    r->n_upper[slot] = (int)std::min(keys, (size_t)K); // (the count stays on the device)
    return MSLAM_HIP_OK;
}

extern "C" {

int mslam_hip_set_union_descriptor(mslam_hip_ctx* c, int mode)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    if(mode != MSLAM_HIP_UNION_DESC_RECENT && mode != MSLAM_HIP_UNION_DESC_DISTINCTIVE)
        return fail(c, MSLAM_HIP_E_INVALID, "set_union_descriptor: mode outside 0..1");
    c->union_descriptor = mode;
    return MSLAM_HIP_OK;
}

int mslam_hip_get_union_descriptor(mslam_hip_ctx* c, int* mode)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    if(mode)
        *mode = c->union_descriptor;
    return MSLAM_HIP_OK;
}

int mslam_hip_kf_union_dev(mslam_hip_ctx* c, int dst_id, const int32_t* ids, int n_ids)
{
    int slot = -1;
    return union_enqueue(c, "kf_union_dev", dst_id, ids, n_ids, 1, &slot);
}

int mslam_hip_kf_union(mslam_hip_ctx* c, int dst_id, const int32_t* ids, int n_ids, int* n_out)
{
    if(n_out)
        *n_out = 0;
    int slot = -1;
    const int rc = union_enqueue(c, "kf_union", dst_id, ids, n_ids, 0, &slot);
    if(rc)
        return rc;
    RelocState* r = c->reloc;
    MSLAM_CHK(c, hipStreamSynchronize(c->stream));
    const int32_t needed = reinterpret_cast<const LmHead*>(r->h_lm.get())->needed;
    if(needed < 0)
        return fail(c, MSLAM_HIP_E_RUNTIME, "kf_union: the kernels reported an impossible count");
    if(n_out)
        *n_out = needed;
    if(needed > c->p.max_keypoints)
    {
        r->n_upper[(size_t)slot] = 0;
        return fail(c, MSLAM_HIP_E_CAPACITY, "kf_union: " + std::to_string(needed) + " distinct landmarks, more than the context's max_keypoints");
    }
    r->n_upper[(size_t)slot] = needed;
    return MSLAM_HIP_OK;
}

int mslam_hip_kf_covisible(mslam_hip_ctx* c, int id, const int32_t* ids, int n_ids, int32_t* counts)
{
    int rc = reloc_enter(c);
    if(rc)
        return rc;
    if(n_ids < 0 || n_ids > kRelocMaxCand || (n_ids > 0 && (!ids || !counts)))
        return fail(c, MSLAM_HIP_E_INVALID, "kf_covisible: bad argument (at most 64 ids)");
    RelocState* r = c->reloc;
    const int K = c->p.max_keypoints;
    LmList list{}, self{};
    rc = store_slot(c, "kf_covisible", "id", id, &self.slot[0]);
    for(int k = 0; !rc && k < n_ids; ++k)
        rc = store_slot(c, "kf_covisible", "id", ids[k], &list.slot[k]);
    if(rc || n_ids == 0)
        return rc;
    const int n_own = r->n_upper[(size_t)self.slot[0]];
    LmTable table{};
    rc = lm_scratch(c, (size_t)n_own, 1, &table);
    if(rc)
        return rc;
    hipStream_t s = c->stream;
    int32_t* h_counts = reinterpret_cast<int32_t*>(r->h_lm + sizeof(LmHead));
    for(int k = 0; k < n_ids; ++k)
        h_counts[k] = -1; // (overwritten by k_lm_covisible; checked after the synchronisation)
    {
        StageScope ts(c, "covisible_clear");
        MSLAM_CHK(c, hipMemsetAsync(table.b, 0xFF, lm_bytes(table), s));
    }
    {
        StageScope ts(c, "covisible_insert");
        hipLaunchKernelGGL(k_lm_insert, dim3((unsigned)std::max((n_own + 255) / 256, 1), 1), dim3(256), 0, s, r->d_lid, r->d_n, self, K, table,
                           1);
    }
    {
        StageScope ts(c, "covisible_count");
        hipLaunchKernelGGL(k_lm_covisible, dim3((unsigned)n_ids), dim3(256), 0, s, r->d_lid, r->d_n, list, K, table,
                           reinterpret_cast<int32_t*>(r->h_lm.dev() + sizeof(LmHead)));
    }
    MSLAM_CHK(c, hipGetLastError());
    MSLAM_CHK(c, hipStreamSynchronize(s));
    for(int k = 0; k < n_ids; ++k)
        if(h_counts[k] < 0 || h_counts[k] > K)
            return fail(c, MSLAM_HIP_E_RUNTIME, "kf_covisible: the kernel left no result");
    std::memcpy(counts, h_counts, (size_t)n_ids * 4);
    return MSLAM_HIP_OK;
}

int mslam_hip_kf_update_world(mslam_hip_ctx* c, const int64_t* landmark_ids, const double* world_xyz, int n, int* n_written)
{
    if(n_written)
        *n_written = 0;
    int rc = reloc_enter(c);
    if(rc)
        return rc;
    if(n < 0 || n > (1 << 24) || (n > 0 && (!landmark_ids || !world_xyz)))
        return fail(c, MSLAM_HIP_E_INVALID, "kf_update_world: bad argument");
    return rewrite_host_list(c, landmark_ids, nullptr, world_xyz, n, "update_world_insert", "update_world_write", n_written);
}

} // extern "C"
