// k_lmcull.hip — landmark culling on the keyframe store: mslam_hip_kf_cull_landmarks_search (the landmarks of the candidate
// entries that fewer than min_observers listed entries hold), mslam_hip_kf_remove_landmarks (the listed landmark ids leave
// every listed entry) and mslam_hip_kf_cull_landmarks (the search, then the removal, with one synchronisation).  The
// semantics are stated at the declarations in include/mslam_hip.h.
//
// AN EXTENSION: the reference has the removal primitive (BasicMap::removeLandmark, basic_map.cpp:133) and no step that
// calls it.  The model is ORB-SLAM's MapPointCulling, of which this is the observer threshold alone (the store keeps no
// found / visible counters).
//
// The search starts with the observer count per landmark id exactly as keyframe culling does (cull_count_enqueue,
// k_cull.hip: the table of lm_table.hpp and a u32 count per bucket).  Then
//   k_lmcull_judge    the grid of k_cull_mark over the candidate entries: a thread finds the bucket of its landmark id and
//                     writes 0 into the bucket's stamp (all-ones after the clear).  Every writer writes the same value, so
//                     neither the order nor the number of writers matters;
//   k_lmcull_gather   one thread per bucket: a bucket that is judged and whose count is below min_observers takes a place
//                     from ONE device counter (one atomicAdd per wave, the lanes' places from the ballot) and, when the
//                     place is below the capacity, writes (id, count) there, into the mapped result block.  THE DEVICE
//                     ORDER IS ARBITRARY: which place a bucket gets depends on the order of the atomics.  The host sorts
//                     the rows by landmark id after the synchronisation (ids are distinct: one bucket each), and that
//                     sort is what makes the bytes of the list a function of the store and the arguments alone.  The
//                     count itself is an integer sum and does not depend on the order;
//   k_lmcull_compact  (fused call) one workgroup per listed entry, compact_entry of compact.hpp (k_prune_compact's chunked
//                     in-place scan) with the drop test "the id's bucket is judged and its count is below min_observers".
//                     The kernel reads the gather's counter first and leaves every entry alone when the count exceeds the
//                     caller's capacity: the decision is taken on the device, as mslam_hip_kf_fuse takes it.  Counts and
//                     stamps are read-only here, so removing a landmark changes no other landmark's verdict.
// The removal of an explicit list builds its table from the list instead:
//   k_lmcull_table    one thread per listed id claims the id's bucket (a repeat claims it once);
//   k_lmcull_compact_list  the same compaction with the drop test "the table holds the id"; a hit is an integer atomicAdd
//                     on the bucket's hit count;
//   k_lmcull_rows     one thread per listed id: the hit count of its bucket, into the mapped result block.
// Every workgroup of a compaction writes its entry's new count and the number it lost into the mapped result block.
#include "compact.hpp"
#include "lm_table.hpp"
#include "reloc.hpp"

#include <algorithm>
#include <climits>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

namespace mslam
{

constexpr uint32_t kLmCullJudged = 0u; // a bucket's stamp once a candidate entry holds its id (all-ones before)

struct LmCullEntry // one listed entry's record in the mapped result block
{
    int32_t new_n, lost;
};

// grid = (blocks of 256 positions, candidate entries).  A candidate is a listed entry: its ids are in the table.
__global__ __launch_bounds__(256) void k_lmcull_judge(const int64_t* __restrict__ store_lid, const int32_t* __restrict__ store_n,
                                                      const int32_t* __restrict__ cand_slots, int K, LmTable t,
                                                      uint32_t* __restrict__ stamp)
{
    const int slot = cand_slots[blockIdx.y], i = blockIdx.x * 256 + threadIdx.x;
    if(i >= entry_count(store_n, slot, K))
        return;
    const long long b = lm_find(t, (unsigned long long)store_lid[(size_t)slot * K + i]);
    if(b >= 0)
        stamp[b] = kLmCullJudged;
}

__device__ __forceinline__ bool lmcull_culled(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ stamp, long long b,
                                              uint32_t min_observers)
{
    return b >= 0 && stamp[b] == kLmCullJudged && counts[b] < min_observers;
}

// one thread per bucket; out_lid / out_obs hold `cap` rows (mapped); *counter is zero beforehand
__global__ __launch_bounds__(256) void k_lmcull_gather(LmTable t, const uint32_t* __restrict__ counts, const uint32_t* __restrict__ stamp,
                                                       uint32_t min_observers, uint32_t cap, uint32_t* __restrict__ counter,
                                                       int64_t* __restrict__ out_lid, int32_t* __restrict__ out_obs)
{
    const size_t b = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    unsigned long long key = kLmEmpty;
    bool hit = false;
    if(b <= t.mask)
    {
        key = t.b[b].key;
        hit = key != kLmEmpty && lmcull_culled(counts, stamp, (long long)b, min_observers);
    }
    const unsigned long long bal = __ballot(hit);
    if(bal == 0) // (wave-uniform)
        return;
    const int leader = __ffsll((long long)bal) - 1;
    uint32_t base = 0;
    if(lane == leader)
        base = atomicAdd(counter, (uint32_t)__popcll(bal));
    base = __shfl(base, leader);
    const uint32_t place = base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    if(hit && place < cap)
    {
        out_lid[place] = (int64_t)key;
        out_obs[place] = (int32_t)counts[b];
    }
}

// grid = listed entries.  *counter: what k_lmcull_gather found; more than cap_limit: nothing is removed.
__global__ __launch_bounds__(kCompactChunk) void k_lmcull_compact(uint8_t* store_desc, double* store_world, int64_t* store_lid,
                                                                  int32_t* store_n, int K, const int32_t* __restrict__ slots, LmTable t,
                                                                  const uint32_t* __restrict__ counts, const uint32_t* __restrict__ stamp,
                                                                  uint32_t min_observers, const uint32_t* __restrict__ counter,
                                                                  uint32_t cap_limit, LmCullEntry* __restrict__ res)
{
    const int slot = slots[blockIdx.x];
    const int n = entry_count(store_n, slot, K);
    int kept = n;
    if(*counter <= cap_limit) // (the same word in every thread: the branch is uniform over the workgroup)
    {
        kept = compact_entry(store_desc, store_world, store_lid, (size_t)slot * K, n, [&](int64_t lid) {
            return lmcull_culled(counts, stamp, lm_find(t, (unsigned long long)lid), min_observers);
        });
        if(threadIdx.x == 0)
            store_n[slot] = kept;
    }
    if(threadIdx.x == 0)
        res[blockIdx.x] = LmCullEntry{kept, n - kept};
}

__global__ __launch_bounds__(256) void k_lmcull_table(const int64_t* __restrict__ ids, int n, LmTable t)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if(p < n)
        (void)lm_claim(t, (unsigned long long)ids[p]);
}

// grid = listed entries.  hits: one u32 per bucket, zero beforehand.
__global__ __launch_bounds__(kCompactChunk) void k_lmcull_compact_list(uint8_t* store_desc, double* store_world, int64_t* store_lid,
                                                                       int32_t* store_n, int K, const int32_t* __restrict__ slots,
                                                                       LmTable t, uint32_t* __restrict__ hits,
                                                                       LmCullEntry* __restrict__ res)
{
    const int slot = slots[blockIdx.x];
    const int n = entry_count(store_n, slot, K);
    const int kept = compact_entry(store_desc, store_world, store_lid, (size_t)slot * K, n, [&](int64_t lid) {
        const long long b = lm_find(t, (unsigned long long)lid);
        if(b >= 0)
            atomicAdd(&hits[b], 1u);
        return b >= 0;
    });
    if(threadIdx.x == 0)
    {
        store_n[slot] = kept;
        res[blockIdx.x] = LmCullEntry{kept, n - kept};
    }
}

__global__ __launch_bounds__(256) void k_lmcull_rows(const int64_t* __restrict__ ids, int n, LmTable t, const uint32_t* __restrict__ hits,
                                                     int32_t* __restrict__ out)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if(p >= n)
        return;
    const long long b = lm_find(t, (unsigned long long)ids[p]);
    out[p] = b >= 0 ? (int32_t)hits[b] : 0;
}

} // namespace mslam

using namespace mslam;

namespace
{
// after the synchronisation of a call that compacted: every listed entry's record -> the host's sizes (now exact),
// entry_removed and the total
int lmcull_collect(mslam_hip_ctx* c, const std::string& me, const CullMap& m, const LmCullEntry* res, int32_t* entry_removed, int* n_removed)
{
    RelocState* r = c->reloc;
    for(size_t k = 0; k < m.slots.size(); ++k)
        if(res[k].new_n < 0 || res[k].new_n > c->p.max_keypoints || res[k].lost < 0 || res[k].lost > c->p.max_keypoints)
            return fail(c, MSLAM_HIP_E_RUNTIME, me + ": the kernel left no result");
    long long total = 0;
    for(size_t k = 0; k < m.slots.size(); ++k)
    {
        r->n_upper[(size_t)m.slots[k]] = res[k].new_n;
        if(entry_removed)
            entry_removed[k] = res[k].lost;
        total += res[k].lost;
    }
    if(n_removed)
        *n_removed = (int)total;
    return MSLAM_HIP_OK;
}

int lmcull_run(mslam_hip_ctx* c, const char* who, bool remove, const int32_t* ids, int n_ids, const int32_t* cand, int n_cand,
               int min_observers, int64_t* landmark_ids, int32_t* observers, int capacity, int* n_found, int32_t* entry_removed,
               int* n_removed)
{
    if(n_found)
        *n_found = 0;
    if(n_removed)
        *n_removed = 0;
    if(entry_removed && n_ids > 0 && n_ids <= MSLAM_HIP_CULL_MAX_ENTRIES)
        std::memset(entry_removed, 0, (size_t)n_ids * 4);
    if(landmark_ids && capacity > 0)
    {
        std::memset(landmark_ids, 0, (size_t)capacity * 8);
        if(observers)
            std::memset(observers, 0, (size_t)capacity * 4);
    }
    int rc = reloc_enter(c);
    if(rc)
        return rc;
    const std::string me = who;
    CullMap m;
    std::unordered_map<int, int> pos_of;
    rc = cull_resolve(c, me, ids, n_ids, &m, &pos_of);
    if(rc)
        return rc;
    if(n_cand < 0 || n_cand > n_ids || (n_cand > 0 && !cand) || !n_found || (landmark_ids && capacity < 0))
        return fail(c, MSLAM_HIP_E_INVALID, me + ": bad argument (0 to n_ids candidates, n_found, a capacity >= 0)");
    if(min_observers < 1 || min_observers > 65535)
        return fail(c, MSLAM_HIP_E_INVALID, me + ": min_observers in 1..65535");
    RelocState* r = c->reloc;
    std::vector<int32_t> cand_slots;
    rc = cull_cand_slots(c, me, m, pos_of, cand, n_cand, &cand_slots);
    if(rc)
        return rc;
    if(n_cand == 0)
        return MSLAM_HIP_OK;
    // no more landmarks can be found than the candidates hold positions
    size_t bound = 0;
    int cand_max = 0;
    for(const int32_t slot : cand_slots)
    {
        bound += (size_t)r->n_upper[(size_t)slot];
        cand_max = std::max(cand_max, r->n_upper[(size_t)slot]);
    }
    const size_t cap_dev = landmark_ids ? std::min((size_t)capacity, bound) : 0;
    const uint32_t cap_limit = landmark_ids ? (uint32_t)capacity : (uint32_t)INT_MAX;
    // one upload: [listed slots | candidate slots | the counter, zero]; the mapped result:
    // [the count, pad x 3 | LmCullEntry x n_ids | ids cap_dev x i64 | counts cap_dev x i32]
    const size_t o_cand = (size_t)n_ids * 4, o_cnt = o_cand + (size_t)n_cand * 4, up = o_cnt + 4;
    const size_t h_ent = 16, h_lid = h_ent + (size_t)n_ids * sizeof(LmCullEntry), h_obs = h_lid + cap_dev * 8, res_bytes = h_obs + cap_dev * 4;
    rc = reloc_scratch(c, up, 0, res_bytes);
    if(rc)
        return rc;
    CullDev d{};
    rc = cull_scratch(c, m.keys, &d);
    if(rc)
        return rc;
    uint8_t *h = r->h_up, *du = r->d_up, *H = r->h_res.get(), *HD = r->h_res.dev();
    std::memcpy(h, m.slots.data(), o_cand);
    std::memcpy(h + o_cand, cand_slots.data(), (size_t)n_cand * 4);
    std::memset(h + o_cnt, 0, 4);
    std::memset(H, 0xFF, h_lid);
    hipStream_t s = c->stream;
    {
        StageScope ts(c, "lmcull_upload");
        MSLAM_CHK(c, hipMemcpyAsync(du, h, up, hipMemcpyHostToDevice, s));
    }
    const int32_t* d_slots = reinterpret_cast<const int32_t*>(du);
    uint32_t* d_counter = reinterpret_cast<uint32_t*>(du + o_cnt);
    rc = cull_count_enqueue(c, m, d_slots, d);
    if(rc)
        return rc;
    {
        StageScope ts(c, "lmcull_judge");
        const dim3 grid((unsigned)std::max((cand_max + 255) / 256, 1), (unsigned)n_cand);
        hipLaunchKernelGGL(k_lmcull_judge, grid, dim3(256), 0, s, r->d_lid.get(), r->d_n.get(), reinterpret_cast<const int32_t*>(du + o_cand),
                           c->p.max_keypoints, d.table, d.stamp);
    }
    {
        StageScope ts(c, "lmcull_gather");
        hipLaunchKernelGGL(k_lmcull_gather, dim3((unsigned)((d.buckets + 255) / 256)), dim3(256), 0, s, d.table, d.counts, d.stamp,
                           (uint32_t)min_observers, (uint32_t)cap_dev, d_counter, reinterpret_cast<int64_t*>(HD + h_lid),
                           reinterpret_cast<int32_t*>(HD + h_obs));
    }
    if(remove)
    {
        StageScope ts(c, "lmcull_compact");
        hipLaunchKernelGGL(k_lmcull_compact, dim3((unsigned)n_ids), dim3(kCompactChunk), 0, s, r->d_desc.get(), r->d_world.get(),
                           r->d_lid.get(), r->d_n.get(), c->p.max_keypoints, d_slots, d.table, d.counts, d.stamp, (uint32_t)min_observers,
                           d_counter, cap_limit, reinterpret_cast<LmCullEntry*>(HD + h_ent));
    }
    MSLAM_CHK(c, hipGetLastError());
    MSLAM_CHK(c, hipMemcpyAsync(H, d_counter, 4, hipMemcpyDeviceToHost, s));
    MSLAM_CHK(c, hipStreamSynchronize(s));
    const uint32_t found = *reinterpret_cast<const uint32_t*>(H);
    if((size_t)found > bound)
        return fail(c, MSLAM_HIP_E_RUNTIME, me + ": the kernels left no result");
    *n_found = (int)found;
    if(landmark_ids && found > (uint32_t)capacity)
        return fail(c, MSLAM_HIP_E_CAPACITY, me + ": " + std::to_string(found) + " landmarks, more than `capacity`");
    if(remove)
    {
        rc = lmcull_collect(c, me, m, reinterpret_cast<const LmCullEntry*>(H + h_ent), entry_removed, n_removed);
        if(rc)
            return rc;
    }
    if(landmark_ids)
    {
        // the device order is arbitrary: ascending ids (distinct) make the list deterministic
        const int64_t* lid = reinterpret_cast<const int64_t*>(H + h_lid);
        const int32_t* obs = reinterpret_cast<const int32_t*>(H + h_obs);
        std::vector<uint32_t> order(found);
        std::iota(order.begin(), order.end(), 0u);
        std::sort(order.begin(), order.end(), [lid](uint32_t a, uint32_t b) { return lid[a] < lid[b]; });
        for(uint32_t p = 0; p < found; ++p)
        {
            landmark_ids[p] = lid[order[p]];
            if(observers)
                observers[p] = obs[order[p]];
        }
    }
    return MSLAM_HIP_OK;
}
} // namespace

extern "C" {

int mslam_hip_kf_remove_landmarks(mslam_hip_ctx* c, const int32_t* ids, int n_ids, const int64_t* landmark_ids, int n, int32_t* removed,
                                  int32_t* entry_removed, int* n_removed)
{
    if(n_removed)
        *n_removed = 0;
    if(removed && n > 0 && n <= (1 << 24))
        std::memset(removed, 0, (size_t)n * 4);
    if(entry_removed && n_ids > 0 && n_ids <= MSLAM_HIP_CULL_MAX_ENTRIES)
        std::memset(entry_removed, 0, (size_t)n_ids * 4);
    int rc = reloc_enter(c);
    if(rc)
        return rc;
    const std::string me = "kf_remove_landmarks";
    CullMap m;
    std::unordered_map<int, int> pos_of;
    rc = cull_resolve(c, me, ids, n_ids, &m, &pos_of);
    if(rc)
        return rc;
    rc = lid_list_check(c, me, n, landmark_ids != nullptr, landmark_ids);
    if(rc)
        return rc;
    RelocState* r = c->reloc;
    // one upload: [listed landmark ids n x i64 | listed slots]; the mapped result: [LmCullEntry x n_ids | removed n x i32]
    const size_t o_slots = (size_t)n * 8, up = o_slots + (size_t)n_ids * 4;
    const size_t h_rows = (size_t)n_ids * sizeof(LmCullEntry), res_bytes = h_rows + (size_t)n * 4;
    rc = reloc_scratch(c, up, 0, res_bytes);
    if(rc)
        return rc;
    CullDev d{};
    rc = cull_scratch(c, (size_t)std::max(n, 1), &d); // (the counts are the buckets' hit counts here; the stamps are not used)
    if(rc)
        return rc;
    uint8_t *h = r->h_up, *du = r->d_up, *H = r->h_res.get(), *HD = r->h_res.dev();
    if(n > 0)
        std::memcpy(h, landmark_ids, (size_t)n * 8);
    std::memcpy(h + o_slots, m.slots.data(), (size_t)n_ids * 4);
    std::memset(H, 0xFF, h_rows);
    hipStream_t s = c->stream;
    {
        StageScope ts(c, "lmcull_upload");
        MSLAM_CHK(c, hipMemcpyAsync(du, h, up, hipMemcpyHostToDevice, s));
    }
    {
        StageScope ts(c, "lmcull_clear");
        MSLAM_CHK(c, hipMemsetAsync(d.table.b, 0xFF, lm_bytes(d.table), s));
        MSLAM_CHK(c, hipMemsetAsync(d.counts, 0, d.buckets * 4, s));
    }
    const int64_t* d_ids = reinterpret_cast<const int64_t*>(du);
    if(n > 0)
    {
        StageScope ts(c, "lmcull_table");
        hipLaunchKernelGGL(k_lmcull_table, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_ids, n, d.table);
    }
    {
        StageScope ts(c, "lmcull_compact");
        hipLaunchKernelGGL(k_lmcull_compact_list, dim3((unsigned)n_ids), dim3(kCompactChunk), 0, s, r->d_desc.get(), r->d_world.get(),
                           r->d_lid.get(), r->d_n.get(), c->p.max_keypoints, reinterpret_cast<const int32_t*>(du + o_slots), d.table,
                           d.counts, reinterpret_cast<LmCullEntry*>(HD));
    }
    if(n > 0)
    {
        StageScope ts(c, "lmcull_rows");
        hipLaunchKernelGGL(k_lmcull_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_ids, n, d.table, d.counts,
                           reinterpret_cast<int32_t*>(HD + h_rows));
    }
    MSLAM_CHK(c, hipGetLastError());
    MSLAM_CHK(c, hipStreamSynchronize(s));
    rc = lmcull_collect(c, me, m, reinterpret_cast<const LmCullEntry*>(H), entry_removed, n_removed);
    if(rc)
        return rc;
    if(removed && n > 0)
        std::memcpy(removed, H + h_rows, (size_t)n * 4);
    return MSLAM_HIP_OK;
}

int mslam_hip_kf_cull_landmarks_search(mslam_hip_ctx* c, const int32_t* ids, int n_ids, const int32_t* cand, int n_cand, int min_observers,
                                       int64_t* landmark_ids, int32_t* observers, int capacity, int* n_found)
{
    return lmcull_run(c, "kf_cull_landmarks_search", false, ids, n_ids, cand, n_cand, min_observers, landmark_ids, observers, capacity,
                      n_found, nullptr, nullptr);
}

int mslam_hip_kf_cull_landmarks(mslam_hip_ctx* c, const int32_t* ids, int n_ids, const int32_t* cand, int n_cand, int min_observers,
                                int64_t* landmark_ids, int32_t* observers, int capacity, int* n_found, int32_t* entry_removed,
                                int* n_removed)
{
    return lmcull_run(c, "kf_cull_landmarks", true, ids, n_ids, cand, n_cand, min_observers, landmark_ids, observers, capacity, n_found,
                      entry_removed, n_removed);
}

} // extern "C"
