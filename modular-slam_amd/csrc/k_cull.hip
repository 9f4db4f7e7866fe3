// k_cull.hip — keyframe culling on the keyframe store: mslam_hip_kf_observers (how many of the listed entries hold a landmark
// id), mslam_hip_kf_cull_search (the greedy pass over a candidate list) and mslam_hip_kf_cull (the search, then the culled
// entries leave the store).  The semantics are stated at the declarations in include/mslam_hip.h.
//
// AN EXTENSION: the reference has the removal primitives (BasicMap::removeKeyframe, basic_map.cpp:110-115;
// IRelocalizer::removeKeyframe, relocalizer.hpp:19) and no policy that calls them.  The model is ORB-SLAM's KeyFrameCulling.
//
// All three start with the observer count per landmark id, on the table of lm_table.hpp ({key, val} buckets cleared to
// all-ones) and a u32 count per bucket:
//   k_cull_mark    the listed entries in chunks of 64, the grid of k_lm_insert (blockIdx.y = position in the chunk): a thread
//                  claims the bucket of its landmark id and CLEARS bit k of the value, so a repeat inside an entry clears
//                  one bit once and the cleared table needs no second pass to become "no bit set";
//   k_cull_count   one thread per bucket: the count grows by the popcount of the cleared bits and the value goes back to
//                  all-ones for the next chunk.  Integer sums of a fixed set of bits: the order does not matter.
// (cull_resolve, cull_cand_slots, cull_scratch and cull_count_enqueue are declared in reloc.hpp: landmark culling,
// k_lmcull.hip, starts with the same counts.)  Then
//   k_cull_lookup  (observers) one thread per asked id: the count of its bucket, 0 without one;
//   k_cull_greedy  (search) ONE workgroup of 1024 threads walks the candidates in order.  Per candidate, three phases with a
//                  workgroup barrier between them: (A) every position finds its bucket and lowers the bucket's stamp to
//                  its position with atomicMin — the first position of an id inside the entry wins; (B) the winners read
//                  the count, a ballot per wave and one LDS sum give n_landmarks and n_redundant, and every thread
//                  evaluates the one comparison; (C) the winners put the stamp back to all-ones and, when the candidate
//                  goes, lower the count by one.  Stamps and counts are read and written with device-scope atomics only,
//                  so every access is performed at the L2 and no line of the CU's vector cache is relied on; the barriers
//                  (with __threadfence_block) order the phases.  One workgroup: no grid-wide synchronisation.  Thread 0
//                  writes the candidate's record into the mapped result block.
#include "lm_table.hpp"
#include "reloc.hpp"

#include <cstring>
#include <string>
#include <vector>

namespace mslam
{

constexpr int kCullChunk = 64;      // listed entries per mark launch: one bit of the bucket's value each
constexpr int kCullThreads = 1024;  // k_cull_greedy's workgroup = its stride over an entry (tests/cull_ref.py: STRIDE)
constexpr uint32_t kCullNoStamp = 0xFFFFFFFFu;

struct CullRes // one candidate's record in the mapped result block
{
    int32_t n_landmarks, n_redundant, culled, pad;
};

// grid = (blocks of 256 positions, entries of the chunk).  slots = the chunk's part of the uploaded slot list.
__global__ __launch_bounds__(256) void k_cull_mark(const int64_t* __restrict__ store_lid, const int32_t* __restrict__ store_n,
                                                   const int32_t* __restrict__ slots, int K, LmTable t)
{
    const int k = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int slot = slots[k];
    if(i >= entry_count(store_n, slot, K))
        return;
    const long long b = lm_claim(t, (unsigned long long)store_lid[(size_t)slot * K + i]);
    if(b >= 0)
        atomicAnd(&t.b[b].val, ~(1ull << k));
}

// one thread per bucket
__global__ __launch_bounds__(256) void k_cull_count(LmTable t, uint32_t* __restrict__ counts)
{
    const size_t b = (size_t)blockIdx.x * 256 + threadIdx.x;
    if(b > t.mask)
        return;
    const unsigned long long v = t.b[b].val;
    if(v != kLmEmpty)
    {
        counts[b] += (uint32_t)__popcll(~v);
        t.b[b].val = kLmEmpty;
    }
}

__global__ __launch_bounds__(256) void k_cull_lookup(const int64_t* __restrict__ ids, int n, LmTable t, const uint32_t* __restrict__ counts,
                                                     int32_t* __restrict__ out)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if(p >= n)
        return;
    const long long b = lm_find(t, (unsigned long long)ids[p]);
    out[p] = b >= 0 ? (int32_t)counts[b] : 0;
}

__device__ __forceinline__ uint32_t cull_load(const uint32_t* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One workgroup.  bkt[K]: the bucket of every position of the candidate at its turn (a thread reads only what it wrote).
// An entry holds at most 65535 landmarks, so a thread has at most 64 positions and one 64-bit word names its winners.
__global__ __launch_bounds__(kCullThreads) void k_cull_greedy(const int64_t* __restrict__ store_lid, const int32_t* __restrict__ store_n,
                                                              const int32_t* __restrict__ cand_slots, int n_cand, int K, LmTable t,
                                                              uint32_t* counts, uint32_t* stamp, uint32_t* __restrict__ bkt,
                                                              int min_observers, double ratio, int min_landmarks,
                                                              CullRes* __restrict__ res, int32_t* __restrict__ done)
{
    constexpr int kWaves = kCullThreads / 64;
    __shared__ int s_l[kWaves], s_r[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for(int c = 0; c < n_cand; ++c)
    {
        const int slot = cand_slots[c];
        const int n = min(entry_count(store_n, slot, K), 65535);
        const int64_t* lid = store_lid + (size_t)slot * K;
        // (A) the first position of every id
        for(int base = 0; base < n; base += kCullThreads)
        {
            const int i = base + tid;
            if(i < n)
            {
                const long long b = lm_find(t, (unsigned long long)lid[i]);
                bkt[i] = b >= 0 ? (uint32_t)b : kCullNoStamp; // (a candidate is a listed entry: its ids are in the table)
                if(b >= 0)
                    atomicMin(&stamp[b], (uint32_t)i);
            }
        }
        __threadfence_block();
        __syncthreads();
        // (B) the winners count themselves and the redundant among them
        unsigned long long won = 0;
        int n_l = 0, n_r = 0; // (wave-uniform)
        for(int base = 0, round = 0; base < n; base += kCullThreads, ++round)
        {
            const int i = base + tid;
            bool w = false, red = false;
            if(i < n)
            {
                const uint32_t b = bkt[i];
                if(b != kCullNoStamp && cull_load(&stamp[b]) == (uint32_t)i)
                {
                    w = true;
                    red = (long long)cull_load(&counts[b]) - 1 >= (long long)min_observers;
                }
            }
            if(w)
                won |= 1ull << round;
            n_l += (int)__popcll(__ballot(w));
            n_r += (int)__popcll(__ballot(red));
        }
        if(lane == 0)
            s_l[wave] = n_l, s_r[wave] = n_r;
        __threadfence_block();
        __syncthreads();
        int tot_l = 0, tot_r = 0;
        for(int w = 0; w < kWaves; ++w)
            tot_l += s_l[w], tot_r += s_r[w];
        const bool cull = tot_l >= min_landmarks && (double)tot_r > ratio * (double)tot_l;
        if(tid == 0)
            res[c] = CullRes{tot_l, tot_r, cull ? 1 : 0, 0};
        // (C) the stamps go back; a culled candidate observes nothing any more
        for(int base = 0, round = 0; base < n; base += kCullThreads, ++round)
        {
            if((won >> round) & 1ull)
            {
                const uint32_t b = bkt[base + tid];
                if(cull)
                    atomicSub(&counts[b], 1u);
                atomicExch(&stamp[b], kCullNoStamp);
            }
        }
        __threadfence_block();
        __syncthreads(); // (also: s_l / s_r are free again)
    }
    if(tid == 0)
        *done = n_cand;
}

} // namespace mslam

using namespace mslam;

// ---- the observer counts (declared in reloc.hpp: k_lmcull.hip starts with them too)
int mslam::cull_resolve(mslam_hip_ctx* c, const std::string& me, const int32_t* ids, int n_ids, CullMap* m, std::unordered_map<int, int>* pos_of)
{
    RelocState* r = c->reloc;
    if(!ids || n_ids < 1 || n_ids > MSLAM_HIP_CULL_MAX_ENTRIES)
        return fail(c, MSLAM_HIP_E_INVALID, me + ": bad argument (1 to " + std::to_string(MSLAM_HIP_CULL_MAX_ENTRIES) + " listed ids)");
    m->slots.resize((size_t)n_ids);
    pos_of->reserve((size_t)n_ids);
    for(int k = 0; k < n_ids; ++k)
    {
        const int rc = store_slot(c, me, "id", ids[k], &m->slots[(size_t)k]);
        if(rc)
            return rc;
        if(!pos_of->emplace(ids[k], k).second)
            return fail(c, MSLAM_HIP_E_INVALID, me + ": id " + std::to_string(ids[k]) + " is listed twice");
        m->keys += (size_t)r->n_upper[(size_t)m->slots[(size_t)k]];
    }
    if(m->keys > (size_t)MSLAM_HIP_CULL_MAX_LANDMARKS)
        return fail(c, MSLAM_HIP_E_CAPACITY, me + ": the listed entries hold up to " + std::to_string(m->keys) + " landmarks, more than " +
                                                 std::to_string(MSLAM_HIP_CULL_MAX_LANDMARKS));
    return MSLAM_HIP_OK;
}

int mslam::cull_cand_slots(mslam_hip_ctx* c, const std::string& me, const CullMap& m, const std::unordered_map<int, int>& pos_of,
                           const int32_t* cand, int n_cand, std::vector<int32_t>* cand_slots)
{
    cand_slots->resize((size_t)n_cand);
    std::vector<uint8_t> seen(m.slots.size(), 0);
    for(int k = 0; k < n_cand; ++k)
    {
        const auto it = pos_of.find(cand[k]);
        if(it == pos_of.end())
            return fail(c, MSLAM_HIP_E_INVALID, me + ": candidate " + std::to_string(cand[k]) + " is not one of the listed ids");
        if(seen[(size_t)it->second])
            return fail(c, MSLAM_HIP_E_INVALID, me + ": candidate " + std::to_string(cand[k]) + " is listed twice");
        seen[(size_t)it->second] = 1;
        (*cand_slots)[(size_t)k] = m.slots[(size_t)it->second];
    }
    return MSLAM_HIP_OK;
}

int mslam::cull_scratch(mslam_hip_ctx* c, size_t keys, CullDev* d)
{
    RelocState* r = c->reloc;
    d->table = lm_table_grow(c, keys);
    if(!d->table.b)
        return MSLAM_HIP_E_RUNTIME;
    d->buckets = (size_t)d->table.mask + 1;
    MSLAM_CHK(c, grow(r->d_cull, (2 * d->buckets + (size_t)c->p.max_keypoints) * 4, c->stream));
    d->counts = reinterpret_cast<uint32_t*>(r->d_cull.get());
    d->stamp = d->counts + d->buckets;
    d->bkt = d->stamp + d->buckets;
    return MSLAM_HIP_OK;
}

int mslam::cull_count_enqueue(mslam_hip_ctx* c, const CullMap& m, const int32_t* d_slots, const CullDev& d)
{
    RelocState* r = c->reloc;
    hipStream_t s = c->stream;
    const int K = c->p.max_keypoints;
    {
        StageScope ts(c, "cull_clear");
        MSLAM_CHK(c, hipMemsetAsync(d.table.b, 0xFF, lm_bytes(d.table), s));
        MSLAM_CHK(c, hipMemsetAsync(d.counts, 0, d.buckets * 4, s));
        MSLAM_CHK(c, hipMemsetAsync(d.stamp, 0xFF, d.buckets * 4, s));
    }
    StageScope ts(c, "cull_count");
    for(size_t base = 0; base < m.slots.size(); base += kCullChunk)
    {
        const size_t len = std::min(m.slots.size() - base, (size_t)kCullChunk);
        int n_max = 0;
        for(size_t k = 0; k < len; ++k)
            n_max = std::max(n_max, r->n_upper[(size_t)m.slots[base + k]]);
        const dim3 grid((unsigned)std::max((n_max + 255) / 256, 1), (unsigned)len);
        hipLaunchKernelGGL(k_cull_mark, grid, dim3(256), 0, s, r->d_lid.get(), r->d_n.get(), d_slots + base, K, d.table);
        hipLaunchKernelGGL(k_cull_count, dim3((unsigned)((d.buckets + 255) / 256)), dim3(256), 0, s, d.table, d.counts);
    }
    MSLAM_CHK(c, hipGetLastError());
    return MSLAM_HIP_OK;
}

namespace
{
int cull_run(mslam_hip_ctx* c, const char* who, bool remove, const int32_t* ids, int n_ids, const int32_t* cand, int n_cand,
             int min_observers, double ratio, int min_landmarks, uint8_t* culled, int32_t* n_landmarks, int32_t* n_redundant,
             int* n_culled)
{
    if(n_culled)
        *n_culled = 0;
    if(n_cand > 0 && n_cand <= MSLAM_HIP_CULL_MAX_ENTRIES)
    {
        if(culled)
            std::memset(culled, 0, (size_t)n_cand);
        if(n_landmarks)
            std::memset(n_landmarks, 0, (size_t)n_cand * 4);
        if(n_redundant)
            std::memset(n_redundant, 0, (size_t)n_cand * 4);
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
    if(n_cand < 0 || n_cand > n_ids || (n_cand > 0 && (!cand || !culled)))
        return fail(c, MSLAM_HIP_E_INVALID, me + ": bad argument (0 to n_ids candidates, a `culled` array)");
    if(min_observers < 1 || min_observers > 65535 || !(ratio >= 0.0 && ratio <= 1.0) || min_landmarks < 1)
        return fail(c, MSLAM_HIP_E_INVALID, me + ": min_observers in 1..65535, ratio in [0, 1], min_landmarks >= 1");
    RelocState* r = c->reloc;
    std::vector<int32_t> cand_slots;
    rc = cull_cand_slots(c, me, m, pos_of, cand, n_cand, &cand_slots);
    if(rc)
        return rc;
    if(n_cand == 0)
        return MSLAM_HIP_OK;
    // one upload: [listed slots | candidate slots]; the mapped result: [done, pad x 3 | CullRes x n_cand]
    const size_t o_cand = (size_t)n_ids * 4, up = o_cand + (size_t)n_cand * 4, res_bytes = 16 + (size_t)n_cand * sizeof(CullRes);
    rc = reloc_scratch(c, up, 0, res_bytes);
    if(rc)
        return rc;
    CullDev d{};
    rc = cull_scratch(c, m.keys, &d);
    if(rc)
        return rc;
    uint8_t *h = r->h_up, *du = r->d_up;
    std::memcpy(h, m.slots.data(), o_cand);
    std::memcpy(h + o_cand, cand_slots.data(), (size_t)n_cand * 4);
    std::memset(r->h_res.get(), 0xFF, res_bytes);
    hipStream_t s = c->stream;
    {
        StageScope ts(c, "cull_upload");
        MSLAM_CHK(c, hipMemcpyAsync(du, h, up, hipMemcpyHostToDevice, s));
    }
    rc = cull_count_enqueue(c, m, reinterpret_cast<const int32_t*>(du), d);
    if(rc)
        return rc;
    {
        StageScope ts(c, "cull_greedy");
        hipLaunchKernelGGL(k_cull_greedy, dim3(1), dim3(kCullThreads), 0, s, r->d_lid.get(), r->d_n.get(),
                           reinterpret_cast<const int32_t*>(du + o_cand), n_cand, c->p.max_keypoints, d.table, d.counts, d.stamp,
                           d.bkt, min_observers, ratio, min_landmarks,
                           reinterpret_cast<CullRes*>(r->h_res.dev() + 16), reinterpret_cast<int32_t*>(r->h_res.dev()));
    }
    MSLAM_CHK(c, hipGetLastError());
    MSLAM_CHK(c, hipStreamSynchronize(s));
    const int32_t done = *reinterpret_cast<const int32_t*>(r->h_res.get());
    const CullRes* res = reinterpret_cast<const CullRes*>(r->h_res.get() + 16);
    bool ok = done == n_cand;
    for(int k = 0; ok && k < n_cand; ++k)
        ok = res[k].n_landmarks >= 0 && res[k].n_redundant >= 0 && res[k].n_redundant <= res[k].n_landmarks && (res[k].culled | 1) == 1;
    if(!ok)
        return fail(c, MSLAM_HIP_E_RUNTIME, me + ": the kernel left no result");
    int total = 0;
    for(int k = 0; k < n_cand; ++k)
    {
        culled[k] = (uint8_t)res[k].culled;
        if(n_landmarks)
            n_landmarks[k] = res[k].n_landmarks;
        if(n_redundant)
            n_redundant[k] = res[k].n_redundant;
        total += res[k].culled;
        if(remove && res[k].culled)
            store_release(r, cand[k], cand_slots[(size_t)k]);
    }
    if(n_culled)
        *n_culled = total;
    return MSLAM_HIP_OK;
}
} // namespace

extern "C" {

int mslam_hip_kf_observers(mslam_hip_ctx* c, const int32_t* ids, int n_ids, const int64_t* landmark_ids, int n, int32_t* counts)
{
    if(counts && n > 0 && n <= (1 << 24))
        std::memset(counts, 0, (size_t)n * 4);
    int rc = reloc_enter(c);
    if(rc)
        return rc;
    const std::string me = "kf_observers";
    CullMap m;
    std::unordered_map<int, int> pos_of;
    rc = cull_resolve(c, me, ids, n_ids, &m, &pos_of);
    if(rc)
        return rc;
    rc = lid_list_check(c, me, n, landmark_ids && counts, landmark_ids);
    if(rc)
        return rc;
    if(n == 0)
        return MSLAM_HIP_OK;
    RelocState* r = c->reloc;
    // one upload: [asked ids n x i64 | listed slots | the counts n x i32, which come back]
    const size_t o_slots = (size_t)n * 8, o_out = o_slots + (size_t)n_ids * 4, up = o_out + (size_t)n * 4;
    rc = reloc_scratch(c, up, 0, (size_t)n * 4);
    if(rc)
        return rc;
    CullDev d{};
    rc = cull_scratch(c, m.keys, &d);
    if(rc)
        return rc;
    uint8_t *h = r->h_up, *du = r->d_up;
    std::memcpy(h, landmark_ids, (size_t)n * 8);
    std::memcpy(h + o_slots, m.slots.data(), (size_t)n_ids * 4);
    hipStream_t s = c->stream;
    {
        StageScope ts(c, "cull_upload");
        MSLAM_CHK(c, hipMemcpyAsync(du, h, o_out, hipMemcpyHostToDevice, s));
    }
    rc = cull_count_enqueue(c, m, reinterpret_cast<const int32_t*>(du + o_slots), d);
    if(rc)
        return rc;
    {
        StageScope ts(c, "cull_lookup");
        hipLaunchKernelGGL(k_cull_lookup, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const int64_t*>(du), n, d.table,
                           d.counts, reinterpret_cast<int32_t*>(du + o_out));
    }
    MSLAM_CHK(c, hipGetLastError());
    MSLAM_CHK(c, hipMemcpyAsync(r->h_res.get(), du + o_out, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    MSLAM_CHK(c, hipStreamSynchronize(s));
    std::memcpy(counts, r->h_res.get(), (size_t)n * 4);
    return MSLAM_HIP_OK;
}

int mslam_hip_kf_cull_search(mslam_hip_ctx* c, const int32_t* ids, int n_ids, const int32_t* cand, int n_cand, int min_observers,
                             double ratio, int min_landmarks, uint8_t* culled, int32_t* n_landmarks, int32_t* n_redundant, int* n_culled)
{
    return cull_run(c, "kf_cull_search", false, ids, n_ids, cand, n_cand, min_observers, ratio, min_landmarks, culled, n_landmarks,
                    n_redundant, n_culled);
}

int mslam_hip_kf_cull(mslam_hip_ctx* c, const int32_t* ids, int n_ids, const int32_t* cand, int n_cand, int min_observers, double ratio,
                      int min_landmarks, uint8_t* culled, int32_t* n_landmarks, int32_t* n_redundant, int* n_culled)
{
    return cull_run(c, "kf_cull", true, ids, n_ids, cand, n_cand, min_observers, ratio, min_landmarks, culled, n_landmarks, n_redundant,
                    n_culled);
}

} // extern "C"
