// k_prune.hip — mslam_hip_kf_remove_observations: the named (entry, landmark id) observations leave the keyframe store and
// the entries they leave are compacted in place (the semantics are stated at the declaration in include/mslam_hip.h).
//
// This is the body the reference leaves commented out: RgbdFeatureFrontend::removeObservation
// (rgbd_feature_frontend.cpp:469-487), which update(const BackendOutputType&) calls for every outlier observation of a
// bundle adjustment (:224-230).
//
//   k_prune_compact  one workgroup per affected entry.  The host sorts and de-duplicates the (slot, landmark id) rows, so
//                    an entry's rows are one ascending segment [begin, end) of the uploaded id list.  The workgroup walks
//                    its entry in chunks of kPruneChunk positions (compact_entry, compact.hpp, which k_lmcull.hip shares):
//                    a thread loads its landmark (id, descriptor, world point: 8 + 32 + 24 bytes) into registers,
//                    binary-searches the id in the segment, and a workgroup scan of the keep flags gives the landmark's
//                    destination.  The scan's barrier separates the chunk's loads from its stores; a destination never
//                    lies above its source and a chunk's stores end below the next chunk's loads, so the compaction needs
//                    no second buffer.  A hit is an integer atomicAdd on its row's count: the value does not depend on
//                    the order.  Thread 0 leaves the new count.
//
// No workgroup reads or writes another workgroup's entry, and the row counts are the only words two threads share.
#include "compact.hpp"
#include "reloc.hpp"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace mslam
{

constexpr int kPruneChunk = kCompactChunk; // positions per chunk = threads per workgroup (tests/prune_ref.py: T)

struct PruneSeg // one affected entry: its slot and its rows [begin, end) of the distinct list
{
    int32_t slot, begin, end, pad;
};

// the position of `id` in the ascending ids[begin, end), or -1
__device__ __forceinline__ int prune_find(const int64_t* __restrict__ ids, int begin, int end, int64_t id)
{
    int lo = begin, hi = end;
    while(lo < hi)
    {
        const int mid = lo + ((hi - lo) >> 1);
        if(ids[mid] < id)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < end && ids[lo] == id ? lo : -1;
}

// grid = affected entries.  store_* are read and written through the same pointers: no __restrict__ on them.
__global__ __launch_bounds__(kPruneChunk) void k_prune_compact(uint8_t* store_desc, double* store_world, int64_t* store_lid,
                                                               int32_t* store_n, int K, const PruneSeg* __restrict__ segs,
                                                               const int64_t* __restrict__ row_lid, uint32_t* __restrict__ row_hits,
                                                               int32_t* __restrict__ new_n)
{
    const PruneSeg seg = segs[blockIdx.x];
    const int n = entry_count(store_n, seg.slot, K);
    const int kept = compact_entry(store_desc, store_world, store_lid, (size_t)seg.slot * K, n, [&](int64_t lid) {
        const int row = prune_find(row_lid, seg.begin, seg.end, lid);
        if(row >= 0)
            atomicAdd(&row_hits[row], 1u);
        return row >= 0;
    });
    if(threadIdx.x == 0)
    {
        store_n[seg.slot] = kept;
        new_n[blockIdx.x] = kept;
    }
}

} // namespace mslam

using namespace mslam;

extern "C" {

int mslam_hip_kf_remove_observations(mslam_hip_ctx* c, const int32_t* kf_ids, const int64_t* landmark_ids, int n, int32_t* removed,
                                     int* n_removed)
{
    if(n_removed)
        *n_removed = 0;
    if(removed && n > 0 && n <= (1 << 24))
        std::memset(removed, 0, (size_t)n * 4);
    int rc = reloc_enter(c);
    if(rc)
        return rc;
    const std::string me = "kf_remove_observations";
    if(n < 0 || n > (1 << 24) || (n > 0 && (!kf_ids || !landmark_ids)))
        return fail(c, MSLAM_HIP_E_INVALID, me + ": bad argument");
    RelocState* r = c->reloc;
    struct Row
    {
        int32_t slot;
        int64_t lid;
        int32_t p;
    };
    std::vector<Row> listed((size_t)n);
    std::vector<int32_t> first((size_t)r->slots + 1, 0); // rows per slot, then where each slot's rows begin
    int last_id = 0, last_slot = -1;                     // (consecutive rows often name one keyframe)
    for(int p = 0; p < n; ++p)
    {
        if(landmark_ids[p] < 0)
            return fail(c, MSLAM_HIP_E_INVALID, me + ": a landmark id lies outside [0, 2^63)");
        if(last_slot < 0 || kf_ids[p] != last_id)
        {
            rc = store_slot(c, me, "id", kf_ids[p], &last_slot);
            if(rc)
                return rc;
            last_id = kf_ids[p];
        }
        listed[(size_t)p] = Row{last_slot, landmark_ids[p], p};
        ++first[(size_t)last_slot + 1];
    }
    if(n == 0)
        return MSLAM_HIP_OK;
    // (slot, id) order: a counting pass groups the rows by slot, then each group is sorted by id, unless it is in order already
    for(size_t s = 0; s < (size_t)r->slots; ++s)
        first[s + 1] += first[s];
    std::vector<Row> rows((size_t)n);
    {
        std::vector<int32_t> at(first.begin(), first.end() - 1);
        for(const Row& row : listed)
            rows[(size_t)at[(size_t)row.slot]++] = row;
    }
    const auto by_lid = [](const Row& a, const Row& b) { return a.lid < b.lid; };
    for(size_t s = 0; s < (size_t)r->slots; ++s)
        if(first[s + 1] - first[s] > 1 && !std::is_sorted(rows.begin() + first[s], rows.begin() + first[s + 1], by_lid))
            std::sort(rows.begin() + first[s], rows.begin() + first[s + 1], by_lid);
    // the distinct rows in (slot, id) order, the segment of every affected slot, and where each caller's row went
    std::vector<int64_t> lids;
    std::vector<PruneSeg> segs;
    std::vector<int32_t> row_of((size_t)n);
    for(size_t k = 0; k < rows.size(); ++k)
    {
        const bool new_slot = k == 0 || rows[k].slot != rows[k - 1].slot;
        if(new_slot || rows[k].lid != rows[k - 1].lid)
        {
            if(new_slot)
                segs.push_back(PruneSeg{rows[k].slot, (int32_t)lids.size(), (int32_t)lids.size(), 0});
            lids.push_back(rows[k].lid);
            segs.back().end = (int32_t)lids.size();
        }
        row_of[(size_t)rows[k].p] = (int32_t)lids.size() - 1;
    }
    const size_t D = lids.size(), A = segs.size();
    // one upload: [distinct ids D x i64 | segments A x 16 | row counts D x u32, zero | new entry counts A x i32, -1];
    // the last two blocks come back in one copy
    const size_t o_seg = D * 8, o_hits = o_seg + A * sizeof(PruneSeg), o_n = o_hits + D * 4, up = o_n + A * 4, back = up - o_hits;
    rc = reloc_scratch(c, up, 0, back);
    if(rc)
        return rc;
    uint8_t *h = r->h_up, *d = r->d_up;
    std::memcpy(h, lids.data(), D * 8);
    std::memcpy(h + o_seg, segs.data(), A * sizeof(PruneSeg));
    std::memset(h + o_hits, 0, D * 4);
    std::memset(h + o_n, 0xFF, A * 4);
    hipStream_t s = c->stream;
    {
        StageScope ts(c, "prune_upload");
        MSLAM_CHK(c, hipMemcpyAsync(d, h, up, hipMemcpyHostToDevice, s));
    }
    {
        StageScope ts(c, "prune_compact");
        hipLaunchKernelGGL(k_prune_compact, dim3((unsigned)A), dim3(kPruneChunk), 0, s, r->d_desc.get(), r->d_world.get(), r->d_lid.get(),
                           r->d_n.get(), c->p.max_keypoints, reinterpret_cast<const PruneSeg*>(d + o_seg), reinterpret_cast<const int64_t*>(d),
                           reinterpret_cast<uint32_t*>(d + o_hits), reinterpret_cast<int32_t*>(d + o_n));
    }
    MSLAM_CHK(c, hipGetLastError());
    uint8_t* res = r->h_res.get();
    MSLAM_CHK(c, hipMemcpyAsync(res, d + o_hits, back, hipMemcpyDeviceToHost, s));
    MSLAM_CHK(c, hipStreamSynchronize(s));
    const uint32_t* hits = reinterpret_cast<const uint32_t*>(res);
    const int32_t* counts = reinterpret_cast<const int32_t*>(res + D * 4);
    for(size_t k = 0; k < A; ++k)
    {
        if(counts[k] < 0 || counts[k] > c->p.max_keypoints)
            return fail(c, MSLAM_HIP_E_RUNTIME, me + ": the kernel left no result");
        r->n_upper[(size_t)segs[k].slot] = counts[k]; // now known exactly
    }
    size_t total = 0;
    for(size_t k = 0; k < D; ++k)
        total += hits[k];
    if(removed)
        for(int p = 0; p < n; ++p)
            removed[p] = (int32_t)hits[(size_t)row_of[(size_t)p]];
    if(n_removed)
        *n_removed = (int)total;
    return MSLAM_HIP_OK;
}

} // extern "C"
