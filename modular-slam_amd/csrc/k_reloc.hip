// k_reloc.hip — verified relocalisation: a device-resident keyframe store and one query frame against N stored keyframes.
//
// What RgbdFeatureFrontend::relocalize is written to do with the relocalizer's candidates (reference
// rgbd_feature_frontend.cpp:495-534; the body is commented out there): per candidate matchLandmarks (:509 -> :237), solvePnp
// on the matched landmarks (:519), the candidate with the most inliers (:527-529).  Landmarks enter the store the way
// addNewLandmarks creates them (:402-431): valid depth, z <= zThreshold, toGlobalCoordinates (projection.cpp:51-54).
//
// The matcher and the PnP solver are the existing kernels (k_match.hip through launch_match_knn2 / launch_ratio_compact with
// from_stride = 0: the query descriptors are uploaded once and are every pair's train side; k_pnp.hip through
// pnp_launch_batch).  New here: the store, the gather of the candidates' descriptor blocks into the contiguous layout the
// matcher addresses, the match -> correspondence gather, and the ranking.  One upload, one synchronisation per call.
// Gather to PnP are seq_enqueue, which a tracking window (k_track_window.hip) enqueues as well, with its frames as the rows
// and one entry for all of them; the scratch blocks of every such call are grown by reloc_scratch.
#include "reloc.hpp"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace mslam
{

void reloc_destroy(RelocState* r) { delete r; }

// ---- kernels ----------------------------------------------------------------------------------------------------------

// One workgroup lifts one frame of the last batch into a store slot: keypoints with a valid depth and z <= z_max, in
// keypoint order (ballot / popcount compaction, as k_pnp_gather), world = R p + t in f64; landmark o of the entry gets the
// fresh id lid_base | o.
__global__ __launch_bounds__(256) void k_kf_lift(const uint8_t* __restrict__ desc, const double* __restrict__ xyz,
                                                 const uint8_t* __restrict__ valid, const int32_t* __restrict__ count, int cap,
                                                 KfPose pose, uint8_t* __restrict__ out_desc, double* __restrict__ out_world,
                                                 int32_t* __restrict__ out_n, int64_t* __restrict__ out_lid, int64_t lid_base)
{
    __shared__ uint32_t wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(max(*count, 0), cap);
    uint32_t running = 0;
    for(int base = 0; base < n; base += 256)
    {
        const int i = base + tid;
        bool ok = false;
        double px = 0, py = 0, pz = 0;
        if(i < n && valid[i] != 0)
        {
            px = xyz[3 * (size_t)i], py = xyz[3 * (size_t)i + 1], pz = xyz[3 * (size_t)i + 2];
            ok = pz <= pose.z_max;
        }
        const unsigned long long b = __ballot(ok);
        if(lane == 0)
            wsum[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t pre = 0, tot = 0;
        for(int k = 0; k < 4; ++k)
        {
            pre += k < wave ? wsum[k] : 0;
            tot += wsum[k];
        }
        if(ok)
        {
            const size_t o = running + pre + (uint32_t)__popcll(b & ((1ull << lane) - 1ull)); // < n <= cap
            copy_desc(desc + (size_t)i * 32, out_desc + o * 32);
            out_world[o * 3] = ((pose.R[0] * px + pose.R[1] * py) + pose.R[2] * pz) + pose.t[0];
            out_world[o * 3 + 1] = ((pose.R[3] * px + pose.R[4] * py) + pose.R[5] * pz) + pose.t[1];
            out_world[o * 3 + 2] = ((pose.R[6] * px + pose.R[7] * py) + pose.R[8] * pz) + pose.t[2];
            out_lid[o] = lid_base | (int64_t)o;
        }
        running += tot;
        __syncthreads();
    }
    if(tid == 0)
        *out_n = (int32_t)running;
}

// The matcher addresses row r's query side as base + r * stride: the descriptor block of store slot slots[p] is copied into
// row p of a contiguous scratch; blockIdx.y = p, one uint4 (half a descriptor) per thread.  Gathered row p is the entry
// of `share` rows of the sequence (1: its own; all of them when there is one entry, share <= 256: block 0), which each
// get its landmark count.
__global__ __launch_bounds__(256) void k_reloc_gather_desc(const uint8_t* __restrict__ store_desc, const int32_t* __restrict__ store_n,
                                                           const int32_t* __restrict__ slots, int K, int S, int share,
                                                           uint8_t* __restrict__ g_desc, int32_t* __restrict__ g_cnt)
{
    const int p = blockIdx.y;
    const int slot = slots[p];
    const int n = min(min(max(store_n[slot], 0), K), S);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if(i < share)
        g_cnt[(size_t)p * share + i] = n;
    if(i < 2 * n)
        reinterpret_cast<uint4*>(g_desc + (size_t)p * S * 32)[i] = reinterpret_cast<const uint4*>(store_desc + (size_t)slot * K * 32)[i];
}

// row p (one workgroup): its matches whose keypoint is not masked out become correspondences, in match order:
// object = (float) world point of landmark `to` of the row's entry, image = xy of keypoint `from`.  Rows are from_stride
// keypoints and slot_stride list positions apart (0: shared); n_kp == nullptr: every row has nq keypoints.
// ALIGN (mslam_hip_set_track_pose): the destination of a pair is the camera-frame point of keypoint `from` (cam_xyz, f64 x 3,
// rows from_stride keypoints apart) cast to float, written to dst (x 3); img is not written.
template <bool ALIGN>
__global__ __launch_bounds__(256) void k_reloc_corr(const int32_t* __restrict__ mfrom, const int32_t* __restrict__ mto,
                                                    const int32_t* __restrict__ mcount, const int32_t* __restrict__ g_cnt,
                                                    const int32_t* __restrict__ slots, int slot_stride,
                                                    const double* __restrict__ store_world, int K, int S,
                                                    const float* __restrict__ xy_all, const uint8_t* __restrict__ valid_all,
                                                    long long from_stride, const int32_t* __restrict__ n_kp, int nq,
                                                    float* __restrict__ obj, float* __restrict__ img, uint8_t* __restrict__ mask,
                                                    int32_t* __restrict__ n_out, const double* __restrict__ cam_xyz,
                                                    float* __restrict__ dst)
{
    __shared__ uint32_t wsum[4];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = min(max(mcount[p], 0), S), n_to = g_cnt[p];
    if(n_kp)
        nq = (int)min((long long)max(n_kp[p], 0), from_stride);
    const float* xy = xy_all + (size_t)p * from_stride * 2;
    const uint8_t* valid = valid_all ? valid_all + (size_t)p * from_stride : nullptr;
    const size_t row = (size_t)p * S;
    const double* world = store_world + (size_t)slots[(size_t)p * slot_stride] * K * 3;
    uint32_t running = 0;
    for(int base = 0; base < m; base += 256)
    {
        const int i = base + tid;
        int from = 0, to = 0;
        bool ok = false;
        if(i < m)
        {
            from = mfrom[row + i], to = mto[row + i];
            ok = (unsigned)from < (unsigned)nq && (unsigned)to < (unsigned)n_to && (!valid || valid[from] != 0);
        }
        const unsigned long long b = __ballot(ok);
        if(lane == 0)
            wsum[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t pre = 0, tot = 0;
        for(int k = 0; k < 4; ++k)
        {
            pre += k < wave ? wsum[k] : 0;
            tot += wsum[k];
        }
        if(ok)
        {
            const size_t o = row + running + pre + (uint32_t)__popcll(b & ((1ull << lane) - 1ull)); // < row + m <= row + S
            const double* P = world + (size_t)to * 3;
            obj[o * 3] = (float)P[0], obj[o * 3 + 1] = (float)P[1], obj[o * 3 + 2] = (float)P[2];
            if constexpr(ALIGN)
            {
                const double* Q = cam_xyz + ((size_t)p * from_stride + (size_t)from) * 3;
                dst[o * 3] = (float)Q[0], dst[o * 3 + 1] = (float)Q[1], dst[o * 3 + 2] = (float)Q[2];
            }
            else
                img[o * 2] = xy[(size_t)from * 2], img[o * 2 + 1] = xy[(size_t)from * 2 + 1];
        }
        running += tot;
        __syncthreads();
    }
    // fewer than 4 correspondences: the PnP kernel reports "no model" without touching the mask (the alignment kernel does
    // so below 3 and writes every byte at 3)
    if(running < 4 && tid < (int)running)
        mask[row + tid] = 0;
    if(tid == 0)
        n_out[p] = (int32_t)running;
}

// block 0: the ranking (one wave, lane k = candidate k <= 63) and the per-candidate records; block 1 + p (want_pairs): the
// matches and the consensus mask of candidate p.  Everything lands in the page-locked, device-mapped result block: these
// stores are the transfer.
__global__ __launch_bounds__(256) void k_reloc_rank(const int32_t* __restrict__ mcount, const int32_t* __restrict__ ncorr,
                                                    const double* __restrict__ pnp_out, int n_cand, int min_inliers, int S,
                                                    const int32_t* __restrict__ mfrom, const int32_t* __restrict__ mto,
                                                    const uint8_t* __restrict__ mask, uint8_t* __restrict__ res)
{
    const int tid = threadIdx.x;
    if(blockIdx.x == 0)
    {
        if(tid >= 64)
            return;
        const bool live = tid < n_cand;
        RelocRes r{};
        if(live)
        {
            r = reloc_record(pnp_out + (size_t)tid * 16, mcount[tid], ncorr[tid]);
            reinterpret_cast<RelocRes*>(res + 16)[tid] = r;
        }
        // most inliers among the candidates with a model, the first one on ties (max_element): key = (inliers + 1, 63 - k)
        int key = live && r.status ? ((r.n_inliers + 1) << 6) | (63 - tid) : 0;
        for(int o = 32; o > 0; o >>= 1)
            key = max(key, __shfl_xor(key, o));
        if(tid == 0)
        {
            int best = -1;
            if(key != 0 && (key >> 6) - 1 >= min_inliers)
                best = 63 - (key & 63);
            reinterpret_cast<int32_t*>(res)[0] = best;
        }
        return;
    }
    const int p = blockIdx.x - 1;
    const size_t row = (size_t)p * S, all = (size_t)n_cand * S;
    int32_t* h_from = reinterpret_cast<int32_t*>(res + 16 + kRelocMaxCand * sizeof(RelocRes));
    int32_t* h_to = h_from + all;
    uint8_t* h_mask = reinterpret_cast<uint8_t*>(h_to + all);
    const int m = min(max(mcount[p], 0), S), nc = min(max(ncorr[p], 0), S);
    for(int i = tid; i < m; i += 256)
    {
        h_from[row + i] = mfrom[row + i];
        h_to[row + i] = mto[row + i];
    }
    for(int i = tid; i < nc; i += 256)
        h_mask[row + i] = mask[row + i];
}

} // namespace mslam

using namespace mslam;

// ---- host side ---------------------------------------------------------------------------------------------------------

int mslam::reloc_enter(mslam_hip_ctx* c)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    MSLAM_CHK(c, hipSetDevice(c->p.device));
    if(!c->reloc)
        c->reloc = new RelocState();
    return MSLAM_HIP_OK;
}

// at least `want` slots; the live entries move with the store
int mslam::store_reserve(mslam_hip_ctx* c, int want)
{
    RelocState* r = c->reloc;
    if(want <= r->slots)
        return MSLAM_HIP_OK;
    const size_t K = (size_t)c->p.max_keypoints;
    const int slots = std::max({want, 2 * r->slots, 16});
    // fresh blocks, the live slots copied across; one wait, then the swap — a failure leaves the store as it was
    const size_t n = (size_t)slots, old = (size_t)r->slots;
    DevBuf<uint8_t> nd;
    DevBuf<double> nw;
    DevBuf<int32_t> nn;
    DevBuf<int64_t> nl;
    hipError_t e = grown_copy(nd, r->d_desc, n * K * 32, old * K * 32, false, c->stream);
    if(e == hipSuccess)
        e = grown_copy(nw, r->d_world, n * K * 3, old * K * 3, false, c->stream);
    if(e == hipSuccess)
        e = grown_copy(nn, r->d_n, n, old, true, c->stream);
    if(e == hipSuccess)
        e = grown_copy(nl, r->d_lid, n * K, old * K, false, c->stream);
    if(e == hipSuccess)
        e = hipStreamSynchronize(c->stream); // everything that reads the old blocks has finished before they are freed
    if(e != hipSuccess)
        return fail(c, MSLAM_HIP_E_RUNTIME, std::string("kf store: ") + hipGetErrorString(e));
    r->d_desc = std::move(nd), r->d_world = std::move(nw), r->d_n = std::move(nn), r->d_lid = std::move(nl);
    for(int s = slots - 1; s >= r->slots; --s)
        r->free_slots.push_back(s); // (handed out in ascending order)
    r->n_upper.resize((size_t)slots, 0);
    r->slots = slots;
    return MSLAM_HIP_OK;
}

// the slot of `id`: its own when the id exists (the entry is replaced), a free one otherwise
int mslam::store_slot_for(mslam_hip_ctx* c, int id, int* slot)
{
    RelocState* r = c->reloc;
    auto it = r->slot_of.find(id);
    if(it != r->slot_of.end())
    {
        *slot = it->second;
        return MSLAM_HIP_OK;
    }
    if(r->free_slots.empty())
    {
        const int rc = store_reserve(c, r->slots + 1);
        if(rc)
            return rc;
    }
    *slot = r->free_slots.back();
    r->free_slots.pop_back();
    r->slot_of[id] = *slot;
    return MSLAM_HIP_OK;
}

int mslam::store_slot_missing(mslam_hip_ctx* c, const std::string& me, const char* what, int id)
{
    return fail(c, MSLAM_HIP_E_INVALID, me + ": " + what + " " + std::to_string(id) + " is not in the keyframe store");
}

int64_t mslam::store_next_lid_base(mslam_hip_ctx* c)
{
    return fresh_lid_base(++c->reloc->serial);
}

int mslam::lid_list_check(mslam_hip_ctx* c, const std::string& me, int n, bool present, const int64_t* ids, const int64_t* more)
{
    if(n < 0 || n > (1 << 24) || (n > 0 && !present))
        return fail(c, MSLAM_HIP_E_INVALID, me + ": bad argument");
    for(int i = 0; i < n; ++i)
        if(ids[i] < 0 || (more && more[i] < 0))
            return fail(c, MSLAM_HIP_E_INVALID, me + ": a landmark id lies outside [0, 2^63)");
    return MSLAM_HIP_OK;
}

LmTable mslam::lm_table_grow(mslam_hip_ctx* c, size_t keys, size_t bytes, size_t offset)
{
    RelocState* r = c->reloc;
    const size_t buckets = lm_bucket_count(keys);
    const hipError_t e = grow(r->d_lm_table, std::max(bytes, offset + buckets * sizeof(LmBucket)), c->stream);
    if(e != hipSuccess)
    {
        c->err = std::string("the landmark-id table: ") + hipGetErrorString(e);
        return LmTable{nullptr, 0};
    }
    return LmTable{reinterpret_cast<LmBucket*>(r->d_lm_table + offset), (unsigned long long)(buckets - 1)};
}

int TrackSlots::resolve(mslam_hip_ctx* c, const char* who, int ref_id, const int32_t* vote_ids, int n_vote, int new_id_)
{
    const std::string me = who;
    new_id = new_id_;
    int rc = store_slot(c, me, "reference id", ref_id, &ref_slot);
    bool collides = new_id >= 0 && new_id == ref_id;
    for(int k = 0; !rc && k < n_vote; ++k)
    {
        rc = store_slot(c, me, "vote id", vote_ids[k], &vote_slots[k]);
        collides = collides || (new_id >= 0 && vote_ids[k] == new_id);
    }
    if(rc)
        return rc;
    if(collides)
        return fail(c, MSLAM_HIP_E_INVALID, me + ": new_id names the reference keyframe or a keyframe of the vote list");
    return MSLAM_HIP_OK;
}

int TrackSlots::reserve(mslam_hip_ctx* c)
{
    if(new_id < 0)
        return MSLAM_HIP_OK;
    existed = c->reloc->slot_of.count(new_id) != 0;
    const int rc = store_slot_for(c, new_id, &new_slot);
    if(rc)
        return rc;
    lid_base = store_next_lid_base(c);
    return MSLAM_HIP_OK;
}

void TrackSlots::commit(mslam_hip_ctx* c, int n_entry)
{
    c->reloc->n_upper[(size_t)new_slot] = n_entry;
}

void TrackSlots::rollback(mslam_hip_ctx* c, bool enqueued_work_may_still_run)
{
    RelocState* r = c->reloc;
    if(enqueued_work_may_still_run)
    {
        const std::string msg = c->err;
        (void)hipStreamSynchronize(c->stream);
        c->err = msg;
        if(existed)
            r->n_upper[(size_t)new_slot] = c->p.max_keypoints;
    }
    if(new_id >= 0 && !existed)
    {
        r->slot_of.erase(new_id);
        r->free_slots.push_back(new_slot);
    }
}

// mslam_hip_kf_add (landmark_ids == nullptr: fresh ids) and mslam_hip_kf_add_ids
static int kf_add_host(mslam_hip_ctx* c, const char* who, int id, const uint8_t* desc, const double* world_xyz,
                       const int64_t* landmark_ids, bool own_ids, int n)
{
    int rc = reloc_enter(c);
    if(rc)
        return rc;
    if(n < 0 || (n > 0 && (!desc || !world_xyz || (own_ids && !landmark_ids))))
        return fail(c, MSLAM_HIP_E_INVALID, std::string(who) + ": bad argument");
    if(n > c->p.max_keypoints)
        return fail(c, MSLAM_HIP_E_CAPACITY, std::string(who) + ": more landmarks than the context's max_keypoints");
    for(int i = 0; own_ids && i < n; ++i)
        if(landmark_ids[i] < 0 || landmark_ids[i] >= kFreshLidBit)
            return fail(c, MSLAM_HIP_E_INVALID, std::string(who) + ": landmark ids lie in [0, 2^62)");
    int slot = -1;
    rc = store_slot_for(c, id, &slot);
    if(rc)
        return rc;
    RelocState* r = c->reloc;
    const size_t K = (size_t)c->p.max_keypoints;
    const int32_t n32 = n;
    const int64_t base = store_next_lid_base(c);
    std::vector<int64_t> fresh;
    if(!own_ids)
    {
        fresh.resize((size_t)n);
        for(int i = 0; i < n; ++i)
            fresh[(size_t)i] = base | (int64_t)i;
        landmark_ids = fresh.data();
    }
    if(n > 0)
    {
        MSLAM_CHK(c, hipMemcpyAsync(r->d_desc + (size_t)slot * K * 32, desc, (size_t)n * 32, hipMemcpyHostToDevice, c->stream));
        MSLAM_CHK(c, hipMemcpyAsync(r->d_world + (size_t)slot * K * 3, world_xyz, (size_t)n * 24, hipMemcpyHostToDevice, c->stream));
        MSLAM_CHK(c, hipMemcpyAsync(r->d_lid + (size_t)slot * K, landmark_ids, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    }
    MSLAM_CHK(c, hipMemcpyAsync(r->d_n + slot, &n32, 4, hipMemcpyHostToDevice, c->stream));
    MSLAM_CHK(c, hipStreamSynchronize(c->stream)); // host-pointer entry point: the caller's buffers are free on return
    r->n_upper[(size_t)slot] = n;
    return MSLAM_HIP_OK;
}

// what mslam_hip_kf_read and mslam_hip_kf_read_ids start with: the slot of entry `id` and its landmark count, read from the
// device
static int kf_entry_count(mslam_hip_ctx* c, const char* who, int id, int capacity, int* n, size_t* slot)
{
    int rc = reloc_enter(c);
    if(rc)
        return rc;
    const std::string me = who;
    if(!n || capacity < 0)
        return fail(c, MSLAM_HIP_E_INVALID, me + ": bad argument");
    RelocState* r = c->reloc;
    auto it = r->slot_of.find(id);
    if(it == r->slot_of.end())
        return fail(c, MSLAM_HIP_E_INVALID, me + ": no such keyframe id");
    *slot = (size_t)it->second;
    int32_t n32 = 0;
    MSLAM_CHK(c, hipMemcpyAsync(&n32, r->d_n + *slot, 4, hipMemcpyDeviceToHost, c->stream));
    MSLAM_CHK(c, hipStreamSynchronize(c->stream));
    if(n32 < 0 || n32 > c->p.max_keypoints)
        return fail(c, MSLAM_HIP_E_RUNTIME, me + ": impossible landmark count");
    *n = n32;
    r->n_upper[*slot] = n32; // now known exactly
    return MSLAM_HIP_OK;
}

extern "C" {

int mslam_hip_kf_reserve(mslam_hip_ctx* c, int max_entries)
{
    int rc = reloc_enter(c);
    if(rc)
        return rc;
    if(max_entries < 0)
        return fail(c, MSLAM_HIP_E_INVALID, "kf_reserve: bad argument");
    return store_reserve(c, max_entries);
}

int mslam_hip_kf_size(mslam_hip_ctx* c, int* n_entries)
{
    if(!c || !n_entries)
        return MSLAM_HIP_E_INVALID;
    *n_entries = c->reloc ? (int)c->reloc->slot_of.size() : 0;
    return MSLAM_HIP_OK;
}

int mslam_hip_kf_add(mslam_hip_ctx* c, int id, const uint8_t* desc, const double* world_xyz, int n)
{
    return kf_add_host(c, "kf_add", id, desc, world_xyz, nullptr, false, n);
}

int mslam_hip_kf_add_ids(mslam_hip_ctx* c, int id, const uint8_t* desc, const double* world_xyz, const int64_t* landmark_ids, int n)
{
    return kf_add_host(c, "kf_add_ids", id, desc, world_xyz, landmark_ids, true, n);
}

int mslam_hip_kf_add_from_batch_dev(mslam_hip_ctx* c, int id, int frame, const double* R, const double* t, double z_max)
{
    int rc = reloc_enter(c);
    if(rc)
        return rc;
    if(!R || !t || !(z_max == z_max))
        return fail(c, MSLAM_HIP_E_INVALID, "kf_add_from_batch_dev: bad argument");
    if(frame < 0 || frame >= c->n_last)
        return fail(c, MSLAM_HIP_E_INVALID, "kf_add_from_batch_dev: no such frame in the last detect batch");
    if(!c->d_xyz || c->points_seq != c->detect_seq)
        return fail(c, MSLAM_HIP_E_INVALID, "kf_add_from_batch_dev: the last detect batch has not been back-projected");
    int slot = -1;
    rc = store_slot_for(c, id, &slot);
    if(rc)
        return rc;
    RelocState* r = c->reloc;
    const size_t K = (size_t)c->p.max_keypoints;
    KfPose pose;
    std::memcpy(pose.R, R, sizeof(pose.R));
    std::memcpy(pose.t, t, sizeof(pose.t));
    pose.z_max = z_max;
    const int64_t lid_base = store_next_lid_base(c);
    {
        StageScope ts(c, "kf_lift");
        // frame f of the batch: descriptors in output slot f + 1, points in row f of the back-projection
        hipLaunchKernelGGL(k_kf_lift, dim3(1), dim3(256), 0, c->stream, cur_out(c).desc + (size_t)(frame + 1) * K * 32,
                           c->d_xyz + (size_t)frame * K * 3, c->d_valid + (size_t)frame * K, cur_out(c).count + 1 + frame,
                           c->p.max_keypoints, pose, r->d_desc + (size_t)slot * K * 32, r->d_world + (size_t)slot * K * 3,
                           r->d_n + slot, r->d_lid + (size_t)slot * K, lid_base);
    }
    MSLAM_CHK(c, hipGetLastError());
    r->n_upper[(size_t)slot] = c->p.max_keypoints; // (the count stays on the device)
    return MSLAM_HIP_OK;
}

int mslam_hip_kf_remove(mslam_hip_ctx* c, int id)
{
    int rc = reloc_enter(c);
    if(rc)
        return rc;
    RelocState* r = c->reloc;
    auto it = r->slot_of.find(id);
    if(it == r->slot_of.end())
        return fail(c, MSLAM_HIP_E_INVALID, "kf_remove: no such keyframe id");
    store_release(r, id, it->second);
    return MSLAM_HIP_OK;
}

int mslam_hip_kf_clear(mslam_hip_ctx* c)
{
    int rc = reloc_enter(c);
    if(rc)
        return rc;
    RelocState* r = c->reloc;
    r->slot_of.clear();
    r->free_slots.clear();
    for(int s = r->slots - 1; s >= 0; --s)
        r->free_slots.push_back(s);
    return MSLAM_HIP_OK;
}

int mslam_hip_kf_read(mslam_hip_ctx* c, int id, uint8_t* desc, double* world_xyz, int capacity, int* n)
{
    size_t slot = 0;
    const int rc = kf_entry_count(c, "kf_read", id, capacity, n, &slot);
    if(rc || (!desc && !world_xyz))
        return rc;
    RelocState* r = c->reloc;
    const size_t K = (size_t)c->p.max_keypoints, n32 = (size_t)*n;
    if(*n > capacity)
        return fail(c, MSLAM_HIP_E_CAPACITY, "kf_read: the entry has more landmarks than `capacity`");
    if(desc && n32 > 0)
        MSLAM_CHK(c, hipMemcpyAsync(desc, r->d_desc + slot * K * 32, n32 * 32, hipMemcpyDeviceToHost, c->stream));
    if(world_xyz && n32 > 0)
        MSLAM_CHK(c, hipMemcpyAsync(world_xyz, r->d_world + slot * K * 3, n32 * 24, hipMemcpyDeviceToHost, c->stream));
    MSLAM_CHK(c, hipStreamSynchronize(c->stream));
    return MSLAM_HIP_OK;
}

int mslam_hip_kf_read_ids(mslam_hip_ctx* c, int id, int64_t* landmark_ids, int capacity, int* n)
{
    size_t slot = 0;
    const int rc = kf_entry_count(c, "kf_read_ids", id, capacity, n, &slot);
    if(rc || !landmark_ids)
        return rc;
    RelocState* r = c->reloc;
    const size_t K = (size_t)c->p.max_keypoints, n32 = (size_t)*n;
    if(*n > capacity)
        return fail(c, MSLAM_HIP_E_CAPACITY, "kf_read_ids: the entry has more landmarks than `capacity`");
    if(n32 > 0)
        MSLAM_CHK(c, hipMemcpyAsync(landmark_ids, r->d_lid + slot * K, n32 * 8, hipMemcpyDeviceToHost, c->stream));
    MSLAM_CHK(c, hipStreamSynchronize(c->stream));
    return MSLAM_HIP_OK;
}

} // extern "C"

int mslam::reloc_scratch(mslam_hip_ctx* c, size_t up, size_t arena, size_t res)
{
    RelocState* r = c->reloc;
    // (never less than a 4096-keypoint relocalize query takes, whichever call grows the block first: small callers such as
    // mslam_hip_kf_visible share the 168 KB instead of holding blocks of their own)
    if(up > r->h_up.size() || up > r->d_up.size())
    {
        const size_t bytes = std::max(up, (size_t)4096 * 41 + kRelocMaxCand * 4);
        MSLAM_CHK(c, grow(r->h_up, bytes, c->stream));
        MSLAM_CHK(c, grow(r->d_up, bytes, c->stream));
    }
    MSLAM_CHK(c, grow(r->d_arena, arena, c->stream));
    MSLAM_CHK(c, grow(r->h_res, res, c->stream));
    return MSLAM_HIP_OK;
}

// ---- the match-to-PnP sequence -----------------------------------------------------------------------------------------

namespace
{
// where the sequence's arrays lie in the arena, each 256-byte aligned
struct SeqArena
{
    size_t gdesc, gcnt, idx0, idx1, dist0, dist1, mfrom, mto, mcount, obj, img, ncorr, mask, hyp, counts, out, cells, list, ldesc, adst, bytes;
};

SeqArena seq_carve(int rows, size_t S, int iterations, bool one_slot, bool guided, int cap_from, bool align)
{
    size_t off = 0;
    auto carve = [&](size_t bytes) {
        const size_t o = off;
        off += al256(bytes);
        return o;
    };
    const size_t R = (size_t)rows, RS = R * S, it = (size_t)iterations;
    SeqArena a{};
    a.gdesc = carve((one_slot ? S : RS) * 32), a.gcnt = carve(R * 4);
    a.idx0 = carve(RS * 4), a.idx1 = carve(RS * 4), a.dist0 = carve(RS * 4), a.dist1 = carve(RS * 4);
    a.mfrom = carve(RS * 4), a.mto = carve(RS * 4), a.mcount = carve(R * 4);
    a.obj = carve(RS * 12), a.img = carve(RS * 8), a.ncorr = carve(R * 4), a.mask = carve(RS);
    a.hyp = carve(R * it * 96), a.counts = carve(R * it * 4), a.out = carve(R * 128);
    // the guided stage's lists come last: without them every array lies where it always did
    a.cells = carve(guided ? R * (kGuidedMaxCells + 1) * 4 : 0), a.list = carve(guided ? R * (size_t)std::max(cap_from, 1) * 16 : 0);
    a.ldesc = carve(guided ? R * (size_t)std::max(cap_from, 1) * 32 : 0);
    a.adst = carve(align ? RS * 12 : 0); // the alignment's destination points, behind everything else for the same reason
    a.bytes = off;
    return a;
}
} // namespace

size_t mslam::seq_arena_bytes(int rows, size_t S, int iterations, bool one_slot, bool guided, int cap_from, bool align)
{
    return seq_carve(rows, S, iterations, one_slot, guided, cap_from, align).bytes;
}

int mslam::seq_enqueue(mslam_hip_ctx* c, const SeqArgs& a, uint8_t* A, SeqDev* out)
{
    RelocState* r = c->reloc;
    const int K = c->p.max_keypoints, R = a.rows, S = (int)a.S;
    const bool align = a.align_distance > 0 && a.cam_xyz;
    const SeqArena o = seq_carve(R, a.S, a.iterations, a.one_slot, a.guided, a.cap_from, align);
    hipStream_t s = c->stream;
    int32_t* g_cnt = reinterpret_cast<int32_t*>(A + o.gcnt);
    {
        StageScope ts(c, "reloc_gather_desc");
        hipLaunchKernelGGL(k_reloc_gather_desc, dim3((unsigned)((2 * a.S + 255) / 256), a.one_slot ? 1u : (unsigned)R), dim3(256), 0, s,
                           r->d_desc, r->d_n, a.slots, K, S, a.one_slot ? R : 1, A + o.gdesc, g_cnt);
    }
    // match(from = keypoints of row r, to = landmarks of its entry): knn-2 with query = `to` and train = `from`
    MatchArgs m{};
    m.from_desc = a.desc;
    m.from_stride = (long long)a.from_stride * 32;
    m.from_cnt = a.from_cnt;
    m.n_from_fixed = a.n_from_fixed;
    m.to_desc = A + o.gdesc;
    m.to_stride = a.one_slot ? 0 : (long long)S * 32;
    m.to_cnt = g_cnt;
    m.cap = S;
    m.cap_from = a.cap_from;
    m.popcount_only = c->matcher_kind == MSLAM_HIP_MATCHER_POPCOUNT;
    m.idx0 = reinterpret_cast<int32_t*>(A + o.idx0);
    m.idx1 = reinterpret_cast<int32_t*>(A + o.idx1);
    m.dist0 = reinterpret_cast<int32_t*>(A + o.dist0);
    m.dist1 = reinterpret_cast<int32_t*>(A + o.dist1);
    RatioArgs q{};
    q.idx0 = m.idx0, q.dist0 = m.dist0, q.dist1 = m.dist1;
    q.from_cnt = a.from_cnt, q.n_from_fixed = a.n_from_fixed;
    q.to_cnt = g_cnt;
    q.cap = S;
    q.thr = c->d_ratio_thr;
    q.from_idx = reinterpret_cast<int32_t*>(A + o.mfrom);
    q.to_idx = reinterpret_cast<int32_t*>(A + o.mto);
    q.n_out = reinterpret_cast<int32_t*>(A + o.mcount);
    if(a.guided)
    {
        // the same operands, addressed the same way; the pose is the guess as the PnP launch below turns it into R0
        GuidedArgs g{};
        g.kp_desc = a.desc, g.kp_xy = a.xy, g.kp_stride = (long long)a.from_stride;
        g.kp_cnt = a.from_cnt, g.n_kp_fixed = a.n_from_fixed, g.kp_cap = std::max(a.cap_from, 1);
        g.lm_desc = m.to_desc, g.lm_stride = m.to_stride, g.lm_cnt = g_cnt, g.cap = S;
        g.world = r->d_world, g.slots = a.slots, g.slot_stride = a.one_slot ? 0 : 1, g.world_slot = (long long)K * 3;
        pnp_rvec_to_rotation(a.rvec, g.R);
        g.t[0] = a.tvec[0], g.t[1] = a.tvec[1], g.t[2] = a.tvec[2];
        g.fx = a.fx, g.fy = a.fy, g.cx = a.cx, g.cy = a.cy, g.radius = c->guided_radius;
        g.width = c->guided_width, g.height = c->guided_height, g.grid = guided_grid(g.width, g.height);
        g.cell_off = reinterpret_cast<int32_t*>(A + o.cells), g.list = reinterpret_cast<float4*>(A + o.list);
        g.list_desc = A + o.ldesc;
        g.idx0 = m.idx0, g.idx1 = m.idx1, g.dist0 = m.dist0, g.dist1 = m.dist1;
        {
            StageScope ts(c, "guided_bin");
            launch_guided_bin(g, R, s);
        }
        {
            StageScope ts(c, "match_guided");
            launch_match_guided(g, R, s);
        }
        c->last_match_kernel = 3;
        StageScope ts(c, "ratio_guided");
        launch_ratio_guided(q, c->guided_max_distance, R, s);
    }
    else
    {
        {
            StageScope ts(c, "match_knn2");
            c->last_match_kernel = launch_match_knn2(m, R, s);
        }
        StageScope ts(c, "ratio_compact");
        launch_ratio_compact(q, R, s);
    }
    float* d_obj = reinterpret_cast<float*>(A + o.obj);
    float* d_img = reinterpret_cast<float*>(A + o.img);
    int32_t* d_ncorr = reinterpret_cast<int32_t*>(A + o.ncorr);
    uint8_t* d_mask = A + o.mask;
    {
        StageScope ts(c, "reloc_corr");
        if(align)
            hipLaunchKernelGGL(k_reloc_corr<true>, dim3((unsigned)R), dim3(256), 0, s, q.from_idx, q.to_idx, q.n_out, g_cnt, a.slots,
                               a.one_slot ? 0 : 1, r->d_world, K, S, a.xy, a.valid, (long long)a.from_stride, a.from_cnt,
                               a.n_from_fixed, d_obj, d_img, d_mask, d_ncorr, a.cam_xyz, reinterpret_cast<float*>(A + o.adst));
        else
            hipLaunchKernelGGL(k_reloc_corr<false>, dim3((unsigned)R), dim3(256), 0, s, q.from_idx, q.to_idx, q.n_out, g_cnt, a.slots,
                               a.one_slot ? 0 : 1, r->d_world, K, S, a.xy, a.valid, (long long)a.from_stride, a.from_cnt,
                               a.n_from_fixed, d_obj, d_img, d_mask, d_ncorr, nullptr, nullptr);
    }
    MSLAM_CHK(c, hipGetLastError());
    if(align)
    {
        AlignBatchLaunch l{};
        l.src = d_obj, l.dst = reinterpret_cast<const float*>(A + o.adst), l.n = d_ncorr;
        l.n_problems = R, l.cap = S;
        l.iterations = a.iterations, l.max_distance = a.align_distance;
        l.seed = a.seed; // problem r samples with seed + r
        l.hyp = reinterpret_cast<double*>(A + o.hyp);
        l.counts = reinterpret_cast<int32_t*>(A + o.counts);
        l.mask = d_mask;
        l.out = reinterpret_cast<double*>(A + o.out);
        const int rc = align_launch_batch(c, l);
        if(rc)
            return rc;
        out->g_cnt = g_cnt, out->mfrom = q.from_idx, out->mto = q.to_idx, out->mcount = q.n_out, out->ncorr = d_ncorr;
        out->mask = d_mask, out->pnp_out = l.out, out->S = S;
        return MSLAM_HIP_OK;
    }
    PnpBatchLaunch l{};
    l.obj = d_obj, l.img = d_img, l.n = d_ncorr;
    l.n_problems = R, l.cap = S;
    l.fx = a.fx, l.fy = a.fy, l.cx = a.cx, l.cy = a.cy;
    l.use_guess = a.use_guess ? 1 : 0;
    for(int j = 0; j < 3; ++j)
    {
        l.rvec[j] = a.use_guess ? a.rvec[j] : 0.0;
        l.tvec[j] = a.use_guess ? a.tvec[j] : 0.0;
    }
    l.iterations = a.iterations;
    l.reprojection_error = a.reprojection_error;
    l.seed = a.seed; // problem r samples with seed + r
    l.hyp = reinterpret_cast<double*>(A + o.hyp);
    l.counts = reinterpret_cast<int32_t*>(A + o.counts);
    l.mask = d_mask;
    l.out = reinterpret_cast<double*>(A + o.out);
    const int rc = pnp_launch_batch(c, l);
    if(rc)
        return rc;
    out->g_cnt = g_cnt, out->mfrom = q.from_idx, out->mto = q.to_idx, out->mcount = q.n_out, out->ncorr = d_ncorr;
    out->mask = d_mask, out->pnp_out = l.out, out->S = S;
    return MSLAM_HIP_OK;
}

int mslam::reloc_run(mslam_hip_ctx* c, const uint8_t* desc, const float* xy, const uint8_t* valid, int n, const int32_t* cand_ids,
                     int n_cand, double fx, double fy, double cx, double cy, double ratio, int iterations, double reprojection_error,
                     unsigned long long seed, int use_extrinsic_guess, const double* rvec, const double* tvec, int min_inliers,
                     mslam_hip_reloc_candidate* out, int* best, int32_t* pair_from, int32_t* pair_to, uint8_t* inliers,
                     int pair_stride, const RelocHooks* hooks)
{
    int rc = reloc_enter(c);
    if(rc)
        return rc;
    if(best)
        *best = -1;
    const bool want_pairs = pair_from || pair_to || inliers;
    if(!best || n < 0 || n_cand < 0 || n_cand > kRelocMaxCand || (n > 0 && (!desc || !xy)) || (n_cand > 0 && (!cand_ids || !out)) ||
       iterations < 1 || iterations > 4096 || !(reprojection_error > 0) || !(fx != 0.0) || !(fy != 0.0) ||
       (use_extrinsic_guess && (!rvec || !tvec)) || (want_pairs && pair_stride < 0))
        return fail(c, MSLAM_HIP_E_INVALID, "relocalize: bad argument (at most 64 candidates, 1..4096 iterations)");
    if(n > 65535)
        return fail(c, MSLAM_HIP_E_INVALID, "relocalize: more than 65535 query keypoints are not supported");
    RelocState* r = c->reloc;
    int32_t slots[kRelocMaxCand];
    int n_max = 0;
    for(int k = 0; k < n_cand; ++k)
    {
        rc = store_slot(c, "relocalize", "candidate id", cand_ids[k], &slots[k]);
        if(rc)
            return rc;
        n_max = std::max(n_max, r->n_upper[(size_t)slots[k]]);
    }
    for(int k = 0; k < n_cand; ++k)
        out[k] = mslam_hip_reloc_candidate{};
    if(n_cand == 0 || n < 2)
        return fail(c, MSLAM_HIP_E_NO_MODEL, "relocalize: no candidate, or fewer than 2 query keypoints (no matches)");
    rc = mslam_ratio_table(c, ratio);
    if(rc)
        return rc;

    // per-candidate row stride of every scratch array: the largest candidate, in whole 256-row blocks
    const size_t S = seq_row_stride(n_max), P = (size_t)n_cand, PS = P * S;
    // ---- upload block: [desc n x 32 | xy n x 8 | slots 64 x 4 | valid n], one copy
    const size_t off_xy = (size_t)n * 32, off_slots = off_xy + (size_t)n * 8, off_valid = off_slots + kRelocMaxCand * 4;
    const size_t off_extra = al256(off_valid + (valid ? (size_t)n : 0)); // a hook's own upload, 256-byte aligned
    const size_t extra_bytes = hooks ? hooks->extra_up_bytes[0] + hooks->extra_up_bytes[1] : 0;
    const size_t up = extra_bytes ? off_extra + extra_bytes : off_valid + (valid ? (size_t)n : 0);
    // ---- device arena: the sequence's arrays, then a hook's own
    const bool guided = seq_guided(c, use_extrinsic_guess);
    // (a call with depth — tracking, whose after_upload hook leaves the camera-frame points — may estimate by alignment)
    const double align_distance = hooks && hooks->after_upload ? seq_align_distance(c) : 0.0;
    const size_t o_extra = seq_arena_bytes(n_cand, S, iterations, false, guided, n, align_distance > 0);
    // ---- result block (mapped): [best, pad | RelocRes[64] | pair_from P x S | pair_to P x S | inliers P x S]
    const size_t res_head = 16 + kRelocMaxCand * sizeof(RelocRes);
    const size_t res_extra = (res_head + (want_pairs ? PS * 9 : 0) + 15) & ~(size_t)15; // a hook's own results
    const size_t res = hooks && hooks->extra_res_bytes ? res_extra + hooks->extra_res_bytes : res_head + (want_pairs ? PS * 9 : 0);
    rc = reloc_scratch(c, up, o_extra + al256(hooks ? hooks->extra_arena_bytes : 0), res);
    if(rc)
        return rc;

    std::memcpy(r->h_up, desc, (size_t)n * 32);
    std::memcpy(r->h_up + off_xy, xy, (size_t)n * 8);
    std::memcpy(r->h_up + off_slots, slots, P * 4);
    if(valid)
        std::memcpy(r->h_up + off_valid, valid, (size_t)n);
    for(int k = 0; hooks && k < 2; ++k) // straight from the caller's buffers into the staging block
        if(hooks->extra_up_bytes[k])
            std::memcpy(r->h_up + off_extra + (k ? hooks->extra_up_bytes[0] : 0), hooks->extra_up[k], hooks->extra_up_bytes[k]);
    reinterpret_cast<int32_t*>(r->h_res.get())[0] = -2; // (overwritten by k_reloc_rank; checked after the synchronisation)
    hipStream_t s = c->stream;
    MSLAM_CHK(c, hipMemcpyAsync(r->d_up, r->h_up, up, hipMemcpyHostToDevice, s));
    // every candidate's train side is the one uploaded query block
    SeqArgs a{};
    a.rows = n_cand, a.S = S;
    a.desc = r->d_up, a.xy = reinterpret_cast<const float*>(r->d_up + off_xy), a.valid = valid ? r->d_up + off_valid : nullptr;
    a.n_from_fixed = a.cap_from = n;
    a.slots = reinterpret_cast<const int32_t*>(r->d_up + off_slots);
    a.fx = fx, a.fy = fy, a.cx = cx, a.cy = cy;
    a.use_guess = use_extrinsic_guess, a.rvec = rvec, a.tvec = tvec;
    a.iterations = iterations, a.reprojection_error = reprojection_error, a.seed = seed;
    a.guided = guided;
    RelocDev dev{};
    if(hooks)
    {
        dev.desc = a.desc, dev.xy = a.xy, dev.n = n, dev.valid = a.valid;
        dev.extra_up = r->d_up + off_extra, dev.extra_arena = r->d_arena + o_extra;
        dev.extra_res = r->h_res.dev() + res_extra, dev.h_extra_res = r->h_res + res_extra;
        if(hooks->after_upload)
        {
            rc = hooks->after_upload(c, hooks->user, dev);
            if(rc)
                return rc;
            a.valid = dev.valid;
            a.cam_xyz = dev.cam_xyz, a.align_distance = dev.cam_xyz ? align_distance : 0.0;
        }
    }
    rc = seq_enqueue(c, a, r->d_arena, &dev.seq);
    if(rc)
        return rc;
    {
        StageScope ts(c, "reloc_rank");
        hipLaunchKernelGGL(k_reloc_rank, dim3(want_pairs ? 1u + (unsigned)P : 1u), dim3(256), 0, s, dev.seq.mcount, dev.seq.ncorr,
                           dev.seq.pnp_out, n_cand, min_inliers, (int)S, dev.seq.mfrom, dev.seq.mto, dev.seq.mask, r->h_res.dev());
    }
    MSLAM_CHK(c, hipGetLastError());
    if(hooks && hooks->before_sync)
    {
        rc = hooks->before_sync(c, hooks->user, dev);
        if(rc)
            return rc;
    }
    MSLAM_CHK(c, hipStreamSynchronize(s));

    const int32_t b = reinterpret_cast<const int32_t*>(r->h_res.get())[0];
    if(b < -1 || b >= n_cand)
        return fail(c, MSLAM_HIP_E_RUNTIME, "relocalize: the ranking kernel left no result");
    const RelocRes* rr = reinterpret_cast<const RelocRes*>(r->h_res + 16);
    bool fits = true;
    for(int k = 0; k < n_cand; ++k)
    {
        // (counts from mapped memory size the copies below: never trust them blindly)
        if(rr[k].n_matches < 0 || (size_t)rr[k].n_matches > S || rr[k].n_corr < 0 || rr[k].n_corr > rr[k].n_matches)
            return fail(c, MSLAM_HIP_E_RUNTIME, "relocalize: the kernels reported impossible counts");
        out[k].n_matches = rr[k].n_matches;
        out[k].n_correspondences = rr[k].n_corr;
        out[k].n_inliers = rr[k].n_inliers;
        out[k].status = rr[k].status;
        if(rr[k].status)
        {
            pnp_rotation_to_rvec(rr[k].R, out[k].rvec);
            out[k].tvec[0] = rr[k].t[0], out[k].tvec[1] = rr[k].t[1], out[k].tvec[2] = rr[k].t[2];
        }
        if(want_pairs && rr[k].n_matches > pair_stride)
            fits = false;
    }
    if(want_pairs && !fits)
        return fail(c, MSLAM_HIP_E_CAPACITY, "relocalize: a candidate has more matches than pair_stride");
    if(want_pairs)
    {
        const int32_t* h_from = reinterpret_cast<const int32_t*>(r->h_res + res_head);
        const int32_t* h_to = h_from + PS;
        const uint8_t* h_mask = reinterpret_cast<const uint8_t*>(h_to + PS);
        for(int k = 0; k < n_cand; ++k)
        {
            const size_t src = (size_t)k * S, dst = (size_t)k * (size_t)pair_stride;
            if(pair_from)
                std::memcpy(pair_from + dst, h_from + src, (size_t)rr[k].n_matches * 4);
            if(pair_to)
                std::memcpy(pair_to + dst, h_to + src, (size_t)rr[k].n_matches * 4);
            if(inliers)
                std::memcpy(inliers + dst, h_mask + src, (size_t)rr[k].n_corr);
        }
    }
    *best = b;
    if(b < 0)
        return fail(c, MSLAM_HIP_E_NO_MODEL, "relocalize: no candidate reached min_inliers");
    return MSLAM_HIP_OK;
}

extern "C" int mslam_hip_relocalize(mslam_hip_ctx* c, const uint8_t* desc, const float* xy, const uint8_t* valid, int n,
                                    const int32_t* cand_ids, int n_cand, double fx, double fy, double cx, double cy, double ratio,
                                    int iterations, double reprojection_error, uint64_t seed, int use_extrinsic_guess,
                                    const double* rvec, const double* tvec, int min_inliers, mslam_hip_reloc_candidate* out,
                                    int* best, int32_t* pair_from, int32_t* pair_to, uint8_t* inliers, int pair_stride)
{
    return reloc_run(c, desc, xy, valid, n, cand_ids, n_cand, fx, fy, cx, cy, ratio, iterations, reprojection_error, seed,
                     use_extrinsic_guess, rvec, tvec, min_inliers, out, best, pair_from, pair_to, inliers, pair_stride, nullptr);
}
