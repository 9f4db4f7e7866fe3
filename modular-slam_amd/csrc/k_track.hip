// k_track.hip — the keyframe tracking step against the keyframe store: RgbdFeatureFrontend::track
// (reference rgbd_feature_frontend.cpp:279-400) in one call, and findBetterReferenceKeyframe's count (:544-575 with
// isVisibleInFrame / projectOnImage, projection.cpp:42-62) on its own.
//
// The depth filter is k_backproject on the uploaded depth frame (k_points.hip); matching, ratio test, correspondences and
// PnP are mslam_hip_relocalize's sequence for one candidate (reloc_run, k_reloc.hip), unchanged.  New here: the vote over
// the stored world points and the construction of the new keyframe's entry in its store slot.  Both kernels read the PnP
// kernel's own record on the device (16 doubles: R, t, inliers, -, status, -) and leave at once when the step failed; the
// pose never visits the host between PnP and them.  All arithmetic is f64, every operation rounded on its own
// (-ffp-contract=off), in the order written.
#include "track_kernels.hpp"

#include <algorithm>
#include <cstring>
#include <string>

namespace mslam
{

// One workgroup per listed keyframe (track_vote_block).
__global__ __launch_bounds__(256) void k_track_vote(const double* __restrict__ store_world, const int32_t* __restrict__ store_n,
                                                    const int32_t* __restrict__ slots, int K, const double* __restrict__ rec,
                                                    const int32_t* __restrict__ ncorr, int min_matched, VoteCam cam,
                                                    int32_t* __restrict__ counts)
{
    track_vote_block(store_world, store_n, slots[blockIdx.x], K, rec, ncorr, min_matched, cam, counts + blockIdx.x);
}

// One wave: the first maximum in list order (max-butterfly on (count + 1) << 6 | 63 - k, as k_reloc_rank), and the
// counts; everything lands in mapped host memory.
__global__ __launch_bounds__(64) void k_track_vote_pick(const int32_t* __restrict__ counts, int n_vote, int32_t* __restrict__ h_best,
                                                        int32_t* __restrict__ h_counts)
{
    const int k = threadIdx.x;
    const bool live = k < n_vote;
    const int cnt = live ? counts[k] : 0;
    if(live)
        h_counts[k] = cnt;
    int key = live ? ((cnt + 1) << 6) | (63 - k) : 0;
    for(int o = 32; o > 0; o >>= 1)
        key = max(key, __shfl_xor(key, o));
    if(k == 0)
    {
        h_best[0] = key ? 63 - (key & 63) : -1;
        h_best[1] = key ? (key >> 6) - 1 : 0;
    }
}

// One workgroup builds the new keyframe's entry in its store slot (track_keyframe_block).
__global__ __launch_bounds__(256) void k_track_keyframe(KeyframeArgs a)
{
    track_keyframe_block(a);
}

} // namespace mslam

using namespace mslam;

static VoteCam vote_cam(double fx, double fy, double cx, double cy, int width, int height)
{
    return VoteCam{fx, fy, cx, cy, (double)(float)width, (double)(float)height};
}

namespace
{
// one mslam_hip_track call: what its two hooks into the relocalize sequence need
struct TrackCall
{
    const uint16_t* depth;
    int width, height;
    float factor;
    double fx, fy, cx, cy;
    int n, n_vote, ref_slot, new_slot;
    int min_matched, kf_min_landmarks;
    double z_max;
    int64_t lid_base;
    size_t off_depth;              // in the extra upload block: [vote slots 64 x i32 | depth]
    size_t off_valid, off_counts;  // in the extra arena: [xyz n x 3 f64 | valid n | vote counts 64 x i32]
    double* d_xyz = nullptr;
    const uint8_t* d_valid = nullptr;
    uint8_t* h_res = nullptr;      // host address of the extra result block, once the kernels are enqueued
};

int track_after_upload(mslam_hip_ctx* c, void* user, RelocDev& d)
{
    TrackCall* t = static_cast<TrackCall*>(user);
    t->d_xyz = reinterpret_cast<double*>(d.extra_arena);
    uint8_t* valid = d.extra_arena + t->off_valid;
    {
        StageScope ts(c, "backproject");
        launch_backproject(c->stream, reinterpret_cast<const uint16_t*>(d.extra_up + t->off_depth), t->width, t->height, t->factor,
                           t->fx, t->fy, t->cx, t->cy, d.xy, t->n, t->d_xyz, valid);
    }
    MSLAM_CHK(c, hipGetLastError());
    d.valid = t->d_valid = valid; // the depth filter of :317-334 is the matcher's mask
    d.cam_xyz = t->d_xyz;         // ... and its points are the alignment's destinations (mslam_hip_set_track_pose)
    return MSLAM_HIP_OK;
}

int track_before_sync(mslam_hip_ctx* c, void* user, const RelocDev& d)
{
    TrackCall* t = static_cast<TrackCall*>(user);
    RelocState* r = c->reloc;
    const int K = c->p.max_keypoints;
    TrackRes* res = reinterpret_cast<TrackRes*>(d.extra_res);
    int32_t* res_counts = reinterpret_cast<int32_t*>(d.extra_res + sizeof(TrackRes));
    // (host stores into the mapped block before the kernels that may overwrite it are enqueued)
    TrackRes* h = reinterpret_cast<TrackRes*>(d.h_extra_res);
    *h = TrackRes{0, 0, -1, 0};
    std::memset(d.h_extra_res + sizeof(TrackRes), 0, kRelocMaxCand * 4);
    if(t->n_vote > 0)
    {
        int32_t* counts = reinterpret_cast<int32_t*>(d.extra_arena + t->off_counts);
        {
            StageScope ts(c, "track_vote");
            hipLaunchKernelGGL(k_track_vote, dim3((unsigned)t->n_vote), dim3(256), 0, c->stream, r->d_world, r->d_n,
                               reinterpret_cast<const int32_t*>(d.extra_up), K, d.seq.pnp_out, d.seq.ncorr, t->min_matched,
                               vote_cam(t->fx, t->fy, t->cx, t->cy, t->width, t->height), counts);
        }
        {
            StageScope ts(c, "track_vote_pick");
            hipLaunchKernelGGL(k_track_vote_pick, dim3(1), dim3(64), 0, c->stream, counts, t->n_vote, &res->vote_best, res_counts);
        }
    }
    if(t->new_slot >= 0)
    {
        KeyframeArgs a{};
        a.mfrom = d.seq.mfrom, a.mto = d.seq.mto, a.mcount = d.seq.mcount, a.g_cnt = d.seq.g_cnt, a.ncorr = d.seq.ncorr;
        a.mask = d.seq.mask, a.rec = d.seq.pnp_out;
        a.min_matched = t->min_matched, a.kf_min_landmarks = t->kf_min_landmarks;
        a.desc = d.desc, a.xyz = t->d_xyz, a.valid = t->d_valid, a.nq = t->n, a.S = d.seq.S, a.z_max = t->z_max;
        a.ref_world = r->d_world + (size_t)t->ref_slot * K * 3;
        a.ref_lid = r->d_lid + (size_t)t->ref_slot * K;
        a.out_lid = r->d_lid + (size_t)t->new_slot * K;
        a.lid_base = t->lid_base;
        a.out_desc = r->d_desc + (size_t)t->new_slot * K * 32;
        a.out_world = r->d_world + (size_t)t->new_slot * K * 3;
        a.out_n = r->d_n + t->new_slot;
        a.cap = K;
        a.h_res = res;
        a.h_src = res_counts + kRelocMaxCand;
        a.h_kp = a.h_src + K;
        StageScope ts(c, "track_keyframe");
        hipLaunchKernelGGL(k_track_keyframe, dim3(1), dim3(256), 0, c->stream, a);
    }
    MSLAM_CHK(c, hipGetLastError());
    t->h_res = d.h_extra_res;
    return MSLAM_HIP_OK;
}
} // namespace

extern "C" {

int mslam_hip_kf_visible(mslam_hip_ctx* c, const int32_t* ids, int n_ids, const double* R, const double* t, double fx, double fy,
                         double cx, double cy, int width, int height, int32_t* counts, int* best)
{
    int rc = reloc_enter(c);
    if(rc)
        return rc;
    if(best)
        *best = -1;
    if(!best || n_ids < 0 || n_ids > kRelocMaxCand || (n_ids > 0 && (!ids || !counts)) || !R || !t || width <= 0 || height <= 0)
        return fail(c, MSLAM_HIP_E_INVALID, "kf_visible: bad argument (at most 64 ids)");
    RelocState* r = c->reloc;
    // upload block: [slots 64 x i32 | pose record 16 x f64]; counts 64 x i32 in the arena; result [best, best count, pad | counts]
    struct
    {
        int32_t slots[kRelocMaxCand];
        double rec[16];
    } up{};
    for(int k = 0; k < n_ids; ++k)
    {
        rc = store_slot(c, "kf_visible", "id", ids[k], &up.slots[k]);
        if(rc)
            return rc;
    }
    if(n_ids == 0)
        return MSLAM_HIP_OK;
    std::memcpy(up.rec, R, 9 * sizeof(double));
    std::memcpy(up.rec + 9, t, 3 * sizeof(double));
    up.rec[14] = 1.0; // (the PnP record's "model found")
    rc = reloc_scratch(c, sizeof(up), kRelocMaxCand * 4, 16 + kRelocMaxCand * 4);
    if(rc)
        return rc;
    std::memcpy(r->h_up, &up, sizeof(up));
    int32_t* h = reinterpret_cast<int32_t*>(r->h_res.get());
    h[0] = -2; // (overwritten by k_track_vote_pick; checked after the synchronisation)
    hipStream_t s = c->stream;
    MSLAM_CHK(c, hipMemcpyAsync(r->d_up, r->h_up, sizeof(up), hipMemcpyHostToDevice, s));
    int32_t* d_counts = reinterpret_cast<int32_t*>(r->d_arena.get());
    {
        StageScope ts(c, "track_vote");
        hipLaunchKernelGGL(k_track_vote, dim3((unsigned)n_ids), dim3(256), 0, s, r->d_world, r->d_n,
                           reinterpret_cast<const int32_t*>(r->d_up.get()), c->p.max_keypoints,
                           reinterpret_cast<const double*>(r->d_up + sizeof(up.slots)), nullptr, 0,
                           vote_cam(fx, fy, cx, cy, width, height), d_counts);
    }
    {
        StageScope ts(c, "track_vote_pick");
        hipLaunchKernelGGL(k_track_vote_pick, dim3(1), dim3(64), 0, s, d_counts, n_ids, reinterpret_cast<int32_t*>(r->h_res.dev()),
                           reinterpret_cast<int32_t*>(r->h_res.dev() + 16));
    }
    MSLAM_CHK(c, hipGetLastError());
    MSLAM_CHK(c, hipStreamSynchronize(s));
    if(h[0] < 0 || h[0] >= n_ids)
        return fail(c, MSLAM_HIP_E_RUNTIME, "kf_visible: the vote kernel left no result");
    std::memcpy(counts, r->h_res + 16, (size_t)n_ids * 4);
    *best = h[0];
    return MSLAM_HIP_OK;
}

int mslam_hip_track(mslam_hip_ctx* c, const uint8_t* desc, const float* xy, int n, const uint16_t* depth, int width, int height,
                    float factor, double fx, double fy, double cx, double cy, int ref_id, const int32_t* vote_ids, int n_vote,
                    double ratio, int iterations, double reprojection_error, uint64_t seed, int use_extrinsic_guess,
                    const double* rvec, const double* tvec, int min_matched_points, int new_keyframe_min_landmarks, int new_id,
                    double z_max, mslam_hip_track_result* out, int32_t* vote_counts, int32_t* pair_from, int32_t* pair_to,
                    uint8_t* inliers, int pair_stride, int32_t* entry_src, int32_t* entry_kp, int entry_capacity)
{
    int rc = reloc_enter(c);
    if(rc)
        return rc;
    if(out)
    {
        *out = mslam_hip_track_result{};
        out->vote_best = -1;
    }
    if(!out || !depth || width <= 0 || height <= 0 || n < 0 || n_vote < 0 || n_vote > kRelocMaxCand || (n_vote > 0 && !vote_ids) ||
       !(z_max == z_max) || ((entry_src || entry_kp) && entry_capacity < 0))
        return fail(c, MSLAM_HIP_E_INVALID, "track: bad argument (at most 64 vote ids)");
    const int K = c->p.max_keypoints;
    if(n > K)
        return fail(c, MSLAM_HIP_E_CAPACITY, "track: more query keypoints than the context's max_keypoints (a store entry's capacity)");
    RelocState* r = c->reloc;
    TrackSlots slots;
    rc = slots.resolve(c, "track", ref_id, vote_ids, n_vote, new_id);
    if(!rc)
        rc = slots.reserve(c);
    if(rc)
        return rc;
    TrackCall tc{};
    tc.ref_slot = slots.ref_slot, tc.new_slot = slots.new_slot, tc.lid_base = slots.lid_base;
    tc.depth = depth, tc.width = width, tc.height = height, tc.factor = factor;
    tc.fx = fx, tc.fy = fy, tc.cx = cx, tc.cy = cy;
    tc.n = n, tc.n_vote = n_vote;
    tc.min_matched = min_matched_points, tc.kf_min_landmarks = new_keyframe_min_landmarks;
    tc.z_max = z_max;
    // extra upload: [vote slots | depth], copied by reloc_run from these two spans into its page-locked staging block
    const size_t npx = (size_t)width * height;
    tc.off_depth = sizeof(slots.vote_slots);
    tc.off_valid = (size_t)std::max(n, 1) * 24;
    tc.off_counts = al256(tc.off_valid + (size_t)std::max(n, 1));
    RelocHooks hooks{};
    hooks.extra_up[0] = slots.vote_slots, hooks.extra_up_bytes[0] = sizeof(slots.vote_slots);
    hooks.extra_up[1] = depth, hooks.extra_up_bytes[1] = npx * 2;
    hooks.extra_arena_bytes = tc.off_counts + kRelocMaxCand * 4;
    hooks.extra_res_bytes = sizeof(TrackRes) + kRelocMaxCand * 4 + (size_t)K * 8;
    hooks.user = &tc;
    hooks.after_upload = track_after_upload;
    hooks.before_sync = track_before_sync;
    mslam_hip_reloc_candidate cand{};
    int best = -1;
    const int32_t ref_id32 = ref_id;
    rc = reloc_run(c, desc, xy, nullptr, n, &ref_id32, 1, fx, fy, cx, cy, ratio, iterations, reprojection_error, seed,
                   use_extrinsic_guess, rvec, tvec, 0, &cand, &best, pair_from, pair_to, inliers, pair_stride, &hooks);
    if(rc != MSLAM_HIP_OK && rc != MSLAM_HIP_E_NO_MODEL && rc != MSLAM_HIP_E_CAPACITY)
    {
        slots.rollback(c, true); // the sequence failed part-way (reloc_run's message stays)
        return rc;
    }
    out->n_matches = cand.n_matches, out->n_correspondences = cand.n_correspondences;
    out->n_inliers = cand.n_inliers, out->status = cand.status;
    std::memcpy(out->rvec, cand.rvec, sizeof(cand.rvec));
    std::memcpy(out->tvec, cand.tvec, sizeof(cand.tvec));
    if(!tc.h_res)
    {
        // nothing ran (fewer than 2 query keypoints): no matches, not tracked
        slots.rollback(c, false);
        return rc;
    }
    if(cand.status)
        std::memcpy(out->R, reinterpret_cast<const RelocRes*>(r->h_res + 16)[0].R, sizeof(out->R));
    out->tracked = cand.status && cand.n_correspondences >= min_matched_points ? 1 : 0;
    out->keyframe_required = out->tracked && cand.n_inliers < new_keyframe_min_landmarks ? 1 : 0;
    out->keyframe_added = out->keyframe_required && new_id >= 0 ? 1 : 0;
    const TrackRes* tr = reinterpret_cast<const TrackRes*>(tc.h_res);
    const int32_t* h_counts = reinterpret_cast<const int32_t*>(tc.h_res + sizeof(TrackRes));
    if(tr->n_entry < 0 || tr->n_entry > K || tr->n_inherited < 0 || tr->n_inherited > tr->n_entry || tr->vote_best < -1 ||
       tr->vote_best >= std::max(n_vote, 1) || (!out->keyframe_added && tr->n_entry != 0))
    {
        slots.rollback(c, true);
        return fail(c, MSLAM_HIP_E_RUNTIME, "track: the kernels reported impossible counts");
    }
    if(out->keyframe_added)
    {
        out->n_entry = tr->n_entry, out->n_inherited = tr->n_inherited;
        slots.commit(c, tr->n_entry);
    }
    else
        slots.rollback(c, false);
    if(out->tracked && n_vote > 0)
        out->vote_best = tr->vote_best, out->vote_best_count = tr->vote_best_count;
    if(vote_counts && n_vote > 0)
        std::memcpy(vote_counts, h_counts, (size_t)n_vote * 4);
    if(rc == MSLAM_HIP_E_CAPACITY)
        return rc; // (the pair rows; reloc_run left the message)
    if(out->keyframe_added && (entry_src || entry_kp))
    {
        if(out->n_entry > entry_capacity)
            return fail(c, MSLAM_HIP_E_CAPACITY, "track: the new entry has more landmarks than entry_capacity");
        if(entry_src)
            std::memcpy(entry_src, h_counts + kRelocMaxCand, (size_t)out->n_entry * 4);
        if(entry_kp)
            std::memcpy(entry_kp, h_counts + kRelocMaxCand + K, (size_t)out->n_entry * 4);
    }
    if(!out->tracked)
        return fail(c, MSLAM_HIP_E_NO_MODEL, "track: fewer than min_matched_points correspondences, or no model");
    return MSLAM_HIP_OK;
}

} // extern "C"
