// k_track_window.hip — the keyframe tracking step for a window of S frames against ONE store entry in one call:
// mslam_hip_track_window (host arrays) and mslam_hip_track_window_dev (frames of the last detect + back-project batch).
//
// Between two events of the front end's loop (a new keyframe, a change of the reference keyframe, a tracking failure)
// consecutive frames are matched against the same landmarks and do not depend on each other, so they run as one batch:
//   k_backproject       S depth frames in one launch (host form only; the _dev form reads the points view)
//   seq_enqueue         mslam_hip_relocalize's own sequence (k_reloc.hip) with S rows on one entry: k_reloc_gather_desc once,
//                       match_knn2 / ratio_compact for S pairs (train side = frame s: stride, device count), k_reloc_corr
//                       per frame on the keypoints with a valid depth, k_pnp_ransac_batch (problem s samples with seed + s)
//   k_tw_vote           (n_vote, S) workgroups, each reading its frame's pose record (track_vote_block)
//   k_tw_scan           one workgroup: per frame the record, the vote's winner and the event flag; the first event of the
//                       window by ballot + a four-entry minimum; everything the host reads lands in mapped memory
//   k_tw_keyframe       reads the event index on the device and builds that frame's entry (track_keyframe_block)
// One upload and one synchronisation per window.  Every per-frame stage runs the code mslam_hip_track runs for that frame
// alone, on the same operands in the same order: the records are equal bit for bit.
#include "track_kernels.hpp"

#include <algorithm>
#include <cstring>
#include <string>

namespace mslam
{

constexpr int kWindowMax = 256; // frames per window: one lane of k_tw_scan's workgroup each

// per frame, in the mapped result block
struct WinRec
{
    RelocRes res;
    int32_t tracked, required, vote_best, vote_best_count;
};

// head of the mapped result block: [WinHead | WinRec[S] | vote counts S x 64 | entry_src K | entry_kp K]
struct WinHead
{
    int32_t first_event, pad;
    TrackRes entry; // n_entry, n_inherited of the keyframe the window made (vote fields unused)
};

// workgroup (k, s): listed keyframe k seen from frame s's pose
__global__ __launch_bounds__(256) void k_tw_vote(const double* __restrict__ store_world, const int32_t* __restrict__ store_n,
                                                 const int32_t* __restrict__ slots, int K, const double* __restrict__ rec,
                                                 const int32_t* __restrict__ ncorr, int min_matched, VoteCam cam,
                                                 int32_t* __restrict__ counts)
{
    const int s = blockIdx.y;
    track_vote_block(store_world, store_n, slots[blockIdx.x], K, rec + (size_t)s * 16, ncorr + s, min_matched, cam,
                     counts + (size_t)s * kRelocMaxCand + blockIdx.x);
}

struct ScanArgs
{
    const int32_t *mcount, *ncorr, *counts; // counts: [S][64]
    const double* rec;                      // [S][16]
    int n_frames, n_vote, ref_vote_pos, min_matched, kf_min_landmarks;
    int32_t* d_event; // device copy of the event index, for k_tw_keyframe
    WinHead* h_head;  // mapped
    WinRec* h_rec;
    int32_t* h_counts; // [S][64]
};

// One workgroup, lane s = frame s (n_frames <= 256).  Per frame: the record, the first maximum of its vote counts, the
// event flag.  The first event: each wave's lowest flagged lane from its ballot, then the minimum of the four.
__global__ __launch_bounds__(256) void k_tw_scan(ScanArgs a)
{
    __shared__ int32_t wfirst[4];
    const int s = threadIdx.x, lane = s & 63, wave = s >> 6;
    bool event = false;
    if(s < a.n_frames)
    {
        WinRec r{};
        r.res = reloc_record(a.rec + (size_t)s * 16, a.mcount[s], a.ncorr[s]);
        r.tracked = r.res.status && r.res.n_corr >= a.min_matched ? 1 : 0;
        r.required = r.tracked && r.res.n_inliers < a.kf_min_landmarks ? 1 : 0;
        r.vote_best = -1, r.vote_best_count = 0;
        int top = -1;
        for(int k = 0; k < a.n_vote; ++k)
        {
            const int cnt = a.counts[(size_t)s * kRelocMaxCand + k]; // (0 when not tracked: k_tw_vote)
            a.h_counts[(size_t)s * kRelocMaxCand + k] = cnt;
            if(r.tracked && cnt > top) // the first maximum in list order
                r.vote_best = k, r.vote_best_count = top = cnt;
        }
        a.h_rec[s] = r;
        event = !r.tracked || r.required || (a.n_vote > 0 && a.ref_vote_pos >= 0 && r.vote_best != a.ref_vote_pos);
    }
    const unsigned long long b = __ballot(event);
    if(lane == 0)
        wfirst[wave] = b ? wave * 64 + (int)__ffsll((long long)b) - 1 : a.n_frames;
    __syncthreads();
    if(s == 0)
    {
        const int first = min(min(wfirst[0], wfirst[1]), min(wfirst[2], wfirst[3]));
        *a.d_event = first;
        a.h_head->first_event = first;
    }
}

// the window's one keyframe: frame d_event[0]'s rows of every per-frame array, then track_keyframe_block — which leaves at
// once unless that frame is tracked and requires a keyframe
__global__ __launch_bounds__(256) void k_tw_keyframe(KeyframeArgs a, const int32_t* __restrict__ d_event,
                                                     const int32_t* __restrict__ n_kp, int n_frames, long long stride)
{
    const int e = d_event[0];
    if(e < 0 || e >= n_frames)
        return; // no event in the window
    const size_t row = (size_t)e * a.S;
    a.mfrom += row, a.mto += row, a.mask += row;
    a.mcount += e, a.g_cnt += e, a.ncorr += e;
    a.rec += (size_t)e * 16;
    a.desc += (size_t)e * stride * 32;
    a.xyz += (size_t)e * stride * 3;
    a.valid += (size_t)e * stride;
    a.nq = (int)min((long long)max(n_kp[e], 0), stride);
    track_keyframe_block(a);
}

} // namespace mslam

using namespace mslam;

namespace
{

// where the frames of one window come from: host arrays (uploaded) or the last detect + back-project batch
struct WindowSource
{
    // host form
    const uint8_t* desc = nullptr;
    const float* xy = nullptr;
    const int32_t* n = nullptr;
    const uint16_t* depth = nullptr;
    float factor = 0.f;
    // _dev form
    const uint8_t* d_desc = nullptr;
    const float* d_xy = nullptr;
    const int32_t* d_n = nullptr;
    const double* d_xyz = nullptr;
    const uint8_t* d_valid = nullptr;
    // both
    int stride = 0, S = 0, width = 0, height = 0, cap_from = 0;
};

struct WindowParams
{
    double fx, fy, cx, cy;
    int ref_id;
    const int32_t* vote_ids;
    int n_vote, ref_vote_pos;
    double ratio;
    int iterations;
    double reprojection_error;
    unsigned long long seed;
    int use_guess;
    const double *rvec, *tvec;
    int min_matched, kf_min_landmarks, new_id;
    double z_max;
    mslam_hip_track_window_result* out;
    int* first_event;
    int32_t *vote_counts, *entry_src, *entry_kp;
    int entry_capacity;
};

// everything between the upload and the synchronisation; a failure in here leaves work enqueued (the caller waits for it)
int window_enqueue(mslam_hip_ctx* c, const WindowSource& w, const WindowParams& p, const TrackSlots& slots, WinHead** h_head)
{
    RelocState* r = c->reloc;
    const int K = c->p.max_keypoints, S = w.S, ref_slot = slots.ref_slot, new_slot = slots.new_slot;
    const bool host = w.d_desc == nullptr;
    const size_t stride = (size_t)w.stride, st1 = std::max(stride, (size_t)1);
    const size_t Srow = seq_row_stride(r->n_upper[(size_t)ref_slot]);
    const size_t npx = (size_t)w.width * w.height;
    // ---- upload block: [vote slots 64 x i32, reference slot | n S x i32 | desc S x stride x 32 | xy S x stride x 8 |
    // depth S x h x w x 2]
    const size_t u_n = al256((kRelocMaxCand + 1) * 4), u_desc = u_n + al256((size_t)S * 4);
    const size_t u_xy = host ? u_desc + al256((size_t)S * st1 * 32) : u_desc;
    const size_t u_depth = host ? u_xy + al256((size_t)S * st1 * 8) : u_desc;
    const size_t up = host ? u_depth + al256((size_t)S * npx * 2) : u_desc;
    // ---- device arena: the sequence's arrays, then the window's own
    const bool guided = seq_guided(c, p.use_guess);
    const double align_distance = seq_align_distance(c);
    size_t off = seq_arena_bytes(S, Srow, p.iterations, true, guided, w.cap_from, align_distance > 0);
    auto carve = [&](size_t bytes) {
        const size_t o = off;
        off += al256(bytes);
        return o;
    };
    const size_t o_xyz = carve(host ? (size_t)S * st1 * 24 : 0), o_valid = carve(host ? (size_t)S * st1 : 0),
                 o_vote = carve((size_t)S * kRelocMaxCand * 4), o_event = carve(4);
    // ---- mapped result block
    const size_t r_rec = sizeof(WinHead), r_counts = r_rec + (size_t)S * sizeof(WinRec),
                 r_src = r_counts + (size_t)S * kRelocMaxCand * 4, res = r_src + (size_t)K * 8;
    int rc = reloc_scratch(c, up, off, res);
    if(rc)
        return rc;

    int32_t* h_slots = reinterpret_cast<int32_t*>(r->h_up.get());
    std::memcpy(h_slots, slots.vote_slots, kRelocMaxCand * 4);
    h_slots[kRelocMaxCand] = ref_slot;
    if(host)
    {
        std::memcpy(r->h_up + u_n, w.n, (size_t)S * 4);
        for(int s = 0; s < S; ++s) // the rows that exist; padding rows are never read
        {
            if(w.n[s] == 0)
                continue;
            std::memcpy(r->h_up + u_desc + (size_t)s * stride * 32, w.desc + (size_t)s * stride * 32, (size_t)w.n[s] * 32);
            std::memcpy(r->h_up + u_xy + (size_t)s * stride * 8, w.xy + (size_t)s * stride * 2, (size_t)w.n[s] * 8);
        }
        std::memcpy(r->h_up + u_depth, w.depth, (size_t)S * npx * 2);
    }
    WinHead* hh = reinterpret_cast<WinHead*>(r->h_res.get());
    *hh = WinHead{-2, 0, TrackRes{0, 0, -1, 0}}; // (first_event is overwritten by k_tw_scan; checked after the synchronisation)
    hipStream_t s = c->stream;
    MSLAM_CHK(c, hipMemcpyAsync(r->d_up, r->h_up, up, hipMemcpyHostToDevice, s));
    uint8_t* A = r->d_arena;
    const int32_t* d_slots = reinterpret_cast<const int32_t*>(r->d_up.get());
    const uint8_t* d_desc = host ? r->d_up + u_desc : w.d_desc;
    const float* d_xy = host ? reinterpret_cast<const float*>(r->d_up + u_xy) : w.d_xy;
    const int32_t* d_n = host ? reinterpret_cast<const int32_t*>(r->d_up + u_n) : w.d_n;
    const double* d_xyz = host ? reinterpret_cast<const double*>(A + o_xyz) : w.d_xyz;
    const uint8_t* d_valid = host ? A + o_valid : w.d_valid;
    if(host && stride > 0)
    {
        StageScope ts(c, "backproject");
        launch_backproject_batch(s, reinterpret_cast<const uint16_t*>(r->d_up + u_depth), w.width, w.height, w.factor, p.fx, p.fy, p.cx,
                                 p.cy, d_xy, d_n, w.stride, S, reinterpret_cast<double*>(A + o_xyz), A + o_valid);
    }
    // every frame's query side is the one reference entry; its train side is the frame (stride, device count), masked by
    // its valid depths
    SeqArgs a{};
    a.rows = S, a.S = Srow;
    a.desc = d_desc, a.xy = d_xy, a.valid = d_valid;
    a.from_stride = stride, a.from_cnt = d_n, a.cap_from = w.cap_from;
    a.slots = d_slots + kRelocMaxCand, a.one_slot = true;
    a.fx = p.fx, a.fy = p.fy, a.cx = p.cx, a.cy = p.cy;
    a.use_guess = p.use_guess, a.rvec = p.rvec, a.tvec = p.tvec;
    a.iterations = p.iterations, a.reprojection_error = p.reprojection_error, a.seed = p.seed;
    a.guided = guided;
    a.cam_xyz = d_xyz, a.align_distance = align_distance;
    SeqDev d{};
    rc = seq_enqueue(c, a, A, &d);
    if(rc)
        return rc;
    int32_t* d_vote = reinterpret_cast<int32_t*>(A + o_vote);
    if(p.n_vote > 0)
    {
        StageScope ts(c, "track_window_vote");
        const VoteCam cam{p.fx, p.fy, p.cx, p.cy, (double)(float)w.width, (double)(float)w.height};
        hipLaunchKernelGGL(k_tw_vote, dim3((unsigned)p.n_vote, (unsigned)S), dim3(256), 0, s, r->d_world, r->d_n, d_slots, K, d.pnp_out,
                           d.ncorr, p.min_matched, cam, d_vote);
    }
    int32_t* d_event = reinterpret_cast<int32_t*>(A + o_event);
    {
        ScanArgs sa{};
        sa.mcount = d.mcount, sa.ncorr = d.ncorr, sa.counts = d_vote, sa.rec = d.pnp_out;
        sa.n_frames = S, sa.n_vote = p.n_vote, sa.ref_vote_pos = p.ref_vote_pos;
        sa.min_matched = p.min_matched, sa.kf_min_landmarks = p.kf_min_landmarks;
        sa.d_event = d_event;
        sa.h_head = reinterpret_cast<WinHead*>(r->h_res.dev());
        sa.h_rec = reinterpret_cast<WinRec*>(r->h_res.dev() + r_rec);
        sa.h_counts = reinterpret_cast<int32_t*>(r->h_res.dev() + r_counts);
        StageScope ts(c, "track_window_scan");
        hipLaunchKernelGGL(k_tw_scan, dim3(1), dim3(256), 0, s, sa);
    }
    if(new_slot >= 0)
    {
        KeyframeArgs ka{};
        ka.mfrom = d.mfrom, ka.mto = d.mto, ka.mcount = d.mcount, ka.g_cnt = d.g_cnt, ka.ncorr = d.ncorr;
        ka.mask = d.mask, ka.rec = d.pnp_out;
        ka.min_matched = p.min_matched, ka.kf_min_landmarks = p.kf_min_landmarks;
        ka.desc = d_desc, ka.xyz = d_xyz, ka.valid = d_valid, ka.nq = 0, ka.S = d.S, ka.z_max = p.z_max;
        ka.ref_world = r->d_world + (size_t)ref_slot * K * 3;
        ka.ref_lid = r->d_lid + (size_t)ref_slot * K;
        ka.out_lid = r->d_lid + (size_t)new_slot * K;
        ka.lid_base = slots.lid_base;
        ka.out_desc = r->d_desc + (size_t)new_slot * K * 32;
        ka.out_world = r->d_world + (size_t)new_slot * K * 3;
        ka.out_n = r->d_n + new_slot;
        ka.cap = K;
        ka.h_res = &reinterpret_cast<WinHead*>(r->h_res.dev())->entry;
        ka.h_src = reinterpret_cast<int32_t*>(r->h_res.dev() + r_src);
        ka.h_kp = ka.h_src + K;
        StageScope ts(c, "track_window_keyframe");
        hipLaunchKernelGGL(k_tw_keyframe, dim3(1), dim3(256), 0, s, ka, d_event, d_n, S, (long long)stride);
    }
    MSLAM_CHK(c, hipGetLastError());
    MSLAM_CHK(c, hipStreamSynchronize(s));
    *h_head = hh;
    return MSLAM_HIP_OK;
}

int window_run(mslam_hip_ctx* c, const char* who, const WindowSource& w, const WindowParams& p)
{
    RelocState* r = c->reloc;
    const int K = c->p.max_keypoints, S = w.S;
    const std::string me = who;
    for(int s = 0; s < S; ++s)
    {
        p.out[s] = mslam_hip_track_window_result{};
        p.out[s].vote_best = -1;
    }
    *p.first_event = S;
    TrackSlots slots;
    int rc = slots.resolve(c, who, p.ref_id, p.vote_ids, p.n_vote, p.new_id);
    if(!rc)
        rc = mslam_ratio_table(c, p.ratio);
    if(!rc)
        rc = slots.reserve(c);
    if(rc)
        return rc;
    WinHead* head = nullptr;
    rc = window_enqueue(c, w, p, slots, &head);
    if(rc)
    {
        slots.rollback(c, true);
        return rc;
    }
    const WinRec* rec = reinterpret_cast<const WinRec*>(r->h_res + sizeof(WinHead));
    const int32_t* h_counts = reinterpret_cast<const int32_t*>(r->h_res + sizeof(WinHead) + (size_t)S * sizeof(WinRec));
    const int32_t* h_src = h_counts + (size_t)S * kRelocMaxCand;
    const size_t Srow = seq_row_stride(r->n_upper[(size_t)slots.ref_slot]);
    const int first = head->first_event;
    const TrackRes tr = head->entry;
    bool sane = first >= 0 && first <= S && tr.n_entry >= 0 && tr.n_entry <= K && tr.n_inherited >= 0 && tr.n_inherited <= tr.n_entry;
    for(int s = 0; sane && s < S; ++s) // (counts from mapped memory: never trust them blindly)
    {
        const RelocRes& q = rec[s].res;
        sane = q.n_matches >= 0 && (size_t)q.n_matches <= Srow && q.n_corr >= 0 && q.n_corr <= q.n_matches &&
               rec[s].vote_best >= -1 && rec[s].vote_best < std::max(p.n_vote, 1);
    }
    const bool added = sane && first < S && rec[first].required && p.new_id >= 0;
    if(!sane || (!added && tr.n_entry != 0))
    {
        slots.rollback(c, true);
        return fail(c, MSLAM_HIP_E_RUNTIME, me + ": the kernels reported impossible counts");
    }
    for(int s = 0; s < S; ++s)
    {
        mslam_hip_track_window_result& o = p.out[s];
        const RelocRes& q = rec[s].res;
        o.n_matches = q.n_matches, o.n_correspondences = q.n_corr;
        o.n_inliers = q.n_inliers, o.status = q.status;
        if(q.status)
        {
            std::memcpy(o.R, q.R, sizeof(o.R));
            std::memcpy(o.tvec, q.t, sizeof(o.tvec));
            pnp_rotation_to_rvec(q.R, o.rvec);
        }
        o.tracked = rec[s].tracked, o.keyframe_required = rec[s].required;
        o.vote_best = rec[s].vote_best, o.vote_best_count = rec[s].vote_best_count;
        if(p.vote_counts && p.n_vote > 0)
            std::memcpy(p.vote_counts + (size_t)s * p.n_vote, h_counts + (size_t)s * kRelocMaxCand, (size_t)p.n_vote * 4);
    }
    *p.first_event = first;
    if(added)
    {
        p.out[first].keyframe_added = 1;
        p.out[first].n_entry = tr.n_entry, p.out[first].n_inherited = tr.n_inherited;
        slots.commit(c, tr.n_entry);
    }
    else
        slots.rollback(c, false);
    if(added && (p.entry_src || p.entry_kp))
    {
        if(tr.n_entry > p.entry_capacity)
            return fail(c, MSLAM_HIP_E_CAPACITY, me + ": the new entry has more landmarks than entry_capacity");
        if(p.entry_src)
            std::memcpy(p.entry_src, h_src, (size_t)tr.n_entry * 4);
        if(p.entry_kp)
            std::memcpy(p.entry_kp, h_src + K, (size_t)tr.n_entry * 4);
    }
    if(!p.out[0].tracked)
        return fail(c, MSLAM_HIP_E_NO_MODEL, me + ": frame 0 has fewer than min_matched_points correspondences, or no model");
    return MSLAM_HIP_OK;
}

// what both forms check the same way; out / first_event are known to be there
int window_check(mslam_hip_ctx* c, const char* who, int S, double fx, double fy, const int32_t* vote_ids, int n_vote, int ref_vote_pos,
                 int iterations, double reprojection_error, int use_guess, const double* rvec, const double* tvec, double z_max,
                 const int32_t* entry_src, const int32_t* entry_kp, int entry_capacity)
{
    if(S < 1 || S > kWindowMax || n_vote < 0 || n_vote > kRelocMaxCand || (n_vote > 0 && !vote_ids) || ref_vote_pos < -1 ||
       ref_vote_pos >= n_vote || iterations < 1 || iterations > 4096 || !(reprojection_error > 0) || !(fx != 0.0) ||
       !(fy != 0.0) || (use_guess && (!rvec || !tvec)) || !(z_max == z_max) || ((entry_src || entry_kp) && entry_capacity < 0))
        return fail(c, MSLAM_HIP_E_INVALID,
                    std::string(who) + ": bad argument (1..256 frames, at most 64 vote ids, ref_vote_pos in [-1, n_vote), 1..4096 iterations)");
    return MSLAM_HIP_OK;
}

} // namespace

extern "C" {

int mslam_hip_track_window(mslam_hip_ctx* c, const uint8_t* desc, const float* xy, const int32_t* n, int stride, const uint16_t* depth,
                           int S, int width, int height, float factor, double fx, double fy, double cx, double cy, int ref_id,
                           const int32_t* vote_ids, int n_vote, int ref_vote_pos, double ratio, int iterations,
                           double reprojection_error, uint64_t seed, int use_extrinsic_guess, const double* rvec, const double* tvec,
                           int min_matched_points, int new_keyframe_min_landmarks, int new_id, double z_max,
                           mslam_hip_track_window_result* out, int* first_event, int32_t* vote_counts, int32_t* entry_src,
                           int32_t* entry_kp, int entry_capacity)
{
    const char* who = "track_window";
    int rc = reloc_enter(c);
    if(rc)
        return rc;
    if(first_event)
        *first_event = 0;
    if(!out || !first_event || !n || !depth || width <= 0 || height <= 0 || stride < 0 || (stride > 0 && (!desc || !xy)))
        return fail(c, MSLAM_HIP_E_INVALID, "track_window: bad argument");
    rc = window_check(c, who, S, fx, fy, vote_ids, n_vote, ref_vote_pos, iterations, reprojection_error, use_extrinsic_guess, rvec, tvec,
                      z_max, entry_src, entry_kp, entry_capacity);
    if(rc)
        return rc;
    int n_max = 0;
    for(int s = 0; s < S; ++s)
    {
        if(n[s] < 0 || n[s] > stride)
            return fail(c, MSLAM_HIP_E_INVALID, "track_window: a frame's keypoint count is negative or exceeds stride");
        n_max = std::max(n_max, n[s]);
    }
    if(n_max > c->p.max_keypoints)
        return fail(c, MSLAM_HIP_E_CAPACITY,
                    "track_window: a frame has more keypoints than the context's max_keypoints (a store entry's capacity)");
    WindowSource w{};
    w.desc = desc, w.xy = xy, w.n = n, w.depth = depth, w.factor = factor;
    w.stride = stride, w.S = S, w.width = width, w.height = height, w.cap_from = n_max;
    WindowParams p{fx, fy, cx, cy, ref_id, vote_ids, n_vote, ref_vote_pos, ratio, iterations, reprojection_error, seed,
                   use_extrinsic_guess, rvec, tvec, min_matched_points, new_keyframe_min_landmarks, new_id, z_max, out, first_event,
                   vote_counts, entry_src, entry_kp, entry_capacity};
    return window_run(c, who, w, p);
}

int mslam_hip_track_window_dev(mslam_hip_ctx* c, int first_frame, int n_frames, double fx, double fy, double cx, double cy, int ref_id,
                               const int32_t* vote_ids, int n_vote, int ref_vote_pos, double ratio, int iterations,
                               double reprojection_error, uint64_t seed, int use_extrinsic_guess, const double* rvec,
                               const double* tvec, int min_matched_points, int new_keyframe_min_landmarks, int new_id, double z_max,
                               mslam_hip_track_window_result* out, int* first_event, int32_t* vote_counts, int32_t* entry_src,
                               int32_t* entry_kp, int entry_capacity)
{
    const char* who = "track_window_dev";
    int rc = reloc_enter(c);
    if(rc)
        return rc;
    if(first_event)
        *first_event = 0;
    if(!out || !first_event)
        return fail(c, MSLAM_HIP_E_INVALID, "track_window_dev: bad argument");
    rc = window_check(c, who, n_frames, fx, fy, vote_ids, n_vote, ref_vote_pos, iterations, reprojection_error, use_extrinsic_guess, rvec,
                      tvec, z_max, entry_src, entry_kp, entry_capacity);
    if(rc)
        return rc;
    if(first_frame < 0 || first_frame + n_frames > c->n_last)
        return fail(c, MSLAM_HIP_E_INVALID, "track_window_dev: no such frames in the last detect batch");
    if(!c->d_xyz || c->points_seq != c->detect_seq)
        return fail(c, MSLAM_HIP_E_INVALID, "track_window_dev: the last detect batch has not been back-projected");
    const size_t K = (size_t)c->p.max_keypoints, f = (size_t)first_frame;
    WindowSource w{};
    // frame f of the batch: descriptors / coordinates / count in output slot f + 1, points in row f of the back-projection
    w.d_desc = cur_out(c).desc + (f + 1) * K * 32;
    w.d_xy = cur_out(c).xy + (f + 1) * K * 2;
    w.d_n = cur_out(c).count + 1 + f;
    w.d_xyz = c->d_xyz + f * K * 3;
    w.d_valid = c->d_valid + f * K;
    w.stride = (int)K, w.S = n_frames, w.width = c->p.width, w.height = c->p.height, w.cap_from = (int)K;
    WindowParams p{fx, fy, cx, cy, ref_id, vote_ids, n_vote, ref_vote_pos, ratio, iterations, reprojection_error, seed,
                   use_extrinsic_guess, rvec, tvec, min_matched_points, new_keyframe_min_landmarks, new_id, z_max, out, first_event,
                   vote_counts, entry_src, entry_kp, entry_capacity};
    return window_run(c, who, w, p);
}

} // extern "C"
