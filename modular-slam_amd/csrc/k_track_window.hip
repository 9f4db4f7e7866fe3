// k_track_window.hip — the keyframe tracking step for a window of S frames against ONE store entry in one call:
// mslam_hip_track_window (host arrays) and mslam_hip_track_window_dev (frames of the last detect + back-project batch).
//
// Between two events of the front end's loop (a new keyframe, a change of the reference keyframe, a tracking failure)
// consecutive frames are matched against the same landmarks and do not depend on each other, so they run as one batch:
//   k_backproject       S depth frames in one launch (host form only; the _dev form reads the points view)
//   k_tw_gather         the reference entry's descriptors, once, into the contiguous block the matcher addresses
//   match_knn2 / ratio  S pairs in one launch: train side = frame s (stride, device count), query side = that block
//   k_tw_corr           per frame: matches with a valid depth -> correspondences (k_reloc_corr's rule and order)
//   k_pnp_ransac_batch  S problems, problem s samples with seed + s, one guess for all
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
    int32_t n_matches, n_corr, n_inliers, status, tracked, required, vote_best, vote_best_count;
    double R[9], t[3];
};

// head of the mapped result block: [WinHead | WinRec[S] | vote counts S x 64 | entry_src K | entry_kp K]
struct WinHead
{
    int32_t first_event, pad;
    TrackRes entry; // n_entry, n_inherited of the keyframe the window made (vote fields unused)
};

// the reference entry's descriptor block, copied once; g_cnt[s] = its landmark count for every pair s
__global__ __launch_bounds__(256) void k_tw_gather(const uint8_t* __restrict__ store_desc, const int32_t* __restrict__ store_n, int slot,
                                                   int K, int Srow, int n_frames, uint8_t* __restrict__ g_desc,
                                                   int32_t* __restrict__ g_cnt)
{
    const int n = min(min(max(store_n[slot], 0), K), Srow);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if(i < n_frames) // n_frames <= 256: block 0
        g_cnt[i] = n;
    if(i < 2 * n)
        reinterpret_cast<uint4*>(g_desc)[i] = reinterpret_cast<const uint4*>(store_desc + (size_t)slot * K * 32)[i];
}

// frame s (one workgroup): its matches whose keypoint has a valid depth become correspondences, in match order — k_reloc_corr
// with the frame's own xy / valid / count and the one reference entry
__global__ __launch_bounds__(256) void k_tw_corr(const int32_t* __restrict__ mfrom, const int32_t* __restrict__ mto,
                                                 const int32_t* __restrict__ mcount, const int32_t* __restrict__ g_cnt,
                                                 const double* __restrict__ world, int Srow, const float* __restrict__ xy_all,
                                                 const uint8_t* __restrict__ valid_all, const int32_t* __restrict__ n_kp,
                                                 long long stride, float* __restrict__ obj, float* __restrict__ img,
                                                 uint8_t* __restrict__ mask, int32_t* __restrict__ n_out)
{
    __shared__ uint32_t wsum[4];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = min(max(mcount[s], 0), Srow), n_to = g_cnt[s];
    const int nq = (int)min((long long)max(n_kp[s], 0), stride);
    const float* xy = xy_all + (size_t)s * stride * 2;
    const uint8_t* valid = valid_all + (size_t)s * stride;
    const size_t row = (size_t)s * Srow;
    uint32_t running = 0;
    for(int base = 0; base < m; base += 256)
    {
        const int i = base + tid;
        int from = 0, to = 0;
        bool ok = false;
        if(i < m)
        {
            from = mfrom[row + i], to = mto[row + i];
            ok = (unsigned)from < (unsigned)nq && (unsigned)to < (unsigned)n_to && valid[from] != 0;
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
            const size_t o = row + running + pre + (uint32_t)__popcll(b & ((1ull << lane) - 1ull)); // < row + m <= row + Srow
            const double* P = world + (size_t)to * 3;
            obj[o * 3] = (float)P[0], obj[o * 3 + 1] = (float)P[1], obj[o * 3 + 2] = (float)P[2];
            img[o * 2] = xy[(size_t)from * 2], img[o * 2 + 1] = xy[(size_t)from * 2 + 1];
        }
        running += tot;
        __syncthreads();
    }
    // fewer than 4 correspondences: the PnP kernel reports "no model" without touching the mask
    if(running < 4 && tid < (int)running)
        mask[row + tid] = 0;
    if(tid == 0)
        n_out[s] = (int32_t)running;
}

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
        const double* o = a.rec + (size_t)s * 16;
        WinRec r{};
        r.n_matches = a.mcount[s];
        r.n_corr = a.ncorr[s];
        r.status = o[14] == 1.0 ? 1 : 0;
        r.n_inliers = r.status ? (int32_t)o[12] : 0;
        for(int j = 0; j < 9; ++j)
            r.R[j] = r.status ? o[j] : 0.0;
        for(int j = 0; j < 3; ++j)
            r.t[j] = r.status ? o[9 + j] : 0.0;
        r.tracked = r.status && r.n_corr >= a.min_matched ? 1 : 0;
        r.required = r.tracked && r.n_inliers < a.kf_min_landmarks ? 1 : 0;
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

#define WCHK(c, call)                                                                                                  \
    do                                                                                                                 \
    {                                                                                                                  \
        hipError_t e_ = (call);                                                                                        \
        if(e_ != hipSuccess)                                                                                           \
        {                                                                                                              \
            (c)->err = std::string(#call) + ": " + hipGetErrorString(e_);                                              \
            return MSLAM_HIP_E_RUNTIME;                                                                                \
        }                                                                                                              \
    } while(0)

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

size_t al256(size_t x)
{
    return (x + 255) & ~(size_t)255;
}

// the relocalize scratch, grown as reloc_run grows it (a call of either kind finds blocks at least as large as it needs)
int grow_scratch(mslam_hip_ctx* c, size_t up, size_t arena, size_t res)
{
    RelocState* r = c->reloc;
    if(up > r->up_bytes)
    {
        WCHK(c, hipStreamSynchronize(c->stream));
        if(r->h_up)
            (void)hipHostFree(r->h_up);
        if(r->d_up)
            (void)hipFree(r->d_up);
        r->h_up = r->d_up = nullptr;
        r->up_bytes = 0;
        WCHK(c, hipHostMalloc(reinterpret_cast<void**>(&r->h_up), up, hipHostMallocDefault));
        WCHK(c, hipMalloc(reinterpret_cast<void**>(&r->d_up), up));
        r->up_bytes = up;
    }
    if(arena > r->arena_bytes)
    {
        WCHK(c, hipStreamSynchronize(c->stream));
        if(r->d_arena)
            (void)hipFree(r->d_arena);
        r->d_arena = nullptr;
        r->arena_bytes = 0;
        WCHK(c, hipMalloc(reinterpret_cast<void**>(&r->d_arena), arena));
        r->arena_bytes = arena;
    }
    if(res > r->res_bytes)
    {
        WCHK(c, hipStreamSynchronize(c->stream));
        if(r->h_res)
            (void)hipHostFree(r->h_res);
        r->h_res = r->d_h_res = nullptr;
        r->res_bytes = 0;
        WCHK(c, hipHostMalloc(reinterpret_cast<void**>(&r->h_res), res, hipHostMallocMapped));
        WCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&r->d_h_res), r->h_res, 0));
        r->res_bytes = res;
    }
    return MSLAM_HIP_OK;
}

// everything between the upload and the synchronisation; a failure in here leaves work enqueued (the caller waits for it)
int window_enqueue(mslam_hip_ctx* c, const WindowSource& w, const WindowParams& p, int ref_slot, int new_slot, int64_t lid_base,
                   const int32_t* vote_slots, WinHead** h_head)
{
    RelocState* r = c->reloc;
    const int K = c->p.max_keypoints, S = w.S;
    const bool host = w.d_desc == nullptr;
    const size_t stride = (size_t)w.stride, st1 = std::max(stride, (size_t)1);
    const size_t Srow = ((size_t)std::max(r->n_upper[(size_t)ref_slot], 1) + 255) & ~(size_t)255, PS = (size_t)S * Srow;
    const size_t npx = (size_t)w.width * w.height;
    // ---- upload block: [vote slots 64 x i32 | n S x i32 | desc S x stride x 32 | xy S x stride x 8 | depth S x h x w x 2]
    const size_t u_n = al256(kRelocMaxCand * 4), u_desc = u_n + al256((size_t)S * 4);
    const size_t u_xy = host ? u_desc + al256((size_t)S * st1 * 32) : u_desc;
    const size_t u_depth = host ? u_xy + al256((size_t)S * st1 * 8) : u_desc;
    const size_t up = host ? u_depth + al256((size_t)S * npx * 2) : u_desc;
    // ---- device arena
    size_t off = 0;
    auto carve = [&](size_t bytes) {
        const size_t o = off;
        off += al256(bytes);
        return o;
    };
    const size_t o_gdesc = carve(Srow * 32), o_gcnt = carve((size_t)S * 4), o_idx0 = carve(PS * 4), o_idx1 = carve(PS * 4),
                 o_dist0 = carve(PS * 4), o_dist1 = carve(PS * 4), o_mfrom = carve(PS * 4), o_mto = carve(PS * 4),
                 o_mcount = carve((size_t)S * 4), o_obj = carve(PS * 12), o_img = carve(PS * 8), o_ncorr = carve((size_t)S * 4),
                 o_mask = carve(PS), o_hyp = carve((size_t)S * p.iterations * 96), o_counts = carve((size_t)S * p.iterations * 4),
                 o_out = carve((size_t)S * 128), o_xyz = carve(host ? (size_t)S * st1 * 24 : 0),
                 o_valid = carve(host ? (size_t)S * st1 : 0), o_vote = carve((size_t)S * kRelocMaxCand * 4), o_event = carve(4);
    // ---- mapped result block
    const size_t r_rec = sizeof(WinHead), r_counts = r_rec + (size_t)S * sizeof(WinRec),
                 r_src = r_counts + (size_t)S * kRelocMaxCand * 4, res = r_src + (size_t)K * 8;
    int rc = grow_scratch(c, up, off, res);
    if(rc)
        return rc;

    std::memset(r->h_up, 0, kRelocMaxCand * 4);
    std::memcpy(r->h_up, vote_slots, (size_t)p.n_vote * 4);
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
    WinHead* hh = reinterpret_cast<WinHead*>(r->h_res);
    *hh = WinHead{-2, 0, TrackRes{0, 0, -1, 0}}; // (first_event is overwritten by k_tw_scan; checked after the synchronisation)
    hipStream_t s = c->stream;
    WCHK(c, hipMemcpyAsync(r->d_up, r->h_up, up, hipMemcpyHostToDevice, s));
    uint8_t* A = r->d_arena;
    const int32_t* d_slots = reinterpret_cast<const int32_t*>(r->d_up);
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
    int32_t* g_cnt = reinterpret_cast<int32_t*>(A + o_gcnt);
    {
        StageScope ts(c, "track_window_gather");
        hipLaunchKernelGGL(k_tw_gather, dim3((unsigned)((2 * Srow + 255) / 256)), dim3(256), 0, s, r->d_desc, r->d_n, ref_slot, K, (int)Srow,
                           S, A + o_gdesc, g_cnt);
    }
    // match(from = keypoints of frame s, to = landmarks of the reference entry): knn-2 with query = `to` and train = `from`
    MatchArgs m{};
    m.from_desc = d_desc;
    m.from_stride = (long long)stride * 32;
    m.from_cnt = d_n;
    m.n_from_fixed = 0;
    m.to_desc = A + o_gdesc;
    m.to_stride = 0; // every pair's query side is the one gathered entry
    m.to_cnt = g_cnt;
    m.cap = (int)Srow;
    m.cap_from = w.cap_from;
    m.popcount_only = c->matcher_kind == MSLAM_HIP_MATCHER_POPCOUNT;
    m.idx0 = reinterpret_cast<int32_t*>(A + o_idx0);
    m.idx1 = reinterpret_cast<int32_t*>(A + o_idx1);
    m.dist0 = reinterpret_cast<int32_t*>(A + o_dist0);
    m.dist1 = reinterpret_cast<int32_t*>(A + o_dist1);
    {
        StageScope ts(c, "match_knn2");
        c->last_match_kernel = launch_match_knn2(m, S, s);
    }
    RatioArgs q{};
    q.idx0 = m.idx0, q.dist0 = m.dist0, q.dist1 = m.dist1;
    q.from_cnt = d_n, q.n_from_fixed = 0;
    q.to_cnt = g_cnt;
    q.cap = (int)Srow;
    q.thr = c->d_ratio_thr;
    q.from_idx = reinterpret_cast<int32_t*>(A + o_mfrom);
    q.to_idx = reinterpret_cast<int32_t*>(A + o_mto);
    q.n_out = reinterpret_cast<int32_t*>(A + o_mcount);
    {
        StageScope ts(c, "ratio_compact");
        launch_ratio_compact(q, S, s);
    }
    float* d_obj = reinterpret_cast<float*>(A + o_obj);
    float* d_img = reinterpret_cast<float*>(A + o_img);
    int32_t* d_ncorr = reinterpret_cast<int32_t*>(A + o_ncorr);
    uint8_t* d_mask = A + o_mask;
    const double* ref_world = r->d_world + (size_t)ref_slot * K * 3;
    {
        StageScope ts(c, "track_window_corr");
        hipLaunchKernelGGL(k_tw_corr, dim3((unsigned)S), dim3(256), 0, s, q.from_idx, q.to_idx, q.n_out, g_cnt, ref_world, (int)Srow, d_xy,
                           d_valid, d_n, (long long)stride, d_obj, d_img, d_mask, d_ncorr);
    }
    WCHK(c, hipGetLastError());
    PnpBatchLaunch l{};
    l.obj = d_obj, l.img = d_img, l.n = d_ncorr;
    l.n_problems = S, l.cap = (int)Srow;
    l.fx = p.fx, l.fy = p.fy, l.cx = p.cx, l.cy = p.cy;
    l.use_guess = p.use_guess ? 1 : 0;
    for(int j = 0; j < 3; ++j)
    {
        l.rvec[j] = p.use_guess ? p.rvec[j] : 0.0;
        l.tvec[j] = p.use_guess ? p.tvec[j] : 0.0;
    }
    l.iterations = p.iterations;
    l.reprojection_error = p.reprojection_error;
    l.seed = p.seed; // problem s samples with seed + s
    l.hyp = reinterpret_cast<double*>(A + o_hyp);
    l.counts = reinterpret_cast<int32_t*>(A + o_counts);
    l.mask = d_mask;
    l.out = reinterpret_cast<double*>(A + o_out);
    rc = pnp_launch_batch(c, l);
    if(rc)
        return rc;
    int32_t* d_vote = reinterpret_cast<int32_t*>(A + o_vote);
    if(p.n_vote > 0)
    {
        StageScope ts(c, "track_window_vote");
        const VoteCam cam{p.fx, p.fy, p.cx, p.cy, (double)(float)w.width, (double)(float)w.height};
        hipLaunchKernelGGL(k_tw_vote, dim3((unsigned)p.n_vote, (unsigned)S), dim3(256), 0, s, r->d_world, r->d_n, d_slots, K, l.out, d_ncorr,
                           p.min_matched, cam, d_vote);
    }
    int32_t* d_event = reinterpret_cast<int32_t*>(A + o_event);
    {
        ScanArgs a{};
        a.mcount = q.n_out, a.ncorr = d_ncorr, a.counts = d_vote, a.rec = l.out;
        a.n_frames = S, a.n_vote = p.n_vote, a.ref_vote_pos = p.ref_vote_pos;
        a.min_matched = p.min_matched, a.kf_min_landmarks = p.kf_min_landmarks;
        a.d_event = d_event;
        a.h_head = reinterpret_cast<WinHead*>(r->d_h_res);
        a.h_rec = reinterpret_cast<WinRec*>(r->d_h_res + r_rec);
        a.h_counts = reinterpret_cast<int32_t*>(r->d_h_res + r_counts);
        StageScope ts(c, "track_window_scan");
        hipLaunchKernelGGL(k_tw_scan, dim3(1), dim3(256), 0, s, a);
    }
    if(new_slot >= 0)
    {
        KeyframeArgs a{};
        a.mfrom = q.from_idx, a.mto = q.to_idx, a.mcount = q.n_out, a.g_cnt = g_cnt, a.ncorr = d_ncorr;
        a.mask = d_mask, a.rec = l.out;
        a.min_matched = p.min_matched, a.kf_min_landmarks = p.kf_min_landmarks;
        a.desc = d_desc, a.xyz = d_xyz, a.valid = d_valid, a.nq = 0, a.S = (int)Srow, a.z_max = p.z_max;
        a.ref_world = ref_world;
        a.ref_lid = r->d_lid + (size_t)ref_slot * K;
        a.out_lid = r->d_lid + (size_t)new_slot * K;
        a.lid_base = lid_base;
        a.out_desc = r->d_desc + (size_t)new_slot * K * 32;
        a.out_world = r->d_world + (size_t)new_slot * K * 3;
        a.out_n = r->d_n + new_slot;
        a.cap = K;
        a.h_res = &reinterpret_cast<WinHead*>(r->d_h_res)->entry;
        a.h_src = reinterpret_cast<int32_t*>(r->d_h_res + r_src);
        a.h_kp = a.h_src + K;
        StageScope ts(c, "track_window_keyframe");
        hipLaunchKernelGGL(k_tw_keyframe, dim3(1), dim3(256), 0, s, a, d_event, d_n, S, (long long)stride);
    }
    WCHK(c, hipGetLastError());
    WCHK(c, hipStreamSynchronize(s));
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
    int32_t vote_slots[kRelocMaxCand] = {0};
    auto ref = r->slot_of.find(p.ref_id);
    if(ref == r->slot_of.end())
        return reloc_fail(c, MSLAM_HIP_E_INVALID, me + ": reference id " + std::to_string(p.ref_id) + " is not in the keyframe store");
    bool collides = p.new_id >= 0 && p.new_id == p.ref_id;
    for(int k = 0; k < p.n_vote; ++k)
    {
        auto it = r->slot_of.find(p.vote_ids[k]);
        if(it == r->slot_of.end())
            return reloc_fail(c, MSLAM_HIP_E_INVALID, me + ": vote id " + std::to_string(p.vote_ids[k]) + " is not in the keyframe store");
        vote_slots[k] = it->second;
        collides = collides || (p.new_id >= 0 && p.vote_ids[k] == p.new_id);
    }
    if(collides)
        return reloc_fail(c, MSLAM_HIP_E_INVALID, me + ": new_id names the reference keyframe or a keyframe of the vote list");
    int rc = mslam_ratio_table(c, p.ratio);
    if(rc)
        return rc;
    const int ref_slot = ref->second;
    // the store grows here, on the host, before anything is enqueued (slots keep their numbers)
    int new_slot = -1;
    int64_t lid_base = 0;
    const bool existed = p.new_id >= 0 && r->slot_of.count(p.new_id) != 0;
    if(p.new_id >= 0)
    {
        rc = store_slot_for(c, p.new_id, &new_slot);
        if(rc)
            return rc;
        lid_base = store_next_lid_base(c); // (the serial advances whether or not the window makes the keyframe)
    }
    auto release = [&]() { // a slot reserved for new_id that received no entry
        if(p.new_id >= 0 && !existed)
        {
            r->slot_of.erase(p.new_id);
            r->free_slots.push_back(new_slot);
        }
    };
    WinHead* head = nullptr;
    rc = window_enqueue(c, w, p, ref_slot, new_slot, lid_base, vote_slots, &head);
    if(rc)
    {
        // what was enqueued may still run and may write the slot: wait for it before the slot goes back to the free list
        const std::string msg = c->err;
        (void)hipStreamSynchronize(c->stream);
        c->err = msg;
        if(existed)
            r->n_upper[(size_t)new_slot] = K;
        release();
        return rc;
    }
    const WinRec* rec = reinterpret_cast<const WinRec*>(r->h_res + sizeof(WinHead));
    const int32_t* h_counts = reinterpret_cast<const int32_t*>(r->h_res + sizeof(WinHead) + (size_t)S * sizeof(WinRec));
    const int32_t* h_src = h_counts + (size_t)S * kRelocMaxCand;
    const size_t Srow = ((size_t)std::max(r->n_upper[(size_t)ref_slot], 1) + 255) & ~(size_t)255;
    const int first = head->first_event;
    const TrackRes tr = head->entry;
    bool sane = first >= 0 && first <= S && tr.n_entry >= 0 && tr.n_entry <= K && tr.n_inherited >= 0 && tr.n_inherited <= tr.n_entry;
    for(int s = 0; sane && s < S; ++s) // (counts from mapped memory: never trust them blindly)
        sane = rec[s].n_matches >= 0 && (size_t)rec[s].n_matches <= Srow && rec[s].n_corr >= 0 && rec[s].n_corr <= rec[s].n_matches &&
               rec[s].vote_best >= -1 && rec[s].vote_best < std::max(p.n_vote, 1);
    const bool added = sane && first < S && rec[first].required && p.new_id >= 0;
    if(!sane || (!added && tr.n_entry != 0))
    {
        if(existed)
            r->n_upper[(size_t)new_slot] = K;
        release();
        return reloc_fail(c, MSLAM_HIP_E_RUNTIME, me + ": the kernels reported impossible counts");
    }
    for(int s = 0; s < S; ++s)
    {
        mslam_hip_track_window_result& o = p.out[s];
        o.n_matches = rec[s].n_matches, o.n_correspondences = rec[s].n_corr;
        o.n_inliers = rec[s].n_inliers, o.status = rec[s].status;
        if(rec[s].status)
        {
            std::memcpy(o.R, rec[s].R, sizeof(o.R));
            std::memcpy(o.tvec, rec[s].t, sizeof(o.tvec));
            pnp_rotation_to_rvec(rec[s].R, o.rvec);
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
        r->n_upper[(size_t)new_slot] = tr.n_entry;
    }
    else
        release();
    if(added && (p.entry_src || p.entry_kp))
    {
        if(tr.n_entry > p.entry_capacity)
            return reloc_fail(c, MSLAM_HIP_E_CAPACITY, me + ": the new entry has more landmarks than entry_capacity");
        if(p.entry_src)
            std::memcpy(p.entry_src, h_src, (size_t)tr.n_entry * 4);
        if(p.entry_kp)
            std::memcpy(p.entry_kp, h_src + K, (size_t)tr.n_entry * 4);
    }
    if(!p.out[0].tracked)
        return reloc_fail(c, MSLAM_HIP_E_NO_MODEL, me + ": frame 0 has fewer than min_matched_points correspondences, or no model");
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
        return reloc_fail(c, MSLAM_HIP_E_INVALID,
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
        return reloc_fail(c, MSLAM_HIP_E_INVALID, "track_window: bad argument");
    rc = window_check(c, who, S, fx, fy, vote_ids, n_vote, ref_vote_pos, iterations, reprojection_error, use_extrinsic_guess, rvec, tvec,
                      z_max, entry_src, entry_kp, entry_capacity);
    if(rc)
        return rc;
    int n_max = 0;
    for(int s = 0; s < S; ++s)
    {
        if(n[s] < 0 || n[s] > stride)
            return reloc_fail(c, MSLAM_HIP_E_INVALID, "track_window: a frame's keypoint count is negative or exceeds stride");
        n_max = std::max(n_max, n[s]);
    }
    if(n_max > c->p.max_keypoints)
        return reloc_fail(c, MSLAM_HIP_E_CAPACITY,
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
        return reloc_fail(c, MSLAM_HIP_E_INVALID, "track_window_dev: bad argument");
    rc = window_check(c, who, n_frames, fx, fy, vote_ids, n_vote, ref_vote_pos, iterations, reprojection_error, use_extrinsic_guess, rvec,
                      tvec, z_max, entry_src, entry_kp, entry_capacity);
    if(rc)
        return rc;
    if(first_frame < 0 || first_frame + n_frames > c->n_last)
        return reloc_fail(c, MSLAM_HIP_E_INVALID, "track_window_dev: no such frames in the last detect batch");
    if(!c->d_xyz || c->points_seq != c->detect_seq)
        return reloc_fail(c, MSLAM_HIP_E_INVALID, "track_window_dev: the last detect batch has not been back-projected");
    const size_t K = (size_t)c->p.max_keypoints, f = (size_t)first_frame;
    WindowSource w{};
    // frame f of the batch: descriptors / coordinates / count in output slot f + 1, points in row f of the back-projection
    w.d_desc = c->d_desc + (f + 1) * K * 32;
    w.d_xy = c->d_xy + (f + 1) * K * 2;
    w.d_n = c->d_count + 1 + f;
    w.d_xyz = c->d_xyz + f * K * 3;
    w.d_valid = c->d_valid + f * K;
    w.stride = (int)K, w.S = n_frames, w.width = c->p.width, w.height = c->p.height, w.cap_from = (int)K;
    WindowParams p{fx, fy, cx, cy, ref_id, vote_ids, n_vote, ref_vote_pos, ratio, iterations, reprojection_error, seed,
                   use_extrinsic_guess, rvec, tvec, min_matched_points, new_keyframe_min_landmarks, new_id, z_max, out, first_event,
                   vote_counts, entry_src, entry_kp, entry_capacity};
    return window_run(c, who, w, p);
}

} // extern "C"
