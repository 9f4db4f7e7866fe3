// reloc.hpp — what k_reloc.hip (keyframe store, mslam_hip_relocalize) shares with k_track.hip (mslam_hip_track,
// mslam_hip_kf_visible): the store's state, the one-query-against-N-keyframes sequence with two places where a caller can
// enqueue work of its own, and the launcher of k_backproject.
#pragma once
#include "context.hpp"

#include <string>
#include <unordered_map>
#include <vector>

namespace mslam
{

constexpr int kRelocMaxCand = 64; // the BoW query's own limit (mslam_hip_bow_db_query callers ask for at most 64)

// what k_reloc_rank leaves per candidate in the mapped result block
struct RelocRes
{
    int32_t n_matches, n_corr, n_inliers, status;
    double R[9], t[3];
};

struct RelocState
{
    // ---- keyframe store: slot s holds up to K landmarks at desc + s * K * 32, world + s * K * 3, count n[s]
    int slots = 0;
    uint8_t* d_desc = nullptr;
    double* d_world = nullptr;
    int32_t* d_n = nullptr;
    int64_t* d_lid = nullptr;             // [slots][K] landmark ids: what makes a landmark the same one in two entries
    uint64_t serial = 0;                  // creation serial of the last entry made (the first one is 1): part of its fresh ids
    std::unordered_map<int, int> slot_of; // id -> slot
    std::vector<int> free_slots;
    std::vector<int> n_upper;             // per slot: an upper bound of n the host knows (exact for host adds, K for device lifts)
    // ---- scratch of mslam_hip_relocalize, grown on demand
    uint8_t* h_up = nullptr;  // page-locked staging of the upload: [desc | xy | valid | slots]
    uint8_t* d_up = nullptr;
    size_t up_bytes = 0;
    uint8_t* d_arena = nullptr; // every per-candidate array of one call
    size_t arena_bytes = 0;
    uint8_t *h_res = nullptr, *d_h_res = nullptr; // page-locked, device-mapped: [best | RelocRes[64] | pair_from | pair_to | inliers]
    size_t res_bytes = 0;
    // ---- scratch of mslam_hip_kf_visible: [slots 64 x i32 | pose record 16 x f64 | counts 64 x i32] on the device, the
    // result [best, best count, pad | counts 64 x i32] page-locked and device-mapped
    uint8_t* d_vote = nullptr;
    uint8_t *h_vote = nullptr, *d_h_vote = nullptr;
    // ---- scratch of mslam_hip_kf_union / mslam_hip_kf_covisible (k_localmap.hip), grown on demand: the hash table
    // ({u64 key, u64 val} buckets), the per-block arrays [win masks | counts | offsets], and the mapped result
    // [needed count, pad | covisibility counts 64 x i32]
    uint8_t* d_lm_table = nullptr;
    size_t lm_buckets = 0;
    uint8_t* d_lm_blocks = nullptr;
    size_t lm_blocks = 0;
    uint8_t *h_lm = nullptr, *d_h_lm = nullptr;
};

// A fresh landmark id: (1 << 62) | (serial << 16) | position in the entry.  Entries hold at most 65535 landmarks and the
// serial is known on the host before anything is enqueued, so no device counter is involved.  Caller-supplied ids lie in
// [0, 2^62) and can never collide with these.
constexpr int64_t kFreshLidBit = (int64_t)1 << 62;
inline int64_t fresh_lid_base(uint64_t serial)
{
    return kFreshLidBit | (int64_t)((serial << 16) & (((uint64_t)1 << 62) - 1));
}

struct KfPose
{
    double R[9], t[3], z_max;
};

// Device addresses of one relocalize sequence, for the hooks below.  Rows of the per-candidate arrays are S entries apart.
struct RelocDev
{
    const uint8_t* desc = nullptr; // the uploaded query: n x 32
    const float* xy = nullptr;     // n x 2
    int n = 0, S = 0;
    const uint8_t* valid = nullptr; // the mask k_reloc_corr applies; after_upload may point it at a mask it produces
    const uint8_t* extra_up = nullptr; // the hook's own upload block, on the device
    uint8_t* extra_arena = nullptr;    // the hook's own device scratch
    uint8_t *extra_res = nullptr, *h_extra_res = nullptr; // the hook's own part of the mapped result block (device / host address)
    const int32_t *g_cnt = nullptr, *mfrom = nullptr, *mto = nullptr, *mcount = nullptr, *ncorr = nullptr;
    const uint8_t* mask = nullptr;    // consensus masks, correspondence order
    const double* pnp_out = nullptr;  // 16 doubles per candidate: R, t, inliers, -, status, -
};

// A caller's own work inside the sequence: after_upload runs when the upload is enqueued (before the gather and the
// matcher), before_sync after the ranking kernel and before the call's one synchronisation.  Both enqueue on c->stream and
// return a MSLAM_HIP_* status.
struct RelocHooks
{
    const void* extra_up[2] = {nullptr, nullptr}; // two host spans, copied back to back into the upload block behind the query
    size_t extra_up_bytes[2] = {0, 0};
    size_t extra_arena_bytes = 0, extra_res_bytes = 0;
    void* user = nullptr;
    int (*after_upload)(mslam_hip_ctx*, void* user, RelocDev& d) = nullptr;
    int (*before_sync)(mslam_hip_ctx*, void* user, const RelocDev& d) = nullptr;
};

// mslam_hip_relocalize's body (k_reloc.hip); hooks = nullptr is the plain call
int reloc_run(mslam_hip_ctx* c, const uint8_t* desc, const float* xy, const uint8_t* valid, int n, const int32_t* cand_ids, int n_cand,
              double fx, double fy, double cx, double cy, double ratio, int iterations, double reprojection_error,
              unsigned long long seed, int use_extrinsic_guess, const double* rvec, const double* tvec, int min_inliers,
              mslam_hip_reloc_candidate* out, int* best, int32_t* pair_from, int32_t* pair_to, uint8_t* inliers, int pair_stride,
              const RelocHooks* hooks);
int reloc_enter(mslam_hip_ctx* c);
int reloc_fail(mslam_hip_ctx* c, int code, const std::string& msg);
int store_reserve(mslam_hip_ctx* c, int want);
int store_slot_for(mslam_hip_ctx* c, int id, int* slot);
int64_t store_next_lid_base(mslam_hip_ctx* c); // advances the creation serial: call once per entry made, after store_slot_for

// k_points.hip: k_backproject on one frame of n keypoints, device pointers, enqueued on `s`
void launch_backproject(hipStream_t s, const uint16_t* d_depth, int width, int height, float factor, double fx, double fy, double cx,
                        double cy, const float* d_xy, int n, double* d_xyz, uint8_t* d_valid);
// ... and on n_frames frames in one launch (per-frame device counts, rows `stride` apart)
void launch_backproject_batch(hipStream_t s, const uint16_t* d_depth, int width, int height, float factor, double fx, double fy,
                              double cx, double cy, const float* d_xy, const int32_t* d_n, int stride, int n_frames, double* d_xyz,
                              uint8_t* d_valid);

} // namespace mslam
