// reloc.hpp — what the files on the keyframe store share (k_reloc.hip: the store and mslam_hip_relocalize; k_track.hip,
// k_track_window.hip, k_localmap.hip, k_fuse.hip, k_cull.hip, k_lmcull.hip, k_prune.hip): the store's state and scratch, the lookup of an
// id's slot, the landmark-id table in device scratch, the list rewrite of kf_update_world / kf_replace_ids / kf_fuse, the
// match-to-PnP sequence over R rows that relocalize (one query, R entries) and a tracking window (R frames, one entry) both
// enqueue, relocalize's body with two places where a caller can enqueue work of its own, and the launchers of k_backproject.
#pragma once
#include "context.hpp"
#include "lm_table.hpp"

#include <string>
#include <unordered_map>
#include <vector>

namespace mslam
{

constexpr int kRelocMaxCand = 64; // the BoW query's own limit (mslam_hip_bow_db_query callers ask for at most 64)

// what one row of the sequence comes to, in the mapped result block: per candidate (k_reloc_rank) or per frame (k_tw_scan)
struct RelocRes
{
    int32_t n_matches, n_corr, n_inliers, status;
    double R[9], t[3];
};

// the PnP kernel's record of a row (16 doubles: R, t, inliers, -, status, -) and the row's counts as a RelocRes; inliers,
// R and t are zero when there is no model
__device__ __forceinline__ RelocRes reloc_record(const double* __restrict__ o, int32_t n_matches, int32_t n_corr)
{
    RelocRes r{};
    r.n_matches = n_matches;
    r.n_corr = n_corr;
    r.status = o[14] == 1.0 ? 1 : 0;
    r.n_inliers = r.status ? (int32_t)o[12] : 0;
    for(int j = 0; j < 9; ++j)
        r.R[j] = r.status ? o[j] : 0.0;
    for(int j = 0; j < 3; ++j)
        r.t[j] = r.status ? o[9 + j] : 0.0;
    return r;
}

__device__ __forceinline__ void copy_desc(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst)
{
    const uint4* s = reinterpret_cast<const uint4*>(src);
    uint4* d = reinterpret_cast<uint4*>(dst);
    d[0] = s[0];
    d[1] = s[1];
}

// an entry's landmark count as every kernel on the store reads it: whatever the word holds, no position lies outside the slot
__device__ __forceinline__ int entry_count(const int32_t* __restrict__ store_n, int slot, int K)
{
    return min(max(store_n[slot], 0), K);
}

struct RelocState
{
    // ---- keyframe store: slot s holds up to K landmarks at desc + s * K * 32, world + s * K * 3, count n[s]
    int slots = 0;
    DevBuf<uint8_t> d_desc;
    DevBuf<double> d_world;
    DevBuf<int32_t> d_n;
    DevBuf<int64_t> d_lid;                // [slots][K] landmark ids: what makes a landmark the same one in two entries
    uint64_t serial = 0;                  // creation serial of the last entry made (the first one is 1): part of its fresh ids
    std::unordered_map<int, int> slot_of; // id -> slot
    std::vector<int> free_slots;
    std::vector<int> n_upper;             // per slot: an upper bound of n the host knows (exact for host adds, K for device lifts)
    // ---- scratch of every call that ends in a synchronisation (relocalize, track, track_window, kf_visible), grown on
    // demand by reloc_scratch; the layout inside each block is the call's own
    PinnedBuf<uint8_t> h_up{/*mapped=*/false};     // page-locked staging of the call's one upload
    DevBuf<uint8_t> d_up;                          // as large as h_up
    DevBuf<uint8_t> d_arena;                       // every device array of one call
    PinnedBuf<uint8_t> h_res;                      // mapped: what the host reads after the synchronisation
    // ---- the landmark-id table ({u64 key, u64 val} buckets, lm_table.hpp) of every call that builds one, grown on demand by
    // lm_table_grow: union, covisibility and the list rewrite (k_localmap.hip), the observer counts (k_cull.hip), and the
    // fusion search (k_fuse.hip), which carves [keep table | drop table | replacement table | best] from the one block
    DevBuf<uint8_t> d_lm_table;
    // ---- scratch of mslam_hip_kf_union / mslam_hip_kf_covisible (k_localmap.hip), grown on demand: the per-block arrays
    // [win masks | counts | offsets], and the mapped result [needed count, pad | covisibility counts 64 x i32]
    DevBuf<uint8_t> d_lm_blocks;
    PinnedBuf<uint8_t> h_lm;
    // ---- the observation table of a union in DISTINCTIVE descriptor mode (mslam_hip_set_union_descriptor), grown on demand:
    // [union row][list position] = 1 + the highest position at which that listed entry holds the row's landmark, 0: nowhere
    DevBuf<uint32_t> d_lm_obs;
    // ---- scratch of keyframe culling (k_cull.hip), grown on demand: [observer counts, one u32 per table bucket |
    // first-position stamps, one u32 per bucket | the bucket of every position of one entry, max_keypoints x u32].  Landmark
    // culling (k_lmcull.hip) uses the counts as they are (or as per-bucket hit counts) and the stamps as its judged flags
    DevBuf<uint8_t> d_cull;
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

// One match-to-PnP sequence over `rows` rows: gather the entries' descriptors, knn-2, ratio test, matches ->
// correspondences, batched PnP (problem r samples with seed + r, one guess for all).  Row r matches its keypoints ("from")
// against the landmarks of its store entry ("to").  Addressed as MatchArgs is: a stride of 0 means all rows share the one
// block, a null count array the fixed count.
struct SeqArgs
{
    int rows = 0;
    size_t S = 0; // row stride of every per-row array: seq_row_stride of the largest entry
    // from: device pointers, row r at + r * from_stride keypoints
    const uint8_t* desc = nullptr; // x 32
    const float* xy = nullptr;     // x 2
    const uint8_t* valid = nullptr; // x 1, or nullptr: every keypoint counts
    size_t from_stride = 0;
    const int32_t* from_cnt = nullptr; // [rows], clamped to from_stride
    int n_from_fixed = 0, cap_from = 0; // cap_from: an upper bound of every row's count
    // to: device list of store slots, one per row or (one_slot) one for all rows
    const int32_t* slots = nullptr;
    bool one_slot = false;
    // PnP
    double fx = 0, fy = 0, cx = 0, cy = 0;
    int use_guess = 0;
    const double *rvec = nullptr, *tvec = nullptr; // host, read when use_guess
    int iterations = 0;
    double reprojection_error = 0;
    unsigned long long seed = 0;
    // seq_guided(): the guided stage (k_match_guided.hip) in place of the brute-force matcher, every row projecting with
    // the guess
    bool guided = false;
    // mslam_hip_set_track_pose's ALIGN (align_distance > 0): the rows' poses come from RANSAC rigid alignment (k_align.hip) of
    // (world point of `to`, camera-frame point of `from`) instead of PnP; cam_xyz: x 3 f64, rows from_stride keypoints apart
    const double* cam_xyz = nullptr;
    double align_distance = 0;
};

// the mode of mslam_hip_set_guided_match applies to a call that has a guess: there is no pose to project with otherwise
inline bool seq_guided(const mslam_hip_ctx* c, int use_guess) { return c->guided_radius > 0.0 && use_guess != 0; }
// the setting of mslam_hip_set_track_pose for a tracking call (which has the camera-frame points); 0: PnP
inline double seq_align_distance(const mslam_hip_ctx* c)
{
    return c->track_pose_kind == MSLAM_HIP_TRACK_POSE_ALIGN ? c->track_align_distance : 0.0;
}

// what the sequence leaves on the device; rows of the per-row arrays are S entries apart
struct SeqDev
{
    const int32_t *g_cnt = nullptr, *mfrom = nullptr, *mto = nullptr, *mcount = nullptr, *ncorr = nullptr;
    const uint8_t* mask = nullptr;   // consensus masks, correspondence order
    const double* pnp_out = nullptr; // 16 doubles per row: R, t, inliers, -, status, -
    int S = 0;
};

inline size_t seq_row_stride(int n_upper) // an entry of at most n_upper landmarks, in whole 256-row blocks
{
    return al256((size_t)(n_upper > 1 ? n_upper : 1));
}
// a multiple of 256: a caller's own arrays follow.  guided: with the cell offsets and the keypoint list (cap_from entries of coordinates, index and descriptor) of
// every row behind the sequence's own arrays, which keep their places; align: with the rows' destination points behind those
size_t seq_arena_bytes(int rows, size_t S, int iterations, bool one_slot, bool guided = false, int cap_from = 0, bool align = false);
// enqueues the sequence on c->stream, its arrays carved from `arena`; sets c->last_match_kernel
int seq_enqueue(mslam_hip_ctx* c, const SeqArgs& a, uint8_t* arena, SeqDev* out);

// Device addresses of one relocalize call, for the hooks below.
struct RelocDev
{
    const uint8_t* desc = nullptr; // the uploaded query: n x 32
    const float* xy = nullptr;     // n x 2
    int n = 0;
    const uint8_t* valid = nullptr; // the mask k_reloc_corr applies; after_upload may point it at a mask it produces
    const double* cam_xyz = nullptr; // n x 3 camera-frame points: after_upload of a call that has depth sets it (tracking)
    const uint8_t* extra_up = nullptr; // the hook's own upload block, on the device
    uint8_t* extra_arena = nullptr;    // the hook's own device scratch
    uint8_t *extra_res = nullptr, *h_extra_res = nullptr; // the hook's own part of the mapped result block (device / host address)
    SeqDev seq;                     // filled in when the sequence is enqueued: before_sync reads it
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
// at least `up` bytes of h_up / d_up, `arena` of d_arena, `res` of h_res; growing waits for the stream first
int reloc_scratch(mslam_hip_ctx* c, size_t up, size_t arena, size_t res);
int store_reserve(mslam_hip_ctx* c, int want);
int store_slot_for(mslam_hip_ctx* c, int id, int* slot);
// *slot = the slot of entry `id`, or the failure "<me>: <what> <id> is not in the keyframe store".  The lookup is inline
// (kf_remove_observations asks once per row), the failure is not.
int store_slot_missing(mslam_hip_ctx* c, const std::string& me, const char* what, int id);
inline int store_slot(mslam_hip_ctx* c, const std::string& me, const char* what, int id, int* slot)
{
    const auto it = c->reloc->slot_of.find(id);
    if(it == c->reloc->slot_of.end())
        return store_slot_missing(c, me, what, id);
    *slot = it->second;
    return MSLAM_HIP_OK;
}
// entry `id` leaves the store: its slot goes to the free list, the serial stays.  (Work already enqueued on the slot runs
// before anything a later add enqueues: one stream.)
inline void store_release(RelocState* r, int id, int slot)
{
    r->free_slots.push_back(slot);
    r->slot_of.erase(id);
}
// a caller's list of n landmark ids (and a second list of n, or nullptr): 0 .. 2^24 of them, `present` = the caller's own
// test of its pointers, every id in [0, 2^63)
int lid_list_check(mslam_hip_ctx* c, const std::string& me, int n, bool present, const int64_t* ids, const int64_t* more = nullptr);
// The table of `keys` keys that begins `offset` bytes into d_lm_table, which holds at least `bytes` bytes afterwards
// (bytes = 0: what this table needs; growing waits for the stream first).  b == nullptr: the allocation failed and
// c->err says why.
LmTable lm_table_grow(mslam_hip_ctx* c, size_t keys, size_t bytes = 0, size_t offset = 0);

// The list rewrite (k_localmap.hip): every landmark of the listed live slots whose id is l.from[p] takes l.to[p] (nullptr:
// the ids stay) and the point l.xyz + 3 p (nullptr: the points stay); of a `from` listed twice the later place wins.  All
// device pointers.  The launches cover n places; with n_dev, *n_dev of them count when that fits `cap`, none otherwise.
struct ReplaceList
{
    const int64_t *from, *to;
    const double* xyz;
    const int32_t* n_dev;
    int n, cap;
};
// the live slots in ascending order and the largest count among them
int live_slots(const RelocState* r, std::vector<int32_t>* slots);
// enqueues the two launches under the caller's stage names: the table of l.from in `t` (cleared beforehand), then one thread
// per (slot of d_slots, position below n_max); *d_count, zero beforehand, counts the landmarks that matched
int rewrite_enqueue(mslam_hip_ctx* c, const ReplaceList& l, LmTable t, const int32_t* d_slots, int n_slots, int n_max, uint32_t* d_count,
                    const char* stage_table, const char* stage_write);
// the count comes back: the call's one synchronisation
int rewrite_count(mslam_hip_ctx* c, const uint32_t* d_count, int* n_out);
// kf_update_world and kf_replace_ids after their own checks: a host list of n places (`to`, `xyz`: or nullptr) is uploaded
// with the live slots, rewritten and counted
int rewrite_host_list(mslam_hip_ctx* c, const int64_t* from, const int64_t* to, const double* xyz, int n, const char* stage_table,
                      const char* stage_write, int* n_out);
int64_t store_next_lid_base(mslam_hip_ctx* c); // advances the creation serial: call once per entry made, after store_slot_for

// ---- the observer counts (k_cull.hip), which keyframe culling and landmark culling (k_lmcull.hip) both start with
// the listed entries of one call: their slots and the sum of the sizes the host knows (n_upper)
struct CullMap
{
    std::vector<int32_t> slots;
    size_t keys = 0;
};
// where the count arrays lie in d_cull: [counts buckets x u32 | stamps buckets x u32 | buckets of a candidate's positions K x u32]
struct CullDev
{
    LmTable table;
    uint32_t *counts, *stamp, *bkt;
    size_t buckets;
};
// ids[0, n_ids): 1..MSLAM_HIP_CULL_MAX_ENTRIES distinct ids of the store; pos_of: id -> position in the list
int cull_resolve(mslam_hip_ctx* c, const std::string& me, const int32_t* ids, int n_ids, CullMap* m, std::unordered_map<int, int>* pos_of);
// cand[0, n_cand): distinct, each one of the listed ids -> their slots
int cull_cand_slots(mslam_hip_ctx* c, const std::string& me, const CullMap& m, const std::unordered_map<int, int>& pos_of,
                    const int32_t* cand, int n_cand, std::vector<int32_t>* cand_slots);
// the table of `keys` keys and the arrays behind it
int cull_scratch(mslam_hip_ctx* c, size_t keys, CullDev* d);
// the clears and the 2 x ceil(n_ids / 64) launches that leave the observer count of every bucket (the stamps: all-ones);
// d_slots: the uploaded list
int cull_count_enqueue(mslam_hip_ctx* c, const CullMap& m, const int32_t* d_slots, const CullDev& d);

// The store slots of one tracking call (mslam_hip_track, mslam_hip_track_window[_dev]).  resolve() looks the reference and the vote list up and rejects a
// new_id that names one of them; reserve() then takes new_id's slot (its own when the id exists: the entry is replaced)
// and the landmark id base — on the host, before anything is enqueued; slots keep their numbers, and the serial advances
// whether or not the call makes the keyframe.  Every path after reserve() ends in commit() or rollback().
struct TrackSlots
{
    int ref_slot = -1, new_slot = -1; // new_slot = -1: the call makes no keyframe (new_id < 0)
    int64_t lid_base = 0;
    int32_t vote_slots[kRelocMaxCand] = {};
    int new_id = -1;
    bool existed = false; // new_id named an entry before the call

    int resolve(mslam_hip_ctx* c, const char* who, int ref_id, const int32_t* vote_ids, int n_vote, int new_id_);
    int reserve(mslam_hip_ctx* c);
    // the keyframe was made: the host knows its size
    void commit(mslam_hip_ctx* c, int n_entry);
    // no keyframe: the slot goes back to the free list unless its id existed before.  enqueued_work_may_still_run: wait for
    // the stream first (keeping c->err) — what was enqueued may write the slot, and of an entry that may have been
    // replaced all the host still knows is the capacity (also passed after a synchronisation that found impossible
    // counts: the wait is then idle, the size just as unknown)
    void rollback(mslam_hip_ctx* c, bool enqueued_work_may_still_run);
};

// k_points.hip: k_backproject on one frame of n keypoints, device pointers, enqueued on `s`
void launch_backproject(hipStream_t s, const uint16_t* d_depth, int width, int height, float factor, double fx, double fy, double cx,
                        double cy, const float* d_xy, int n, double* d_xyz, uint8_t* d_valid);
// ... and on n_frames frames in one launch (per-frame device counts, rows `stride` apart)
void launch_backproject_batch(hipStream_t s, const uint16_t* d_depth, int width, int height, float factor, double fx, double fy,
                              double cx, double cy, const float* d_xy, const int32_t* d_n, int stride, int n_frames, double* d_xyz,
                              uint8_t* d_valid);

} // namespace mslam
