// context.hpp — the object behind mslam_hip_ctx: host-built tables, device buffers, stream.
#pragma once
#include "common.hpp"
#include "devmem.hpp"
#include "../../include/mslam_hip.h"
#include <array>
#include <string>
#include <vector>

namespace mslam
{
struct BowState; // k_bow.hip
void bow_destroy(BowState*);
struct RelocState; // k_reloc.hip: keyframe store + scratch of mslam_hip_relocalize
void reloc_destroy(RelocState*);
struct TsdfState; // tsdf.hpp / k_tsdf.hip: the dense map of mslam_hip_tsdf_*
void tsdf_destroy(TsdfState*);
struct IcpState; // icp.hpp / k_icp.hip: the scratch of mslam_hip_icp_* and mslam_hip_tsdf_icp*
void icp_destroy(IcpState*);
void set_blur_taps(const int* taps);
void build_blur_waves(const Geometry& g, int first_level, std::vector<BlurWave>& out);

struct StageTimer
{
    const char* name;
    hipEvent_t start, stop;
};
} // namespace mslam

// One set of per-batch output buffers.  Two sets alternate so that the matcher of batch i (on its own
// stream) can run while the detector of batch i+1 fills the other set.
struct mslam_out_set
{
    // slot 0 = last frame of the previous batch, slots 1..max_batch = current batch
    mslam::DevBuf<float> xy;
    mslam::DevBuf<uint8_t> desc;
    mslam::DevBuf<int32_t> octave;
    mslam::DevBuf<float> angle, response;
    mslam::DevBuf<int32_t> count;
    mslam::DevBuf<int32_t> idx0, idx1, dist0, dist1; // matcher
    mslam::DevBuf<int32_t> mfrom, mto, mcount;
    hipEvent_t ev_detect = nullptr, ev_match = nullptr;
    bool match_pending = false;
};

struct mslam_hip_ctx
{
    mslam_hip_params p{};
    mslam::Geometry geom{};
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // side streams for chunked batches (see mslam_hip_detect_batch_dev)
    int n_side = 2;
    hipStream_t side[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[4] = {nullptr, nullptr, nullptr, nullptr};
    // the blur of a chunk runs on a stream of its own beside the chunk's quadtree (both only read the pyramid)
    hipStream_t blur_stream[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_blur_fork[4] = {nullptr, nullptr, nullptr, nullptr}, ev_blur_join[4] = {nullptr, nullptr, nullptr, nullptr};
    bool fork_blur = false;
    std::string err;

    // host copies of the tables
    std::vector<mslam::CellDesc> cells;

    // device tables
    mslam::DevBuf<mslam::CellDesc> d_cells;
    mslam::DevBuf<int32_t> d_rs_ofs;   // resize offsets, all levels
    mslam::DevBuf<uint32_t> d_rs_coef; // resize coefficients, all levels
    std::vector<size_t> rs_x, rs_y; // per-level start index into d_rs_*
    mslam::DevBuf<uint4> d_rs_qt;   // quad tables (k_resize_col), all levels, 3 x uint4 per quad
    std::vector<size_t> rs_q;       // per-level start (in quads) into the quad tables; SIZE_MAX = use the generic kernel
    std::vector<int> rs_need;       // per level: which pixel positions of a quad ever use the upper dword pair
    mslam::DevBuf<uint4> d_rs_qt8;  // octet tables (k_level.hip's eight-pixel lanes), 5 x uint4 per octet
    std::vector<size_t> rs_q8;      // per-level start (in octets) into the octet tables; SIZE_MAX = the level keeps the four-pixel walk
    // cv::ORB mode: INTER_LINEAR_EXACT tables (all levels) and per-level quota
    mslam::DevBuf<int32_t> d_cv_ofs;
    mslam::DevBuf<uint32_t> d_cv_coef;
    std::vector<size_t> cv_x, cv_y;           // per-level start index into d_cv_*
    std::vector<std::array<int, 4>> cv_range; // per level: xmin, xmax, ymin, ymax
    std::vector<int> cv_window12;             // per level: k_resize_exact may use its 12-byte-window form
    int cv_quota[mslam::kMaxLevels] = {0};
    mslam::DevBuf<int32_t> d_ratio_thr;  // [257]
    mslam::DevBuf<uint32_t> d_orient_w; // [2][256] intensity-centroid disc weights
    hipGraphExec_t detect_graph[2] = {nullptr, nullptr}; // mslam_hip_detect's kernel + copy sequence, per output set
    bool use_graph = true;
    int cv_order = 0; // MSLAM_HIP_CV_ORDER_*: the cv::ORB mode's keypoint order inside a level (mslam_hip_set_cv_keypoint_order)
    bool mirror_results = false; // set by mslam_hip_detect around its enqueue: k_describe writes the results into h_out as well (no packing kernel)
    // mslam_hip_match's sequence (descriptor upload + matcher + merge + ratio test) as a graph: sizes come from a mapped word pair,
    // the launch shapes from the staging capacities, so one graph serves every call until the capacities or the matcher change
    hipGraphExec_t match_graph = nullptr;
    int match_graph_from_cap = 0, match_graph_to_cap = 0, match_graph_kind = -1, match_graph_kernel = 0;
    mslam::PinnedBuf<uint8_t> h_out; // mapped staging of mslam_hip_detect's results: [count, flags | xy | desc | octave | angle | response] for K keypoints
    double ratio_cached = -1.0;

    // device working set (sized for max_batch frames)
    mslam::DevBuf<uint8_t> d_stage;    // one frame of BGR for the host-pointer entry point
    mslam::PinnedBuf<uint8_t> h_stage; // the same as page-locked, device-mapped host memory (zero-copy upload, MSLAM_HIP_ZERO_COPY_FRAME)
    mslam::DevBuf<uint8_t> d_pyr, d_blur;
    mslam::DevBuf<mslam::BlurWave> d_blur_waves; // k_blur2 wave descriptors of one frame
    int blur_wpf = 0;
    int fused_levels = 0;  // levels 0 .. fused_levels-1 are produced and blurred by k_level.hip; k_blur2 takes the rest
    int level_k6 = 5;      // k_level.hip: rows per block = 6 k6 + 2
    bool knob_mirror_results = true, knob_zero_copy = true, knob_match_graph = true; // MSLAM_HIP_MIRROR_RESULTS / _ZERO_COPY_FRAME / _MATCH_GRAPH at creation
    size_t zero_copy_max_bytes = 1200000; // frames above this size are copied by DMA instead of read over PCIe by the gray kernel
    int level_chain = 0, level_chain_frames = 2, level_chain_waves = 8, level_chain_k6 = 9; // k_level_chain (k_level.hip)
    int level_k6_small = 1; // the same for batches of fewer than 8 frames (latency: one wave's walk is the launch's duration)
    mslam::DevBuf<uint32_t> d_cell_cnt, d_cell_kp;
    // the quadtree's arrays; `quad` (passed to the kernels by value) holds their addresses and owns nothing
    mslam::DevBuf<uint32_t> q_cand, q_cand_cnt, q_sel, q_sel_cnt, q_kp_node, q_ncnt_a, q_ncnt_b, q_child_cnt, q_ninfo, q_best;
    mslam::DevBuf<uint2> q_nodes_a, q_nodes_b;
    mslam::QuadArgs quad{};
    mslam::DevBuf<uint32_t> d_flags;

    // two alternating output sets; out[cur] (cur_out) is the set of the last detect batch
    mslam_out_set out[2];
    int cur = 0;
    hipStream_t stream_m = nullptr; // matcher stream
    bool overlap_match = true;
    int matcher_kind = 0; // MSLAM_HIP_MATCHER_*
    int last_match_kernel = 0; // kernel of the last matcher launch: 0 none yet, 1 matrix cores, 2 xor/popcount, 3 guided
    // mslam_hip_set_guided_match: radius > 0 = the match-to-PnP sequence takes the guided stage when the call has a guess
    double guided_radius = 0.0;
    int guided_max_distance = 256, guided_width = 0, guided_height = 0;
    // mslam_hip_set_union_descriptor: read by mslam_hip_kf_union[_dev] when they are called
    int union_descriptor = MSLAM_HIP_UNION_DESC_RECENT;
    int n_last = 0;         // frames in the last detect batch
    unsigned long long detect_seq = 0; // counts detect batches; points_seq = the batch the back-projected points belong to
    unsigned long long points_seq = ~0ull;
    unsigned long long match_seq = ~0ull; // the detect batch mslam_hip_match_batch_dev last matched (mslam_hip_pack_batch_dev packs no stale pairs)
    bool have_prev = false; // slot 0 holds a real predecessor of the current batch

    // host-pointer matcher scratch (grown on demand)
    mslam::DevBuf<uint8_t> d_hm_from;
    uint8_t* d_hm_to = nullptr;        // this call's query rows inside d_hm_from
    mslam::DevBuf<int32_t> d_hm_out;   // 6 arrays x cap + 1
    int hm_from_cap = 0, hm_to_cap = 0;
    mslam::DevBuf<uint32_t> d_hm_partial; // per-slice top-2 keys of the sliced single-pair matcher
    mslam::PinnedBuf<uint8_t> h_hm;       // page-locked, mapped staging of the host-pointer matcher

    // RGB-D back-projection outputs (allocated on first use)
    mslam::DevBuf<double> d_xyz;
    mslam::DevBuf<uint8_t> d_valid;
    // batched PnP (allocated on first use)
    mslam::DevBuf<float> d_pnp_obj, d_pnp_img;
    mslam::DevBuf<int32_t> d_pnp_n, d_pnp_counts;
    mslam::DevBuf<double> d_pnp_hyp, d_pnp_out;
    mslam::DevBuf<uint8_t> d_pnp_mask;
    int pnp_iterations = 0;
    double pnp_confidence = 0.99; // cv_ransac_pnp.cpp:57 (mslam_hip_pnp_set_confidence)
    // mslam_hip_set_ba_loss: read by both bundle adjustment entry points when they are called; NONE keeps scale 0
    int ba_loss_kind = MSLAM_HIP_BA_LOSS_NONE;
    double ba_loss_scale = 0.0;
    // single-problem PnP scratch (mslam_hip_pnp_ransac), grown on demand
    mslam::DevBuf<float> d_pnp1_obj, d_pnp1_img;
    mslam::DevBuf<double> d_pnp1_hyp, d_pnp1_out;
    mslam::DevBuf<int32_t> d_pnp1_counts;
    mslam::DevBuf<uint8_t> d_pnp1_mask;
    int pnp1_n_cap = 0, pnp1_it_cap = 0;
    // single-problem min-MSE PnP scratch (mslam_hip_pnp_min_mse): [obj | img | pose | info | n] in one block, grown on demand
    mslam::DevBuf<double> d_mse1;
    // RANSAC rigid alignment (k_align.hip).  Single problem (mslam_hip_align_ransac): scratch grown on demand; batched
    // (mslam_hip_align_batch_dev): allocated on first use
    mslam::DevBuf<float> d_align1_src, d_align1_dst;
    mslam::DevBuf<double> d_align1_hyp, d_align1_out;
    mslam::DevBuf<int32_t> d_align1_counts;
    mslam::DevBuf<uint8_t> d_align1_mask;
    int align1_n_cap = 0, align1_it_cap = 0;
    mslam::DevBuf<float> d_align_src, d_align_dst;
    mslam::DevBuf<int32_t> d_align_n, d_align_counts;
    mslam::DevBuf<double> d_align_hyp, d_align_out;
    mslam::DevBuf<uint8_t> d_align_mask;
    int align_iterations = 0;
    // mslam_hip_set_track_pose: read by mslam_hip_track and mslam_hip_track_window[_dev] when they are called
    int track_pose_kind = MSLAM_HIP_TRACK_POSE_PNP;
    double track_align_distance = 0.0;
    bool pnp_attr_set = false; // the > 64 KB dynamic-LDS attribute of the PnP kernels, per context (= per device)
    // bundle adjustment (mslam_hip_bundle_adjust, k_ba.hip), grown on demand: every device array of one solve, and the
    // mapped termination word the host reads between batches of iterations
    mslam::DevBuf<uint8_t> d_ba;
    mslam::PinnedBuf<int32_t> h_ba;
    // the padded dense reduced system of mslam_hip_bundle_adjust_global, an owner of its own: a global solve leaves d_ba,
    // which the local solve sizes, as small as the local solve needs it
    mslam::DevBuf<double> d_ba_S;
    // pose-graph optimisation (mslam_hip_pose_graph, k_posegraph.hip), grown on demand: every device array of one solve but
    // the normal equations, which live in d_ba_S; the termination word is h_ba
    mslam::DevBuf<uint8_t> d_pg;
    // mslam_hip_set_pose_graph_solver: read by mslam_hip_pose_graph when it is called
    int pg_solver = MSLAM_HIP_PG_SOLVER_DENSE;
    // mslam_hip_set_pose_graph_loss: read by mslam_hip_pose_graph and mslam_hip_pose_graph_edge_weights when they are called;
    // mslam_hip_set_pnp_mse_loss: read by mslam_hip_pnp_min_mse[_batch_dev].  Kinds are MSLAM_HIP_BA_LOSS_*; NONE keeps scale 0
    int pg_loss_kind = MSLAM_HIP_BA_LOSS_NONE;
    double pg_loss_scale = 0.0;
    int mse_loss_kind = MSLAM_HIP_BA_LOSS_NONE;
    double mse_loss_scale = 0.0;
    // mslam_hip_set_ba_global_solver: read by mslam_hip_bundle_adjust_global when it is called; SPARSE keeps the envelope in
    // d_ba_S
    int bag_solver = MSLAM_HIP_BA_GLOBAL_SOLVER_DENSE;
    // mslam_hip_set_ba_global_pcg: read by mslam_hip_bundle_adjust_global when it is called; enabled, it takes the place of
    // bag_solver's kind and leaves bag_solver as it is.  The blocks live in d_ba_S.  bag_pcg_stats: the last global solve's
    int bag_pcg = 0, bag_pcg_max_iterations = MSLAM_HIP_BA_GLOBAL_PCG_MAX_ITERATIONS;
    double bag_pcg_tolerance = MSLAM_HIP_BA_GLOBAL_PCG_TOLERANCE;
    mslam_hip_pcg_stats bag_pcg_stats{};
    // mslam_hip_set_pose_graph_pcg: read by mslam_hip_pose_graph when it is called; enabled, it takes the place of pg_solver's
    // kind and leaves pg_solver as it is.  The blocks live in d_ba_S.  pg_pcg_stats: the last pose-graph solve's
    int pg_pcg = 0, pg_pcg_max_iterations = MSLAM_HIP_POSE_GRAPH_PCG_MAX_ITERATIONS;
    double pg_pcg_tolerance = MSLAM_HIP_POSE_GRAPH_PCG_TOLERANCE;
    mslam_hip_pcg_stats pg_pcg_stats{};

    mslam::BowState* bow = nullptr;
    mslam::RelocState* reloc = nullptr;
    mslam::TsdfState* tsdf = nullptr;
    mslam::IcpState* icp = nullptr;

    bool profiling = false;      // mode 1: every stage timed, everything serialised on the context's stream
    bool inplace_timing = false; // mode 2: every stage launch is timed in place on the stream it runs on
    std::vector<mslam::StageTimer> timers;
    size_t timers_used = 0;
};

// a failed HIP call ends the entry point: the call's own text and HIP's message become the context's error
#define MSLAM_CHK(c, call)                                                                                             \
    do                                                                                                                 \
    {                                                                                                                  \
        hipError_t e_ = (call);                                                                                        \
        if(e_ != hipSuccess)                                                                                           \
        {                                                                                                              \
            (c)->err = std::string(#call) + ": " + hipGetErrorString(e_);                                              \
            return MSLAM_HIP_E_RUNTIME;                                                                                \
        }                                                                                                              \
    } while(0)

namespace mslam
{
// the output set of the last detect batch
inline mslam_out_set& cur_out(mslam_hip_ctx* c) { return c->out[c->cur]; }

inline int fail(mslam_hip_ctx* c, int code, const std::string& msg)
{
    c->err = msg;
    return code;
}

// Records a [start, stop] HIP-event pair around a stage.  Mode 1 (profiling): everything runs on the context's
// stream, so the events go there and the stages do not overlap.  Mode 2 (inplace_timing): the events are
// recorded on the stream the stage is launched on, which does not change the schedule; entries accumulate until
// mslam_hip_get_stage_times reads them.  Scopes may nest (a stage inside a stage): a scope keeps the index of its entry, not
// a pointer, because an inner scope's push_back may move the vector while the outer one is open.
struct StageScope
{
    mslam_hip_ctx* c;
    size_t slot = ~(size_t)0; // index into c->timers; ~0: not timed
    hipStream_t st;
    StageScope(mslam_hip_ctx* ctx, const char* name, hipStream_t launch_stream = nullptr) : c(ctx)
    {
        if(!c->profiling && !c->inplace_timing)
            return;
        if(c->timers_used >= 8192)
            return; // mode 2 accumulates until read: bound the number of live events
        st = (c->profiling || !launch_stream) ? c->stream : launch_stream;
        if(c->timers_used == c->timers.size())
        {
            mslam::StageTimer nt{name, nullptr, nullptr};
            if(hipEventCreate(&nt.start) != hipSuccess || hipEventCreate(&nt.stop) != hipSuccess)
                return;
            c->timers.push_back(nt);
        }
        slot = c->timers_used++;
        c->timers[slot].name = name;
        (void)hipEventRecord(c->timers[slot].start, st);
    }
    ~StageScope()
    {
        if(slot != ~(size_t)0)
            (void)hipEventRecord(c->timers[slot].stop, st);
    }
};

// bow entry points used by api.hip
int bow_batch(mslam_hip_ctx* c, int add_to_db);

// k_pnp.hip for k_reloc.hip: k_pnp_ransac_batch on caller-owned device arrays — problem p reads obj / img / mask at
// p * cap, hyp / counts at p * iterations, writes out[p * 16 ..] and samples with seed + p; the guess (when use_guess) is
// shared by all problems.  The launch is enqueued on c->stream; returns a MSLAM_HIP_* status.
struct PnpBatchLaunch
{
    const float* obj;
    const float* img;
    const int32_t* n; // [n_problems]
    int n_problems, cap;
    double fx, fy, cx, cy;
    int use_guess;
    double rvec[3], tvec[3];
    int iterations;
    double reprojection_error;
    unsigned long long seed;
    double* hyp;
    int32_t* counts;
    uint8_t* mask;
    double* out;
};
int pnp_launch_batch(mslam_hip_ctx* c, const PnpBatchLaunch& l);
void pnp_rotation_to_rvec(const double R[9], double rvec[3]);
void pnp_rvec_to_rotation(const double rvec[3], double R[9]); // the R0 the PnP launch makes of its guess

// k_align.hip for k_reloc.hip: k_align_ransac_batch on caller-owned device arrays, addressed as PnpBatchLaunch's are (src /
// dst / mask at p * cap, hyp / counts at p * iterations, out[p * 16 ..], seed + p).  Enqueued on c->stream.
struct AlignBatchLaunch
{
    const float* src;
    const float* dst;
    const int32_t* n; // [n_problems]
    int n_problems, cap;
    int iterations;
    double max_distance;
    unsigned long long seed;
    double* hyp;
    int32_t* counts;
    uint8_t* mask;
    double* out;
};
int align_launch_batch(mslam_hip_ctx* c, const AlignBatchLaunch& l);
} // namespace mslam

// api.hip: uploads the ratio-test table of `ratio` unless it is the cached one (not part of the C ABI)
extern "C" int mslam_ratio_table(mslam_hip_ctx* c, double ratio);
