/* mslam_hip.h — C ABI of the MI355X-native ORB / Hamming-match / BoW front end.
 *
 * This is the drop-in boundary for modular-slam's feature hot path.  Each entry point names the
 * reference interface it replaces (paths relative to the reference repo,
 * src/lib/modular_slam/...).  Plain C types only; no exceptions cross this boundary; every function
 * returns an int status (0 = MSLAM_HIP_OK) and mslam_hip_last_error() gives the text.
 *
 * Threading: a context is NOT thread-safe (the reference detector is not re-entrant either — it owns
 * its pyramid scratch, distributed_cv_feature.cpp:651).  Use one context per GPU / per caller thread.
 * Host-pointer entry points are synchronous (they return after the D2H copy); *_dev entry points
 * enqueue on the context's HIP stream and return without synchronising.
 */
#ifndef MSLAM_HIP_H_
#define MSLAM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSLAM_HIP_ABI_VERSION 5

enum
{
    MSLAM_HIP_OK = 0,
    MSLAM_HIP_E_INVALID = 1,  /* bad argument / unsupported size */
    MSLAM_HIP_E_RUNTIME = 2,  /* HIP runtime failure (no device, launch failure, OOM...) */
    MSLAM_HIP_E_CAPACITY = 3, /* an output or scratch capacity was exceeded; no partial result is valid */
    MSLAM_HIP_E_NO_VOCABULARY = 4,
    MSLAM_HIP_E_FORMAT = 5,   /* vocabulary stream not understood */
    MSLAM_HIP_E_NO_MODEL = 6  /* RANSAC found no model (cv::solvePnPRansac returning false) */
};

typedef struct mslam_hip_ctx mslam_hip_ctx;

/* Detector parameters.  Defaults are the reference's hard-coded operating point
 * (distributed_cv_feature.cpp:1184-1186): orb_params("orb", 1.2f, 8, 20, 7), min node area 1000. */
typedef struct
{
    int32_t width, height;  /* frame size every call on this context uses (reference: 640x480); 0 x 0 = a
                             * context without detector (matcher / BoW only: no pyramid buffers are allocated)    */
    int32_t max_batch;      /* frames per batched device launch, >= 1                                      */
    int32_t n_levels;       /* pyramid levels (8)                                                          */
    float scale_factor;     /* pyramid scale (1.2f); level scales are the float32 chain of :411-420        */
    int32_t ini_fast_thr;   /* first FAST threshold (20)                                                   */
    int32_t min_fast_thr;   /* fallback threshold for cells that found nothing (7), :922-926               */
    uint32_t min_node_area; /* quadtree stop area in level-0 px^2 (1000), :1002,:1186                      */
    int32_t max_keypoints;  /* per-frame keypoint capacity of the output buffers                           */
    int32_t max_candidates; /* per-(frame,level) FAST candidate capacity feeding the quadtree              */
    int32_t device;         /* HIP device ordinal                                                          */
    void* stream;           /* hipStream_t to enqueue on; NULL = the context creates its own               */
    /* which of the reference's two IFeatureDetector implementations this context is a drop-in for: */
    int32_t detector;       /* MSLAM_HIP_DETECTOR_DISTRIBUTED (default) or MSLAM_HIP_DETECTOR_CV_ORB               */
    int32_t n_features;     /* CV_ORB: cv::ORB::create(nfeatures) (1000, orb_feature.cpp:25)                       */
    int32_t edge_threshold; /* CV_ORB: edgeThreshold (31, cv::ORB default); FAST threshold = ini_fast_thr (20)      */
} mslam_hip_params;

enum
{
    /* DistributedOrbOpenCvDetector (distributed_cv_feature.cpp:1181-1222): 64-px FAST cells + quadtree, util::cos/sin */
    MSLAM_HIP_DETECTOR_DISTRIBUTED = 0,
    /* OrbOpenCvDetector (orb_feature.cpp:25,33-65): toGrayScale + cv::ORB::create(n)->detectAndCompute — INTER_LINEAR_EXACT
     * pyramid, whole-level FAST, retainBest(2n) / Harris response / retainBest(n) per level, libm-style cos/sin.
     * Keypoint ORDER inside a level: what KeyPointsFilter::retainBest's std::nth_element + std::partition leave behind —
     * defined by the C++ library, not by the standard.  The reference is a GCC build, so the default reproduces libstdc++'s
     * introselect / partition step by step (mslam_hip_set_cv_keypoint_order); the raster order of FAST is the alternative.
     * cos / sin of the keypoint angle come from include/mslam_sincos.h, which equals the host library's
     * (float)cos((double)angle) / (float)sin((double)angle) — the expression orb.cpp evaluates in a GCC build — for every
     * float in [0, 6.5] (checked exhaustively against glibc 2.35).  n_levels, scale_factor, ini_fast_thr keep their meaning;
     * min_fast_thr / min_node_area are unused. */
    MSLAM_HIP_DETECTOR_CV_ORB = 1
};
/* CV_ORB detector: where the two retainBest calls of a level leave their survivors (the kept SET is the same either way).
 * LIBSTDCXX (default) = the order of a GCC build of the reference, hence its keypoint ids and DescriptorMatch indices;
 * RASTER = FAST's (y, x) order — a little faster (the selection is then a threshold and a compaction). */
enum
{
    MSLAM_HIP_CV_ORDER_LIBSTDCXX = 0,
    MSLAM_HIP_CV_ORDER_RASTER = 1
};
int mslam_hip_set_cv_keypoint_order(mslam_hip_ctx* ctx, int order);

void mslam_hip_default_params(mslam_hip_params* p);
int mslam_hip_abi_version(void);

int mslam_hip_create(const mslam_hip_params* p, mslam_hip_ctx** out);
void mslam_hip_destroy(mslam_hip_ctx* ctx);
/* ctx may be NULL: returns the message of the last failed mslam_hip_create on this thread. */
const char* mslam_hip_last_error(const mslam_hip_ctx* ctx);
/* Block until everything enqueued on the context's stream has finished; also surfaces capacity
 * overflows recorded by *_dev launches (returns MSLAM_HIP_E_CAPACITY once, then clears). */
int mslam_hip_sync(mslam_hip_ctx* ctx);

/* ---- IFeatureDetector<RgbFrame,uint8_t,32>::detect ------------------------------------------------
 * Replaces DistributedOrbOpenCvDetector::detect (distributed_cv_feature.cpp:1190-1222; interface
 * frontend/feature/feature_interface.hpp:50-56).  `bgr` is the RgbFrame::data buffer: interleaved
 * 3-channel u8, row-major, no padding (types/rgb_frame.hpp:12-16).  Outputs are SoA, caller
 * allocated, `max_out` entries each: xy = scale-corrected float coordinates (x0,y0,x1,y1,...) in
 * the reference's order (level 0..L-1, quadtree node-list order inside a level); desc = 32 bytes per
 * keypoint; octave/angle/response may be NULL.  The reference's Keypoint::id is the output index. */
int mslam_hip_detect(mslam_hip_ctx* ctx, const uint8_t* bgr, int width, int height, int max_out, float* xy,
                     uint8_t* desc, int32_t* octave, float* angle, float* response, int* n_out);

/* Device-resident batched form of the same operator: `d_bgr` holds n_frames (<= max_batch)
 * back-to-back frames in HBM.  Results stay in context-owned device buffers (mslam_hip_batch_view). */
int mslam_hip_detect_batch_dev(mslam_hip_ctx* ctx, const uint8_t* d_bgr, int n_frames);

typedef struct
{
    int32_t n_frames;     /* frames in the last detect batch                                     */
    int32_t capacity;     /* max_keypoints: per-frame stride (in keypoints) of the arrays below  */
    const float* xy;      /* [max_batch][capacity][2]                                            */
    const uint8_t* desc;  /* [max_batch][capacity][32]                                           */
    const int32_t* octave;
    const float* angle;
    const float* response;
    const int32_t* count; /* [max_batch] keypoints per frame                                     */
    /* results of mslam_hip_match_batch_dev, frame t matched against frame t-1: */
    const int32_t* match_from; /* [max_batch][capacity] index into frame t   (fromIndex)         */
    const int32_t* match_to;   /* [max_batch][capacity] index into frame t-1 (toIndex)           */
    const int32_t* match_count; /* [max_batch]; 0 for a frame without predecessor                */
} mslam_hip_batch_view;
int mslam_hip_get_batch_view(mslam_hip_ctx* ctx, mslam_hip_batch_view* view);

/* ---- IFeatureMatcher<uint8_t,32>::match ------------------------------------------------------------
 * Replaces OrbOpenCvMatcher::match(from, to) (orb_feature.cpp:84-117; interface
 * feature_interface.hpp:62-70): BFMatcher(HAMMING).knnMatch(query = to, train = from, k = 2) and the
 * ratio test (double)d0 < ratio*(double)d1 (:96-105, reference ratio 0.7).  Descriptors are packed
 * 32-byte rows.  Outputs (capacity n_to each) are ordered by query (= to) index (:110-114).
 * n_from < 2 is undefined behaviour in the reference (:101); here it yields zero matches. */
int mslam_hip_match(mslam_hip_ctx* ctx, const uint8_t* from_desc, int n_from, const uint8_t* to_desc, int n_to,
                    double ratio, int32_t* from_idx, int32_t* to_idx, int* n_out);
/* The knnMatch(k=2) result itself, per query row of `to`: train indices (-1 if absent) and integer
 * Hamming distances (INT32_MAX if absent), best first; ties rank the lower train index first. */
int mslam_hip_match_knn2(mslam_hip_ctx* ctx, const uint8_t* from_desc, int n_from, const uint8_t* to_desc,
                         int n_to, int32_t* idx0, int32_t* idx1, int32_t* dist0, int32_t* dist1);
/* Batched device form: for every frame t of the last detect batch, match(from = frame t,
 * to = frame t-1); frame 0 is matched against the last frame of the previous batch when
 * `chain_previous` is non-zero and one exists.  Results: mslam_hip_batch_view.match_*. */
int mslam_hip_match_batch_dev(mslam_hip_ctx* ctx, double ratio, int chain_previous);
/* The batched matcher runs on a stream of its own behind the detect batch it reads.  This makes the context's
 * stream wait (on the device, no host synchronisation) for every matcher launch enqueued so far, so that work the
 * caller enqueues on the context's stream afterwards — e.g. an asynchronous copy of the match results — sees them. */
int mslam_hip_join_matcher(mslam_hip_ctx* ctx);
/* Which kernel computes the 256-bit Hamming distances (results are identical, tests run both):
 * AUTO = matrix cores (bits as FP4 +-1, exact) up to 32736 train rows and xor/popcount beyond; POPCOUNT = the
 * xor/__popc form BASELINE.json's north_star names, always.  The initial value comes from the environment
 * variable MSLAM_HIP_MATCHER ("popcount") read at mslam_hip_create. */
enum
{
    MSLAM_HIP_MATCHER_AUTO = 0,
    MSLAM_HIP_MATCHER_POPCOUNT = 1
};
int mslam_hip_set_matcher(mslam_hip_ctx* ctx, int kind);
int mslam_hip_get_matcher(const mslam_hip_ctx* ctx);
/* which kernel the last matcher launch of this context took: 0 = none yet, 1 = matrix cores, 2 = xor/popcount (AUTO decides on
 * the CAPACITY of the train side: max_keypoints on the batched path, n_from on the host-pointer calls), 3 = the guided stage
 * below */
int mslam_hip_last_match_kernel(const mslam_hip_ctx* ctx);

/* ---- guided matching: landmarks matched in a window round their projection ---------------------------
 * matchLandmarks (rgbd_feature_frontend.cpp:237-254) matches the local map's landmarks against ALL keypoints of the frame
 * and carries "TODO: use boost geometry rtree for keypoints" (:242); track() projects every matched landmark with
 * currentPose (:300), but only to draw it.  Here the projection gates the matcher, as ORB-SLAM's SearchByProjection does.
 *
 * Inputs: keypoints i < n_kp (descriptor 32 B, xy f32), landmarks j < n_lm (descriptor 32 B, world point 3 x f64), a pose
 * world -> camera R (9 f64, row-major) and t (3 f64), the intrinsics, a frame extent width x height, radius (f64, > 0).
 *
 *   projection   SAME as mslam_hip_kf_visible's, in f64 with every operation rounded on its own:
 *                c_r = ((R[r][0] X + R[r][1] Y) + R[r][2] Z) + t[r],  u = (c_0 / c_2) fx + cx,  v = (c_1 / c_2) fy + cy.
 *   candidate    keypoint i is a candidate of landmark j iff  c_2 > 0,  x_i and y_i are finite with
 *                0 <= (double)x_i < width and 0 <= (double)y_i < height,  and
 *                fabs((double)x_i - u) <= radius && fabs((double)y_i - v) <= radius.  The window is square; every
 *                comparison is written so that a NaN anywhere gives "not a candidate".  Keypoints a caller masks out
 *                (relocalize's `valid`, the depth filter of track) are candidates like any other: the mask is applied to
 *                the matches afterwards, as it is after the brute-force matcher.
 *   knn-2        SAME rule as mslam_hip_match_knn2, over the candidates only: per landmark the two candidates of least
 *                Hamming distance, ties to the lower keypoint index; absent: index -1, distance INT32_MAX.
 *                n_cand[j] = the number of candidates of landmark j.
 *   acceptance   d0 <= max_distance && (no second candidate || (double)d0 < ratio * (double)d1) — mslam_hip_match's
 *                expression and its table where a second candidate exists, so the two accept alike bit for bit.
 *                max_distance lies in 0..256; 256 = no gate.  DEVIATES from mslam_hip_match in that a lone candidate is
 *                accepted: there is no "fewer than two keypoints" rule here.
 *   order        by landmark index, at most one match per landmark; two landmarks may name one keypoint, as in
 *                mslam_hip_match.
 *   vs reference DEVIATES: the reference matches brute force, so a landmark whose descriptor has a look-alike anywhere in
 *                the frame fails its ratio test; here only look-alikes inside the window count.  With a window that
 *                covers the frame and every keypoint in the frame, knn-2 equals mslam_hip_match_knn2's.
 *
 * Returns MSLAM_HIP_E_INVALID for a radius that is not > 0 (NaN included), max_distance outside 0..256, an extent outside
 * 1..8192, fx or fy zero or NaN, and n_kp or n_lm above 65535.  n_kp = 0 or n_lm = 0 is OK with no matches (knn2: every
 * landmark absent).  Outputs have capacity n_lm; n_cand may be NULL. */
int mslam_hip_match_guided_knn2(mslam_hip_ctx* ctx, const uint8_t* kp_desc, const float* kp_xy, int n_kp, const uint8_t* lm_desc,
                                const double* lm_world, int n_lm, const double* R, const double* t, double fx, double fy,
                                double cx, double cy, int width, int height, double radius, int32_t* idx0, int32_t* idx1,
                                int32_t* dist0, int32_t* dist1, int32_t* n_cand /* may be NULL */);
/* from_idx = keypoint, to_idx = landmark, as mslam_hip_match(from = keypoints, to = landmarks) */
int mslam_hip_match_guided(mslam_hip_ctx* ctx, const uint8_t* kp_desc, const float* kp_xy, int n_kp, const uint8_t* lm_desc,
                           const double* lm_world, int n_lm, const double* R, const double* t, double fx, double fy, double cx,
                           double cy, int width, int height, double radius, int max_distance, double ratio, int32_t* from_idx,
                           int32_t* to_idx, int* n_out);
/* The mode.  With a radius > 0 set, mslam_hip_relocalize, mslam_hip_track, mslam_hip_track_window and
 * mslam_hip_track_window_dev take the guided stage in place of the brute-force matcher WHEN use_extrinsic_guess != 0: the
 * pose is the call's guess (rvec turned into R on the host, exactly as the PnP stage turns it into its starting rotation),
 * the intrinsics are the call's, the extent and max_distance are the mode's, the ratio is the call's.  Every frame of a
 * window, and every candidate of a relocalisation, shares that pose, as they share the guess: a window's radius has to
 * cover the camera's motion across the window.  Without a guess there is no pose to project with: the brute-force stage
 * runs and the outputs are byte-identical to mode off.  The PnP, the vote and the keyframe construction are untouched; they
 * consume the same match arrays.  mslam_hip_last_match_kernel returns 3 after a guided stage.
 * radius <= 0 switches the mode off (the default; width and height are then not checked).  MSLAM_HIP_E_INVALID for a NaN
 * radius, max_distance outside 0..256, and — with radius > 0 — an extent outside 1..8192. */
int mslam_hip_set_guided_match(mslam_hip_ctx* ctx, double radius, int max_distance, int width, int height);
int mslam_hip_get_guided_match(mslam_hip_ctx* ctx, double* radius, int* max_distance, int* width, int* height);

/* ---- IRelocalizer / ILoopDetector: DBoW3 bag of words ---------------------------------------------
 * Replaces what OrbRelocalizer is wired for (orb_relocalizer.cpp:26-50, relocalizer.hpp:11-20,
 * loop_detection.hpp:10-15): DBoW3::Vocabulary::transform and Database add/query with L1 scoring.
 * `blob` is a DBoW3 binary vocabulary stream (Vocabulary::toStream/fromStream,
 * conan_recipes/dbow3/dbow3.patch:2252-2355,2544-2651), plain or saved with compressed = true (QuickLZ 1.5 packets,
 * levels 1 and 3; the decoder is a restatement of the published format, see csrc/quicklz_decode.hip). */
enum /* DBoW3 WeightingType / ScoringType as stored in the vocabulary stream */
{
    MSLAM_BOW_TF_IDF = 0,
    MSLAM_BOW_TF = 1,
    MSLAM_BOW_IDF = 2,
    MSLAM_BOW_BINARY = 3
};
enum
{
    MSLAM_BOW_L1_NORM = 0,
    MSLAM_BOW_L2_NORM = 1,
    MSLAM_BOW_CHI_SQUARE = 2,
    MSLAM_BOW_KL = 3,
    MSLAM_BOW_BHATTACHARYYA = 4,
    MSLAM_BOW_DOT_PRODUCT = 5
};
/* Only L1_NORM scoring vocabularies are accepted (the ORB vocabularies DBoW3 ships are TF_IDF / L1_NORM).
 * The database (DBoW3::Database(voc, false, 0), orb_relocalizer.cpp:29) is an inverted file on the device: word ->
 * rows of (entry, value).  It is unbounded: storage grows by doubling (mslam_hip_bow_db_reserve pre-allocates);
 * mslam_hip_bow_db_query scores against EVERY entry ever added and not removed.  The batched device form
 * (mslam_hip_bow_batch_dev) scores every frame against the 64 entries that precede it and
 * adds its vectors to the same database. */
int mslam_hip_bow_load(mslam_hip_ctx* ctx, const void* blob, size_t size);
int mslam_hip_bow_info(mslam_hip_ctx* ctx, int* k, int* L, int* n_nodes, int* n_words, int* scoring,
                       int* weighting);
/* How a descriptor is assigned to a word, for every entry point below:
 * TREE = Vocabulary::transform's descent (dbow3.patch:1760-1860: at each level the child with the least Hamming
 * distance, first child on ties) — what DBoW3 does, the default;
 * FLAT = the exhaustive descriptor-vs-vocabulary search the descent approximates (BASELINE.json north_star's
 * "batched descriptor-vs-vocabulary Hamming kernel", SURVEY.md §8d bow_flat): the leaf with the least distance
 * over ALL words, lower word id on ties.  n x n_words distance evaluations: a stress mode, not a DBoW3 drop-in.
 * FLAT is available only when the vocabulary's word table maps one-to-one onto its leaves (distinct word ids, one per
 * leaf, none on an inner node) and holds at most 2^20 words; otherwise setting it fails with MSLAM_HIP_E_INVALID and
 * the mode stays as it was, whatever modes were set before. */
enum
{
    MSLAM_BOW_ASSIGN_TREE = 0,
    MSLAM_BOW_ASSIGN_FLAT = 1
};
int mslam_hip_bow_set_assignment(mslam_hip_ctx* ctx, int mode);
/* Vocabulary::transform(feature, word_id, weight) for n descriptors (dbow3.patch:1760-1860). */
int mslam_hip_bow_words(mslam_hip_ctx* ctx, const uint8_t* desc, int n, uint32_t* word, double* weight);
/* Vocabulary::transform(features, BowVector) (dbow3.patch:1432-1530): ascending word ids, values
 * normalised as the vocabulary's scoring requires.  Capacity of words/values: n. */
int mslam_hip_bow_transform(mslam_hip_ctx* ctx, const uint8_t* desc, int n, uint32_t* words, double* values,
                            int* n_words);
/* DBoW3 L1Scoring::score of two BoW vectors, in [0,1]. */
int mslam_hip_bow_score(mslam_hip_ctx* ctx, const uint32_t* w1, const double* v1, int n1, const uint32_t* w2,
                        const double* v2, int n2, double* score);
/* Database: add(features) -> entry id (IRelocalizer::addKeyframe's feed, rgbd_feature_frontend.cpp:176)
 * and query(features) -> the best max_results entries by L1 score, best first, ties by lower entry
 * id (IRelocalizer::relocalize / ILoopDetector::detectLoop). */
int mslam_hip_bow_db_add(mslam_hip_ctx* ctx, const uint8_t* desc, int n, int* entry_id);
int mslam_hip_bow_db_query(mslam_hip_ctx* ctx, const uint8_t* desc, int n, int max_results, int32_t* entry_ids,
                           double* scores, int* n_results);
/* IRelocalizer::removeKeyframe: the entry is never reported again (its id is not reused). */
int mslam_hip_bow_db_remove(mslam_hip_ctx* ctx, int entry_id);
int mslam_hip_bow_db_clear(mslam_hip_ctx* ctx);
int mslam_hip_bow_db_reserve(mslam_hip_ctx* ctx, int max_entries);
int mslam_hip_bow_db_size(mslam_hip_ctx* ctx, int* n_entries);
/* Batched device form: transform every frame of the last detect batch into a BoW vector, score it
 * against the database (all entries), then add it as a new entry.  Per frame: best entry and score. */
int mslam_hip_bow_batch_dev(mslam_hip_ctx* ctx, int add_to_db);
typedef struct
{
    int32_t capacity;        /* per-frame stride of words/values                */
    const uint32_t* words;   /* [max_batch][capacity]                           */
    const double* values;    /* [max_batch][capacity]                           */
    const int32_t* n_words;  /* [max_batch]                                     */
    const int32_t* best_entry; /* [max_batch] (-1 if the database was empty)    */
    const double* best_score;  /* [max_batch]                                   */
} mslam_hip_bow_view;
int mslam_hip_get_bow_view(mslam_hip_ctx* ctx, mslam_hip_bow_view* view);

/* Cross-stream loop candidates (multi-camera / multi-GPU): score the BoW vector of
 * every frame t of the last mslam_hip_bow_batch_dev against vector [r][t] of n_sets foreign vector
 * sets (e.g. the all-gathered vectors of the other ranks).  Device arrays: d_words / d_values are
 * [n_sets][max_batch][capacity], d_n is [n_sets][max_batch], d_scores (out) is [max_batch][n_sets];
 * a pair without a common word scores exactly 0. */
int mslam_hip_bow_cross_score_dev(mslam_hip_ctx* ctx, const uint32_t* d_words, const double* d_values,
                                  const int32_t* d_n, int n_sets, int capacity, double* d_scores);

/* The exchange step itself, in the wire format of the all-gather (one "set" = one stream's batch):
 *   uint2 {u32 word, f32 value} vec[n_frames][k_max]  (ascending words, zero padded), then int32 count[n_frames]
 *   = n_frames * (2 * k_max + 1) dwords per set; k_max = 2048 gives the 16 KB per frame SURVEY.md §8e sizes.
 * pack: the BoW vectors of the last mslam_hip_bow_batch_dev into d_out (device), on the context's stream; a vector
 * with more than k_max words is reported by mslam_hip_sync as MSLAM_HIP_E_CAPACITY.
 * cross_score_packed: d_sets = n_sets gathered sets; d_scores[t][r] (f64, [n_frames][n_sets]) = L1 score of frame t
 * of set self_set against frame t of set r, on the f32 values as transmitted, summed in ascending word order.  It
 * reads nothing but d_sets and may be enqueued on any stream (`stream` = hipStream_t, NULL = the context's): e.g.
 * the communication stream right behind the collective, while the context's stream extracts the next batch. */
int mslam_hip_bow_pack_dev(mslam_hip_ctx* ctx, int k_max, uint32_t* d_out);
int mslam_hip_bow_cross_score_packed_dev(mslam_hip_ctx* ctx, const uint32_t* d_sets, int n_sets, int self_set,
                                         int n_frames, int k_max, double* d_scores, void* stream);

/* Host-only helper (no GPU, no context): decode `n_packets` consecutive QuickLZ packets, as DBoW3 writes them after the
 * nChunks word of a compressed vocabulary.  dst_size receives the decoded size (also when dst is too small). */
int mslam_hip_qlz_decompress(const void* src, size_t src_size, uint32_t n_packets, void* dst, size_t dst_capacity,
                             size_t* dst_size);

/* ---- RGB-D back-projection (the step after the matcher) ----------------------------
 * Replaces pointsFromRgbdKeypoints / reconstructPoint (rgbd_feature_frontend.cpp:101-138) with getDepth /
 * isDepthValid (types/depth_frame.hpp:20-30).  depth = DepthFrame::data (u16, row-major, width*height),
 * factor / focal / principal point = CameraParameters (sensors/camera_parameters.hpp:7-12; TUM: 1/5000, 525,
 * 525, 319.5, 239.5 — rgbd_file_provider.cpp:136-145).  xy = keypoint coordinates as returned by detect.
 * xyz[3i..3i+2] is the camera-frame point, valid[i] = 1 iff the depth is valid (std::optional engaged).
 * The pixel is the coordinate truncated toward zero (-0.5 is pixel 0, -1.0 is outside).  A coordinate that is not finite
 * (NaN, +-inf), or whose pixel is outside the image, gives valid[i] = 0 and the point (0, 0, 0), as every invalid depth
 * does.  fx or fy of zero or NaN: MSLAM_HIP_E_INVALID. */
int mslam_hip_backproject(mslam_hip_ctx* ctx, const uint16_t* depth, int width, int height, float factor, double fx,
                          double fy, double cx, double cy, const float* xy, int n, double* xyz, uint8_t* valid);
/* Batched device form: every keypoint of the last detect batch against d_depth = n_frames back-to-back
 * u16 depth frames in HBM.  Results: mslam_hip_points_view. */
int mslam_hip_backproject_batch_dev(mslam_hip_ctx* ctx, const uint16_t* d_depth, float factor, double fx, double fy,
                                    double cx, double cy);
typedef struct
{
    int32_t capacity;     /* per-frame stride (in keypoints) */
    const double* xyz;    /* [max_batch][capacity][3]        */
    const uint8_t* valid; /* [max_batch][capacity]           */
} mslam_hip_points_view;
int mslam_hip_get_points_view(mslam_hip_ctx* ctx, mslam_hip_points_view* view);

/* ---- packed results of a batch (one transfer instead of capacity-strided arrays) --------------------------------------
 * The batch views above are [max_batch][max_keypoints]-strided; copied back as they are, more than half of the bytes are
 * padding.  mslam_hip_pack_batch_dev writes, on the context's stream (after the matcher has been joined), a header, the
 * per-frame offset tables and then exactly count[t] keypoint records / match_count[t] match records per frame, back to
 * back, into `out`: device memory (follow with ONE copy of header.bytes) or page-locked, device-mapped host memory (the
 * kernel's stores are the transfer; read the header after synchronising).  Frame t's keypoints are records
 * kp_offset[t] .. kp_offset[t+1]-1 of every keypoint array, its matches records match_offset[t] .. match_offset[t+1]-1
 * (match indices are relative to the frame, as in the views).  A batch that mslam_hip_match_batch_dev has not run on is packed
 * with zero matches (never with an older batch's pairs).  If the results do not fit capacity_bytes, header.fits is 0,
 * header.bytes tells what was needed, no record is written (the two offset tables still are when they fit) and
 * mslam_hip_sync reports MSLAM_HIP_E_CAPACITY.
 * mslam_hip_packed_capacity: an upper bound for n_frames frames (every frame at max_keypoints). */
typedef struct
{
    int32_t n_frames, total_keypoints, total_matches, with_points;
    uint64_t off_kp_offset, off_match_offset;            /* int32[n_frames + 1] each                         */
    uint64_t off_xy, off_desc, off_octave, off_angle, off_response; /* f32[.][2], u8[.][32], i32, f32, f32   */
    uint64_t off_xyz, off_valid;                         /* f64[.][3], u8[.] (with_points)                   */
    uint64_t off_match_from, off_match_to;               /* i32[total_matches] each                          */
    uint64_t bytes;                                      /* bytes used (or needed, when fits == 0)           */
    int32_t fits, pad;
} mslam_hip_packed_header;
int mslam_hip_pack_batch_dev(mslam_hip_ctx* ctx, void* out, size_t capacity_bytes, int with_points);
size_t mslam_hip_packed_capacity(const mslam_hip_ctx* ctx, int n_frames, int with_points);

/* ---- IPnpAlgorithm::solvePnp (the consumer of the matches) ------------------------------------
 * Replaces OpenCvRansacPnp::solvePnp's cv::solvePnPRansac call (cv_ransac_pnp.cpp:56-57: useExtrinsicGuess = true, 100
 * iterations, 5 px, confidence 0.99, no distortion).  object_points = n x 3 f32 (landmark states cast to float, :22-31),
 * image_points = n x 2 f32 (:33-40), pin-hole intrinsics as in :52-53.  rvec / tvec (3 doubles each, Rodrigues vector
 * and translation of the world -> camera transform, OpenCV's convention) are the extrinsic guess on input when
 * use_extrinsic_guess is non-zero, and the result on output; inliers (n bytes, may be NULL) is the consensus mask of
 * the best hypothesis.  Returns MSLAM_HIP_E_NO_MODEL when no hypothesis reaches 5 inliers (solvePnPRansac == false).
 * Against cv::solvePnPRansac as OpenCV 4.8.1 runs it for this call (restated piece by piece in
 * oracle/mslam_cv_pnp_oracle.py from the library's published algorithm), of the four pieces and two edges
 *   1 sampler          DEVIATES: splitmix64 counter streams keyed by (`seed`, hypothesis) — hypotheses are independent of
 *                      each other, which is what lets them run in parallel — not cv::RNG((uint64)-1)'s one sequential
 *                      multiply-with-carry stream drawing 5-point subsets;
 *   2 minimal solver   DEVIATES: P3P on three points, the fourth picks the branch — not EPnP on five points; a sample
 *                      whose three P3P pixels are not pairwise distinct yields no hypothesis;
 *   3 consensus loop   SAME: squared reprojection error <= 5^2 px, a hypothesis replaces the best one only with MORE inliers
 *                      (and at least 5: goodCount > max(maxGoodCount, modelPoints - 1), modelPoints = 5; a best
 *                      hypothesis of 4 inliers is no model), RANSACUpdateNumIters(confidence, outlier share, 5 model points) after every new
 *                      best one, hypotheses looked at in order (the kernel scores them in parallel rounds and walks each
 *                      round in order);
 *   4 final refit      SAME objective and set (reprojection error over the inliers of the best hypothesis, all in double),
 *                      other minimiser and start: damped Gauss-Newton to convergence from the caller's guess (or the best
 *                      hypothesis) — OpenCV runs <= 20 Levenberg-Marquardt steps from the LAST hypothesis its loop
 *                      evaluated (the callback writes every hypothesis into the guess buffers);
 *   5 points behind    DEVIATES: a point is an inlier only in front of the camera (depth > 1e-9).  cv::projectPoints
 *     the camera       divides by a negative depth, so OpenCV counts a point behind the camera whose mirrored projection
 *                      lands within 5 px; such a point is no evidence for the pose, and the library keeps its test;
 *   6 n <= 5           DEVIATES: when n equals its model points (n = 4: P3P, n = 5: EPnP), solvePnPRansac solves on all
 *                      n points and reports every one an inlier, with no consensus test (from OpenCV's published
 *                      solvepnp.cpp; not checked against a build).  This library runs the same RANSAC loop for every n >= 4:
 *                      n = 4 never has a model, n = 5 has one only when all five agree within 5 px.
 * So the hypothesis sequence differs, the result the call site consumes (success, consensus set, refined pose,
 * cv_ransac_pnp.cpp:59-83) agrees wherever the consensus set is unambiguous: tests/test_pnp.py compares both entry
 * points with that oracle (masks equal, rvec / tvec within 1e-6 on noise-free scenes with 0 - 60 % outliers; within
 * 0.02 degrees / 2 mm with pixel noise, where borderline points may fall either side of 5 px).  The call site's confidence
 * (0.99, :57) ends the loop as in OpenCV's RANSACPointSetRegistrator: every new best hypothesis lowers the iteration
 * count to log(1 - confidence) / log(1 - w^5) (w = its inlier share; 5 = the model points cv::solvePnPRansac samples for this
 * call's flags, although this library's own minimal sample is 3 + 1 points), hypotheses beyond it are not looked at. */
int mslam_hip_pnp_ransac(mslam_hip_ctx* ctx, const float* object_points, const float* image_points, int n, double fx,
                         double fy, double cx, double cy, int use_extrinsic_guess, int iterations,
                         double reprojection_error, uint64_t seed, double* rvec, double* tvec, uint8_t* inliers,
                         int* n_inliers);

/* The RANSAC confidence of both PnP entry points (default 0.99 = the reference's call, cv_ransac_pnp.cpp:57); a value
 * outside (0, 1) switches the early exit off: all `iterations` hypotheses are scored. */
int mslam_hip_pnp_set_confidence(mslam_hip_ctx* ctx, double confidence);

/* Batched device form (the frame-to-frame tracking step of the RGB-D front end on device data): for every frame t >= 1 of
 * the last batch, the matches (frame t -> frame t-1) of mslam_hip_match_batch_dev whose train keypoint has a valid
 * back-projected point (mslam_hip_backproject_batch_dev) become the 3-D / 2-D correspondences
 *   object = xyz[t-1][to] (cast to float, rgbd_feature_frontend.cpp:232-254 / cv_ransac_pnp.cpp:22-31), image = xy[t][from],
 * in match order, and one RANSAC PnP per frame (one workgroup each, no extrinsic guess, seed + t as the sampling seed)
 * estimates the pose of camera t in the coordinates of camera t-1.  Frame 0 has no predecessor inside the batch
 * (status 0).  Results: mslam_hip_pnp_view. */
int mslam_hip_pnp_batch_dev(mslam_hip_ctx* ctx, double fx, double fy, double cx, double cy, int iterations,
                            double reprojection_error, uint64_t seed);
typedef struct
{
    int32_t capacity;          /* per-frame stride of the correspondence arrays (max_keypoints)                 */
    const double* pose;        /* [max_batch][16]: R row-major (9), t (3), inliers, best hypothesis, status, cost;
                                * status 1 = a model was found, 0 = none (fewer than 4 points / 5 inliers)      */
    const int32_t* n_points;   /* [max_batch] correspondences of the frame                                      */
    const float* object_points; /* [max_batch][capacity][3]                                                     */
    const float* image_points;  /* [max_batch][capacity][2]                                                     */
    const uint8_t* inliers;     /* [max_batch][capacity] consensus mask of the best hypothesis                  */
} mslam_hip_pnp_view;
int mslam_hip_get_pnp_view(mslam_hip_ctx* ctx, mslam_hip_pnp_view* view);

/* ---- RANSAC rigid alignment of two 3-D point sets (k_align.hip) -----------------------------------------------------------
 * The least-squares rigid transform between corresponding 3-D points inside a RANSAC loop: the estimator of the metric the
 * back end minimises (the 3-D difference in the camera frame, mslam_hip_bundle_adjust), where RANSAC PnP estimates the
 * reprojection error.  The reference tree has no such estimator (nothing to replace, no file:line): this is an extension,
 * modelled on the fixed-scale Sim3Solver of ORB-SLAM's RGB-D tracking.
 * src = n x 3 f32 (object / world points), dst = n x 3 f32 (camera-frame points); the result is the proper rotation R and
 * translation t with dst_i ~ R src_i + t, i.e. world -> camera as in mslam_hip_pnp_ransac, returned as rvec (Rodrigues) and
 * tvec, 3 doubles each, outputs only: no guess takes part.  inliers (n bytes, may be NULL) is the consensus mask of the best
 * hypothesis, n_inliers (may be NULL) its size.  max_distance is in the unit of the points (metres in the keyframe store).
 * Returns MSLAM_HIP_OK, or MSLAM_HIP_E_NO_MODEL when no hypothesis reaches 4 inliers (n = 3 never has a model) with rvec,
 * tvec and inliers as they were and *n_inliers = 0; MSLAM_HIP_E_INVALID for n < 3, iterations outside 1..4096, a
 * max_distance that is not > 0 (NaN included) or a NULL ctx, src, dst, rvec or tvec.
 * Against mslam_hip_pnp_ransac's loop, piece by piece:
 *   1 sampler          SAME rule (splitmix64 counter streams keyed by (`seed`, hypothesis), a repeated draw is drawn again, more
 *                      than 64 redraws give no hypothesis), three draws instead of four;
 *   2 minimal solver   DEVIATES: the closed-form least-squares rigid transform of the three pairs (centroids, then Horn's unit
 *                      quaternion: the eigenvector of the largest eigenvalue of the 4 x 4 matrix of the cross-covariance, by
 *                      cyclic Jacobi sweeps), never a reflection.  A sample whose source or destination triple has
 *                      |a x b|^2 <= 1e-6 |a|^2 |b|^2 (collinear, coincident, NaN) yields no hypothesis;
 *   3 consensus loop   SAME form: |R src_i + t - dst_i|^2 <= max_distance^2 (a non-finite value is no inlier), a hypothesis
 *                      replaces the best one only with MORE inliers and more than 3 (the sample's own three points prove
 *                      nothing), RANSACUpdateNumIters(confidence, outlier share, 3 model points) after every new best one with
 *                      the confidence of mslam_hip_pnp_set_confidence, hypotheses looked at in order;
 *   4 final refit      DEVIATES: the same closed form over the inliers of the best hypothesis (the optimum of the sum of squared
 *                      3-D distances, no iterations, no start), sums in one fixed order.
 * Two calls on the same input return the same bits.  All arithmetic is f64: + - * / sqrt. */
int mslam_hip_align_ransac(mslam_hip_ctx* ctx, const float* src, const float* dst, int n, int iterations, double max_distance,
                           uint64_t seed, double* rvec, double* tvec, uint8_t* inliers, int* n_inliers);

/* Batched device form, the mirror of mslam_hip_pnp_batch_dev: for every frame t >= 1 of the last batch, the matches (frame t ->
 * frame t-1) whose train keypoint AND query keypoint both have a valid back-projected point become the 3-D / 3-D
 * correspondences
 *   src = (float)xyz[t-1][to], dst = (float)xyz[t][from],
 * in match order, and one alignment per frame (one workgroup each, the problem body of mslam_hip_align_ransac: the same bits,
 * seed + t as the sampling seed) estimates the pose of camera t in the coordinates of camera t-1.  Frame 0 and every frame
 * with fewer than 3 correspondences have status 0.  The buffers are allocated on first use.  Results: mslam_hip_align_view. */
int mslam_hip_align_batch_dev(mslam_hip_ctx* ctx, int iterations, double max_distance, uint64_t seed);
typedef struct
{
    int32_t capacity;          /* per-frame stride of the correspondence arrays (max_keypoints)                      */
    const double* pose;        /* [max_batch][16]: R row-major (9), t (3), inliers, best hypothesis, status, 0;
                                * status 1 = a model was found, 0 = none; NULL before the first batch call          */
    const int32_t* n_points;   /* [max_batch] correspondences of the frame                                           */
    const float* src_points;   /* [max_batch][capacity][3]                                                           */
    const float* dst_points;   /* [max_batch][capacity][3]                                                           */
    const uint8_t* inliers;    /* [max_batch][capacity] consensus mask of the best hypothesis                        */
    const double* single_pose; /* [16] the same record of the last mslam_hip_align_ransac call; NULL before the first */
} mslam_hip_align_view;
/* MSLAM_HIP_E_INVALID until one of the two alignment calls has run. */
int mslam_hip_get_align_view(mslam_hip_ctx* ctx, mslam_hip_align_view* view);

/* Which estimator gives a tracked row its pose.  Context state, the idiom of mslam_hip_set_guided_match: mslam_hip_track,
 * mslam_hip_track_window and mslam_hip_track_window_dev read it when they are called.
 *   MSLAM_HIP_TRACK_POSE_PNP    (default) RANSAC PnP on (landmark, pixel): every entry point enqueues the launches and returns
 *                               the bits it did before this setting existed; max_distance is ignored;
 *   MSLAM_HIP_TRACK_POSE_ALIGN  RANSAC rigid alignment on the same correspondences (matches whose keypoint has a valid depth, in
 *                               match order): src = (float)world[to], dst = (float) the camera-frame point of keypoint `from`,
 *                               which the depth filter of the call already computes on the device; row r runs the call's
 *                               `iterations` with seed + r and this setting's max_distance.  reprojection_error is not used
 *                               (it is still checked), the guess does not reach the estimator and still drives guided
 *                               matching.  Everything behind the pose record (tracked, the vote, the new entry, the window's
 *                               event scan, the MSLAM_HIP_E_* rules) is unchanged.
 * mslam_hip_relocalize has no depth: it runs PnP under either setting.
 * set returns MSLAM_HIP_E_INVALID for an unknown kind, or for ALIGN with a max_distance that is not > 0, and the setting stays.
 * get: either output may be NULL. */
#define MSLAM_HIP_TRACK_POSE_PNP 0
#define MSLAM_HIP_TRACK_POSE_ALIGN 1
int mslam_hip_set_track_pose(mslam_hip_ctx* ctx, int kind, double max_distance);
int mslam_hip_get_track_pose(mslam_hip_ctx* ctx, int* kind, double* max_distance);

/* ---- MinMseTracker::solvePnp (ceres_reprojection_error_pnp.cpp:18-110): min-MSE PnP -----------------------------------
 * The reference's second IPnpAlgorithm: a Ceres Levenberg-Marquardt solve over x = (r, t), r an angle-axis vector and t a
 * translation, of cost = 1/2 sum_i |observed_i - projected_i|^2 with
 *   projected_i = (fx X/Z + cx, fy Y/Z + cy),  (X, Y, Z) = ceres::AngleAxisRotatePoint(r, P_i) + t,
 * no loss function (mslam_hip_set_pnp_mse_loss below sets one: an extension, off by default), all in double, started from
 * the caller's (r, t).  Every point takes part (no outlier rejection).
 * object_points = n x 3 f64, image_points = n x 2 f64, rvec / tvec = the start on input, the result on output.
 * termination (ceres::TerminationType: 0 CONVERGENCE, 1 NO_CONVERGENCE, 2 FAILURE), iterations (trust-region iterations
 * after iteration 0: the index of the iteration that ended the solve) and final_cost may be NULL.
 * Returns MSLAM_HIP_OK for 0 and 1 (Summary::IsSolutionUsable()), MSLAM_HIP_E_NO_MODEL for FAILURE with rvec / tvec left
 * unchanged, MSLAM_HIP_E_INVALID for bad arguments.  n = 0 is OK, termination 0, pose unchanged, cost 0: Ceres's
 * solver.cc Minimize() reports "No non-constant parameter blocks found" as CONVERGENCE for a problem whose reduced
 * program has no parameter blocks (restated from the published source; not checked against a build).
 * Against Ceres 2.2 as the call site configures it (gradient / function / parameter tolerance 1e-8, :88-90; all else the
 * Solver::Options defaults), restated from the published trust_region_minimizer.cc, levenberg_marquardt_strategy.cc,
 * trust_region_step_evaluator.cc and solver.h.  PARITY UNPINNED: no Ceres build exists to compare with; the tests compare
 * with an independent numpy restatement (tests/mse_pnp_ref.py) and with ground truth.
 *   residual + derivatives   SAME function (AngleAxisRotatePoint with its theta^2 <= DBL_EPSILON branch p + r x p, then
 *                            the pin-hole, then observed - projected); derivatives by forward-mode dual numbers with
 *                            jet.h's formulas (the rotation on 3-slot jets: its translation slots are exactly 0);
 *   sin / cos                DEVIATES in the last bits: the device's f64 sin / cos, not the host C library's;
 *   sums                     DEVIATES in rounding: cost, J^T J and J^T f are summed per lane, then by a fixed butterfly,
 *                            not in Ceres's evaluation order;
 *   linear solver            DEVIATES in rounding: Cholesky of the 6x6 normal equations (J_s^T J_s + D^2) y = J_s^T f
 *                            with D^2 = clamp(diag(J_s^T J_s), 1e-6, 1e32) / radius, instead of DENSE_QR (or
 *                            SPARSE_NORMAL_CHOLESKY) on the D-augmented system; the model cost change
 *                            -(f^T J_s d + |J_s d|^2 / 2) is evaluated from the normal equations.  A non-positive pivot
 *                            or a non-finite step is a linear-solver failure = an invalid step, as in Ceres;
 *   Jacobi scaling           SAME: 1 / (1 + |J_col|) from the Jacobian at the start, once;
 *   trust region             SAME: radius 1e4 .. 1e16, ends below 1e-32; accepted step (relative decrease > 1e-3,
 *                            monotonic): radius /= max(1/3, 1 - (2 rho - 1)^3), decrease factor 2; rejected step:
 *                            radius /= factor, factor *= 2; 5 invalid steps in a row: FAILURE;
 *   candidate point          SAME: a candidate whose cost is not finite counts as cost DBL_MAX (a rejected step, as
 *                            ComputeCandidatePointAndEvaluateCost does; it is not an "invalid step");
 *   termination              SAME order: iteration 50 -> NO_CONVERGENCE; successful step with |x - (x - g)|_inf <= 1e-8,
 *                            radius <= 1e-32, |x - x_candidate| <= 1e-8 (|x| + 1e-8) or |cost change| <= 1e-8 cost
 *                            -> CONVERGENCE (the candidate of the last two is not taken); non-finite cost or Jacobian
 *                            at the start or at an accepted point -> FAILURE;
 *   evaluation valid         DEVIATES for derivatives above about 1.3e154 (sqrt(DBL_MAX)): the kernel keeps sums, not
 *                            entries, and calls an evaluation valid when the cost, the diagonal of J^T J and J^T f are
 *                            finite.  A NaN or infinite residual or derivative always shows there.  A finite residual
 *                            derivative whose square overflows also does, and is treated as a failed evaluation
 *                            (FAILURE at the start or at an accepted point); Ceres tests the entries themselves
 *                            (ResidualBlock::Evaluate) and would continue.  It takes a point at a depth near 1e-150 of
 *                            its lateral offset; tests/test_gpu_mse_pnp_edges.py pins the case;
 *   FAILURE result           DEVIATES: the pose is left unchanged (Ceres writes its best point back; the reference
 *                            discards it: IsSolutionUsable() is false);
 *   progress printout        not reproduced (minimizer_progress_to_stdout, :91). */
int mslam_hip_pnp_min_mse(mslam_hip_ctx* ctx, const double* object_points /* n x 3 */, const double* image_points /* n x 2 */,
                          int n, double fx, double fy, double cx, double cy,
                          double* rvec /* in: start, out: result */, double* tvec /* in/out */,
                          int* termination /* may be NULL */, int* iterations /* may be NULL */, double* final_cost /* may be NULL */);
/* Batched, device pointers, asynchronous on the context's stream (one wave64 per problem): problem p has n[p] <= capacity
 * points at object[p*capacity*3], image[p*capacity*2]; pose[p*6 .. +6] = (r, t) in / out (out only when the termination
 * is not FAILURE); info[p*4 .. +4] = termination, iterations, initial cost, final cost.  n[p] outside [0, capacity] is
 * FAILURE.  The single-problem call launches this same kernel, so a problem gives bit-identical results either way. */
int mslam_hip_pnp_min_mse_batch_dev(mslam_hip_ctx* ctx, const double* d_object, const double* d_image, const int32_t* d_n,
                                    int n_problems, int capacity, double fx, double fy, double cx, double cy,
                                    double* d_pose, double* d_info);

/* ---- CeresBackend::bundleAdjustment (ceres_backend.cpp:185-240): bundle adjustment ------------------------------------
 * What the reference's backend solves on every new keyframe: Levenberg-Marquardt over keyframe poses and landmarks of
 *   cost = 1/2 sum_m |r_m|^2,   r_m = rot(q^-1, X) - rot(q^-1, p) - obs_cam[m]      (ReprojectionError::operator(), :31-47)
 * with (q, p) the state of keyframe obs_kf[m] (orientation x y z w, position; camera -> world), X landmark obs_lm[m] and
 * obs_cam[m] the camera-frame point ReprojectionError's constructor forms from the keypoint and its depth (:24-28); no loss
 * function, all in double (mslam_hip_set_ba_loss below sets one: an extension, off by default).  The problem is handed over
 * explicitly:
 *   poses      K x 7 (qx qy qz qw px py pz), K in 0..64, in: start, out: result; fixed[k] != 0 holds pose k constant (the
 *              reference fixes keyframe id 1, :155-159); fixed == NULL: none;
 *   landmarks  L x 3, in / out;   obs_kf, obs_lm, obs_cam: M observations, indices into poses / landmarks.
 * A free pose has 6 tangent dimensions (EigenQuaternionManifold's Plus, q_delta (x) q with q_delta = (sin|d| d/|d|, cos|d|),
 * and the position), a landmark 3.  A pose or landmark without an observation is not part of the problem and stays as it is.
 * After the solve outlier[m] (may be NULL) = |r_m|^2 > outlier_threshold^2 at the returned state (createOutput, :212-230;
 * the reference's threshold is 0.15); nothing is removed (removeObservation's body is commented out there).
 * summary (may be NULL): termination (ceres::TerminationType 0 CONVERGENCE / 1 NO_CONVERGENCE / 2 FAILURE), iterations (the
 * index of the trust-region iteration that ended the solve), rejected and invalid steps, initial and final cost, n_outliers.
 * Returns MSLAM_HIP_OK for terminations 0 and 1; MSLAM_HIP_E_NO_MODEL for FAILURE: poses and landmarks are left unchanged
 * and the outliers are judged at the inputs.  MSLAM_HIP_E_INVALID: K outside 0..64, a negative count, an index out of range,
 * max_iterations < 0, a threshold that is not >= 0, or a quaternion whose norm is off 1 by more than 1e-6 (DEVIATES: the
 * reference's quaternions are unit by construction).  M = 0 is CONVERGENCE at cost 0, nothing touched (as n = 0 is for
 * mslam_hip_pnp_min_mse).  Two calls on the same input return the same bits: no sum uses an atomic, every sum has one order.
 * Against Ceres 2.2 with the Solver::Options bundleAdjustment sets (:193-195: max_num_iterations; everything else default,
 * restated from the published solver.h: function tolerance 1e-6, gradient tolerance 1e-10, parameter tolerance 1e-8, initial
 * radius 1e4, monotonic steps, Jacobi scaling).  PARITY UNPINNED: no Ceres build exists to compare with; the tests compare
 * with an independent numpy restatement (tests/ba_ref.py, two linear solvers) and with ground truth.
 *   residual                 SAME expression: Eigen's inverse() (conjugate / squared norm) and _transformVector
 *                            (v + w 2(u x v) + u x 2(u x v)) on both X and p;
 *   derivatives              DEVIATES in rounding: analytic, dr/dX = R^T, dr/dp = -R^T, dr/d(delta) = 2 R^T [X - p]x with R^T
 *                            the matrix of the same linear map, instead of jets times PlusJacobian; equal for unit q;
 *   sums                     DEVIATES in rounding: per landmark in row order, per keyframe by lane stride then a fixed
 *                            butterfly, costs by a fixed two-stage tree; not Ceres's evaluation order;
 *   linear solver            DEVIATES in rounding: Schur complement on the landmarks (3x3 blocks inverted in closed form),
 *                            dense Cholesky of the reduced camera system (at most 384 x 384) in global memory, back-
 *                            substitution; the reference asks for SPARSE_NORMAL_CHOLESKY on the whole system.  A non-positive
 *                            pivot or a non-finite step is an invalid step, as a linear-solver failure is in Ceres;
 *   Jacobi scaling           SAME: 1 / (1 + |J_col|) per tangent column from the Jacobian at the start, once;
 *   trust region             SAME as mslam_hip_pnp_min_mse: radius 1e4 .. 1e16, D^2 = clamp(diag, 1e-6, 1e32) / radius,
 *                            model cost change -(J_s s) . (f + J_s s / 2) summed per observation without the damping,
 *                            relative decrease > 1e-3, radius /= max(1/3, 1 - (2 rho - 1)^3), rejected: radius /= factor,
 *                            factor *= 2; 5 invalid steps in a row: FAILURE;
 *   termination              SAME order, on the ambient parameters (7 per pose, 3 per landmark) of the blocks that have
 *                            observations and are not constant: max_iterations -> NO_CONVERGENCE; successful step with
 *                            |x - Plus(x, -g)|_inf <= 1e-10, radius <= 1e-32, |x - x_candidate| <= 1e-8 (|x| + 1e-8) or
 *                            |cost change| <= 1e-6 cost -> CONVERGENCE; non-finite cost or gradient -> FAILURE;
 *   FAILURE result           DEVIATES: the state is left unchanged (Ceres writes its best point back);
 *   sizes                    DEVIATES: at most 64 keyframes per solve (the reduced system is dense); the reference has no
 *                            bound. */
typedef struct
{
    int32_t termination, iterations, rejected_steps, invalid_steps, n_outliers, reserved;
    double initial_cost, final_cost;
} mslam_hip_ba_summary;
int mslam_hip_bundle_adjust(mslam_hip_ctx* ctx, double* poses /* K x 7, in/out */, const uint8_t* fixed /* K, or NULL */,
                            int K /* 0..64 */, double* landmarks /* L x 3, in/out */, int L, const int32_t* obs_kf,
                            const int32_t* obs_lm, const double* obs_cam /* M x 3 */, int M, int max_iterations /* 100 */,
                            double outlier_threshold /* 0.15 */, uint8_t* outlier /* M, may be NULL */,
                            mslam_hip_ba_summary* summary /* may be NULL */);
/* ---- CeresBackend::globalBundleAdjustment (ceres_backend.cpp:173-183): the same solve over every keyframe of the map ----
 * The reference's only loop correction (closeLoop is a TODO there).  Arguments, summary, residual, manifold, trust region,
 * termination order, FAILURE behaviour, outlier mask, determinism and the MSLAM_HIP_E_INVALID rules are those of
 * mslam_hip_bundle_adjust, with K in 0..MSLAM_HIP_BA_GLOBAL_MAX_KEYFRAMES, and the reduced camera system is always built and
 * solved by the blocked solver below, at any K (so small problems compare the two solvers).  No loss function either, unless
 * mslam_hip_set_ba_loss below sets one.  Every row of
 * mslam_hip_bundle_adjust's SAME / DEVIATES table holds here except these two:
 *   linear solver            DEVIATES in rounding: Schur complement on the landmarks (3x3 blocks inverted in closed form) over
 *                            the covisible pairs of keyframes only (pairs that share a landmark, from a sorted list built on
 *                            the host), blocked dense Cholesky of the reduced camera system over many workgroups (panels of
 *                            48 columns: the diagonal block in one workgroup, the panel's triangular solve by row tiles, the
 *                            trailing update on the f64 matrix cores; the right-hand side is carried as one more row), blocked
 *                            back-substitution; the reference asks for SPARSE_NORMAL_CHOLESKY on the whole system.  A
 *                            non-positive pivot in any panel or a non-finite step is an invalid step.  UNTESTED: no test
 *                            reaches a non-positive pivot (the damping keeps the reduced system positive definite for
 *                            finite input and no scene found so far loses that to rounding), so the path from a panel's
 *                            pivot flag through the invalid-step handling to a retry or FAILURE has never run, here or
 *                            in mslam_hip_bundle_adjust;
 *   sizes                    DEVIATES: at most 1024 keyframes per solve: the reduced system is kept dense, 6144^2 doubles
 *                            = 302 MB of device memory at the bound; the reference has no bound.  With
 *                            mslam_hip_set_ba_global_solver(SPARSE), further down, 16384 keyframes and an envelope of
 *                            1048576 blocks. */
#define MSLAM_HIP_BA_GLOBAL_MAX_KEYFRAMES 1024
int mslam_hip_bundle_adjust_global(mslam_hip_ctx* ctx, double* poses /* K x 7, in/out */, const uint8_t* fixed /* K, or NULL */,
                                   int K /* 0..1024 */, double* landmarks /* L x 3, in/out */, int L, const int32_t* obs_kf,
                                   const int32_t* obs_lm, const double* obs_cam /* M x 3 */, int M, int max_iterations /* 100 */,
                                   double outlier_threshold /* 0.15 */, uint8_t* outlier /* M, may be NULL */,
                                   mslam_hip_ba_summary* summary /* may be NULL */);
/* ---- A loss function for both bundle adjustment entries (an extension: the reference passes lossFunction = nullptr) ----
 * Context state, the idiom of mslam_hip_set_guided_match: mslam_hip_bundle_adjust and mslam_hip_bundle_adjust_global read it
 * when they are called.  mslam_hip_pose_graph and mslam_hip_pnp_min_mse do NOT read it (they have settings of their own:
 * mslam_hip_set_pose_graph_loss and mslam_hip_set_pnp_mse_loss below).  The default is NONE: both entries
 * then launch the kernels they launched before this setting existed, and every result keeps its bits.
 * The loss is per residual block, s = |r_m|^2 (the three camera-frame components together), scale a in metres, b = a^2:
 *   HUBER    s <= b: rho = s, rho' = 1;   else rho = 2 a sqrt(s) - b, rho' = max(DBL_MIN, a / sqrt(s))
 *   CAUCHY   rho = b log(1 + s / b), rho' = max(DBL_MIN, 1 / (1 + s / b))
 * cost = 1/2 sum_m rho(|r_m|^2): initial_cost and final_cost of mslam_hip_ba_summary report that.  The residual and the
 * three Jacobian blocks of observation m are scaled by sqrt(rho'); U, V, W, both gradients, the Jacobi scaling taken at the
 * start, the model cost change, the gradient test and the function and parameter tolerances follow from the corrected
 * blocks.  The outlier mask stays |r_m|^2 > outlier_threshold^2 on the UNCORRECTED residual at the returned state.  There is
 * no default scale.  Two calls on the same input and setting return the same bits.
 * set returns MSLAM_HIP_E_INVALID for a kind outside 0..2 or, for HUBER / CAUCHY, a scale that is not finite or not > 0; the
 * setting is then unchanged.  With NONE the scale is ignored and reported as 0.  get: either pointer may be NULL.
 * Against Ceres 2.2 (loss_function.h, corrector.cc, restated from the published text).  PARITY UNPINNED as for the solver:
 * the tests compare with tests/ba_loss_ref.py, which applies the corrector to tests/ba_ref.py's residuals and Jacobians.
 *   loss formulas            SAME: HuberLoss::Evaluate and CauchyLoss::Evaluate, s == b on Huber's inlier branch, Cauchy's
 *                            1 + s c with c = 1 / b;
 *   corrector                SAME branch: rho'' <= 0 everywhere for both kinds, so Corrector takes `sq_norm == 0 || rho[2] <=
 *                            0`: sqrt(rho') on residual and Jacobians, no curvature term.  The other branch cannot occur;
 *   weight                   DEVIATES in rounding: rho' multiplies every product of observation m (J^T J, J^T r, the model
 *                            term) where Ceres scales the rows by sqrt(rho') first;
 *   other losses             not built: SoftLOne, Arctan, Tolerant, Tukey (Tukey has rho'' > 0 and needs the full
 *                            corrector), per-observation scales. */
#define MSLAM_HIP_BA_LOSS_NONE 0
#define MSLAM_HIP_BA_LOSS_HUBER 1
#define MSLAM_HIP_BA_LOSS_CAUCHY 2
int mslam_hip_set_ba_loss(mslam_hip_ctx* ctx, int kind, double scale);
int mslam_hip_get_ba_loss(mslam_hip_ctx* ctx, int* kind, double* scale);
/* ---- RgbdFeatureFrontend::closeLoop (rgbd_feature_frontend.cpp:577-580, an empty body; called at :198-205): pose graph ----
 * The correction a detected loop asks for: Levenberg-Marquardt over keyframe poses of
 *   cost = 1/2 sum_e |r_e|^2,   r_e = sqrt_info_e [p_ab - p_meas ; 2 vec(delta)]
 *   p_ab = rot(q_a^-1, p_b - p_a),  q_ab = q_a^-1 (x) q_b,  delta = q_meas (x) q_ab^-1
 * the error term of Ceres's published pose_graph_3d example (pose_graph_3d_error_term.h), taken because the reference's
 * backend is Ceres with EigenQuaternionManifold.  NO SIGN FIX is applied on delta: q and -q name one rotation, but a
 * measurement or a pose entered with the other sign turns 2 vec(delta) round (delta is then near (0, 0, 0, -1)); the solve
 * still reaches the same poses, with the quaternion's sign kept, because the rotation error enters squared.
 *   poses      K x 7 (qx qy qz qw px py pz, camera -> world; mslam_hip_bundle_adjust's layout), K in
 *              0..MSLAM_HIP_BA_GLOBAL_MAX_KEYFRAMES (0..MSLAM_HIP_POSE_GRAPH_MAX_KEYFRAMES_SPARSE with the SPARSE solver), in: start, out: result; fixed[k] != 0 holds pose k constant; NULL: none;
 *   edge_a, edge_b   E edges, E in 0..MSLAM_HIP_POSE_GRAPH_MAX_EDGES, indices into poses; duplicates and both directions
 *              between one pair are allowed;
 *   edge_meas  E x 7: q then p of pose b expressed in a's frame (T_a^-1 T_b);
 *   sqrt_info  E x 36, row-major 6 x 6 per edge (rows and columns: position, then rotation), or NULL for identity.
 * A free pose has the 6 tangent dimensions of mslam_hip_bundle_adjust.  A pose without an edge, or a constant one, is not
 * part of the problem and comes back bit for bit.  summary: mslam_hip_ba_summary with n_outliers = 0.
 * Returns MSLAM_HIP_OK for terminations 0 and 1; MSLAM_HIP_E_NO_MODEL for FAILURE: the poses are left unchanged.
 * MSLAM_HIP_E_INVALID: K or E out of range, an index out of range, edge_a[e] == edge_b[e], max_iterations < 0, a pose or
 * measurement quaternion whose norm is off 1 by more than 1e-6, a non-finite sqrt_info.  E = 0 is CONVERGENCE at cost 0,
 * nothing touched.  Two calls on the same input return the same bits: no sum uses an atomic, every sum has one order.  All
 * arithmetic is f64.  Against Ceres 2.2 with default Solver::Options but max_num_iterations.  PARITY UNPINNED: no Ceres build
 * exists to compare with; the tests compare with an independent numpy restatement (tests/pose_graph_ref.py: jets, two linear
 * solvers) and with ground truth.
 *   residual                 SAME expression for unit quaternions: Eigen's inverse() (conjugate / squared norm) where the
 *                            example writes conjugate(), Eigen's quaternion product and _transformVector;
 *   derivatives              DEVIATES in rounding: analytic (the matrices are written out in k_posegraph.hip and DESIGN.md
 *                            4.17) instead of jets times PlusJacobian; equal for unit q;
 *   sums                     DEVIATES in rounding: per pose over its edges by lane stride then a fixed butterfly, per pair of
 *                            poses in edge order, costs by a fixed two-stage tree; not Ceres's evaluation order.  The sum of a
 *                            pair is one wave's serial loop over the pair's edges: bounded by E, and the slow shape when
 *                            many duplicate edges join one pair (65536 between two poses is one loop of 65536 steps);
 *   linear solver            DEVIATES in rounding: the damped normal equations J^T J + D^2 over the free poses.  DENSE (the
 *                            default): dense, by mslam_hip_bundle_adjust_global's blocked Cholesky (the same kernels) at
 *                            every K.  SPARSE (mslam_hip_set_pose_graph_solver below): a Cholesky factor on the block
 *                            envelope after a NATURAL or reverse Cuthill-McKee order, the shape of the example's
 *                            SPARSE_NORMAL_CHOLESKY, though not its ordering (AMD) or its supernodal factor; the diagonal's
 *                            reciprocal is multiplied with where DENSE divides.  In both a pivot that is not > 0 (SPARSE:
 *                            or not finite) or a non-finite step is an invalid step;
 *   Jacobi scaling, trust region, termination order, FAILURE result
 *                            those of mslam_hip_bundle_adjust (SAME / DEVIATES as stated there); termination is judged on
 *                            the ambient parameters (7 per pose) of the free poses that have an edge;
 *   sizes                    DEVIATES: at most 65536 edges per solve and, with DENSE, 1024 poses: the reduced system is then the
 *                            dense 6 K x 6 K matrix of the free poses (6144^2 doubles = 302 MB at the bound, the buffer global
 *                            bundle adjustment uses; no second one is allocated), although a pose graph's normal equations are
 *                            sparse (a chain's are block-tridiagonal).  With SPARSE at most 16384 poses and an envelope of
 *                            1048576 blocks (288 MiB, in the same buffer).  The per-edge blocks (residual, two Jacobians,
 *                            measurement, sqrt_info: 121 doubles) take 63 MB at the edge bound. */
#define MSLAM_HIP_POSE_GRAPH_MAX_EDGES 65536
int mslam_hip_pose_graph(mslam_hip_ctx* ctx, double* poses /* K x 7, in/out */, const uint8_t* fixed /* K, or NULL */,
                         int K /* 0..1024; SPARSE: 0..16384 */, const int32_t* edge_a, const int32_t* edge_b, const double* edge_meas /* E x 7 */,
                         const double* sqrt_info /* E x 36, or NULL */, int E, int max_iterations /* 100 */,
                         mslam_hip_ba_summary* summary /* may be NULL */);
/* ---- The linear solver of mslam_hip_pose_graph (an extension) ----
 * Context state, the idiom of mslam_hip_set_ba_loss and mslam_hip_set_guided_match: mslam_hip_pose_graph reads it when it is
 * called.  DENSE is the default: every launch and every result bit is what it was before this setting existed, and K > 1024
 * is MSLAM_HIP_E_INVALID.  With SPARSE K may reach MSLAM_HIP_POSE_GRAPH_MAX_KEYFRAMES_SPARSE and the linear solve of an
 * iteration is a Cholesky factor on the block envelope (skyline) of the damped normal equations in 6 x 6 blocks; memory and
 * work follow the envelope, not K^2.  Everything else of the solve (blocks, step, trust region, Jacobi scaling, damping,
 * termination order, the FAILURE rule) is shared.  set returns MSLAM_HIP_E_INVALID for a kind outside 0..1 and the setting
 * stays.  Two SPARSE calls on the same input return the same bits; SPARSE and DENSE differ in rounding.
 * The symbolic phase (host, per call).  Nodes are the free poses that have an edge; two nodes are adjacent when an edge joins
 * them (duplicates count once, edges to constant poses not at all).  Two orders are computed:
 *   NATURAL  ascending pose index;
 *   RCM      components one after another; each starts at the unvisited node of least degree (ties: the smallest index; no
 *            pseudo-peripheral search); breadth first from there, the unvisited neighbours of the node being expanded appended in
 *            ascending (degree, index); the whole visiting order reversed at the end.
 * With first[i] the least position among row i's neighbours and i itself, the envelope is sum (i - first[i] + 1) blocks; the
 * order with the smaller envelope is taken, NATURAL on a tie.  An envelope above MSLAM_HIP_POSE_GRAPH_MAX_ENVELOPE_BLOCKS is
 * MSLAM_HIP_E_CAPACITY from mslam_hip_pose_graph (the message names the count; nothing is touched).  One workgroup factors
 * the envelope column by column, so a dense pattern is far slower than with DENSE: SPARSE is for long, thin graphs.
 * mslam_hip_pose_graph_analyze is that phase without a context or a GPU: order (pose index per position) and first take K
 * entries of which *n_free are written; *ordering is 0 NATURAL or 1 RCM; any output may be NULL.  Its checks are those of
 * mslam_hip_pose_graph with SPARSE: K in 0..16384, E in 0..65536, indices in range, no edge from a pose to itself
 * (MSLAM_HIP_E_INVALID, nothing written).  It returns MSLAM_HIP_E_CAPACITY, with every output written, when the envelope is
 * above the bound. */
#define MSLAM_HIP_PG_SOLVER_DENSE 0
#define MSLAM_HIP_PG_SOLVER_SPARSE 1
#define MSLAM_HIP_POSE_GRAPH_MAX_KEYFRAMES_SPARSE 16384
#define MSLAM_HIP_POSE_GRAPH_MAX_ENVELOPE_BLOCKS 1048576
int mslam_hip_set_pose_graph_solver(mslam_hip_ctx* ctx, int kind);
int mslam_hip_get_pose_graph_solver(mslam_hip_ctx* ctx, int* kind);
int mslam_hip_pose_graph_analyze(const uint8_t* fixed /* K, or NULL */, int K, const int32_t* edge_a, const int32_t* edge_b, int E,
                                 int32_t* order /* K: pose index per position, n_free used */, int32_t* first /* K */,
                                 int* n_free, int* ordering /* 0 NATURAL, 1 RCM */, int64_t* envelope_blocks);
/* ---- The linear solver of mslam_hip_bundle_adjust_global (an extension) ----
 * Context state, the idiom of mslam_hip_set_pose_graph_solver: mslam_hip_bundle_adjust_global reads it when it is called;
 * mslam_hip_bundle_adjust (at most 64 keyframes) and mslam_hip_pose_graph do NOT read it.  DENSE is the default: every launch,
 * every result bit and every error code is what it was before this setting existed, and K > 1024 is MSLAM_HIP_E_INVALID.
 * With SPARSE K may reach MSLAM_HIP_BA_GLOBAL_MAX_KEYFRAMES_SPARSE (above it: MSLAM_HIP_E_INVALID; L and M at most 2^24 as
 * before) and the reduced camera system is kept and factored on its block envelope (skyline) in 6 x 6 blocks, by the factor
 * and the substitution of the pose graph's SPARSE solver (the same kernels); the Schur complement over the covisible pairs
 * is written into the envelope, one wave per pair, with the sums of DENSE in their order.  Memory and work follow the
 * envelope, not K^2.  Everything else of the solve is shared with DENSE, one code: the blocks U / V / W, Jacobi scaling,
 * damping, the loss (mslam_hip_set_ba_loss applies unchanged), candidate, evaluation, trust-region control, termination
 * order, the FAILURE rule, the outlier mask, the stage names solver_schur / solver_factor / solver_subst.  A pivot that is
 * not > 0 or not finite is an invalid step.  set returns MSLAM_HIP_E_INVALID for a kind outside 0..1 and the setting stays.
 * Two SPARSE calls on the same input return the same bits; SPARSE and DENSE differ in rounding (another elimination order,
 * and the diagonal's reciprocal is multiplied with where DENSE divides).
 * The symbolic phase (host, per call).  Nodes are the free keyframes that have at least one observation; unlike in the pose
 * graph, a node needs no neighbour: a free keyframe that shares no landmark with another free keyframe is a row all the
 * same, a node of degree 0.  Two nodes are adjacent when they share a landmark (landmarks shared with a constant keyframe
 * only join nothing).  The orders NATURAL and RCM, first[], the envelope and the choice (the smaller envelope, NATURAL on a
 * tie) are those of mslam_hip_set_pose_graph_solver above, word for word; under RCM the nodes of degree 0 start first and so
 * end last.  The bound is MSLAM_HIP_POSE_GRAPH_MAX_ENVELOPE_BLOCKS, the same buffer (288 MiB): an envelope above it is
 * MSLAM_HIP_E_CAPACITY from mslam_hip_bundle_adjust_global; the message names the block count and nothing is touched
 * (poses, landmarks and the outlier array keep their bytes).
 * One workgroup factors the envelope column by column, so a map with wide covisibility (a landmark many keyframes see, a
 * keyframe covisible with most others) is far slower than with DENSE at K <= 1024: SPARSE is for long trajectories whose
 * keyframes share landmarks with their neighbours and at loop closures.  tools/ba_global_sparse_latency.py measures both;
 * DESIGN.md 4.26 has one run of it (thin rings: SPARSE about 3x faster per iteration up to 1024 keyframes; a complete map
 * of 128 keyframes: 12x slower).  A map that revisits its ground has neither a thin envelope nor few keyframes:
 * mslam_hip_set_ba_global_pcg, below, is for it.
 * mslam_hip_bundle_adjust_global_analyze is the symbolic phase without a context or a GPU: order (keyframe index per
 * position) and first take K entries of which *n_free are written; *ordering is 0 NATURAL or 1 RCM; *n_pairs the covisible
 * pairs k1 <= k2, diagonal included (the waves of the Schur kernel); any output may be NULL.  Its checks are those of the
 * solve with SPARSE: K in 0..16384, L and M in 0..2^24, indices in range (MSLAM_HIP_E_INVALID, nothing written).  It returns
 * MSLAM_HIP_E_CAPACITY, with every output written, when the envelope is above the bound. */
#define MSLAM_HIP_BA_GLOBAL_SOLVER_DENSE 0
#define MSLAM_HIP_BA_GLOBAL_SOLVER_SPARSE 1
#define MSLAM_HIP_BA_GLOBAL_MAX_KEYFRAMES_SPARSE 16384
int mslam_hip_set_ba_global_solver(mslam_hip_ctx* ctx, int kind);
int mslam_hip_get_ba_global_solver(mslam_hip_ctx* ctx, int* kind);
int mslam_hip_bundle_adjust_global_analyze(const uint8_t* fixed /* K, or NULL */, int K, const int32_t* obs_kf, const int32_t* obs_lm,
                                           int M, int L, int32_t* order /* K: keyframe index per position, n_free used */,
                                           int32_t* first /* K */, int* n_free, int* ordering /* 0 NATURAL, 1 RCM */,
                                           int64_t* envelope_blocks, int* n_pairs);
/* ---- An iterative linear solver for mslam_hip_bundle_adjust_global (an extension) ----
 * Block-Jacobi preconditioned conjugate gradients (PCG) on the reduced camera system, for maps that revisit their ground:
 * covisibility that is neither thin (SPARSE's envelope passes its bound) nor small (DENSE stops at 1024 keyframes), while the
 * reduced system itself has few non-zero blocks.  A setting of its own, context state, read by mslam_hip_bundle_adjust_global
 * alone when it is called; mslam_hip_bundle_adjust and mslam_hip_pose_graph do not read it.  Off by default: with enable = 0
 * every launch, result bit and error code is what mslam_hip_set_ba_global_solver's kind gives.  With enable = 1 the global
 * solve uses PCG whatever that kind is, and leaves it untouched.  mslam_hip_set_ba_global_solver keeps its two kinds.
 *   max_iterations  the cap on CG iterations per linear solve, >= 1; MSLAM_HIP_BA_GLOBAL_PCG_MAX_ITERATIONS (500) by default;
 *   tolerance       CG ends at |r_k|_2 <= tolerance |b|_2; in (0, 1); MSLAM_HIP_BA_GLOBAL_PCG_TOLERANCE (1e-6) by default.
 * set returns MSLAM_HIP_E_INVALID and changes nothing for enable outside 0..1, max_iterations < 1 or a tolerance that is not
 * inside (0, 1) (a NaN included); the three are checked whatever enable is.  get: any pointer may be NULL.
 * Caps.  K <= MSLAM_HIP_BA_GLOBAL_MAX_KEYFRAMES_SPARSE (above it: MSLAM_HIP_E_INVALID).  The stored 6 x 6 blocks are the free
 * observed keyframes plus the covisible pairs k1 < k2 of them: *n_pairs of mslam_hip_bundle_adjust_global_analyze.  They live
 * in the buffer of the other two solvers and may be at most MSLAM_HIP_POSE_GRAPH_MAX_ENVELOPE_BLOCKS; above that the call is
 * MSLAM_HIP_E_CAPACITY, the message names the count and nothing is touched.  No order and no envelope is computed.
 * The solve.  The Schur complement over the covisible pairs is written block by block, one wave per pair, with the sums of
 * DENSE in their order.  The preconditioner is the inverse of every diagonal block (Cholesky; a pivot that is not > 0 or not
 * finite makes the step invalid, as a bad pivot of the other solvers does).  CG starts at y = 0; b = 0 gives y = 0 with no
 * iteration; p . q that is not > 0 or not finite is a breakdown and makes the step invalid; at the cap the iterate is taken.
 * The step is inexact; the model cost change is taken from J s per observation as before, which holds for any step, so the
 * trust region is unchanged, as are the blocks U / V / W, Jacobi scaling, damping, the loss, the back-substitution, candidate,
 * evaluation, control, termination order, the FAILURE rule and the outlier mask.  Stage names: solver_schur, solver_precond,
 * solver_cg.  Every sum has one order that does not depend on the launch grid, there are no atomics, and the stopping index is
 * decided on the device: two calls on the same input and setting return the same bits.
 * mslam_hip_get_ba_global_pcg_stats reports the last mslam_hip_bundle_adjust_global of the context (all zero after a solve
 * without PCG, or one that formed no system); mslam_hip_ba_summary is unchanged.
 * Against Ceres 2.2's ITERATIVE_SCHUR (iterative_schur_complement_solver.cc, conjugate_gradients_solver.cc, restated from the
 * published text).  PARITY UNPINNED as for every solver here: the tests compare with tests/ba_global_pcg_ref.py.
 *   the system               DEVIATES: S is formed explicitly, block by block; Ceres's default applies it implicitly
 *                            (ImplicitSchurComplement) and forms it only with use_explicit_schur_complement;
 *   preconditioner           the block diagonal of S: Ceres's SCHUR_JACOBI.  DEVIATES from its default for this solver type
 *                            (JACOBI, the block diagonal of the camera blocks U alone);
 *   recurrence               SAME: preconditioned CG from x = 0, beta = r.z / (r.z)_old;
 *   stopping rule            DEVIATES: |r| <= tolerance |b| with a fixed tolerance.  Ceres ends on its Q-tolerance
 *                            (the decrease of the quadratic model, Nash & Sofer) or r_tolerance, with the forcing sequence
 *                            eta of its trust-region strategy; neither is built.  tolerance 0.1 (Ceres's eta) is not safe
 *                            here: DESIGN.md 4.29;
 *   the cap                  SAME: max_linear_solver_iterations = 500, the iterate at the cap is used;
 *   breakdown                Ceres reports LINEAR_SOLVER_FAILURE for a non-positive p . q; here the step is invalid, which
 *                            the trust region treats alike. */
#define MSLAM_HIP_BA_GLOBAL_PCG_MAX_ITERATIONS 500
#define MSLAM_HIP_BA_GLOBAL_PCG_TOLERANCE 1e-6
typedef struct mslam_hip_pcg_stats
{
    int64_t solves;     /* linear solves */
    int64_t iterations; /* CG iterations over all of them */
    int64_t longest;    /* CG iterations of the longest */
    int64_t at_cap;     /* solves that ended at max_iterations */
    int64_t breakdowns; /* solves that ended with p . q not > 0 or not finite */
} mslam_hip_pcg_stats;
int mslam_hip_set_ba_global_pcg(mslam_hip_ctx* ctx, int enable, int max_iterations, double tolerance);
int mslam_hip_get_ba_global_pcg(mslam_hip_ctx* ctx, int* enable, int* max_iterations, double* tolerance);
int mslam_hip_get_ba_global_pcg_stats(mslam_hip_ctx* ctx, mslam_hip_pcg_stats* stats);
/* ---- An iterative linear solver for mslam_hip_pose_graph (an extension) ----
 * The same block-Jacobi preconditioned conjugate gradients, on the pose graph's damped normal equations, for graphs that
 * revisit their ground: HipBackend.close_loop builds its pose graph from the covisibility graph, so on such a map it has the
 * sparsity of the reduced camera system above, which neither DENSE (1024 poses) nor SPARSE (the envelope bound) takes.  A
 * setting of its own, context state, read by mslam_hip_pose_graph alone when it is called: mslam_hip_pose_graph_covariance
 * and mslam_hip_pose_graph_edge_weights do not read it, mslam_hip_set_ba_global_pcg does not touch it and it does not touch
 * that setting.  Off by default: with enable = 0 every launch, result bit and error code is what
 * mslam_hip_set_pose_graph_solver's kind gives.  With enable = 1 mslam_hip_pose_graph uses PCG whatever that kind is, and
 * leaves it untouched.
 *   max_iterations  the cap on CG iterations per linear solve, >= 1; MSLAM_HIP_POSE_GRAPH_PCG_MAX_ITERATIONS (500) by default;
 *   tolerance       CG ends at |r_k|_2 <= tolerance |b|_2; in (0, 1); MSLAM_HIP_POSE_GRAPH_PCG_TOLERANCE (1e-6) by default.
 * set returns MSLAM_HIP_E_INVALID and changes nothing for enable outside 0..1, max_iterations < 1 or a tolerance that is not
 * inside (0, 1) (a NaN included); the three are checked whatever enable is.  get: any pointer may be NULL.
 * Caps.  K <= MSLAM_HIP_POSE_GRAPH_MAX_KEYFRAMES_SPARSE (above it: MSLAM_HIP_E_INVALID).  The stored 6 x 6 blocks are the free
 * poses that have an edge plus the unique pairs of them an edge joins.  They live in
 * the buffer of the other two solvers and may be at most MSLAM_HIP_POSE_GRAPH_MAX_ENVELOPE_BLOCKS; above that the call is
 * MSLAM_HIP_E_CAPACITY, the message names the count and nothing is touched.  While E <= MSLAM_HIP_POSE_GRAPH_MAX_EDGES (65536)
 * and K <= 16384 the count is at most 81920 and the bound is never met: a graph with more edges is MSLAM_HIP_E_INVALID by the
 * edge cap first.  No order and no envelope is computed.
 * The solve.  J^T J + D^2 is written block by block, one wave per pair, with the sums of DENSE in their order (duplicate
 * edges of one pair are that pair's serial sum in list order).  Preconditioner, start, breakdown rule and the iterate at the
 * cap are those stated for mslam_hip_set_ba_global_pcg above: the kernels are the same.  The step is inexact; the model cost
 * change is taken from J s per edge as before, which holds for any step, so the trust region is unchanged, as are the edge
 * blocks, Jacobi scaling, damping, mslam_hip_set_pose_graph_loss (the rows are corrected before the assembly), candidate,
 * evaluation, control, termination order and the FAILURE rule.  Stage names inside pg_iterations: solver_schur (the assembly),
 * solver_precond, solver_cg.  Two calls on the same input and setting return the same bits.
 * A chain is the preconditioner's hard case: CG needs about nine iterations per pose of a thin chain at tolerance 1e-12 and
 * about seven at the default, so at the defaults a chain of more than about 70 poses ends solves at the cap,
 * where the iterate is taken and the result is less exact; thin chains stay SPARSE's ground.  A graph that revisits needs 50 to 200 iterations at any size.
 * mslam_hip_get_pose_graph_pcg_stats reports the last mslam_hip_pose_graph of the context (all zero after a solve without
 * PCG, or one that formed no system: E == 0, or no free pose with an edge); mslam_hip_ba_summary is unchanged.
 * Against Ceres 2.2's conjugate gradients on a pose graph (CGNR, cgnr_solver.cc, and ITERATIVE_SCHUR on a problem without
 * landmarks; restated from the published text).  PARITY UNPINNED as for every solver here: the tests compare with
 * tests/pose_graph_pcg_ref.py.
 *   the system               DEVIATES: the normal equations J^T J + D^2 are formed explicitly, block by block; CGNR applies
 *                            J and J^T in turn and never forms them;
 *   preconditioner           SAME as CGNR's JACOBI: the inverse of the 6 x 6 block diagonal of J^T J + D^2;
 *   recurrence               SAME: preconditioned CG from x = 0, beta = r.z / (r.z)_old;
 *   stopping rule            DEVIATES: |r| <= tolerance |b| with a fixed tolerance; Ceres's Q-tolerance / r_tolerance with
 *                            the forcing sequence eta is not built;
 *   the cap                  SAME: max_linear_solver_iterations = 500, the iterate at the cap is used;
 *   breakdown                Ceres reports LINEAR_SOLVER_FAILURE for a non-positive p . q; here the step is invalid, which
 *                            the trust region treats alike. */
#define MSLAM_HIP_POSE_GRAPH_PCG_MAX_ITERATIONS 500
#define MSLAM_HIP_POSE_GRAPH_PCG_TOLERANCE 1e-6
int mslam_hip_set_pose_graph_pcg(mslam_hip_ctx* ctx, int enable, int max_iterations, double tolerance);
int mslam_hip_get_pose_graph_pcg(mslam_hip_ctx* ctx, int* enable, int* max_iterations, double* tolerance);
int mslam_hip_get_pose_graph_pcg_stats(mslam_hip_ctx* ctx, mslam_hip_pcg_stats* stats);
/* ---- A loss function on the edges of mslam_hip_pose_graph (an extension) ----
 * Context state, the idiom of mslam_hip_set_ba_loss: mslam_hip_pose_graph reads it when it is called, with either linear
 * solver (DENSE and SPARSE), and so does mslam_hip_pose_graph_edge_weights.  The bundle adjustments and mslam_hip_pnp_min_mse
 * do NOT read it, and mslam_hip_set_ba_loss does not reach the pose graph.  The kinds are MSLAM_HIP_BA_LOSS_NONE / _HUBER /
 * _CAUCHY.  The default is NONE: the entry then launches the kernels it launched before this setting existed, whose machine
 * code is what it was, and every result keeps its bits.
 * The loss is per edge, s = |r_e|^2 over all six weighted components (after sqrt_info), the scale a in the unit of the
 * weighted residual (metres and radians times sqrt_info), b = a^2; the formulas are those of mslam_hip_set_ba_loss:
 *   HUBER    s <= b: rho = s, rho' = 1;   else rho = 2 a sqrt(s) - b, rho' = max(DBL_MIN, a / sqrt(s))
 *   CAUCHY   rho = b log(1 + s / b), rho' = max(DBL_MIN, 1 / (1 + s / b))
 * cost = 1/2 sum_e rho(|r_e|^2): initial_cost and final_cost report that.  k_pg_edges_loss stores r_e and both 6 x 6 Jacobians
 * of the edge multiplied by sqrt(rho') at the state; the per-pose sums, the normal equations in both layouts, the Jacobi
 * scaling taken at the start, the gradient test, the model cost change, the function and parameter tolerances and the step
 * acceptance follow from the corrected blocks through the kernels that ran before.  s = 0 gives rho' = 1 (no 0 / 0).  There
 * is no default scale.  Two calls on the same input and setting return the same bits: no atomics, no new order of summation.
 * set returns MSLAM_HIP_E_INVALID for a kind outside 0..2 or, for HUBER / CAUCHY, a scale that is not finite or not > 0; the
 * setting is then unchanged.  With NONE the scale is ignored and reported as 0.  get: either pointer may be NULL.
 * Against Ceres 2.2 (loss_function.h, corrector.cc, restated from the published text).  PARITY UNPINNED as for the solver: the
 * tests compare with tests/pose_graph_loss_ref.py, which applies the corrector to tests/pose_graph_ref.py's residuals and
 * Jacobians.
 *   loss formulas            SAME: HuberLoss::Evaluate and CauchyLoss::Evaluate, s == b on Huber's inlier branch, Cauchy's
 *                            1 + s c with c = 1 / b;
 *   corrector                SAME branch: rho'' <= 0 everywhere for both kinds, so Corrector takes `sq_norm == 0 || rho[2] <=
 *                            0`: sqrt(rho') on residual and Jacobians, no curvature term.  SAME form: the rows are scaled, as
 *                            Corrector::CorrectResiduals and CorrectJacobian do (the bundle adjustment kernels weight the
 *                            products instead);
 *   other losses             not built: SoftLOne, Arctan, Tolerant, Tukey, a loss or a scale chosen per edge.
 * mslam_hip_pose_graph_edge_weights is how a caller sees which edges a solve down-weighted: one launch, a lane per edge,
 * chi2[e] = |r_e|^2 at the given poses and weight[e] = rho'(chi2[e]) under the context's pose-graph loss (1.0 with NONE).
 * Either output may be NULL.  The argument checks are mslam_hip_pose_graph's with K in
 * 0..MSLAM_HIP_POSE_GRAPH_MAX_KEYFRAMES_SPARSE whichever solver is set (no linear system is formed); E = 0 writes nothing. */
int mslam_hip_set_pose_graph_loss(mslam_hip_ctx* ctx, int kind, double scale);
int mslam_hip_get_pose_graph_loss(mslam_hip_ctx* ctx, int* kind, double* scale);
int mslam_hip_pose_graph_edge_weights(mslam_hip_ctx* ctx, const double* poses /* K x 7 */, int K, const int32_t* edge_a,
                                      const int32_t* edge_b, const double* edge_meas /* E x 7 */,
                                      const double* sqrt_info /* E x 36, or NULL */, int E, double* chi2 /* E, may be NULL */,
                                      double* weight /* E, may be NULL */);
/* ---- Marginal covariances of mslam_hip_pose_graph's problem (an extension) ----
 * How certain a pose-graph answer is: blocks of Sigma = (J^T J)^-1 at the given poses, what ceres::Covariance computes next
 * to Solve.  THE PROBLEM is mslam_hip_pose_graph's: the same arguments with the same checks (K in
 * 0..MSLAM_HIP_POSE_GRAPH_MAX_KEYFRAMES_SPARSE, E in 0..MSLAM_HIP_POSE_GRAPH_MAX_EDGES) and the same parameter blocks, the
 * free poses that have an edge.  poses is read only.  J holds the edge Jacobians of mslam_hip_pose_graph on its tangent
 * (delta, dp) per pose; there is no damping.  mslam_hip_set_pose_graph_loss is read: with HUBER / CAUCHY the Jacobians are the
 * corrected ones (rows times sqrt(rho')) at the given poses.  mslam_hip_set_pose_graph_solver is NOT read: the factor runs on
 * the block envelope at every K, in the order and with the envelope of mslam_hip_pose_graph_analyze; an envelope above
 * MSLAM_HIP_POSE_GRAPH_MAX_ENVELOPE_BLOCKS is MSLAM_HIP_E_CAPACITY.
 *   pose_idx   P poses, P in 0..65536;  cov[p] is the 6 x 6 block of pose_idx[p], row-major, rows and columns (delta, dp); it
 *              equals its transpose bit for bit (one triangle is computed and mirrored);
 *   pair_a, pair_b   Q pairs, Q in 0..65536;  cross[q] = E[d_a d_b^T], rows from pair_a[q]; cross of (a, b) and of (b, a) are
 *              transposes of each other bit for bit.
 * THE TANGENT.  Plus(q, delta) = (sin|delta| delta / |delta|, cos|delta|) (x) q: delta is HALF a rotation vector, applied on
 * the left (in the world frame).  The covariance of the rotation vector theta = 2 delta is 4 x the delta block, its cross
 * terms with a position 2 x.  dp is the position's own increment.
 * A CONSTANT pose gives a block of zeros, in cov and in cross (Ceres's rule for constant parameter blocks).
 * MSLAM_HIP_E_INVALID beyond mslam_hip_pose_graph's: P or Q out of range; an index out of range; a free pose without an edge
 * (it is not a parameter block); a pair with a == b; a pair of free poses that no edge joins (its block may lie outside the
 * envelope, and only blocks inside it are computed).
 * RANK.  Two cases are detected, both MSLAM_HIP_E_NO_MODEL: (structural, on the host before any launch) a connected component
 * of the free poses none of whose members has an edge to a constant pose: its gauge is free, the message names its least
 * pose; (numerical, on the device) a pivot of the Cholesky factor that is not > 0 or not finite.  Nothing rank-revealing is
 * promised beyond these two: a problem that is singular in exact arithmetic but whose pivots round to small positive numbers
 * returns large numbers, not an error.
 * On every error nothing is written to cov / cross.  Two calls on the same input return the same bytes: no sum uses an
 * atomic, every sum has one order, all arithmetic is f64, no kernel waits on another workgroup.  The envelope lives in the
 * buffer of the SPARSE solves and the dense reduced systems; every later solve clears and assembles it anew and returns the
 * bits it returns without this call.  One workgroup walks the envelope column by column, backwards, as one workgroup factors it.
 * Against ceres::Covariance (Compute on the requested blocks, GetCovarianceBlockInTangentSpace, Options::apply_loss_function
 * = true), restated from the published text.  PARITY UNPINNED: no Ceres build exists to compare with; the tests compare with
 * tests/pose_graph_cov_ref.py (two dense inverses, R^-1 R^-T of a QR of J and L^-T L^-1 of a Cholesky of J^T J, on
 * tests/pose_graph_ref.py's Jacobians; sparse LU solves at 16384 poses).
 *   quantity                 SAME: (J^T J)^-1 in the tangent space of EigenQuaternionManifold, the loss applied;
 *   constant blocks          SAME: zeros;
 *   algorithm                DEVIATES in rounding: a Cholesky factor of the Jacobi-scaled J^T J on the block envelope and the
 *                            Takahashi recursion over it (the scaling undone at the read-out), where Ceres's default is a
 *                            sparse QR of J (SPARSE_QR) or an SVD (DENSE_SVD); J^T J squares the condition number;
 *   which blocks             DEVIATES: only blocks inside the envelope: every pose, and the pairs an edge joins.  Ceres
 *                            computes any requested pair;
 *   rank deficiency          DEVIATES: Ceres's SPARSE_QR fails on a rank-deficient J by its own test, DENSE_SVD truncates by
 *                            min_reciprocal_condition_number or null_space_rank (a pseudo-inverse); here the two cases above;
 *   ambient space            not built: GetCovarianceBlock (7 x 7 per pose, through PlusJacobian). */
int mslam_hip_pose_graph_covariance(mslam_hip_ctx* ctx, const double* poses /* K x 7 */, const uint8_t* fixed /* K, or NULL */,
                                    int K, const int32_t* edge_a, const int32_t* edge_b, const double* edge_meas /* E x 7 */,
                                    const double* sqrt_info /* E x 36, or NULL */, int E, const int32_t* pose_idx, int P,
                                    double* cov /* P x 36 */, const int32_t* pair_a, const int32_t* pair_b, int Q,
                                    double* cross /* Q x 36 */);
/* ---- A loss function for mslam_hip_pnp_min_mse and mslam_hip_pnp_min_mse_batch_dev (an extension) ----
 * Context state, read by both entries when they are called; independent of mslam_hip_set_ba_loss and
 * mslam_hip_set_pose_graph_loss, which do not reach these entries.  The kinds are MSLAM_HIP_BA_LOSS_*.  The default is NONE:
 * both entries then launch k_pnp_min_mse, whose machine code is what it was, and every result keeps its bits.  With HUBER or
 * CAUCHY they launch k_pnp_min_mse_loss: per point s = |observed_i - projected_i|^2, the scale a in pixels, the formulas
 * above; cost = 1/2 sum_i rho(s_i) (info[2], info[3] and final_cost report that) and rho'(s_i) multiplies the point's share
 * of J^T J and J^T f.  The trust-region loop, the validity test on the sums, the model cost change from the normal
 * equations, the terminations and the 50-iteration cap are untouched.  The single call and the batch call still give the
 * same bits for the same problem.  set / get: the rules of mslam_hip_set_pose_graph_loss.  The RANSAC PnP entries and
 * mslam_hip_track do not use min-MSE PnP and take no loss.
 * PARITY UNPINNED; the tests compare with tests/mse_pnp_loss_ref.py (the corrector on tests/mse_pnp_ref.py's rows).
 *   loss formulas, corrector branch     SAME as stated for mslam_hip_set_pose_graph_loss;
 *   weight                   DEVIATES in rounding: the sweep keeps its sums in registers and has no stored rows to scale,
 *                            so rho' multiplies every product of point i where Ceres scales the rows by sqrt(rho') first
 *                            (as in the bundle adjustment kernels);
 *   other losses             not built. */
int mslam_hip_set_pnp_mse_loss(mslam_hip_ctx* ctx, int kind, double scale);
int mslam_hip_get_pnp_mse_loss(mslam_hip_ctx* ctx, int* kind, double* scale);
/* The reference updates landmark->state in place for everyone who holds the pointer; here every landmark of every store
 * entry whose landmark id is landmark_ids[i] gets world_xyz[i] (an id listed twice: the later one wins; ids the store does
 * not hold are ignored).  One upload, a clear, two launches, one synchronisation; *n_written (may be NULL) = the number of
 * store landmarks written.  Nothing else calls it: the store changes only when the caller asks. */
int mslam_hip_kf_update_world(mslam_hip_ctx* ctx, const int64_t* landmark_ids, const double* world_xyz /* n x 3 */, int n,
                              int* n_written /* may be NULL */);

/* ---- verified relocalisation: keyframe store + one query against N keyframes (match -> correspondences -> PnP) --------
 * What RgbdFeatureFrontend::relocalize is written to do with the relocalizer's candidates (rgbd_feature_frontend.cpp:495-534,
 * its body is commented out there and the function returns nullptr): per candidate keyframe matchLandmarks(keypoints,
 * keyframe) (:509 -> :237), pnpAlgorithm->solvePnp on the matched landmarks (:519), the candidate with the most inliers
 * (boost::range::max_element, :527-529), a score threshold of 60 (:531-533).  track() (:279-400) runs the same
 * match -> correspondences -> PnP step against the reference keyframe's landmarks.
 *
 * Keyframe store: per context, on the device, grown by doubling (mslam_hip_kf_reserve pre-allocates).  An entry is
 * n <= max_keypoints landmarks — a 32-byte descriptor and a world point (3 f64) each — under a caller-chosen integer id
 * (the adapters use the BoW database's entry id, so one id names both).  Adding an id that exists replaces its entry.
 * An id that is not in the store is MSLAM_HIP_E_INVALID everywhere; n > max_keypoints is MSLAM_HIP_E_CAPACITY.
 *
 * Landmark ids: next to its descriptor and world point every landmark carries a 64-bit landmark id, the landmark's
 * identity across entries (the reference's shared_ptr<Landmark>): two landmarks of two entries are the same landmark exactly
 * when their ids are equal.  Every way of making an entry writes them:
 *   fresh ids       (1 << 62) | (serial << 16) | position, position = the landmark's place in the entry (< 65536) and
 *                   serial = the context's creation serial: 1 for the first entry made, one more for every later call
 *                   that fills or replaces a slot — mslam_hip_kf_add, mslam_hip_kf_add_ids,
 *                   mslam_hip_kf_add_from_batch_dev, mslam_hip_kf_union[_dev], and mslam_hip_track with new_id >= 0 (the
 *                   serial is taken on the host before anything is enqueued, so it advances whether or not the step makes
 *                   the keyframe).  mslam_hip_kf_add, mslam_hip_kf_add_from_batch_dev (in kept order) and part B of
 *                   mslam_hip_track's new entry give fresh ids;
 *   inherited ids   part A of mslam_hip_track's new entry copies the id of the reference entry's landmark `to` next to
 *                   its world point; mslam_hip_kf_union copies ids with the observations it keeps;
 *   caller's ids    mslam_hip_kf_add_ids takes them from the caller: each in [0, 2^62) (anything else is
 *                   MSLAM_HIP_E_INVALID), so they never collide with fresh ids.  Keeping them distinct inside one entry
 *                   is the caller's business; a repeat inside an entry is one landmark to mslam_hip_kf_covisible, and
 *                   in a union the higher position wins.
 * Nothing else reads the ids: every entry point of ABI 5 that existed before them gives byte-identical outputs. */
int mslam_hip_kf_add(mslam_hip_ctx* ctx, int id, const uint8_t* desc /* n x 32 */, const double* world_xyz /* n x 3 */, int n);
int mslam_hip_kf_add_ids(mslam_hip_ctx* ctx, int id, const uint8_t* desc /* n x 32 */, const double* world_xyz /* n x 3 */,
                         const int64_t* landmark_ids /* n, each in [0, 2^62) */, int n);
/* Frame `frame` of the last detect batch, which mslam_hip_backproject_batch_dev has run on, lifted as addNewLandmarks does
 * (rgbd_feature_frontend.cpp:402-431): a keypoint becomes a landmark when its depth is valid and its camera-frame z is
 * <= z_max (the reference: zThreshold = 3.f); its world point is R p + t (toGlobalCoordinates, projection.cpp:51-54;
 * R = 9 doubles row-major, t = 3 doubles: the keyframe's sensor pose), evaluated in f64 as ((R0 x + R1 y) + R2 z) + t per
 * row, every operation rounded separately (DEVIATES in the last bits from Eigen's quaternion * vector product, which
 * the reference's pose type uses).  Kept keypoints stay in keypoint order.  Asynchronous on the context's stream. */
int mslam_hip_kf_add_from_batch_dev(mslam_hip_ctx* ctx, int id, int frame, const double* R, const double* t, double z_max);
int mslam_hip_kf_remove(mslam_hip_ctx* ctx, int id);
int mslam_hip_kf_clear(mslam_hip_ctx* ctx);
int mslam_hip_kf_size(mslam_hip_ctx* ctx, int* n_entries);
int mslam_hip_kf_reserve(mslam_hip_ctx* ctx, int max_entries);
/* test / debug read-back of an entry (synchronises): *n = its landmark count; desc / world_xyz (either may be NULL) receive
 * the landmarks when `capacity` holds them, otherwise nothing is copied and the call returns MSLAM_HIP_E_CAPACITY. */
int mslam_hip_kf_read(mslam_hip_ctx* ctx, int id, uint8_t* desc, double* world_xyz, int capacity, int* n);
/* the same for the entry's landmark ids (landmark_ids may be NULL: only *n is written) */
int mslam_hip_kf_read_ids(mslam_hip_ctx* ctx, int id, int64_t* landmark_ids, int capacity, int* n);

/* ---- the local map: covisibility and the union of entries -----------------------------------------------------------
 * BasicMap::updateCovisibility's edge test (basic_map.cpp:141-164): counts[k] = the number of distinct landmark ids of
 * entry `id` that entry ids[k] (n_ids <= 64) holds as well.  `id` may be listed: it then counts its own distinct ids.  No
 * upload (the list travels as a kernel argument), three launches, one synchronisation.  An id that is not in the store:
 * MSLAM_HIP_E_INVALID.
 *   edge     SAME: counts[k] > 0 <=> the reference makes the two keyframes neighbours, provided an entry holds the
 *            landmarks its keyframe observes; the count itself is extra (the reference keeps a set, no weight);
 *   when     DEVIATES: the reference updates the graph inside addKeyframe from the observations handed to it; here the
 *            caller asks, for the entries it names. */
int mslam_hip_kf_covisible(mslam_hip_ctx* ctx, int id, const int32_t* ids, int n_ids /* <= 64 */, int32_t* counts /* n_ids */);

/* getLandmarksWithKeypoints' result (rgbd_feature_frontend.cpp:256-277 with RecentObservationsVisitor, :57-80) as an
 * ordinary store entry: entry dst_id is created — or replaced, under a new serial — and holds one landmark per distinct
 * landmark id found in the n_ids (1..64) listed entries.  For each id the observation kept is the one from the listed entry
 * with the largest keyframe id (`observation.keyframe->id > it->second.keyframe->id`); its descriptor, world point and
 * landmark id are copied bit for bit.  A landmark id repeated inside that entry: the higher position wins.
 * Because the result is an ordinary entry, mslam_hip_track and mslam_hip_relocalize run on it unchanged: pass dst_id as
 * ref_id (entry_src then indexes the union, whose ids mslam_hip_kf_read_ids returns).
 * The caller chooses the listed entries (the reference: BasicMap::getNeighbourKeyframes of the reference keyframe, depth 2).
 * mslam_hip_kf_union_dev is asynchronous on the context's stream (a clear and four launches, nothing uploaded);
 * mslam_hip_kf_union is the same followed by one synchronisation, *n_out (may be NULL) = the number of distinct landmarks.
 * Errors: dst_id among ids, an id listed twice, an id that is not in the store, n_ids outside 1..64: MSLAM_HIP_E_INVALID,
 * the store is untouched.  More than max_keypoints distinct landmarks: MSLAM_HIP_E_CAPACITY, *n_out = the count that was
 * needed, and entry dst_id exists with 0 landmarks (no partial result is valid); the _dev form reports it through
 * mslam_hip_sync, once, like the other *_dev launches.  A context meant for local-map tracking is created with
 * max_keypoints sized for the union, not for one frame.
 *   observation kept   SAME rule (largest keyframe id; ids are distinct, so there are no ties between entries);
 *   order              DEVIATES: by the position of the winning entry in `ids`, then by the landmark's position inside it:
 *                      deterministic.  The reference iterates an unordered_map keyed by the landmarks' pointer values,
 *                      an unspecified order;
 *   size               DEVIATES: at most 64 entries and max_keypoints landmarks; the reference has no bound. */
int mslam_hip_kf_union_dev(mslam_hip_ctx* ctx, int dst_id, const int32_t* ids, int n_ids /* 1..64 */);
int mslam_hip_kf_union(mslam_hip_ctx* ctx, int dst_id, const int32_t* ids, int n_ids /* 1..64 */, int* n_out /* may be NULL */);

/* ---- Which descriptor a union row carries (AN EXTENSION: the reference matches against the most recent observation) ----
 * Context state, the idiom of mslam_hip_set_guided_match and mslam_hip_set_ba_loss: mslam_hip_kf_union and
 * mslam_hip_kf_union_dev read it when they are called.  RECENT is the default: both then launch what they launched before
 * this setting existed, and every result keeps its bits.  The model of DISTINCTIVE is ORB-SLAM's
 * MapPoint::ComputeDistinctiveDescriptors.  For every distinct landmark id L of the listed entries:
 *   observations   O(L) = one observation per listed entry that holds L; an entry that holds L more than once counts at its
 *                  highest position (the union's own rule inside an entry), so N = |O(L)| <= 64;
 *   distance       d(a, b) = popcount of the xor over the 256 bits, 0 .. 256;
 *   median         of a in O(L): the N values d(a, b), b in O(L), d(a, a) = 0 included, sorted ascending; median(a) =
 *                  row[(N - 1) / 2] (integer division: ORB-SLAM's vDists[0.5 * (N - 1)]);
 *   choice         the observation of the least median; of equal medians the one from the entry with the largest keyframe id.
 *                  For N <= 2 every median is 0, so the choice is the most recent observation: those rows keep RECENT's bytes;
 *   result         rows, order, world points, landmark ids, count, *n_out, MSLAM_HIP_E_CAPACITY, the _dev form's flag and the
 *                  creation serial are those of RECENT.  Only the 32 descriptor bytes of a row may differ: they are the chosen
 *                  observation's, bit for bit.  The listed entries are not written: every observation stays what it was.
 * Three more launches and one more clear follow the union's own, on the same stream, nothing uploaded, whatever n_ids is
 * (none at all for n_ids <= 2).  No result depends on the order of atomics.
 * set returns MSLAM_HIP_E_INVALID for a mode outside 0..1 and leaves the setting alone.  get: mode may be NULL.
 *   observations   DEVIATES: ORB-SLAM takes every observation of the map point; here one per listed entry, of the listed
 *                  entries only;
 *   ties           DEVIATES: ORB-SLAM keeps the first least median in the iteration order of a map keyed by pointers
 *                  (unspecified); here the largest keyframe id;
 *   what follows   DEVIATES: no UpdateNormalAndDepth, and the choice is not written back into the keyframes' entries. */
#define MSLAM_HIP_UNION_DESC_RECENT 0
#define MSLAM_HIP_UNION_DESC_DISTINCTIVE 1
int mslam_hip_set_union_descriptor(mslam_hip_ctx* ctx, int mode);
int mslam_hip_get_union_descriptor(mslam_hip_ctx* ctx, int* mode);

/* ---- landmark fusion: one identity for the duplicates a loop closure leaves ------------------------------------------
 * AN EXTENSION, NOT A RESTATEMENT: the reference's closeLoop is an empty body (rgbd_feature_frontend.cpp:577-580) and
 * nothing in it merges landmarks.  The model is ORB-SLAM's SearchAndFuse: project the landmarks of the old side of a loop
 * into the corrected new keyframe, match inside a window, give matched pairs one identity.
 *
 * mslam_hip_kf_fuse_search finds the duplicates between two distinct store entries keep_id and drop_id (ordinary entries
 * or unions) and changes nothing.  R (9 f64, row-major), t (3 f64): a pose world -> camera.
 *   projection   both entries' landmarks are projected with the expression mslam_hip_match_guided_knn2 documents (f64,
 *                every operation rounded on its own, in that order).  A drop landmark is IN FRAME iff c_2 > 0 and
 *                ((float)u, (float)v) passes the in-frame test guided matching applies to a keypoint.  From here on the
 *                drop entry's landmarks play the part of keypoints with xy = ((float)u, (float)v), the keep entry's the
 *                part of landmarks.
 *   eligibility  a keep landmark whose id occurs anywhere in the drop entry is neither a searcher nor a candidate (it is
 *                shared already), and likewise a drop landmark whose id occurs anywhere in the keep entry.  So the two id
 *                sets of a call's pairs are disjoint and no chain of replacements can arise.
 *   candidate    drop landmark i is a candidate of keep landmark j iff both are eligible, the guided window test holds with
 *                `radius` (c_2 of j > 0, i in frame, fabs((double)x_i - u_j) <= radius && fabs((double)y_i - v_j) <= radius),
 *                and ((dx dx + dy dy) + dz dz) <= max_world_distance max_world_distance on the two f64 world points
 *                (d = drop - keep; a NaN gives "not a candidate").  The 3-D gate is applied BEFORE the knn-2, so the ratio
 *                test compares geometrically plausible candidates only; max_world_distance = +inf switches it off.
 *   knn-2, acceptance
 *                guided matching's: key dist << 16 | drop position, ties to the lower drop position, a lone candidate is
 *                accepted, d0 <= max_distance, and (double)d0 < ratio (double)d1 where a second candidate exists.
 *   one to one   of several keep landmarks that accept the same drop position the one with the least (d0, keep position)
 *                keeps the pair; the others get no pair (no second choice).
 *   order        pairs are ordered by keep position.  Row p: keep_pos / drop_pos = the positions inside the entries,
 *                keep_lid / drop_lid = their landmark ids, dist = d0.
 * Errors: MSLAM_HIP_E_INVALID for keep_id == drop_id, an id that is not in the store, a radius that is not > 0,
 * max_distance outside 0..256, an extent outside 1..8192, fx or fy zero or NaN, max_world_distance not > 0 (NaN included),
 * an entry above 65535 landmarks; MSLAM_HIP_E_CAPACITY with *n_pairs = the count needed (nothing is copied) when the pairs
 * exceed `capacity` rows.  An empty entry is OK with 0 pairs.  A clear, five launches (ids, projection, k_guided_bin,
 * search, resolution), one synchronisation; every output is deterministic.
 *
 * mslam_hip_kf_replace_ids is the store-wide pass: every landmark of every live entry whose id equals from_ids[p] gets the
 * id to_ids[p] and, with world_xyz given, that world point bit for bit.  The substitution is simultaneous (the lookup is on
 * the id the landmark had before the call; nothing is applied transitively).  A `from` id listed twice: the later one wins,
 * as in mslam_hip_kf_update_world; from == to is allowed (the world point alone changes); ids outside [0, 2^63) are
 * MSLAM_HIP_E_INVALID; ids the store does not hold are ignored.  *n_rewritten (may be NULL) = the number of store landmarks
 * whose id matched.  One upload, one clear, two launches, one synchronisation.
 *
 * mslam_hip_kf_fuse runs the search and then the replacement drop_lid -> keep_lid with the keep landmark's world point.
 * The pair list never leaves the device between the two (the table is built from the device list) and there is one
 * synchronisation at the end.  The pair arrays may be NULL; `capacity` bounds the pairs either way: when they do not fit,
 * nothing is rewritten and the call returns MSLAM_HIP_E_CAPACITY with *n_pairs = the count needed. */
int mslam_hip_kf_fuse_search(mslam_hip_ctx* ctx, int keep_id, int drop_id, const double* R, const double* t, double fx, double fy,
                             double cx, double cy, int width, int height, double radius, int max_distance, double ratio,
                             double max_world_distance, int32_t* keep_pos, int32_t* drop_pos, int64_t* keep_lid, int64_t* drop_lid,
                             int32_t* dist, int capacity, int* n_pairs);
int mslam_hip_kf_replace_ids(mslam_hip_ctx* ctx, const int64_t* from_ids, const int64_t* to_ids, const double* world_xyz /* n x 3 or NULL */,
                             int n, int* n_rewritten /* may be NULL */);
int mslam_hip_kf_fuse(mslam_hip_ctx* ctx, int keep_id, int drop_id, const double* R, const double* t, double fx, double fy, double cx,
                      double cy, int width, int height, double radius, int max_distance, double ratio, double max_world_distance,
                      int32_t* keep_pos /* may be NULL, as the next four */, int32_t* drop_pos, int64_t* keep_lid, int64_t* drop_lid,
                      int32_t* dist, int capacity, int* n_pairs, int* n_rewritten /* may be NULL */);

/* ---- landmark fusion into many keyframes: SearchAndFuse's loop over the connected keyframes, in one call -------------
 * AN EXTENSION, as the calls above.  mslam_hip_kf_fuse_search_multi finds the duplicates between entry keep_id (an ordinary
 * entry or a union: the landmarks whose ids survive) and n_drop distinct target entries drop_ids[m], target m under its
 * own pose world -> camera R + 9 m, t + 3 m, and changes nothing.
 *   projection, candidate, knn-2, acceptance
 *                per target m exactly those of mslam_hip_kf_fuse_search(keep_id, drop_ids[m], R + 9 m, t + 3 m, ...): the
 *                same f64 expression, every operation rounded on its own; the drop entry's landmarks play the part of
 *                keypoints with xy = ((float)u, (float)v); key dist << 16 | drop position.
 *   eligibility  GLOBAL: a keep landmark whose id occurs anywhere in ANY listed drop entry is neither a searcher nor a
 *                candidate in any target, and a drop landmark whose id occurs anywhere in the keep entry is ineligible.
 *                (Otherwise an entry that shares K already and also holds D would hold K twice after D -> K.)  With
 *                n_drop == 1 this is mslam_hip_kf_fuse_search's rule.  So the two id sets of a call's pairs are disjoint
 *                and no chain of replacements can arise.
 *   one to one   per target, as above: of several keep landmarks that accept the same drop position of target m the one
 *                with the least (d0, keep position) keeps the row; the others get none (no second choice).  Then ACROSS
 *                targets, on landmark ids and again without a second choice: (A) of all rows left, over all targets, that
 *                carry the same drop_lid the one with the least (dist, target, keep_pos) stays; (B) of the rows left after
 *                (A) that carry the same keep_lid the one with the least (dist, target, drop_pos) stays.  The result is one
 *                to one on ids; the same (keep_lid, drop_lid) found in several targets is one row; an id repeated at
 *                several positions of one entry is resolved like any other.
 *   order        rows are ordered by (target, keep_pos).  Row p: target = m, keep_pos / drop_pos = the positions inside
 *                the keep entry and entry drop_ids[m], keep_lid / drop_lid = their landmark ids, dist = d0.
 * Errors: those of mslam_hip_kf_fuse_search, and MSLAM_HIP_E_INVALID for n_drop outside 1..64, a drop id equal to keep_id
 * or listed twice, any entry above 65535 landmarks; MSLAM_HIP_E_CAPACITY with *n_pairs = the count needed (nothing is
 * copied) when the pairs exceed `capacity` rows.  An empty entry, or a target with nothing in front of its camera, is OK
 * with no rows.  One upload (the targets), a clear, eight launches whatever n_drop is (ids, projection, binning, search with
 * the per-target claims, claims A, claims B, count, per-target compaction: the target is a grid dimension), one
 * synchronisation; every output is deterministic.
 *
 * mslam_hip_kf_fuse_multi runs the search and then the replacement drop_lid -> keep_lid with the winning keep position's
 * world point, bit for bit, store-wide (mslam_hip_kf_replace_ids' pass: two launches more).  The pair list never leaves the
 * device between the two and there is one synchronisation at the end.  The pair arrays may be NULL; `capacity` bounds the
 * pairs either way: when they do not fit, nothing is rewritten and the call returns MSLAM_HIP_E_CAPACITY with *n_pairs =
 * the count needed. */
int mslam_hip_kf_fuse_search_multi(mslam_hip_ctx* ctx, int keep_id, const int32_t* drop_ids, int n_drop /* 1..64 */,
                                   const double* R /* n_drop x 9 */, const double* t /* n_drop x 3 */, double fx, double fy, double cx,
                                   double cy, int width, int height, double radius, int max_distance, double ratio,
                                   double max_world_distance, int32_t* target, int32_t* keep_pos, int32_t* drop_pos, int64_t* keep_lid,
                                   int64_t* drop_lid, int32_t* dist, int capacity, int* n_pairs);
int mslam_hip_kf_fuse_multi(mslam_hip_ctx* ctx, int keep_id, const int32_t* drop_ids, int n_drop /* 1..64 */,
                            const double* R /* n_drop x 9 */, const double* t /* n_drop x 3 */, double fx, double fy, double cx, double cy,
                            int width, int height, double radius, int max_distance, double ratio, double max_world_distance,
                            int32_t* target /* may be NULL, as the next five */, int32_t* keep_pos, int32_t* drop_pos, int64_t* keep_lid,
                            int64_t* drop_lid, int32_t* dist, int capacity, int* n_pairs, int* n_rewritten /* may be NULL */);

/* ---- RgbdFeatureFrontend::removeObservation (rgbd_feature_frontend.cpp:469-487, a commented-out body; called at :224-230) ----
 * THE BODY THE REFERENCE LEAVES COMMENTED OUT: update(const BackendOutputType&) calls removeObservation for every outlier
 * observation a bundle adjustment reports; the commented code erased the keyframe <-> landmark link and the landmark itself
 * once no keyframe observed it.  Here the link is a position of a store entry, and the call removes positions.
 *
 * Row p names store entry kf_ids[p] and landmark landmark_ids[p]: every position of that entry whose landmark id equals it
 * is removed.  A repeat inside an entry is one landmark, as for mslam_hip_kf_covisible, so all its positions go.
 *   survivors   keep their relative order inside the entry; descriptor, world point and landmark id move bit for bit; the
 *               entry's count drops by the number removed.  An entry emptied this way stays an entry with 0 landmarks.
 *   untouched   entries that no row names, byte for byte.  What lies behind an entry's new count is unspecified.
 *   removed[p]  (may be NULL) the number of positions of entry kf_ids[p] that held landmark_ids[p] before the call; 0 when
 *               the entry does not hold it.  A row listed twice reports the same number in both places.
 *   *n_removed  (may be NULL) the number of store positions removed, each counted once.
 * Reserved ids of unions are ordinary entries and may be named.  Nothing else is updated: the landmark stays in every other
 * entry that holds it, and a union built earlier keeps its copy until it is rebuilt.
 * Errors: MSLAM_HIP_E_INVALID for n < 0, n > 2^24, NULL lists with n > 0, a landmark id outside [0, 2^63), a keyframe id
 * that is not in the store; on every error the store is untouched and the outputs are zeroed.  n = 0 is OK.
 * One upload, one launch (one workgroup per named entry, compacting in place), one synchronisation; deterministic.
 *   what is erased   SAME as the commented body for the keyframe's side of the link;
 *   the landmark     DEVIATES: the store has no landmark objects; a landmark no entry holds any more is simply gone.  The
 *                    host-side bookkeeping of the commented body's last step is HipBackend.remove_observations'. */
int mslam_hip_kf_remove_observations(mslam_hip_ctx* ctx, const int32_t* kf_ids /* n */, const int64_t* landmark_ids /* n */, int n,
                                     int32_t* removed /* n, may be NULL */, int* n_removed /* may be NULL */);

/* ---- keyframe culling: observer counts and a greedy pass over a candidate list ----------------------------------------
 * AN EXTENSION, NOT A RESTATEMENT: the reference has the removal primitives (BasicMap::removeKeyframe, basic_map.cpp:110-115;
 * IRelocalizer::removeKeyframe, relocalizer.hpp:19) and no policy that calls them.  The model is ORB-SLAM's
 * KeyFrameCulling: a keyframe is redundant when more than 90 % of its landmarks are seen by at least three other keyframes.
 *
 *   the map      ids[0..n_ids) are the store entries that count as observers.  The caller names them because the store also
 *                holds unions under ids of the caller's choosing, and a union must not count as an observer.
 *                1 <= n_ids <= MSLAM_HIP_CULL_MAX_ENTRIES, all distinct, all in the store.
 *   obs(l)       the number of listed entries that hold landmark id l at one position at least.  A repeat inside an entry
 *                counts once, as for mslam_hip_kf_covisible.
 *
 * mslam_hip_kf_observers: counts[p] = obs(landmark_ids[p]), 0 for an id no listed entry holds; an id listed twice reports the
 * same count twice.  0 <= n <= 2^24; ids outside [0, 2^63) are MSLAM_HIP_E_INVALID; n = 0 is OK.
 *
 * mslam_hip_kf_cull_search judges the candidates cand[0..n_cand) in the order given and changes nothing in the store.  The
 * candidates are distinct, each is one of `ids`, 0 <= n_cand <= n_ids; a keyframe the caller wants to protect is simply not
 * a candidate.  At the turn of candidate c, with D = the set of distinct landmark ids of entry cand[c]:
 *   n_landmarks[c] = |D|;
 *   n_redundant[c] = |{ l in D : obs(l) - 1 >= min_observers }| with obs as it stands at that turn (the -1: the candidate
 *                    itself is one of the observers);
 *   culled[c]      = n_landmarks[c] >= min_landmarks && (double)n_redundant[c] > ratio * (double)n_landmarks[c]: one
 *                    multiplication and one strict comparison, the strict `>` of ORB-SLAM's 0.9 * nMPs.  An empty entry is
 *                    never culled;
 *   greedy         when c is culled, obs(l) drops by one for every l in D before the next candidate is judged: two keyframes
 *                    that make each other redundant do not both go.
 * n_landmarks and n_redundant (each may be NULL) report what was seen at the candidate's turn; *n_culled (may be NULL) = the
 * number of culled candidates.  min_observers in 1..65535, ratio in [0, 1] (NaN is MSLAM_HIP_E_INVALID), min_landmarks >= 1.
 *
 * mslam_hip_kf_cull is the search, after which the host removes the culled entries exactly as mslam_hip_kf_remove would
 * (the slot goes to the free list, the serial is untouched).  Every other entry is untouched byte for byte.
 *
 * Errors: MSLAM_HIP_E_INVALID for the limits above, a NULL list or a NULL `culled` / `counts` with a positive count, a
 * listed id that is not in the store or is listed twice, a candidate that is not listed or is named twice;
 * MSLAM_HIP_E_CAPACITY when the sizes the host knows of the listed entries (an entry lifted on the device counts as
 * max_keypoints) sum to more than MSLAM_HIP_CULL_MAX_LANDMARKS: the id table is sized by that sum.  On every error the
 * store is untouched and the outputs are zeroed.
 * One upload (the two lists; for kf_observers the ids and the list), three clears, two launches per 64 listed entries, one
 * more launch (the lookup, or the greedy pass: one workgroup), one synchronisation.  Every output is a function of the store
 * and the arguments alone: two runs give equal bytes.
 *   rule         SAME as KeyFrameCulling's count and threshold (nRedundantObservations > 0.9 * nMPs, thObs = 3);
 *   scale        DEVIATES: ORB-SLAM counts another observation only when it was made at the same or a finer pyramid level;
 *                the store keeps no octave, so that test is absent;
 *   order        DEVIATES: ORB-SLAM visits the local keyframes in covisibility order; here the order is the caller's. */
#define MSLAM_HIP_CULL_MAX_ENTRIES 4096
#define MSLAM_HIP_CULL_MAX_LANDMARKS (1 << 24)
int mslam_hip_kf_observers(mslam_hip_ctx* ctx, const int32_t* ids, int n_ids, const int64_t* landmark_ids, int n, int32_t* counts /* n */);
int mslam_hip_kf_cull_search(mslam_hip_ctx* ctx, const int32_t* ids, int n_ids, const int32_t* cand, int n_cand, int min_observers,
                             double ratio, int min_landmarks, uint8_t* culled /* n_cand */, int32_t* n_landmarks /* n_cand, may be NULL */,
                             int32_t* n_redundant /* n_cand, may be NULL */, int* n_culled /* may be NULL */);
int mslam_hip_kf_cull(mslam_hip_ctx* ctx, const int32_t* ids, int n_ids, const int32_t* cand, int n_cand, int min_observers, double ratio,
                      int min_landmarks, uint8_t* culled /* n_cand */, int32_t* n_landmarks /* n_cand, may be NULL */,
                      int32_t* n_redundant /* n_cand, may be NULL */, int* n_culled /* may be NULL */);

/* ---- landmark culling: the landmarks of the candidate entries that too few listed entries observe --------------------
 * AN EXTENSION, NOT A RESTATEMENT: the reference has the removal primitive (BasicMap::removeLandmark, basic_map.cpp:133) and
 * no step that calls it.  The model is ORB-SLAM's MapPointCulling: some keyframes
 * after a landmark was created, it goes when too few keyframes observe it.  For RGB-D the published threshold
 * (Observations() <= 3, two counts per depth observation) means "fewer than two keyframes": min_observers = 2.
 *
 *   the map      ids[0..n_ids), obs(l), the limits 1 <= n_ids <= MSLAM_HIP_CULL_MAX_ENTRIES and MSLAM_HIP_CULL_MAX_LANDMARKS:
 *                exactly as in the keyframe-culling block above.  The listed entries are the observers and the ONLY entries
 *                changed: an entry that is not listed (a union under a reserved id, say) is untouched byte for byte and does
 *                not count as an observer.  A union built earlier keeps its copy until it is rebuilt, as after
 *                mslam_hip_kf_remove_observations.
 *   judged       cand[0..n_cand) are distinct, each one of `ids`, 0 <= n_cand <= n_ids.  A landmark id is judged iff at least
 *                one candidate entry holds it.  n_cand = 0 is OK: nothing is found.  The rule reads no bits of the id: fresh,
 *                inherited and caller-supplied ids are judged alike.
 *   culled       l is culled iff it is judged and obs(l) < min_observers, min_observers in 1..65535 (1 culls nothing).  The
 *                counts are taken once, before anything is removed: there is no greedy order, and removing a landmark
 *                changes no other landmark's count.
 *   the list     the culled ids in ascending order in landmark_ids[0..*n_found), observers[p] = obs(landmark_ids[p])
 *                (`observers` may be NULL).  With landmark_ids == NULL no list is produced, `capacity` is not consulted and
 *                only *n_found comes back.  Otherwise, when *n_found > capacity, the call returns MSLAM_HIP_E_CAPACITY with
 *                *n_found = the count needed and nothing is copied; mslam_hip_kf_cull_landmarks removes nothing in that
 *                case either (the decision is taken on the device from the device count, as mslam_hip_kf_fuse takes it).
 *
 * mslam_hip_kf_cull_landmarks_search changes nothing in the store.
 *
 * mslam_hip_kf_remove_landmarks removes every position of every listed entry whose landmark id is one of
 * landmark_ids[0..n), 0 <= n <= 2^24, ids in [0, 2^63):
 *   survivors         keep their relative order inside the entry; descriptor, world point and landmark id move bit for bit;
 *                     an entry emptied this way stays an entry with 0 landmarks (mslam_hip_kf_remove_observations'
 *                     guarantees).  What lies behind an entry's new count is unspecified.
 *   removed[p]        (may be NULL) the store positions over the listed entries that held landmark_ids[p] before the call.
 *                     An id listed twice reports the same number twice; an id nobody holds reports 0.
 *   entry_removed[k]  (may be NULL) the positions entry ids[k] lost;  *n_removed (may be NULL) = their sum.
 *   sizes             after the call the host knows the exact size of every listed entry (an entry lifted on the device
 *                     counts as max_keypoints no longer).
 *
 * mslam_hip_kf_cull_landmarks is the search followed by the removal of what it found, with entry_removed / *n_removed as
 * above; the list never has to leave the device in between and there is one synchronisation.
 *
 * Errors: MSLAM_HIP_E_INVALID and MSLAM_HIP_E_CAPACITY as in the keyframe-culling block (the listed ids, the candidates,
 * min_observers), and MSLAM_HIP_E_INVALID for a NULL n_found, a negative capacity with a list, n outside 0..2^24, a NULL
 * id list with n > 0, a landmark id outside [0, 2^63).  On every error the store is untouched and the outputs are zeroed
 * (*n_found excepted when the list does not fit).
 * One upload (the listed and candidate slots, or the id list and the slots), the clears, two launches per 64 listed
 * entries for the counts (the search), at most three more launches (flags, gather, compaction with one workgroup per
 * listed entry; or table, compaction, per-row counts), one synchronisation.  Every output is a function of the store and
 * the arguments alone: two runs give equal bytes (the device gathers in arbitrary order; the host sorts the list by id).
 *   threshold    SAME as MapPointCulling's observer threshold for RGB-D at min_observers = 2;
 *   ratio        DEVIATES: the found / visible ratio test is absent, because the store keeps no such counters;
 *   recent       DEVIATES: MapPointCulling judges the landmarks created in the last keyframes; here "recent" is whatever
 *                the caller lists as `cand`;
 *   inherited    DEVIATES: an inherited landmark of a candidate is judged as well (the rule reads no creation time). */
int mslam_hip_kf_remove_landmarks(mslam_hip_ctx* ctx, const int32_t* ids, int n_ids, const int64_t* landmark_ids, int n,
                                  int32_t* removed /* n, may be NULL */, int32_t* entry_removed /* n_ids, may be NULL */,
                                  int* n_removed /* may be NULL */);
int mslam_hip_kf_cull_landmarks_search(mslam_hip_ctx* ctx, const int32_t* ids, int n_ids, const int32_t* cand, int n_cand,
                                       int min_observers, int64_t* landmark_ids /* capacity, may be NULL */,
                                       int32_t* observers /* capacity, may be NULL */, int capacity, int* n_found);
int mslam_hip_kf_cull_landmarks(mslam_hip_ctx* ctx, const int32_t* ids, int n_ids, const int32_t* cand, int n_cand, int min_observers,
                                int64_t* landmark_ids /* capacity, may be NULL */, int32_t* observers /* capacity, may be NULL */,
                                int capacity, int* n_found, int32_t* entry_removed /* n_ids, may be NULL */,
                                int* n_removed /* may be NULL */);

/* One query frame against n_cand <= 64 stored keyframes (64 = the BoW query's own limit), all on the device, one host
 * synchronisation at the end.  Query: desc = n x 32, xy = n x 2 f32 keypoint coordinates, valid = n bytes or NULL (all
 * valid; a mask is track()'s depth filter, :317-334).  Per candidate c = cand_ids[k]:
 *   matches          match(from = query keypoints, to = keyframe c's landmarks) exactly as mslam_hip_match computes it
 *                    (knn-2 with query = to and train = from, ratio test, ordered by `to`), with either matcher kind;
 *   correspondences  match i -> object = (float)world_xyz[c][to_i], image = xy[from_i], in match order; matches whose
 *                    `from` keypoint is masked out are dropped;
 *   pose             one RANSAC PnP as mslam_hip_pnp_ransac runs it (same kernel code, the context's confidence), sampling
 *                    seed = seed + k, the guess (rvec, tvec; use_extrinsic_guess != 0) shared by all candidates; fewer
 *                    than 4 correspondences: status 0, as in mslam_hip_pnp_batch_dev;
 * best = the position in cand_ids of the candidate with the most inliers among those with a model, the first one on ties
 * (max_element), or -1 when there is none or the winner has fewer than min_inliers inliers.
 * out[k] is always written.  pair_from / pair_to ([n_cand][pair_stride], the first n_matches entries of a row) and inliers
 * ([n_cand][pair_stride], the first n_correspondences entries: the consensus mask in correspondence order) may be NULL;
 * a row that does not fit pair_stride makes the call return MSLAM_HIP_E_CAPACITY.
 * Returns MSLAM_HIP_OK when best >= 0, MSLAM_HIP_E_NO_MODEL when best = -1 (n_cand = 0 and n < 2 included: the matcher
 * defines fewer than 2 `from` rows as zero matches), MSLAM_HIP_E_INVALID for an id that is not in the store.
 * Against the reference's (commented-out) body:
 *   matching, correspondences   SAME: matchLandmarks' call and the landmark / keypoint pairing of :513-517;
 *   PnP                         as mslam_hip_pnp_ransac (see its SAME / DEVIATES list);
 *   ranking                     SAME: most inliers, first maximum; a candidate without a model scores 0 there and is
 *                               never the winner here;
 *   threshold                   DEVIATES: `result->score >= scoreThreshold ? result->keyframe : result->keyframe` (:533)
 *                               returns the keyframe either way; min_inliers is this library's reading of
 *                               scoreThreshold = 60 (pass 0 for the expression as written);
 *   guess, depth filter         DEVIATES: the commented code passes no guess and filters nothing; both are optional here
 *                               so that the same call serves track()'s step (guess = currentPose, mask = valid depth). */
typedef struct
{
    int32_t n_matches;         /* ratio-test survivors                                                     */
    int32_t n_correspondences; /* of those, with an unmasked query keypoint                                */
    int32_t n_inliers;         /* consensus of the best hypothesis (0 without a model)                     */
    int32_t status;            /* 1 = a model was found, 0 = none                                          */
    double rvec[3], tvec[3];   /* world -> camera, OpenCV's convention (zeros without a model)             */
} mslam_hip_reloc_candidate;
int mslam_hip_relocalize(mslam_hip_ctx* ctx, const uint8_t* desc, const float* xy, const uint8_t* valid, int n,
                         const int32_t* cand_ids, int n_cand, double fx, double fy, double cx, double cy, double ratio,
                         int iterations, double reprojection_error, uint64_t seed, int use_extrinsic_guess,
                         const double* rvec, const double* tvec, int min_inliers, mslam_hip_reloc_candidate* out,
                         int* best, int32_t* pair_from, int32_t* pair_to, uint8_t* inliers, int pair_stride);

/* ---- the keyframe tracking step: track, reference vote, keyframe insertion -------------------------------------------
 * findBetterReferenceKeyframe's count (rgbd_feature_frontend.cpp:544-575; isVisibleInFrame / projectOnImage,
 * projection.cpp:42-62): for each of n_ids <= 64 stored keyframes, how many of its landmarks project into a frame of
 * width x height seen from the pose (R = 9 doubles row-major, t = 3 doubles: world -> camera, the library's convention).
 * Per landmark (X, Y, Z), in f64, every operation rounded on its own:
 *   c_r = ((R[r][0] X + R[r][1] Y) + R[r][2] Z) + t[r];   u = (c_0 / c_2) fx + cx;   v = (c_1 / c_2) fy + cy;
 *   visible <=> u >= 0 && u < (double)(float)width && v >= 0 && v < (double)(float)height && c_2 > 0.
 * counts[k] = the visible landmarks of ids[k]; *best = the position in ids of the largest count, the first one on ties, or
 * -1 when n_ids == 0.  One upload, two launches, one synchronisation.  An id that is not in the store: MSLAM_HIP_E_INVALID.
 *   count    SAME as keyframeCount[kf], provided an entry holds the landmarks its keyframe observes (the reference walks
 *            keyframe -> observed landmarks through the map; the store has the entry's own landmarks);
 *   winner   DEVIATES: the first maximum in the caller's list order.  The reference iterates a std::map keyed by the
 *            keyframes' pointer values, an unspecified order, and keeps the first maximum of that;
 *   camera   DEVIATES in the last bits: the camera point is R p + t, not q^-1 p - q^-1 position (toLocalCoordinates). */
int mslam_hip_kf_visible(mslam_hip_ctx* ctx, const int32_t* ids, int n_ids /* <= 64 */, const double* R, const double* t,
                         double fx, double fy, double cx, double cy, int width, int height, int32_t* counts /* n_ids */,
                         int* best /* position in ids, -1 if n_ids == 0 */);

/* RgbdFeatureFrontend::track (rgbd_feature_frontend.cpp:279-400) against the store, in one call with one upload and one
 * host synchronisation: the depth filter, the match against the reference keyframe, PnP, the reference vote and the new
 * keyframe, each a launch on the context's stream.
 *   depth filter   mslam_hip_backproject's kernel on the uploaded depth frame (width x height u16, `factor`): a keypoint
 *                  without a valid depth takes no part in PnP (:286, :317-334);
 *   step           exactly mslam_hip_relocalize with the one candidate ref_id, that mask and the guess: matches,
 *                  correspondences, RANSAC PnP with `seed`;
 *   tracked        n_correspondences >= min_matched_points (:336, the reference: 10) and PnP found a model;
 *   vote           mslam_hip_kf_visible over vote_ids (<= 64) with the PnP kernel's own pose record, read on the device;
 *   keyframe       required <=> tracked && n_inliers < new_keyframe_min_landmarks (:156-162, the reference: 30).  With
 *                  new_id >= 0 the entry is built in the store under new_id (:373-397):
 *                    part A  every inlier correspondence, in correspondence order: the query's descriptor desc[from], the
 *                            reference entry's world point world[to] and landmark id copied bit for bit; entry_src = to,
 *                            entry_kp = from;
 *                    part B  every keypoint that no correspondence used (matched with a valid depth, inlier or not:
 *                            usedKeypointIndices, :314-334; set_difference, :377-385), with a valid depth and z <= z_max, in
 *                            keypoint order, lifted as addNewLandmarks does (:402-431):
 *                            world_r = ((R[0][r] (x - t0) + R[1][r] (y - t1)) + R[2][r] (z - t2)), the inverse of the
 *                            tracked world -> camera pose; a fresh landmark id; entry_src = -1, entry_kp = the keypoint;
 *                  The matcher gives one match per landmark of ref_id, so two landmarks can be matched to the same
 *                  keypoint: part A then lists that keypoint twice (two observations, as the reference would push both).
 *                  Without such duplicates A and B are disjoint subsets of the keypoints and the entry holds at most n
 *                  landmarks; with them it can hold more, and it is cut at max_keypoints (part A first, n_entry says what
 *                  was kept).  n > max_keypoints is MSLAM_HIP_E_CAPACITY (an entry's capacity).
 * `out` is always written.  vote_counts (n_vote), pair_from / pair_to / inliers (one row, as mslam_hip_relocalize) and
 * entry_src / entry_kp (entry_capacity) may be NULL.
 * Returns MSLAM_HIP_OK when tracked; MSLAM_HIP_E_NO_MODEL when not: the store is untouched, a slot reserved for new_id is
 * released; MSLAM_HIP_E_INVALID for a ref_id or vote id that is not in the store, or a new_id that ref_id or the vote list
 * names; MSLAM_HIP_E_CAPACITY when the matches do not fit pair_stride or the entry does not fit entry_capacity: the step has
 * run, `out` is complete and a keyframe that `out` reports as added is in the store; only the rows are not copied.  A
 * new_id that exists is replaced when a keyframe is added and left alone otherwise.  The store grows for new_id on the host
 * before anything is enqueued.
 * Against the reference:
 *   matching       against entry ref_id.  DEVIATES when that is the reference keyframe's own entry: the reference matches
 *                  against the union of the most recent observations within graph depth 2 (getLandmarksWithKeypoints,
 *                  :256-277).  SAME up to the order of the landmarks when ref_id is a mslam_hip_kf_union of that
 *                  neighbourhood (the order decides which of two equally good landmarks the matcher names, nothing else).
 *                  entry_src / entry_kp tell the caller what the new entry is made of: entry i of the new keyframe is
 *                  landmark entry_src[i] of ref_id (or a new landmark), seen at keypoint entry_kp[i]; the landmark ids
 *                  carry the same identity on the device;
 *   PnP            as mslam_hip_pnp_ransac (see its SAME / DEVIATES list); tracked, keyframe_required SAME;
 *   vote           see mslam_hip_kf_visible; the caller chooses the neighbourhood (vote_ids);
 *   new keyframe   SAME observations and landmarks; the lift DEVIATES in the last bits as mslam_hip_kf_add_from_batch_dev's;
 *   debug drawing  (:291-309) not reproduced. */
typedef struct
{
    int32_t n_matches, n_correspondences, n_inliers, status; /* as mslam_hip_reloc_candidate                                */
    double rvec[3], tvec[3], R[9];                           /* the tracked pose; R row-major (zeros without a model)      */
    int32_t tracked;             /* 1: n_correspondences >= min_matched_points and PnP found a model                      */
    int32_t keyframe_required;   /* tracked && n_inliers < new_keyframe_min_landmarks                                     */
    int32_t keyframe_added;      /* keyframe_required && new_id >= 0                                                      */
    int32_t n_entry, n_inherited;/* landmarks of the new entry; how many of them are part A                               */
    int32_t vote_best, vote_best_count; /* position in vote_ids / its count; -1 / 0 when not tracked or n_vote == 0       */
} mslam_hip_track_result;
int mslam_hip_track(mslam_hip_ctx* ctx, const uint8_t* desc, const float* xy, int n, const uint16_t* depth, int width,
                    int height, float factor, double fx, double fy, double cx, double cy, int ref_id,
                    const int32_t* vote_ids, int n_vote, double ratio, int iterations, double reprojection_error,
                    uint64_t seed, int use_extrinsic_guess, const double* rvec, const double* tvec,
                    int min_matched_points /* 10 */, int new_keyframe_min_landmarks /* 30 */, int new_id /* < 0: never insert */,
                    double z_max /* 3.0 */, mslam_hip_track_result* out, int32_t* vote_counts /* n_vote, may be NULL */,
                    int32_t* pair_from, int32_t* pair_to, uint8_t* inliers, int pair_stride,
                    int32_t* entry_src, int32_t* entry_kp, int entry_capacity);

/* mslam_hip_track for a window of S consecutive frames (1 <= S <= 256) against ONE store entry, in one call with one upload
 * and one host synchronisation.  Between two events of the front end's loop — a new keyframe, a change of the reference
 * keyframe, a tracking failure — consecutive frames are matched against the same landmarks and are independent of each
 * other, so the window runs as S matcher pairs, S PnP problems and S votes in one launch each.
 *   layout        desc [S][stride][32] u8, xy [S][stride][2] f32, n [S] keypoint counts (0 <= n[s] <= stride; rows past n[s]
 *                 are never read), depth [S][height][width] u16.  out: S records; vote_counts [S][n_vote] or NULL;
 *   per frame s   out[s] is exactly what mslam_hip_track writes for that frame alone with ref_id, the same vote_ids,
 *                 new_id = -1, the seed `seed + s` and the call's one guess (shared by all frames as mslam_hip_relocalize
 *                 shares its guess among candidates): SAME kernels on the same operands, equal bit for bit;
 *   event         frame s is an event when it is not tracked, or keyframe_required is set, or
 *                 n_vote > 0 && ref_vote_pos >= 0 && vote_best != ref_vote_pos (ref_vote_pos: the position of the current
 *                 reference keyframe in vote_ids, -1: votes never raise an event).  *first_event = the smallest such s, or S;
 *                 found on the device.  Frames behind it are still reported, as computed against ref_id: the caller discards
 *                 them (its state changes at the event);
 *   keyframe      with new_id >= 0, when frame *first_event has keyframe_required the device builds its entry under new_id
 *                 by mslam_hip_track's rules (part A, part B, landmark ids, the cut at max_keypoints, entry_src / entry_kp)
 *                 without a host round trip for the decision; keyframe_added, n_entry and n_inherited are set on that one
 *                 record.  A keyframe-requiring frame behind the first event inserts nothing.
 * Slot reservation, the serial, the release of an unused slot and the MSLAM_HIP_E_INVALID / _E_CAPACITY rules are
 * mslam_hip_track's (n[s] > max_keypoints for any s: E_CAPACITY; S outside 1..256: E_INVALID).  Returns MSLAM_HIP_OK when
 * frame 0 is tracked and MSLAM_HIP_E_NO_MODEL when not (the records and *first_event = 0 are complete).
 * Against the reference:
 *   guess         DEVIATES from a frame-by-frame loop, which hands each frame the previous frame's pose: here the frames of a
 *                 window share the guess of the window's start.  The guess only starts the final refit (see
 *                 mslam_hip_pnp_ransac), so the consensus sets are the same and the poses agree to the refit's convergence;
 *   the rest      as mslam_hip_track. */
typedef mslam_hip_track_result mslam_hip_track_window_result; /* pair rows are not returned; entry fields: see `keyframe` */
int mslam_hip_track_window(mslam_hip_ctx* ctx, const uint8_t* desc, const float* xy, const int32_t* n, int stride,
                           const uint16_t* depth, int S, int width, int height, float factor, double fx, double fy, double cx,
                           double cy, int ref_id, const int32_t* vote_ids, int n_vote, int ref_vote_pos, double ratio,
                           int iterations, double reprojection_error, uint64_t seed, int use_extrinsic_guess,
                           const double* rvec, const double* tvec, int min_matched_points, int new_keyframe_min_landmarks,
                           int new_id, double z_max, mslam_hip_track_window_result* out /* S */, int* first_event,
                           int32_t* vote_counts /* [S][n_vote], may be NULL */, int32_t* entry_src, int32_t* entry_kp,
                           int entry_capacity);
/* The same on frames first_frame .. first_frame + n_frames - 1 of the last mslam_hip_detect_batch_dev that
 * mslam_hip_backproject_batch_dev has run on: descriptors, coordinates and counts from the batch view, points and `valid`
 * from the points view (no depth filter launch of its own), the frame size from the context.  Nothing is uploaded but the
 * vote list; apart from the first stage every kernel is the host form's.  The intrinsics are those of the back-projection. */
int mslam_hip_track_window_dev(mslam_hip_ctx* ctx, int first_frame, int n_frames, double fx, double fy, double cx, double cy,
                               int ref_id, const int32_t* vote_ids, int n_vote, int ref_vote_pos, double ratio, int iterations,
                               double reprojection_error, uint64_t seed, int use_extrinsic_guess, const double* rvec,
                               const double* tvec, int min_matched_points, int new_keyframe_min_landmarks, int new_id,
                               double z_max, mslam_hip_track_window_result* out /* n_frames */, int* first_event,
                               int32_t* vote_counts, int32_t* entry_src, int32_t* entry_kp, int entry_capacity);

/* ---- dense TSDF map that follows the keyframe poses (k_tsdf.hip) ---------------------------------------------------------
 * An extension: the reference's only dense output is the viewer's pointCloudFromRgbd (src/app/viewer/slam_thread.cpp:125-150),
 * which back-projects the current frame on the CPU and keeps nothing.  The model here is the volumetric integration of
 * Curless & Levoy / KinectFusion with BundleFusion's de-integration: a frame can be taken out of the volume at the pose it
 * was integrated with and put back at a corrected one.  One volume per context, two int32 per voxel: S, the sum of quantised
 * truncated signed distances, and W, the number of observations.  Integer accumulators make integration an exact,
 * order-independent add and de-integration its exact inverse, hence the invariant every call keeps:
 *   the volume equals the integration of the retained frames at their stored poses into a zeroed volume, bit for bit.
 * One frame (depth u16 [height][width], pose R row-major / t, world -> camera as in mslam_hip_kf_visible, sign s = +-1)
 * changes voxel (i, j, k) by this rule, all arithmetic f64, every operation rounded on its own, in this order:
 *   X = ox + ((double)i + 0.5) * voxel                                    (Y, Z alike)
 *   c_r = ((R[r][0] X + R[r][1] Y) + R[r][2] Z) + t[r];                   skip unless c_2 > 0
 *   u = (c_0 / c_2) fx + cx;  v = (c_1 / c_2) fy + cy;  uh = u + 0.5;  vh = v + 0.5
 *   skip unless uh >= 0 && uh < (double)width && vh >= 0 && vh < (double)height             (false for NaN)
 *   px = (int)floor(uh);  py = (int)floor(vh);  d = (float)depth[py * width + px] * factor  (one f32 multiply, as
 *                                                                                            mslam_hip_backproject)
 *   skip unless d > FLT_EPSILON && (double)d <= max_depth
 *   sdf = (double)d - c_2;  skip if sdf < -trunc
 *   x = sdf / trunc;  if x > 1 then x = 1;  q = (int)rint(x * 32767.0)                      (round half to even)
 *   S += s q;  W += s
 * With at most 32768 frames |S| < 2^30.  Each voxel is owned by one thread, no atomics.  A batch of up to
 * MSLAM_HIP_TSDF_CHUNK (frame, sign) entries is applied in ONE pass over the volume (every voxel loops over the entries a
 * conservative per-wave frustum / range test leaves), so re-integrating M frames sweeps the volume ceil(2M / CHUNK) times.
 *   pointCloudFromRgbd   DEVIATES: a fused, persistent volume instead of a per-frame cloud; no colour.
 * Surface points (mslam_hip_tsdf_extract): f(a) = (double)S(a) / (double)W(a); a voxel is observed when W >= min_weight.  An
 * observed voxel a = (i, j, k) and an axis e in (x, y, z) give a point when the neighbour b = a + e is inside the volume and
 * observed and exactly one of S(a) < 0, S(b) < 0 holds: the centre of a, moved along e by (f(a) / (f(a) - f(b))) * voxel, in
 * f64, cast to f32.  Its normal is the forward-difference gradient g = (f(a+x) - f(a), f(a+y) - f(a), f(a+z) - f(a)) over
 * sqrt((gx^2 + gy^2) + gz^2), cast to f32, when all three forward neighbours are inside and observed and the length is > 0,
 * else (0, 0, 0); it points from behind the surface towards free space.  Order: ascending (k ny + j) nx + i, then axis
 * (count per workgroup, scan, write: no atomics decide an order).
 * All calls run on the context's stream and return after it has drained (the host-pointer convention).  Every error is found
 * before anything is enqueued: a failed call leaves the volume and the frame table untouched.
 *   MSLAM_HIP_E_INVALID   NULL ctx or required pointer; no volume; nx, ny, nz < 1 or nx ny nz > 2^30; width, height < 1;
 *                         max_frames outside 1..32768; voxel, trunc not finite or not > 0; max_depth not > 0 (+inf is fine);
 *                         a non-finite origin, R or t entry; fx or fy zero or NaN; a frame_id that exists (add), does not
 *                         exist (get / update / remove) or is listed twice (update); min_weight < 1; n < 0;
 *   MSLAM_HIP_E_CAPACITY  a frame beyond max_frames; extract into a capacity that is too small: *n is the count needed and
 *                         no row is written. */
#define MSLAM_HIP_TSDF_CHUNK 64
#define MSLAM_HIP_TSDF_MAX_VOXELS (1 << 30)
#define MSLAM_HIP_TSDF_MAX_FRAMES 32768
typedef struct
{
    int32_t nx, ny, nz;    /* voxels per axis; read-back layout [nz][ny][nx], x fastest                    */
    int32_t max_frames;    /* 1..32768 retained frames                                                      */
    double voxel;          /* edge in metres                                                                */
    double origin[3];      /* world position of the corner of voxel (0, 0, 0)                               */
    double trunc;          /* truncation distance in metres                                                 */
    double max_depth;      /* depths above it are not integrated; may be +inf (reference zThreshold: 3.0)   */
    int32_t width, height; /* the one camera of the volume                                                  */
    float factor;          /* metres per raw depth unit (TUM: 1 / 5000)                                     */
    int32_t reserved;      /* 0                                                                             */
    double fx, fy, cx, cy;
} mslam_hip_tsdf_params;
/* A zeroed volume; replaces an existing one and drops its frames. */
int mslam_hip_tsdf_create(mslam_hip_ctx* ctx, const mslam_hip_tsdf_params* params);
int mslam_hip_tsdf_destroy(mslam_hip_ctx* ctx); /* OK without a volume */
int mslam_hip_tsdf_info(mslam_hip_ctx* ctx, mslam_hip_tsdf_params* out /* may be NULL */, int* n_frames /* may be NULL */);
/* Integrates the frame and retains it (the depth image on the device, the pose) under frame_id. */
int mslam_hip_tsdf_add_frame(mslam_hip_ctx* ctx, int frame_id, const uint16_t* depth, const double* R, const double* t);
/* The same from a device image (copied; the caller's buffer is free again when the call returns). */
int mslam_hip_tsdf_add_frame_dev(mslam_hip_ctx* ctx, int frame_id, const uint16_t* d_depth, const double* R, const double* t);
int mslam_hip_tsdf_get_frame(mslam_hip_ctx* ctx, int frame_id, double* R, double* t);
/* Each listed frame whose 12 doubles are bit-identical to the stored ones is skipped; any other is de-integrated at its
 * stored pose and integrated at the new one (the -1 and +1 entries of all moved frames go through the batched launch), and
 * its stored pose is replaced.  *n_moved (may be NULL) = the frames not skipped. */
int mslam_hip_tsdf_update_poses(mslam_hip_ctx* ctx, const int32_t* frame_ids, const double* R /* n x 9 */,
                                const double* t /* n x 3 */, int n, int* n_moved);
/* De-integrates the frame at its stored pose and forgets it. */
int mslam_hip_tsdf_remove_frame(mslam_hip_ctx* ctx, int frame_id);
/* Test / debug read-back: nx ny nz int32 each, either may be NULL. */
int mslam_hip_tsdf_read(mslam_hip_ctx* ctx, int32_t* S, int32_t* W);
/* xyz / normal: capacity x 3 f32 (normal may be NULL; xyz may be NULL when capacity is 0: the count call). */
int mslam_hip_tsdf_extract(mslam_hip_ctx* ctx, int min_weight, float* xyz, float* normal, int capacity, int* n);

/* ---- ray-cast of the dense TSDF map: depth, point and normal images at a pose (k_tsdf_raycast.hip) --------------------------
 * The view of the model from a pose (R row-major / t, world -> camera) through a render camera (width, height, fx, fy, cx, cy)
 * that is independent of the volume's own: KinectFusion's surface prediction.  Like the volume, every pixel has one defined
 * value, bit for bit: all arithmetic is f64, every operation rounded on its own, in the written order.
 * Ray of pixel (px, py), parametrised by camera depth z (the output depth is z itself, the projective distance integration uses):
 *   C_a = -((R[0][a] t0 + R[1][a] t1) + R[2][a] t2)                        (the camera centre)
 *   dx = ((double)px - cx) / fx;  dy = ((double)py - cy) / fy
 *   D_a = (R[0][a] dx + R[1][a] dy) + R[2][a];  P_a(z) = C_a + z * D_a
 * Field value F(P):
 *   g_a = (P_a - o_a) / voxel - 0.5;  b_a = floor(g_a);  w_a = g_a - b_a
 *   the sample is VALID when for every axis b_a >= 0 and b_a + 1 <= n_a - 1 (false for NaN) and all eight corners
 *   (b_x + {0,1}, b_y + {0,1}, b_z + {0,1}) have W >= min_weight; a corner's value is (double)S / (double)W (units of
 *   trunc / 32767, as in extract); lerp(a, b, w) = a + w * (b - a), along x (four), then y (two), then z (one).
 *   Observed free space therefore evaluates to exactly 32767.0; a sample is NEAR when it is valid and F < 32767.0.
 * March: samples z_n = z_near + (double)n * step, n = 0 .. n_last, n_last the last n with z_n <= z_far (z is never
 * accumulated).  If sample 0 is valid with F <= 0 the pixel is a miss.  From n = 0 repeat:
 *   1. if n + K <= n_last (K = coarse): evaluate sample n + K; if neither sample n nor sample n + K is near, n += K and repeat;
 *   2. otherwise walk m = n + 1 .. n + K one by one; going past n_last is a miss;
 *   3. a sample m that is valid with F_m <= 0 ends the ray: a hit when sample m - 1 is valid (its F is then > 0), a miss
 *      otherwise (a surface entered from behind or from unobserved space);
 *   4. after the walk n += K.
 * A hit gives z* = z_{m-1} + (F_{m-1} / (F_{m-1} - F_m)) * step.  K is part of the rule: a coarse stride may step over a
 * sliver of surface a fine walk would have found.
 * Outputs per pixel (row-major [height][width]): depth = (float)z*; xyz = (float)P_a(z*), world frame; normal: with
 * h_a = F(P + voxel e_a) - F(P - voxel e_a) at the f64 hit point P = P(z*), h / sqrt((hx^2 + hy^2) + hz^2) cast to f32 when
 * all six samples are valid and the length is > 0, else (0, 0, 0); it points towards free space, as extract's.  A miss
 * writes zeros to all three.
 * One thread per pixel, no atomics, nothing shared between pixels.  A per-ray clip of the sample range against the volume's
 * box only skips samples the rule makes invalid.  The call does not change the volume.  *n_hits (may be NULL) = the pixels
 * with a hit, summed from per-workgroup counts in index order.
 *   MSLAM_HIP_E_INVALID   no volume; NULL ctx, params, R, t or depth; width or height < 1 or width height > 2^30; fx or fy
 *                         zero or NaN; a non-finite cx, cy, R or t entry; z_near not finite or < 0; z_far not finite or
 *                         < z_near; step not finite or not > 0; (z_far - z_near) / step >= 2^20; coarse < 1; min_weight < 1.
 * Every error is found before anything is enqueued: the volume, the frames and the output buffers stay untouched. */
typedef struct
{
    int32_t width, height; /* the render camera */
    double fx, fy, cx, cy;
    double z_near, z_far, step; /* metres of camera depth */
    int32_t coarse;             /* K >= 1: samples per coarse stride */
    int32_t min_weight;         /* >= 1 */
} mslam_hip_tsdf_raycast_params;
/* depth: height x width f32; xyz / normal: height x width x 3 f32, either may be NULL.  Host pointers; returns after the
 * stream has drained. */
int mslam_hip_tsdf_raycast(mslam_hip_ctx* ctx, const mslam_hip_tsdf_raycast_params* params, const double* R, const double* t,
                           float* depth, float* xyz, float* normal, int* n_hits);
/* The same into device buffers: enqueued on the context's stream, which is drained only when n_hits is not NULL. */
int mslam_hip_tsdf_raycast_dev(mslam_hip_ctx* ctx, const mslam_hip_tsdf_raycast_params* params, const double* R, const double* t,
                               float* d_depth, float* d_xyz, float* d_normal, int* n_hits);

/* ---- frame-to-model alignment: point-to-plane ICP of a depth frame against a rendered model (k_icp.hip) -------------------
 * An extension (the reference tracks by features only): KinectFusion's third part.  A depth frame is aligned against a model
 * given as two f32 images, xyz and normal [mh][mw][3] in the world frame, a zero normal meaning "no surface": exactly what
 * mslam_hip_tsdf_raycast writes.  Like the volume and its ray-cast the result has one value, bit for bit: all arithmetic is
 * f64, every operation rounded on its own, sums of three written (a + b) + c, in the written order.
 * Inputs: depth u16 [h][w] with its camera (w, h, fx, fy, cx, cy, factor, max_depth); the model images with their camera
 * (mw, mh, mfx, mfy, mcx, mcy), independent of the frame's, and pose (Rm, tm), world -> camera; a guess (R0, t0), world ->
 * camera.  All R are row-major.
 * Frame vertex at (px, py): d = (float)raw * factor (one f32 multiply, as in integration); VALID when d > FLT_EPSILON &&
 *   (double)d <= max_depth; z = (double)d; V = (((double)px - cx) / fx * z, ((double)py - cy) / fy * z, z).
 * Frame normal at (px, py): needs 1 <= px <= w - 2, 1 <= py <= h - 2 and the vertex and its four neighbours valid;
 *   a = V(px+1, py) - V(px-1, py);  b = V(px, py+1) - V(px, py-1);
 *   c = b x a:  c0 = b1 a2 - b2 a1;  c1 = b2 a0 - b0 a2;  c2 = b0 a1 - b1 a0;
 *   len = sqrt((c0 c0 + c1 c1) + c2 c2); needs len > 0 (false for NaN); n_f = c / len.  It points towards the camera, as the
 *   model's normals point towards free space.
 *   KinectFusion   DEVIATES: no bilateral filter; no depth-discontinuity gate (the normal test below rejects most edge
 *   pixels); no smoothed pyramid (a level sub-samples the full-resolution frame, see Levels).
 * State: the camera -> world transform (Q, s).  Q = R0^T;  s_a = -((R0[0][a] t0 + R0[1][a] t1) + R0[2][a] t2) (the ray-cast's
 *   C_a).
 * One pair, for a pixel with a frame normal ("skip": the pixel adds +0.0 to every sum and 0 to the count):
 *   X_r = ((Q[r][0] V0 + Q[r][1] V1) + Q[r][2] V2) + s_r;   N_r = (Q[r][0] n0 + Q[r][1] n1) + Q[r][2] n2
 *   c_r = ((Rm[r][0] X0 + Rm[r][1] X1) + Rm[r][2] X2) + tm[r];  skip unless c_2 > 0
 *   u = (c_0 / c_2) mfx + mcx;  v = (c_1 / c_2) mfy + mcy;  uh = u + 0.5;  vh = v + 0.5
 *   skip unless uh >= 0 && uh < (double)mw && vh >= 0 && vh < (double)mh (false for NaN); the model pixel is
 *   ((int)floor(uh), (int)floor(vh)): integration's projection.  q, m = the model point and normal there, as (double).
 *   skip when m0 == 0 && m1 == 0 && m2 == 0
 *   e = X - q;  skip unless (e0 e0 + e1 e1) + e2 e2 <= dist_max * dist_max
 *   skip unless (N0 m0 + N1 m1) + N2 m2 >= cos_min
 *   r = (m0 e0 + m1 e1) + m2 e2
 *   J = (X1 m2 - X2 m1,  X2 m0 - X0 m2,  X0 m1 - X1 m0,  m0,  m1,  m2)
 *   terms: the 21 products J_i J_j, i <= j (row-major upper triangle: A21), the 6 products J_i r (g), r r (cost), the count.
 * Levels: up to 4 (stride_l, iterations_l), in the given order.  Level l uses the pixels with px % stride == 0 && py % stride
 *   == 0 of the full-resolution frame; frame normals always come from full-resolution neighbours; the model is never
 *   sub-sampled.
 * The sums (their order is part of the rule, as the march's stride K is): the level's pixels are enumerated row-major over
 *   (py / stride, px / stride) as i = 0 .. M - 1, positions past M are +0.0.  Chunk i / 256: within each run of 64 the
 *   butterfly as seen from position 0 (v_p += v_(p + 32) for p < 32, then 16, 8, 4, 2, 1); then the four runs as
 *   ((g0 + g1) + g2) + g3.  The chunk sums are added in ascending chunk index, starting from +0.0.  No atomics.
 * Solve A x = -g, x = (omega, tau), by an LDL^T without pivoting and without square root; for j = 0 .. 5:
 *   v_k = L[j][k] D_k (k < j);  D_j = A[j][j] - L[j][0] v_0 - ... - L[j][j-1] v_(j-1)   (one subtraction after the other)
 *   L[i][j] = (A[i][j] - L[i][0] v_0 - ... - L[i][j-1] v_(j-1)) / D_j   (i > j)
 *   y_i = -g_i - L[i][0] y_0 - ... - L[i][i-1] y_(i-1);   x_i = y_i / D_i - L[i+1][i] x_(i+1) - ... - L[5][i] x_5  (i = 5 .. 0)
 *   If the count < min_pairs (no pivot is computed: all six are reported 0.0) or a pivot D_j is not > 0 (false for NaN; the
 *   later pivots are reported 0.0) the solve ends DEGENERATE.
 * Update by the Cayley map (no transcendental function): a = omega * 0.5;  aa = (a0 a0 + a1 a1) + a2 a2;
 *   dR[i][i] = ((1 - aa) + 2 (a_i a_i)) / (1 + aa);   dR[0][1] = (2 (a0 a1) - 2 a2) / (1 + aa);  dR[1][0] = (2 (a0 a1) + 2 a2) / ..;
 *   dR[0][2] = (2 (a0 a2) + 2 a1) / ..;  dR[2][0] = (2 (a0 a2) - 2 a1) / ..;  dR[1][2] = (2 (a1 a2) - 2 a0) / ..;
 *   dR[2][1] = (2 (a1 a2) + 2 a0) / ..
 *   Q[i][j] <- (dR[i][0] Q[0][j] + dR[i][1] Q[1][j]) + dR[i][2] Q[2][j];   s_i <- ((dR[i][0] s0 + dR[i][1] s1) + dR[i][2] s2) + tau_i
 *   A level ends early when, after an update, (w0 w0 + w1 w1) + w2 w2 <= rot_tol rot_tol && (tau likewise) <= trans_tol
 *   trans_tol (w = omega).  Tolerances of 0 run every iteration (unless a step is exactly zero).
 * Outputs: R = Q^T;  t_r = -((Q[0][r] s0 + Q[1][r] s1) + Q[2][r] s2);  status CONVERGED when the LAST level ended by the step
 *   test, ITERATIONS otherwise, DEGENERATE as above: R and t are then the guess, bit for bit.  The result holds the number of
 *   linearisations made, the level, count, sum r r and the six pivots of the last one; `record` (may be NULL) gets one row per
 *   linearisation (a degenerate one has rot2 = trans2 = 0).  The call does not judge weak geometry: the pivots are reported
 *   so that a caller can.  DEGENERATE is a status of a successful call, not an error code.
 * The whole solve is enqueued up front, two launches per scheduled iteration; launches whose level or solve has ended return
 * at once; the host synchronises once at the end.
 *   MSLAM_HIP_E_INVALID   NULL ctx or required pointer; width, height, model_width or model_height < 1, width height > 2^24 or
 *                         model_width model_height > 2^30; a non-finite fx, fy, cx, cy, mfx, mfy, mcx, mcy, factor or pose entry;
 *                         fx, fy, mfx or mfy zero; max_depth NaN or not > 0 (+inf is fine); n_levels outside 1..4; a stride or an
 *                         iteration count < 1; more than MSLAM_HIP_ICP_MAX_ITERATIONS iterations in all; dist_max not finite or
 *                         not > 0; cos_min outside [-1, 1]; min_pairs < 6; a negative or non-finite tolerance; record given
 *                         with record_capacity below the scheduled iterations; for the tsdf_ forms: no volume, or a frame camera
 *                         (width .. max_depth) that differs from the volume's.
 * Every error is found before anything is enqueued: all outputs stay untouched. */
#define MSLAM_HIP_ICP_MAX_LEVELS 4
#define MSLAM_HIP_ICP_MAX_ITERATIONS 256
enum
{
    MSLAM_HIP_ICP_CONVERGED = 0,
    MSLAM_HIP_ICP_ITERATIONS = 1,
    MSLAM_HIP_ICP_DEGENERATE = 2
};
typedef struct
{
    int32_t width, height; /* the frame camera */
    float factor;          /* metres per raw depth unit */
    int32_t n_levels;      /* 1..4 */
    double fx, fy, cx, cy;
    double max_depth;                  /* deeper pixels have no vertex; may be +inf */
    int32_t model_width, model_height; /* the model camera (not read by the tsdf_ forms: theirs is the ray-cast's) */
    double mfx, mfy, mcx, mcy;
    int32_t stride[MSLAM_HIP_ICP_MAX_LEVELS], iterations[MSLAM_HIP_ICP_MAX_LEVELS];
    double dist_max, cos_min; /* the gates: metres between the pair, cosine between the normals */
    int32_t min_pairs;        /* >= 6 */
    int32_t reserved;         /* 0 */
    double rot_tol, trans_tol; /* the step test; 0: every iteration runs */
} mslam_hip_icp_params;
typedef struct
{
    int32_t status;     /* MSLAM_HIP_ICP_* */
    int32_t iterations; /* linearisations made */
    int32_t count;      /* pairs of the last linearisation */
    int32_t level;      /* its level */
    double cost;        /* its sum r r */
    double pivots[6];   /* its D_0 .. D_5 */
} mslam_hip_icp_result;
typedef struct
{
    int32_t level, count;
    double cost, rot2, trans2; /* sum r r; omega . omega; tau . tau */
} mslam_hip_icp_record;
/* Host pointers: depth u16 [height][width]; model_xyz, model_normal f32 [model_height][model_width][3]; Rm, R0, R: 9 f64;
 * tm, t0, t: 3 f64.  Needs no volume.  Returns after the stream has drained. */
int mslam_hip_icp_point_plane(mslam_hip_ctx* ctx, const mslam_hip_icp_params* params, const uint16_t* depth, const float* model_xyz,
                              const float* model_normal, const double* Rm, const double* tm, const double* R0, const double* t0,
                              double* R, double* t, mslam_hip_icp_result* result, mslam_hip_icp_record* record /* may be NULL */,
                              int record_capacity);
/* The same with the three images on the device (poses, results and record stay host pointers), on the context's stream. */
int mslam_hip_icp_point_plane_dev(mslam_hip_ctx* ctx, const mslam_hip_icp_params* params, const uint16_t* d_depth,
                                  const float* d_model_xyz, const float* d_model_normal, const double* Rm, const double* tm,
                                  const double* R0, const double* t0, double* R, double* t, mslam_hip_icp_result* result,
                                  mslam_hip_icp_record* record, int record_capacity);
/* One linearisation at the world -> camera pose (R, t) with the pixels of `stride` (tests and diagnostics; host pointers; the
 * levels of params are checked but not used): A21 (21 f64), g6 (6 f64), *count, *cost. */
int mslam_hip_icp_linearize(mslam_hip_ctx* ctx, const mslam_hip_icp_params* params, const uint16_t* depth, const float* model_xyz,
                            const float* model_normal, const double* Rm, const double* tm, const double* R, const double* t,
                            int stride, double* A21, double* g6, int* count, double* cost);
/* Renders the volume at the guess with raycast_params into the volume's scratch images (model pose = the guess, model camera
 * = the render camera), then solves: equal to mslam_hip_tsdf_raycast followed by mslam_hip_icp_point_plane, byte for byte.
 * The frame camera is the volume's own. */
int mslam_hip_tsdf_icp(mslam_hip_ctx* ctx, const mslam_hip_icp_params* params, const mslam_hip_tsdf_raycast_params* raycast_params,
                       const uint16_t* depth, const double* R0, const double* t0, double* R, double* t, mslam_hip_icp_result* result,
                       mslam_hip_icp_record* record, int record_capacity);
/* The same for a depth image on the device. */
int mslam_hip_tsdf_icp_dev(mslam_hip_ctx* ctx, const mslam_hip_icp_params* params,
                           const mslam_hip_tsdf_raycast_params* raycast_params, const uint16_t* d_depth, const double* R0,
                           const double* t0, double* R, double* t, mslam_hip_icp_result* result, mslam_hip_icp_record* record,
                           int record_capacity);

/* ---- test / debug access to intermediate stages (host copies; synchronises) -----------------------*/
enum
{
    MSLAM_HIP_DBG_PYRAMID = 0,    /* u8 [h_l][w_l] unblurred level                               */
    MSLAM_HIP_DBG_BLURRED = 1,    /* u8 [h_l][w_l] 7x7 sigma-2 blurred level                     */
    MSLAM_HIP_DBG_CANDIDATES = 2, /* float triples (x, y, response), border-relative, FAST order */
    MSLAM_HIP_DBG_SELECTED = 3,   /* float triples after the quadtree, node-list order           */
    MSLAM_HIP_DBG_CELLS = 4,      /* int32 sextuples (x0, y0, cw, ch, ox, oy): the level's FAST cells in launch order
                                     (in-tree detector; host table, `frame` is not used)         */
    MSLAM_HIP_DBG_FORMS = 5,      /* int32 pair: levels produced by the fused level kernels, blurred slab kept in
                                     tiles (1) or rows (0); host values, `frame` and `level` are not used */
    MSLAM_HIP_DBG_QUAD_DIRECT = 6 /* uint32: bit l set = the quadtree selection of level l runs in its direct form
                                     (k_quadtree_direct) for (level, frame) pairs of at most 1024 candidates; host value,
                                     `frame` and `level` are not used */
};
int mslam_hip_level_geometry(mslam_hip_ctx* ctx, int* widths, int* heights, float* scales);
int mslam_hip_debug_read(mslam_hip_ctx* ctx, int what, int frame, int level, void* dst, size_t dst_bytes,
                         size_t* n_items);

/* Per-(frame, level) counts of the last detect batch (CANDIDATES or SELECTED): the first min(n_frames, frames of the
 * last batch) rows of out[n_frames][n_levels] are written, the rest is left untouched (ABI 3: the row count is an
 * argument; the call used to copy as many rows as the last batch had, whatever the caller had allocated). */
int mslam_hip_debug_counts(mslam_hip_ctx* ctx, int what, int32_t* out, int n_frames);

/* Synchronise the context's stream, then copy `bytes` from a device pointer (e.g. out of a view) to host memory. */
int mslam_hip_copy_to_host(mslam_hip_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);

/* Device timing with HIP events.  enable = 1: every stage of the last detect/match/bow batch, with
 * everything serialised on the context's stream (kernel-by-kernel analysis).  enable = 2: every stage
 * launch, timed in place on the stream it is launched on without changing the schedule; entries accumulate
 * over calls until they are read.  enable = 0: off.  names/ms hold up to cap entries. */
int mslam_hip_set_profiling(mslam_hip_ctx* ctx, int enable);
int mslam_hip_get_stage_times(mslam_hip_ctx* ctx, const char** names, float* ms, int cap, int* n);

#ifdef __cplusplus
}
#endif
#endif /* MSLAM_HIP_H_ */
