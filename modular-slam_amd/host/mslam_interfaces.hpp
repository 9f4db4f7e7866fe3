// mslam_interfaces.hpp — host-side mirror of the reference's plugin interfaces for the feature path.
//
// Same names, template parameters, argument meaning and ownership as the reference:
//   Keypoint / KeypointDescriptor / DescriptorMatch   frontend/feature/feature_interface.hpp:18-41
//   IFeatureDetector / IFeatureMatcher                feature_interface.hpp:50-70
//   RgbFrame / Size                                   types/rgb_frame.hpp:12-16, types/basic_types.hpp:23-27
//   IRelocalizer                                      relocalizer.hpp:11-20
//   ILoopDetector                                     loop_detection.hpp:10-15
//   IOrbFeatureDetector / IOrbMatcher / OrbKeypoint   orb_feature.hpp:15-17
//
// The reference headers pull in Eigen, OpenCV and Boost, none of which exist in this build image, so
// this file declares the same shapes standalone.  When compiled inside the reference tree, define
// MSLAM_USE_REFERENCE_HEADERS and the real headers are used instead (the adapter source is the same).
#pragma once

#ifdef MSLAM_USE_REFERENCE_HEADERS
#include "modular_slam/loop_detection.hpp"
#include "modular_slam/orb_feature.hpp"
#include "modular_slam/pnp.hpp"
#include "modular_slam/relocalizer.hpp"
#include "modular_slam/types/slam3d_types.hpp"
#else

#include <array>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <optional>
#include <utility>
#include <vector>

#include "mslam_camera.hpp"

namespace mslam
{
using Id = std::uint64_t;

struct Size
{
    int width;
    int height;
};

struct RgbFrame
{
    std::vector<std::uint8_t> data; // interleaved 3-channel bytes; B,G,R as both providers deliver them
    Size size;
};

struct Keypoint
{
    Id id;
    Vector2 coordinates;
};

template <typename DescriptorType, int Length = 32>
struct KeypointDescriptor
{
    Keypoint keypoint;
    std::array<DescriptorType, Length> descriptor;
};

struct DescriptorMatch
{
    std::size_t fromIndex;
    std::size_t toIndex;
};

template <typename SensorData, typename DescriptorType, int Length>
class IFeatureDetector
{
  public:
    virtual std::vector<KeypointDescriptor<DescriptorType, Length>> detect(const SensorData& sensorData) = 0;
    virtual ~IFeatureDetector() {}
};

template <typename DescriptorType, int Length>
class IFeatureMatcher
{
  public:
    virtual std::vector<DescriptorMatch>
    match(const std::vector<KeypointDescriptor<DescriptorType, Length>>& firstDescriptors,
          const std::vector<KeypointDescriptor<DescriptorType, Length>>& secondDescriptors) = 0;
    virtual ~IFeatureMatcher() {}
};

// types/keyframe.hpp: only what this path touches
template <typename StateType>
struct Keyframe
{
    Id id;
    StateType state;
};

// Eigen::Vector3d / Eigen::Quaterniond stand-ins: only what the adapters touch (types/basic_types.hpp)
struct Vector3
{
    double v[3]{0, 0, 0};
    Vector3() = default;
    Vector3(double x, double y, double z) : v{x, y, z} {}
    double x() const { return v[0]; }
    double y() const { return v[1]; }
    double z() const { return v[2]; }
    Vector3 operator-() const { return Vector3(-v[0], -v[1], -v[2]); }
};
struct Quaternion
{
    double q[4]{1, 0, 0, 0}; // w, x, y, z
    Quaternion() = default;
    Quaternion(double w, double x, double y, double z) : q{w, x, y, z} {}
    double w() const { return q[0]; }
    double x() const { return q[1]; }
    double y() const { return q[2]; }
    double z() const { return q[3]; }
    Quaternion inverse() const // unit quaternion
    {
        return Quaternion(q[0], -q[1], -q[2], -q[3]);
    }
    Vector3 operator*(const Vector3& p) const // rotate
    {
        const double w = q[0], x = q[1], y = q[2], z = q[3];
        const double tx = 2 * (y * p.z() - z * p.y()), ty = 2 * (z * p.x() - x * p.z()), tz = 2 * (x * p.y() - y * p.x());
        return Vector3(p.x() + w * tx + (y * tz - z * ty), p.y() + w * ty + (z * tx - x * tz), p.z() + w * tz + (x * ty - y * tx));
    }
};

// types/state.hpp, types/landmark.hpp, sensors/camera_parameters.hpp
template <typename PositionType, typename OrientationType>
struct State
{
    PositionType position;
    OrientationType orientation;
};
template <typename StateType>
struct Landmark
{
    Id id;
    StateType state;
};
namespace slam3d
{
using SensorState = State<Vector3, Quaternion>;
} // namespace slam3d

// pnp.hpp:14-36 (PnpResult::inliers is a boost::dynamic_bitset there)
template <typename SensorStateType, typename LandmarkStateType>
class IPnpAlgorithm
{
  public:
    struct PnpResult
    {
        SensorStateType pose;
        std::vector<bool> inliers;
    };
    virtual std::optional<PnpResult> solvePnp(const std::vector<std::shared_ptr<Landmark<LandmarkStateType>>>& landmarks,
                                              const std::vector<Vector2>& imgPoints,
                                              const SensorStateType& initial = SensorStateType()) = 0;
    void setCameraParameters(const CameraParameters& newParameters) { cameraParams = newParameters; }
    [[nodiscard]] const CameraParameters& cameraParameters() const { return cameraParams; }
    virtual ~IPnpAlgorithm() = default;

  protected:
    CameraParameters cameraParams;
};

template <typename StateType, typename DescriptorType, int DescriptorLength>
class IRelocalizer
{
  public:
    virtual std::vector<std::shared_ptr<Keyframe<StateType>>>
    relocalize(const std::vector<KeypointDescriptor<DescriptorType>>& keypoints) = 0;
    virtual void addKeyframe(std::shared_ptr<Keyframe<StateType>> keyframe,
                             const std::vector<KeypointDescriptor<DescriptorType>>& keypoints) = 0;
    virtual void removeKeyframe(std::shared_ptr<Keyframe<StateType>> keyframe) = 0;
};

template <typename StateType>
class ILoopDetector
{
  public:
    virtual std::shared_ptr<Keyframe<StateType>> detectLoop() = 0;
};

using IOrbFeatureDetector = IFeatureDetector<RgbFrame, std::uint8_t, 32>;
using IOrbMatcher = IFeatureMatcher<std::uint8_t, 32>;
using OrbKeypoint = KeypointDescriptor<std::uint8_t, 32>;

} // namespace mslam
#endif // MSLAM_USE_REFERENCE_HEADERS

namespace mslam
{
// the matcher relies on sizeof(OrbKeypoint) as the descriptor row stride (orb_feature.cpp:88-91)
static_assert(sizeof(OrbKeypoint) == 64, "OrbKeypoint is expected to be a 64-byte record");
using IOrbRelocalizer = IRelocalizer<slam3d::SensorState, std::uint8_t, 32>;
using IOrbLoopDetector = ILoopDetector<slam3d::SensorState>;
using ISlam3dPnp = IPnpAlgorithm<slam3d::SensorState, Vector3>;

// ---- the backend (backend/backend_interface.hpp:13-21, backend/backend_output.hpp:13-22, observation.hpp) ---------------
// The reference's BackendInterface::process takes the FrontendOutput and walks its map for the observations of the new
// keyframe's neighbourhood (ceres_backend.cpp:162-171).  The map is host bookkeeping and is not mirrored here, so the
// caller hands those observations over (DEVIATES); what happens to them is the reference's: keyframe->state and
// landmark->state are refined in place for everyone who holds the pointers, keyframe id 1 stays constant (:155-159), and
// the observations whose residual exceeds 0.15 m come back as outliers (:212-230).  `cameraPoint` is the camera-frame point
// ReprojectionError's constructor forms from the keypoint and its depth (:24-28).
struct BackendObservation
{
    std::shared_ptr<Keyframe<slam3d::SensorState>> keyframe;
    std::shared_ptr<Landmark<Vector3>> landmark;
    Vector3 cameraPoint;
};
struct BackendOutput
{
    std::vector<std::shared_ptr<Landmark<Vector3>>> updatedLandmarks;            // (unordered_set in the reference)
    std::vector<std::shared_ptr<Keyframe<slam3d::SensorState>>> updatedKeyframes;
    std::vector<BackendObservation> outlierObservations;
    // extra: what the reference only logs (summary.FullReport(), :199)
    int termination = 0, iterations = 0; // ceres::TerminationType; 2 = FAILURE: nothing was updated
    double initialCost = 0, finalCost = 0;
};
class IBackend
{
  public:
    virtual BackendOutput bundleAdjustment(const std::vector<BackendObservation>& observations, int maxIterations = 100) = 0;
    virtual ~IBackend() = default;
};
// extension: the reference's globalBundleAdjustment (ceres_backend.cpp:173-183) is the same bundleAdjustment over every
// keyframe of the map; here it is a solver of its own (mslam_hip_bundle_adjust_global: up to 1024 keyframes).  IBackend is
// untouched: an adapter that offers the global solve derives from this, and a caller reaches it with dynamic_cast.
class IGlobalBackend : public IBackend
{
  public:
    virtual BackendOutput globalBundleAdjustment(const std::vector<BackendObservation>& observations, int maxIterations = 100) = 0;
};
// extension: the body of RgbdFeatureFrontend::closeLoop (rgbd_feature_frontend.cpp:577-580, empty in the reference): a
// pose-graph optimisation over the listed keyframes (mslam_hip_pose_graph: up to 1024 keyframes, 65536 edges; up to 16384
// keyframes after ISparsePoseGraphBackend::setPoseGraphSolver(1)).  An edge
// carries pose b expressed in a's frame (T_a^-1 T_b) and, optionally, the square root of its 6 x 6 information matrix
// (row-major, position rows first; empty: identity).  keyframe->state is corrected in place, keyframe id 1 stays constant;
// the output lists the keyframes and the summary (no landmarks, no outliers).  Reached with dynamic_cast, like IGlobalBackend.
struct PoseGraphEdge
{
    std::shared_ptr<Keyframe<slam3d::SensorState>> a, b;
    slam3d::SensorState measurement;
    std::vector<double> sqrtInformation;
};
class ILoopClosingBackend : public IGlobalBackend
{
  public:
    virtual BackendOutput closeLoop(const std::vector<std::shared_ptr<Keyframe<slam3d::SensorState>>>& keyframes,
                                    const std::vector<PoseGraphEdge>& edges, int maxIterations = 100) = 0;
};
// extension (the reference passes lossFunction = nullptr, ceres_backend.cpp:143): a loss function for bundleAdjustment and
// globalBundleAdjustment (mslam_hip_set_ba_loss): kind 0 none (the default), 1 Ceres's HuberLoss(scale), 2 CauchyLoss(scale),
// scale in metres.  It holds for every later solve of the object; closeLoop does not read it.  The costs of BackendOutput
// are then 1/2 sum rho; the outliers are still judged on the plain residual.  A kind outside 0..2, or a scale that is not
// finite or not > 0 with kind 1 or 2, throws std::invalid_argument and leaves the setting as it was.  An interface of its
// own, reached with dynamic_cast: IBackend and IGlobalBackend mirror the reference and gain no virtual.
class IRobustBackend
{
  public:
    virtual void setLoss(int kind, double scale) = 0;
    virtual ~IRobustBackend() = default;
};
// extension: the linear solver of closeLoop (mslam_hip_set_pose_graph_solver): kind 0 dense (the default: the blocked Cholesky
// of the dense normal equations, up to 1024 keyframes), 1 sparse (a Cholesky factor on the block envelope after a NATURAL or
// reverse Cuthill-McKee order: up to 16384 keyframes, an envelope of up to 1048576 blocks).  It holds for every later
// closeLoop of the object; the bundle adjustments do not read it.  A kind outside 0..1 throws std::invalid_argument and leaves
// the setting as it was.  An interface of its own, reached with dynamic_cast like IRobustBackend.
class ISparsePoseGraphBackend
{
  public:
    virtual void setPoseGraphSolver(int kind) = 0;
    virtual ~ISparsePoseGraphBackend() = default;
};
// extension: the linear solver of globalBundleAdjustment (mslam_hip_set_ba_global_solver): kind 0 dense (the default: the
// blocked Cholesky of the dense reduced camera system, up to 1024 keyframes), 1 sparse (the reduced camera system on its block
// envelope after a NATURAL or reverse Cuthill-McKee order of the covisibility graph: up to 16384 keyframes, an envelope of up
// to 1048576 blocks).  It holds for every later globalBundleAdjustment of the object; bundleAdjustment and closeLoop do not
// read it.  A kind outside 0..1 throws std::invalid_argument and leaves the setting as it was.  An interface of its own,
// reached with dynamic_cast like ISparsePoseGraphBackend.
class ISparseGlobalBackend
{
  public:
    virtual void setGlobalSolver(int kind) = 0;
    virtual ~ISparseGlobalBackend() = default;
};
// extension: globalBundleAdjustment solves its reduced camera system by block-Jacobi preconditioned conjugate gradients
// (mslam_hip_set_ba_global_pcg) instead of a factor: for maps that revisit their ground, whose covisibility is neither thin
// nor small (up to 16384 keyframes and 1048576 non-zero 6 x 6 blocks).  enable = false is the default; with true CG ends at
// |r| <= tolerance |b| or after maxIterations, whose iterate is taken, whatever ISparseGlobalBackend::setGlobalSolver says.  It
// holds for every later globalBundleAdjustment of the object; bundleAdjustment and closeLoop do not read it.  maxIterations < 1
// or a tolerance outside (0, 1) throws std::invalid_argument and leaves the setting as it was.  globalPcgStats reports the
// linear solves of the last globalBundleAdjustment (zeros without PCG).  An interface of its own, reached with dynamic_cast like
// ISparseGlobalBackend.
struct GlobalPcgStats
{
    long long solves = 0, iterations = 0, longest = 0, atCap = 0, breakdowns = 0;
};
class IIterativeGlobalBackend
{
  public:
    virtual void setGlobalPcg(bool enable, int maxIterations, double tolerance) = 0;
    virtual GlobalPcgStats globalPcgStats() const = 0;
    virtual ~IIterativeGlobalBackend() = default;
};
// extension: closeLoop solves its damped normal equations by the same block-Jacobi preconditioned conjugate gradients
// (mslam_hip_set_pose_graph_pcg) instead of a factor: for pose graphs built from the covisibility graph of a map that revisits
// its ground (up to 16384 keyframes; no envelope and no order).  enable = false is the default; with true CG ends at |r| <=
// tolerance |b| or after maxIterations, whose iterate is taken, whatever ISparsePoseGraphBackend::setPoseGraphSolver says.  It
// holds for every later closeLoop of the object; the bundle adjustments and poseGraphCovariance do not read it, and
// IIterativeGlobalBackend::setGlobalPcg does not reach closeLoop.  maxIterations < 1 or a tolerance outside (0, 1) throws
// std::invalid_argument and leaves the setting as it was.  poseGraphPcgStats reports the linear solves of the last closeLoop
// (zeros without PCG).  An interface of its own, reached with dynamic_cast like IIterativeGlobalBackend, whose mirror it is.
class IIterativePoseGraphBackend
{
  public:
    virtual void setPoseGraphPcg(bool enable, int maxIterations, double tolerance) = 0;
    virtual GlobalPcgStats poseGraphPcgStats() const = 0;
    virtual ~IIterativePoseGraphBackend() = default;
};
// extension: a loss function on the edges of closeLoop (mslam_hip_set_pose_graph_loss): kind 0 none (the default), 1 Ceres's
// HuberLoss(scale), 2 CauchyLoss(scale), scale in the unit of the weighted residual of an edge.  It holds for every later
// closeLoop of the object, with either linear solver; the bundle adjustments do not read it, and IRobustBackend::setLoss does not
// reach closeLoop.  The costs of closeLoop's BackendOutput are then 1/2 sum rho.  A kind outside 0..2, or a scale that is not
// finite or not > 0 with kind 1 or 2, throws std::invalid_argument and leaves the setting as it was.  An interface of its own,
// reached with dynamic_cast like IRobustBackend: ILoopClosingBackend gains no virtual.
class IRobustPoseGraphBackend
{
  public:
    virtual void setPoseGraphLoss(int kind, double scale) = 0;
    virtual ~IRobustPoseGraphBackend() = default;
};
// extension: how certain closeLoop's answer is (mslam_hip_pose_graph_covariance; ceres::Covariance's part next to Solve).  The
// problem is closeLoop's, at the states the keyframes hold now: blocks of (J^T J)^-1 over the keyframes that are not constant
// (id 1 is) and have an edge, on the tangent (delta, dp) per keyframe, delta half a rotation vector in the world frame; under
// the loss of IRobustPoseGraphBackend::setPoseGraphLoss; always on the block envelope, whatever setPoseGraphSolver says.
// `of` lists keyframes, `pairs` pairs of keyframes an edge joins (or one of which is constant).  -> blocks: 36 doubles
// (6 x 6 row-major) per keyframe of `of`; cross: 36 per pair, E[d_first d_second^T].  The constant keyframe gives zeros.  Nothing
// is changed.  A keyframe that is not listed, a free one without an edge, a pair of one keyframe, a pair no edge joins, a
// rank-deficient problem or an envelope above the bound throw std::runtime_error with the library's message.  An interface of
// its own, reached with dynamic_cast like ISparsePoseGraphBackend: ILoopClosingBackend gains no virtual.
struct PoseGraphCovariance
{
    std::vector<double> blocks, cross;
};
class IPoseGraphCovariance
{
  public:
    using KeyframePtr = std::shared_ptr<Keyframe<slam3d::SensorState>>;
    virtual PoseGraphCovariance poseGraphCovariance(const std::vector<KeyframePtr>& keyframes, const std::vector<PoseGraphEdge>& edges,
                                                    const std::vector<KeyframePtr>& of,
                                                    const std::vector<std::pair<KeyframePtr, KeyframePtr>>& pairs) = 0;
    virtual ~IPoseGraphCovariance() = default;
};
// extension (the reference's MinMseTracker gives its residual blocks no loss, so every mismatch pulls the pose with full
// weight): a loss function for solvePnp of hipMinMseTrackerFactory's object (mslam_hip_set_pnp_mse_loss): kinds as above,
// scale in pixels.  It holds for every later solvePnp of the object.  Bad input throws std::invalid_argument and leaves the
// setting as it was.  An interface of its own, reached with dynamic_cast: IPnpAlgorithm mirrors the reference and gains no
// virtual.
class IRobustPnp
{
  public:
    virtual void setLoss(int kind, double scale) = 0;
    virtual ~IRobustPnp() = default;
};
// "huber:<a>" or "cauchy:<a>" -> kind 1 or 2 and a; false (nothing written) for anything else, a trailing character or an a
// that is not finite or not > 0
inline bool parseLoss(const char* text, int& kind, double& scale)
{
    if(!text)
        return false;
    int k = 0;
    const char* number = nullptr;
    if(std::strncmp(text, "huber:", 6) == 0)
        k = 1, number = text + 6;
    else if(std::strncmp(text, "cauchy:", 7) == 0)
        k = 2, number = text + 7;
    else
        return false;
    char* end = nullptr;
    const double a = std::strtod(number, &end);
    if(end == number || *end != '\0' || !std::isfinite(a) || !(a > 0.0))
        return false;
    kind = k, scale = a;
    return true;
}


// ---- extension (not in the reference): candidates verified by match + RANSAC PnP against stored landmarks -----------------
// What RgbdFeatureFrontend::relocalize's commented-out body does with IRelocalizer::relocalize's candidates
// (rgbd_feature_frontend.cpp:495-534).  IRelocalizer / ILoopDetector themselves are untouched: an adapter that offers the
// extension derives from these as well, and a caller reaches it with dynamic_cast.
struct VerifiedCandidate
{
    std::shared_ptr<Keyframe<slam3d::SensorState>> keyframe;
    int matches = 0, correspondences = 0, inliers = 0;
    bool hasModel = false;
};
struct VerifiedRelocalization
{
    std::shared_ptr<Keyframe<slam3d::SensorState>> keyframe; // null: no candidate reached minInliers
    double rvec[3] = {0, 0, 0}, tvec[3] = {0, 0, 0};         // world -> camera (cv::solvePnPRansac's convention)
    int inliers = 0;
    std::vector<VerifiedCandidate> candidates;               // in candidate order
};
class IVerifiedRelocalizer
{
  public:
    // the landmarks of a keyframe addKeyframe has fed: worldPoints[i] belongs to keypoints[i]
    virtual void addKeyframeLandmarks(std::shared_ptr<Keyframe<slam3d::SensorState>> keyframe,
                                      const std::vector<OrbKeypoint>& keypoints, const std::vector<Vector3>& worldPoints) = 0;
    virtual VerifiedRelocalization relocalizePose(const std::vector<OrbKeypoint>& keypoints, const CameraParameters& camera,
                                                  int minInliers = 60) = 0;
    virtual ~IVerifiedRelocalizer() = default;
};
class IVerifiedLoopDetector
{
  public:
    // detectLoop()'s candidate for the keyframe fed last, verified the same way
    virtual VerifiedRelocalization detectLoopVerified(const CameraParameters& camera, int minInliers = 60) = 0;
    virtual ~IVerifiedLoopDetector() = default;
};
// ---- extension (not in the reference): RgbdFeatureFrontend::track against the stored landmarks (mslam_hip_track) ----------
// The adapter that owns the landmark store (the one offering IVerifiedRelocalizer) also runs the frontend's tracking step
// on it: rgbd_feature_frontend.cpp:279-400 in one device call, and findBetterReferenceKeyframe's count (:544-575) alone.
// Poses are world -> camera (cv::solvePnPRansac's convention), R row-major.
struct KeyframeTrackOptions
{
    std::uint64_t seed = 0;
    int minMatchedPoints = 10;        // rgbd_feature_frontend/min_matched_points
    int newKeyframeMinLandmarks = 30; // rgbd_feature_frontend/new_keyframe_min_landmarks (:156-162)
    double zMax = 3.0;                // addNewLandmarks' zThreshold (:407)
};
struct KeyframeTrackResult
{
    bool tracked = false, keyframeRequired = false, keyframeAdded = false;
    int matches = 0, correspondences = 0, inliers = 0;
    double rvec[3] = {0, 0, 0}, tvec[3] = {0, 0, 0}, R[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    std::shared_ptr<Keyframe<slam3d::SensorState>> bestReference; // the vote's winner among `neighbours` (null: not tracked / none given)
    std::vector<int> visible;                                     // per neighbour: its landmarks visible in the frame
    int landmarks = 0, inherited = 0;                             // of the new keyframe's entry; `inherited` of them observe landmarks of `reference`
    std::vector<std::int32_t> entrySource, entryKeypoint;         // entry i: landmark entrySource[i] of `reference` (-1: new), seen at keypoints[entryKeypoint[i]]
};
class IKeyframeTracker
{
  public:
    using KeyframePtr = std::shared_ptr<Keyframe<slam3d::SensorState>>;
    // initFirstKeyframe (:433-470): the keyframe is fed as addKeyframe feeds it, and every keypoint with a valid depth and
    // z <= zMax becomes a landmark at the identity pose; returns the number of landmarks
    virtual int initFirstKeyframe(KeyframePtr keyframe, const std::vector<OrbKeypoint>& keypoints, const std::uint16_t* depth, int width,
                                  int height, const CameraParameters& camera, double zMax = 3.0) = 0;
    // one frame against `reference`; rvecGuess / tvecGuess = currentPose (both null: no guess).  When a keyframe is required
    // and newKeyframe is not null, newKeyframe is fed as addKeyframe feeds it and its landmarks are stored on the device.
    virtual KeyframeTrackResult trackKeyframe(const std::vector<OrbKeypoint>& keypoints, const std::uint16_t* depth, int width, int height,
                                              const CameraParameters& camera, KeyframePtr reference,
                                              const std::vector<KeyframePtr>& neighbours, const double* rvecGuess,
                                              const double* tvecGuess, KeyframePtr newKeyframe,
                                              const KeyframeTrackOptions& options = KeyframeTrackOptions()) = 0;
    // per keyframe of `neighbours` (at most 64, each with stored landmarks): its landmarks that project into a width x height
    // frame seen from (R, t); *best = the position of the first maximum, -1 for an empty list
    virtual std::vector<int> visibleLandmarks(const std::vector<KeyframePtr>& neighbours, const double R[9], const double t[3],
                                              const CameraParameters& camera, int width, int height, int* best) = 0;
    // extension (the reference matches brute force; its matchLandmarks carries "TODO: use boost geometry rtree for
    // keypoints", :242): radius > 0 makes trackKeyframe and trackLocalMap calls that have a guess match every landmark
    // among the keypoints within `radius` px of its projection under that guess, no further than maxDistance bits
    // (mslam_hip_set_guided_match; the frame size is each call's); radius <= 0: brute force, the default
    virtual void setGuidedMatch(double radius, int maxDistance = 256) = 0;
    virtual ~IKeyframeTracker() = default;
};
// ---- extension (not in the reference): tracking against the local map (mslam_hip_kf_union, mslam_hip_kf_covisible) ---------
// What getLandmarksWithKeypoints gives track() (rgbd_feature_frontend.cpp:256-277): the most recent observation of every
// landmark seen from a set of keyframes, built on the device from the landmark ids the store keeps.  The caller owns the
// covisibility graph and chooses the members (BasicMap::getNeighbourKeyframes, basic_map.cpp:209-237); the adapter keeps
// the union under a store id of its own.  Offered by the adapter that offers IKeyframeTracker.
class ILocalMapTracker
{
  public:
    using KeyframePtr = std::shared_ptr<Keyframe<slam3d::SensorState>>;
    // addKeyframeLandmarks with the caller's landmark ids (each in [0, 2^62)): landmarkIds[i] belongs to keypoints[i]
    virtual void addKeyframeLandmarksWithIds(KeyframePtr keyframe, const std::vector<OrbKeypoint>& keypoints,
                                             const std::vector<Vector3>& worldPoints, const std::vector<std::int64_t>& landmarkIds) = 0;
    // the landmark ids of a keyframe's stored landmarks, in entry order
    virtual std::vector<std::int64_t> landmarkIds(KeyframePtr keyframe) = 0;
    // per keyframe of `others` (at most 64): how many distinct landmarks of `keyframe` it observes as well; > 0 is
    // updateCovisibility's edge (basic_map.cpp:141-164)
    virtual std::vector<int> covisibleLandmarks(KeyframePtr keyframe, const std::vector<KeyframePtr>& others) = 0;
    // the local map of `members` (1 to 64 keyframes): per landmark the observation of the member with the largest store
    // id (the one stored last); returns its number of landmarks.  Throws when they exceed the context's max_keypoints.
    virtual int buildLocalMap(const std::vector<KeyframePtr>& members) = 0;
    // IKeyframeTracker::trackKeyframe against the local map built last instead of a reference keyframe's own landmarks;
    // entrySource indexes the local map
    virtual KeyframeTrackResult trackLocalMap(const std::vector<OrbKeypoint>& keypoints, const std::uint16_t* depth, int width, int height,
                                              const CameraParameters& camera, const std::vector<KeyframePtr>& neighbours,
                                              const double* rvecGuess, const double* tvecGuess, KeyframePtr newKeyframe,
                                              const KeyframeTrackOptions& options = KeyframeTrackOptions()) = 0;
    virtual ~ILocalMapTracker() = default;
};
// ---- extension (not in the reference): the most distinctive descriptor per landmark of the local map ----------------------
// (mslam_hip_set_union_descriptor; the model is ORB-SLAM's MapPoint::ComputeDistinctiveDescriptors).  mode 0 (the default):
// every landmark of buildLocalMap carries the descriptor of its most recent observation, the reference's rule.  mode 1: of
// its observations among the members, one per member, the one with the least median Hamming distance to all of them; ties
// go to the member stored last.  Landmarks, their order, points and ids do not depend on the mode.  It applies to every
// buildLocalMap after the call.  An interface of its own, reached with dynamic_cast: ILocalMapTracker gains no virtual.
class IDistinctiveLocalMap
{
  public:
    virtual void setUnionDescriptor(int mode) = 0;
    virtual ~IDistinctiveLocalMap() = default;
};

// ---- extension (not in the reference): the tracked pose from RANSAC rigid alignment (mslam_hip_set_track_pose) -------------
// kind 0 (the default): trackKeyframe / trackLocalMap estimate the pose by RANSAC PnP, the reference's way.  kind 1: by the
// least-squares rigid transform between the matched landmarks' world points and the keypoints' camera-frame points (which the
// depth filter of the call computes anyway) inside the same RANSAC loop; maxDistance is the inlier bound in metres.  The model
// is ORB-SLAM's fixed-scale Sim3Solver.  It applies to every tracking call after this one; relocalizePose has no depth and
// runs PnP.  Bad input throws std::invalid_argument and leaves the setting as it was.  An interface of its own, reached with
// dynamic_cast: IKeyframeTracker gains no virtual.
class IAlignedKeyframeTracker
{
  public:
    virtual void setTrackPose(int kind, double maxDistance) = 0;
    virtual ~IAlignedKeyframeTracker() = default;
};
// ---- extension (not in the reference): RANSAC rigid alignment of two 3-D point sets (mslam_hip_align_ransac) ---------------
// target_i ~ R source_i + t over corresponding points, at least 3 of them: a proper rotation (row-major) and a translation,
// the consensus mask of the best hypothesis, or nullopt when no hypothesis reaches 4 inliers.  maxDistance: the inlier bound in
// the points' unit.  Behind hipRigidAlignerFactory.
struct RigidAlignment
{
    double R[9], t[3];
    std::vector<bool> inliers;
};
class IRigidAligner
{
  public:
    virtual std::optional<RigidAlignment> align(const std::vector<Vector3>& source, const std::vector<Vector3>& target,
                                                double maxDistance, int iterations = 100, std::uint64_t seed = 0) = 0;
    virtual ~IRigidAligner() = default;
};

// ---- extension (not in the reference): a dense TSDF map that follows the keyframe poses (mslam_hip_tsdf_*) -----------------
// The reference's only dense output is the viewer's per-frame cloud (src/app/viewer/slam_thread.cpp:125-150).  One volume of
// integer accumulators per object: addFrame integrates a depth image (row-major, width x height of the camera given to create)
// at a world -> camera pose (R row-major, t) and retains it under an id; updatePoses takes every listed frame whose pose
// changed in any bit out at its old pose and puts it back at the new one, in batched sweeps, and returns how many moved;
// removeFrame takes a frame out for good.  At every moment the volume equals a fresh integration of the retained frames at
// their current poses, bit for bit.  extract: the zero crossings between observed neighbours (weight >= minWeight) in voxel
// order, with forward-difference normals that point towards free space.  Every failure throws, as the other adapters do.
// Behind hipDenseMapFactory.
struct DenseMapParams
{
    int nx = 0, ny = 0, nz = 0;  // voxels; at most 2^30 in all
    int maxFrames = 1024;        // 1..32768
    double voxel = 0;            // metres
    double origin[3] = {0, 0, 0}; // the corner of voxel (0, 0, 0)
    double trunc = 0;            // metres
    double maxDepth = 3.0;       // the reference's zThreshold; may be infinite
    int width = 640, height = 480;
    CameraParameters camera;     // focal, principalPoint, factor
};
struct DensePose
{
    double R[9], t[3];
};
struct DenseSurface
{
    std::vector<float> points, normals; // 3 per point
};
class IDenseMap
{
  public:
    virtual void create(const DenseMapParams& params) = 0;
    virtual void addFrame(int id, const std::vector<std::uint16_t>& depth, const DensePose& pose) = 0;
    virtual int updatePoses(const std::vector<int>& ids, const std::vector<DensePose>& poses) = 0;
    virtual void removeFrame(int id) = 0;
    virtual int frames() = 0;
    virtual void read(std::vector<std::int32_t>& sums, std::vector<std::int32_t>& weights) = 0; // [nz][ny][nx] each
    virtual DenseSurface extract(int minWeight = 1) = 0;
    virtual ~IDenseMap() = default;
};

// extension: the view of the dense map from a pose (mslam_hip_tsdf_raycast): per pixel of a render camera that is independent
// of the volume's own, the depth along the optical axis of the first surface the ray meets, its world point and its normal
// (towards free space); zeros where the ray finds none.  The march samples camera depth zNear + n step up to zFar, `coarse`
// samples per stride through space that is not near a surface, and reads voxels observed at least minWeight times; every
// value is explicit (the Python binding's defaults: zFar the volume's maxDepth, step voxel / 2, coarse
// max(1, floor(trunc / (2 step)))).  The images have one defined value, bit for bit (include/mslam_hip.h has the rule).
// Offered by hipDenseMapFactory's object: dynamic_cast<IDenseMapRenderer*>(denseMap.get()).
struct DenseRenderParams
{
    int width = 640, height = 480;
    CameraParameters camera; // focal, principalPoint
    double zNear = 0.1, zFar = 3.0, step = 0;
    int coarse = 1, minWeight = 1;
};
struct DenseRender
{
    std::vector<float> depth;           // [height][width]
    std::vector<float> points, normals; // [height][width][3]; normals is empty when they were not asked for
    int hits = 0;
};
class IDenseMapRenderer
{
  public:
    virtual DenseRender render(const DenseRenderParams& params, const DensePose& pose, bool normals = true) = 0;
    virtual ~IDenseMapRenderer() = default;
};

// extension: frame-to-model alignment on the dense map (mslam_hip_tsdf_icp): the volume is rendered at the guess through the
// render camera of `render` (every value explicit, as for IDenseMapRenderer), and a depth image of the volume's own camera is
// aligned to that render by point-to-plane ICP over `levels` of (stride, iterations), at most four and 256 iterations in all.
// The pose has one defined value, bit for bit (include/mslam_hip.h has the rule).  status: 0 CONVERGED (the last level ended by
// the step test), 1 ITERATIONS, 2 DEGENERATE (fewer than minPairs pairs or a pivot that is not positive: pose is the guess).
// The pivots of the last linearisation are reported; weak geometry is the caller's to judge.  Argument errors throw.
// Offered by hipDenseMapFactory's object: dynamic_cast<IDenseAligner*>(denseMap.get()).
struct DenseAlignParams
{
    std::vector<std::pair<int, int>> levels = {{4, 4}, {2, 5}, {1, 10}}; // (stride, iterations)
    double distMax = 0.1;               // metres between a frame point and its model point
    double cosMin = 0.8253356149096783; // cos(0.6): between the two normals
    int minPairs = 64;
    double rotTol = 0, transTol = 0; // the step test; 0: every iteration runs
};
struct DenseAlignRecord
{
    std::int32_t level, count;
    double cost, rot2, trans2;
};
struct DenseAlignResult
{
    DensePose pose; // world -> camera
    int status = 2, iterations = 0, count = 0, level = 0;
    double cost = 0, pivots[6] = {0, 0, 0, 0, 0, 0};
    std::vector<DenseAlignRecord> record; // one row per linearisation
};
class IDenseAligner
{
  public:
    virtual DenseAlignResult align(const std::vector<std::uint16_t>& depth, const DensePose& guess, const DenseAlignParams& params,
                                   const DenseRenderParams& render) = 0;
    virtual ~IDenseAligner() = default;
};

// ---- extension (not in the reference): landmark fusion after a loop closure (mslam_hip_kf_fuse) ---------------------------
// The reference's closeLoop is an empty body (rgbd_feature_frontend.cpp:577-580); the model is ORB-SLAM's SearchAndFuse.
// The landmarks of `dropEntry` that duplicate landmarks of `keepEntry` — both projected under one world -> camera pose, each
// keep landmark matched among the drop landmarks inside a window and a 3-D gate, one to one — take the keep landmark's id
// and world point in every stored keyframe.  Offered by the adapter that owns the store (the one that offers
// ILocalMapTracker).
struct LandmarkFuseParams
{
    CameraParameters camera;
    int width = 640, height = 480; // the frame the pose looks into
    double radius = 8.0;           // px, the half edge of the search window
    int maxDistance = 50;          // Hamming
    double ratio = 0.7;
    double maxWorldDistance = 0.1; // metres; infinity switches the gate off
};
struct FusedLandmarkPair
{
    int keepPosition = 0, dropPosition = 0; // inside the two entries
    std::int64_t keepId = 0, dropId = 0;    // landmark ids: every dropId in the store has become keepId
    int distance = 0;
};
struct LandmarkFusion
{
    std::vector<FusedLandmarkPair> pairs; // ordered by keepPosition
    int rewritten = 0;                    // store landmarks whose id was replaced
};
class ILandmarkFuser
{
  public:
    using KeyframePtr = std::shared_ptr<Keyframe<slam3d::SensorState>>;
    virtual LandmarkFusion fuseLandmarks(KeyframePtr keepEntry, KeyframePtr dropEntry, const double R[9], const double t[3],
                                         const LandmarkFuseParams& params) = 0;
    virtual ~ILandmarkFuser() = default;
};

// ---- extension: landmark fusion into many keyframes in one call (mslam_hip_kf_fuse_multi) ----------------------------------
// SearchAndFuse's loop over the keyframes connected to the current one.  Every entry of `dropEntries` (1..64, distinct, none
// of them keepEntry) is a target under its own world -> camera pose R + 9 m, t + 3 m; what the targets find is resolved on
// landmark ids, so that every drop id is replaced by one keep id and every keep id replaces one drop id.  A separate
// interface: ILandmarkFuser stays as it is for the code that implements it.
struct MultiFusedLandmarkPair
{
    int target = 0;                         // position in dropEntries
    int keepPosition = 0, dropPosition = 0; // inside the keep entry and that target
    std::int64_t keepId = 0, dropId = 0;
    int distance = 0;
};
struct MultiLandmarkFusion
{
    std::vector<MultiFusedLandmarkPair> pairs; // ordered by (target, keepPosition)
    int rewritten = 0;                         // store landmarks whose id was replaced
};
class IMultiLandmarkFuser
{
  public:
    using KeyframePtr = std::shared_ptr<Keyframe<slam3d::SensorState>>;
    virtual MultiLandmarkFusion fuseLandmarksMulti(KeyframePtr keepEntry, const std::vector<KeyframePtr>& dropEntries,
                                                   const std::vector<double>& R /* 9 per target */,
                                                   const std::vector<double>& t /* 3 per target */,
                                                   const LandmarkFuseParams& params) = 0;
    virtual ~IMultiLandmarkFuser() = default;
};

// ---- RgbdFeatureFrontend::removeObservation (rgbd_feature_frontend.cpp:469-487; mslam_hip_kf_remove_observations) ----------
// The body the reference leaves commented out: update(const BackendOutputType&) calls it for every outlier observation of a
// bundle adjustment (:224-230).  Observation p names a stored keyframe and a landmark id; every position of that keyframe's
// entry that holds the id is removed, the survivors keep their order.  -> per observation, the number of positions its
// landmark held in its keyframe before the call (0: the keyframe did not hold it; an observation listed twice reports the
// same number twice).  A keyframe that is not stored throws.  Offered by the adapter that owns the store.
class IObservationRemover
{
  public:
    using KeyframePtr = std::shared_ptr<Keyframe<slam3d::SensorState>>;
    virtual std::vector<int> removeObservations(const std::vector<std::pair<KeyframePtr, std::int64_t>>& observations) = 0;
    virtual ~IObservationRemover() = default;
};

// ---- keyframe culling (mslam_hip_kf_cull_search; an extension) -------------------------------------------------------------
// The reference has the removal primitives (BasicMap::removeKeyframe, basic_map.cpp:110-115; IRelocalizer::removeKeyframe,
// relocalizer.hpp:19) and no policy that calls them; the model is ORB-SLAM's KeyFrameCulling.  `map` names the stored
// keyframes that count as observers, `candidates` (distinct, each one of `map`) are judged in the order given: a candidate
// with at least minLandmarks distinct landmark ids goes when more than `ratio` of them are held by at least minObservers
// other keyframes of the map, counted without the candidates that went before it.  -> one verdict per candidate, in order,
// with the two counts seen at its turn.  A culled keyframe has left the adapter the way removeKeyframe removes it (the BoW
// database and the keyframe store).  A keyframe that is not stored throws.  Offered by the adapter that owns the store.
struct KeyframeCullParams
{
    int minObservers = 3;
    double ratio = 0.9;
    int minLandmarks = 1;
};
struct KeyframeCullVerdict
{
    std::shared_ptr<Keyframe<slam3d::SensorState>> keyframe;
    bool culled = false;
    int landmarks = 0, redundant = 0; // distinct landmark ids; those with at least minObservers other observers
};
class IKeyframeCuller
{
  public:
    using KeyframePtr = std::shared_ptr<Keyframe<slam3d::SensorState>>;
    virtual std::vector<KeyframeCullVerdict> cullKeyframes(const std::vector<KeyframePtr>& map, const std::vector<KeyframePtr>& candidates,
                                                           const KeyframeCullParams& params) = 0;
    virtual ~IKeyframeCuller() = default;
};

// ---- landmark culling (mslam_hip_kf_cull_landmarks, mslam_hip_kf_remove_landmarks; an extension) ---------------------------
// The reference has no such step; the model is ORB-SLAM's MapPointCulling, of which this is the observer threshold (fewer
// than two keyframes for RGB-D: minObservers = 2) without the found / visible ratio.  `map` names the stored keyframes that
// count as observers and the only ones changed; a landmark id is judged when at least one of `candidates` (distinct, each
// one of `map`) holds it, and goes from every keyframe of the map, at every position, when fewer than minObservers of them
// hold it.  The counts are taken once, before anything is removed.  cullLandmarks -> the culled ids, ascending, with their
// observer counts.  removeLandmarks removes the listed ids from every keyframe of the map -> per id, the positions that held
// it (0: nobody did; an id listed twice reports the same number twice).  A keyframe that is not stored throws.  Offered by
// the adapter that owns the store.
struct CulledLandmark
{
    std::int64_t id = 0;
    int observers = 0; // keyframes of the map that held it
};
class ILandmarkCuller
{
  public:
    using KeyframePtr = std::shared_ptr<Keyframe<slam3d::SensorState>>;
    virtual std::vector<CulledLandmark> cullLandmarks(const std::vector<KeyframePtr>& map, const std::vector<KeyframePtr>& candidates,
                                                      int minObservers) = 0;
    virtual std::vector<int> removeLandmarks(const std::vector<KeyframePtr>& map, const std::vector<std::int64_t>& ids) = 0;
    virtual ~ILandmarkCuller() = default;
};
} // namespace mslam
