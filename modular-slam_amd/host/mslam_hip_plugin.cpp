// mslam_hip_plugin.cpp — adapters from the reference's plugin interfaces to the C ABI (mslam_hip.h),
// and the factory aliases the reference's loader imports.
//
//   HipOrbDetector    : IFeatureDetector<RgbFrame,u8,32>   drop-in for DistributedOrbOpenCvDetector
//                                                           (distributed_cv_feature.cpp:1181-1222) and, created by
//                                                           hipCvOrbDetectorFactory, for OrbOpenCvDetector
//                                                           (orb_feature.cpp:25,33-65: the cv::ORB mode)
//   HipOrbMatcher     : IFeatureMatcher<u8,32>             drop-in for OrbOpenCvMatcher (orb_feature.cpp:84-130)
//   HipOrbRelocalizer : IRelocalizer                       what OrbRelocalizer is wired for
//                                                           (orb_relocalizer.cpp:26-50, rgbd_feature_frontend.cpp:153,176)
//   HipRansacPnp      : IPnpAlgorithm<SensorState,Vector3>  drop-in for OpenCvRansacPnp (cv_ransac_pnp.cpp:14-85)
//   HipMinMseTracker  : IPnpAlgorithm<SensorState,Vector3>  drop-in for MinMseTracker
//                     : IRobustPnp                          a Huber or Cauchy loss on its reprojection errors (an extension)
//   HipBundleAdjustBackend : ILoopClosingBackend : IGlobalBackend : IBackend      CeresBackend's bundle adjustment, local and global, and closeLoop (hipBundleAdjustBackendFactory)
//                          : IRobustBackend                                       a Huber or Cauchy loss for both bundle adjustments (an extension)
//                          : ISparsePoseGraphBackend                              closeLoop's linear solver: dense or the block-envelope factor (an extension)
//                          : IPoseGraphCovariance                                 marginal covariances of closeLoop's problem (an extension)
//                          : ISparseGlobalBackend                                 globalBundleAdjustment's linear solver, the same choice (an extension)
//                          : IRobustPoseGraphBackend                              a Huber or Cauchy loss on closeLoop's edges (an extension)
//                          : IIterativeGlobalBackend                              globalBundleAdjustment by preconditioned conjugate gradients (an extension)
//                          : IIterativePoseGraphBackend                           closeLoop by preconditioned conjugate gradients (an extension)
//                                                           (ceres_reprojection_error_pnp.cpp:64-110)
//   HipLoopDetector   : ILoopDetector                      (loop_detection.hpp:10-15, rgbd_feature_frontend.cpp:202);
//                                                           both sit on ONE shared BoW database
//
// Errors: the reference interfaces have no status channel, so a non-zero C-ABI status becomes a
// std::runtime_error carrying mslam_hip_last_error() (the reference itself lets OpenCV/DBoW3 throw,
// orb_relocalizer.cpp:28).  No CPU fallback exists.
#include "mslam_interfaces.hpp"
#include "plugin_loader.hpp"

#include "../../include/mslam_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>

namespace mslam
{
namespace
{
[[noreturn]] void raise(mslam_hip_ctx* ctx, const char* what, int rc)
{
    std::string msg = std::string("mslam_hip: ") + what + " failed (" + std::to_string(rc) + "): " + mslam_hip_last_error(ctx);
    std::fprintf(stderr, "[error] %s\n", msg.c_str());
    throw std::runtime_error(msg);
}

struct Ctx
{
    mslam_hip_ctx* h = nullptr;
    int width = -1, height = -1, capacity = 0;
    // width = height = 0: a context without detector buffers (the matcher and the BoW database need none)
    int detector = MSLAM_HIP_DETECTOR_DISTRIBUTED;
    void ensure(int w, int h_, int max_keypoints = 0)
    {
        if(h && w == width && h_ == height && (max_keypoints == 0 || max_keypoints == capacity))
            return;
        if(h)
            mslam_hip_destroy(h);
        h = nullptr;
        mslam_hip_params p;
        mslam_hip_default_params(&p); // the reference's hard-coded operating point
        p.width = w;
        p.height = h_;
        p.detector = detector;
        if(max_keypoints > 0)
        {
            p.max_keypoints = max_keypoints;
            p.max_candidates = std::max(p.max_candidates, 4 * max_keypoints);
        }
        const int rc = mslam_hip_create(&p, &h);
        if(rc != MSLAM_HIP_OK)
            raise(nullptr, "mslam_hip_create", rc);
        width = w;
        height = h_;
        capacity = p.max_keypoints;
    }
    ~Ctx()
    {
        if(h)
            mslam_hip_destroy(h);
    }
};

void gather_descriptors(const std::vector<OrbKeypoint>& kps, std::vector<std::uint8_t>& out)
{
    out.resize(kps.size() * 32);
    for(std::size_t i = 0; i < kps.size(); ++i)
        std::memcpy(&out[i * 32], kps[i].descriptor.data(), 32);
}
void toRodrigues(double w, double x, double y, double z, double r[3])
{
    // Eigen::AngleAxisd(q) (cv_ransac_pnp.cpp:44-48): angle = 2 atan2(|v|, |w|) from the POSITIVE norm, then the axis is
    // v / |v| for w >= 0 and -v / |v| for w < 0 (q and -q are the same rotation)
    const double nv = std::sqrt(x * x + y * y + z * z);
    if(nv < 1e-300)
    {
        r[0] = r[1] = r[2] = 0;
        return;
    }
    const double angle = 2.0 * std::atan2(nv, std::fabs(w));
    const double d = w < 0 ? -nv : nv;
    r[0] = x / d * angle, r[1] = y / d * angle, r[2] = z / d * angle;
}
} // namespace

class HipOrbDetector : public IOrbFeatureDetector
{
  public:
    explicit HipOrbDetector(int detector = MSLAM_HIP_DETECTOR_DISTRIBUTED) { ctx.detector = detector; }
    std::vector<OrbKeypoint> detect(const RgbFrame& sensorData) override
    {
        std::vector<OrbKeypoint> result;
        if(sensorData.data.empty()) // distributed_cv_feature.cpp:724-727: empty image => empty result
            return result;
        const int w = sensorData.size.width, h = sensorData.size.height;
        // The reference's output is unbounded (a std::vector).  Start from a capacity sized for the frame
        // area (8192 at 640x480) and, if a frame yields more, rebuild the context with twice the room and
        // run the frame again: the capacity only ever grows.
        if(ctx.width != w || ctx.height != h)
        {
            const long long area = (long long)w * h;
            wanted = (int)std::min<long long>(65535, std::max<long long>(wanted, 8192 * ((area + 307199) / 307200)));
        }
        int n = 0;
        for(;;)
        {
            ctx.ensure(w, h, wanted);
            xy.resize(2 * (std::size_t)ctx.capacity);
            desc.resize(32 * (std::size_t)ctx.capacity);
            const int rc = mslam_hip_detect(ctx.h, sensorData.data.data(), w, h, ctx.capacity, xy.data(), desc.data(),
                                            nullptr, nullptr, nullptr, &n);
            if(rc == MSLAM_HIP_OK)
                break;
            if(rc != MSLAM_HIP_E_CAPACITY || wanted >= 65535)
                raise(ctx.h, "mslam_hip_detect", rc);
            wanted = std::min(65535, 2 * wanted);
        }
        result.resize(static_cast<std::size_t>(n));
        for(int i = 0; i < n; ++i)
        {
            // distributed_cv_feature.cpp:1203-1213: id = running index, float coordinates widened to double
            result[i].keypoint.id = static_cast<Id>(i);
            result[i].keypoint.coordinates.x() = xy[2 * i];
            result[i].keypoint.coordinates.y() = xy[2 * i + 1];
            std::memcpy(result[i].descriptor.data(), &desc[32 * i], 32);
        }
        return result;
    }

  private:
    Ctx ctx;
    int wanted = 0;
    std::vector<float> xy;
    std::vector<std::uint8_t> desc;
};

class HipOrbMatcher : public IOrbMatcher
{
  public:
    std::vector<DescriptorMatch> match(const std::vector<OrbKeypoint>& fromDescriptors,
                                       const std::vector<OrbKeypoint>& toDescriptors) override
    {
        ctx.ensure(0, 0); // the matcher needs no detector buffers
        gather_descriptors(fromDescriptors, from);
        gather_descriptors(toDescriptors, to);
        fi.resize(toDescriptors.size() + 1);
        ti.resize(toDescriptors.size() + 1);
        int n = 0;
        const int rc = mslam_hip_match(ctx.h, from.data(), static_cast<int>(fromDescriptors.size()), to.data(),
                                       static_cast<int>(toDescriptors.size()), 0.7 /* orb_feature.cpp:101 */, fi.data(),
                                       ti.data(), &n);
        if(rc != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_match", rc);
        std::vector<DescriptorMatch> matches(static_cast<std::size_t>(n));
        for(int i = 0; i < n; ++i)
            matches[i] = DescriptorMatch{static_cast<std::size_t>(fi[i]), static_cast<std::size_t>(ti[i])};
        return matches;
    }

  private:
    Ctx ctx;
    std::vector<std::uint8_t> from, to;
    std::vector<std::int32_t> fi, ti;
};

// The BoW object both interfaces sit on.  The reference frontend holds the relocalizer and the loop detector as
// two separate members (rgbd_feature_frontend.cpp:153 and the loopDetector it is constructed with); keyframes are
// only ever fed through IRelocalizer::addKeyframe (:176), and ILoopDetector::detectLoop() takes no arguments
// (loop_detection.hpp:13).  So the two adapters returned by the two factories share ONE database: what
// addKeyframe feeds is what detectLoop() reports on.
class BowDatabase
{
  public:
    using KeyframePtr = std::shared_ptr<Keyframe<slam3d::SensorState>>;

    // like OrbRelocalizer (orb_relocalizer.cpp:26-30): loads "orbvoc.dbow3" from the working directory and throws
    // when it is missing.  MSLAM_ORB_VOCABULARY overrides the path (the reference hard-codes it).
    BowDatabase()
    {
        const char* env = std::getenv("MSLAM_ORB_VOCABULARY");
        const std::string path = env ? env : "orbvoc.dbow3";
        std::ifstream f(path, std::ios::binary);
        if(!f)
            throw std::runtime_error("HipOrbRelocalizer: could not open vocabulary " + path);
        std::vector<char> blob((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        ctx.ensure(0, 0);
        const int rc = mslam_hip_bow_load(ctx.h, blob.data(), blob.size());
        if(rc != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_bow_load", rc);
    }

    static std::shared_ptr<BowDatabase> shared()
    {
        static std::mutex m;
        static std::weak_ptr<BowDatabase> live;
        std::lock_guard<std::mutex> lock(m);
        auto p = live.lock();
        if(!p)
        {
            p = std::make_shared<BowDatabase>();
            live = p;
        }
        return p;
    }

    std::vector<KeyframePtr> relocalize(const std::vector<OrbKeypoint>& keypoints, std::vector<double>* scoresOut = nullptr)
    {
        gather_descriptors(keypoints, desc);
        std::int32_t ids[64];
        double scores[64];
        int n = 0;
        const int rc = mslam_hip_bow_db_query(ctx.h, desc.data(), static_cast<int>(keypoints.size()), 64, ids, scores, &n);
        if(rc != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_bow_db_query", rc);
        std::vector<KeyframePtr> out;
        for(int i = 0; i < n && out.size() < 4; ++i)
        {
            auto it = entryToKeyframe.find(ids[i]);
            if(it != entryToKeyframe.end())
            {
                out.push_back(it->second);
                if(scoresOut)
                    scoresOut->push_back(scores[i]);
            }
        }
        return out;
    }

    int addKeyframe(KeyframePtr keyframe, const std::vector<OrbKeypoint>& keypoints) // -> the BoW entry id, -1: not fed
    {
        if(keypoints.empty()) // the reference asserts non-empty (orb_relocalizer.cpp:42)
            return -1;
        // loop candidate = best earlier keyframe for the one being added
        const auto candidates = relocalize(keypoints);
        lastLoop = candidates.empty() ? nullptr : candidates.front();
        lastFed = keypoints; // (detectLoopVerified verifies the candidate against these)
        int entry = -1;
        const int rc = mslam_hip_bow_db_add(ctx.h, desc.data(), static_cast<int>(keypoints.size()), &entry);
        if(rc != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_bow_db_add", rc);
        entryToKeyframe[entry] = std::move(keyframe);
        return entry;
    }

    void removeKeyframe(const KeyframePtr& keyframe)
    {
        for(auto it = entryToKeyframe.begin(); it != entryToKeyframe.end();)
        {
            if(it->second == keyframe)
            {
                const int rc = mslam_hip_bow_db_remove(ctx.h, it->first); // never scored again
                if(rc != MSLAM_HIP_OK)
                    raise(ctx.h, "mslam_hip_bow_db_remove", rc);
                auto lm = storeId.find(it->first);
                if(lm != storeId.end()) // its landmarks leave the keyframe store with it
                {
                    const int rk = mslam_hip_kf_remove(ctx.h, lm->second);
                    storeId.erase(lm);
                    if(rk != MSLAM_HIP_OK)
                        raise(ctx.h, "mslam_hip_kf_remove", rk);
                }
                it = entryToKeyframe.erase(it);
            }
            else
                ++it;
        }
        if(lastLoop == keyframe)
            lastLoop = nullptr;
    }

    KeyframePtr detectLoop() const { return lastLoop; }

    // ---- extension: candidates verified against stored landmarks (mslam_hip_relocalize) ----
    void addKeyframeLandmarks(const KeyframePtr& keyframe, const std::vector<OrbKeypoint>& keypoints,
                              const std::vector<Vector3>& worldPoints, const std::vector<std::int64_t>* landmarkIds = nullptr)
    {
        if(keypoints.size() != worldPoints.size() || (landmarkIds && landmarkIds->size() != keypoints.size()))
            throw std::runtime_error("addKeyframeLandmarks: one world point (and one landmark id) per keypoint");
        for(const auto& e : entryToKeyframe)
            if(e.second == keyframe)
            {
                gather_descriptors(keypoints, desc);
                std::vector<double> world(3 * worldPoints.size());
                for(std::size_t i = 0; i < worldPoints.size(); ++i)
                    world[3 * i] = worldPoints[i].x(), world[3 * i + 1] = worldPoints[i].y(), world[3 * i + 2] = worldPoints[i].z();
                // the store's id is the BoW entry id: one id names both (a keyframe track() inserted has an id of its own)
                const int n = static_cast<int>(keypoints.size());
                const int rc = landmarkIds ? mslam_hip_kf_add_ids(ctx.h, e.first, desc.data(), world.data(), landmarkIds->data(), n)
                                           : mslam_hip_kf_add(ctx.h, e.first, desc.data(), world.data(), n);
                if(rc != MSLAM_HIP_OK)
                    raise(ctx.h, landmarkIds ? "mslam_hip_kf_add_ids" : "mslam_hip_kf_add", rc);
                storeId[e.first] = e.first;
                return;
            }
        throw std::runtime_error("addKeyframeLandmarks: the keyframe has not been added");
    }

    // relocalize()'s candidates (those with stored landmarks), each matched and solved; OpenCvRansacPnp's operating point
    // (cv_ransac_pnp.cpp:56-57: 100 iterations, 5 px) and the matcher's ratio (orb_feature.cpp:101), no guess (:519)
    VerifiedRelocalization relocalizePose(const std::vector<OrbKeypoint>& keypoints, const CameraParameters& camera, int minInliers)
    {
        std::vector<std::int32_t> entries;
        gather_descriptors(keypoints, desc);
        std::int32_t ids[64];
        double scores[64];
        int n = 0;
        const int rc = mslam_hip_bow_db_query(ctx.h, desc.data(), static_cast<int>(keypoints.size()), 64, ids, scores, &n);
        if(rc != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_bow_db_query", rc);
        int taken = 0;
        for(int i = 0; i < n && taken < 4; ++i)
            if(entryToKeyframe.count(ids[i]))
            {
                ++taken; // the same four relocalize() returns
                if(storeId.count(ids[i]))
                    entries.push_back(ids[i]);
            }
        return verify(keypoints, entries, camera, minInliers);
    }

    VerifiedRelocalization detectLoopVerified(const CameraParameters& camera, int minInliers)
    {
        std::vector<std::int32_t> entries;
        for(const auto& e : entryToKeyframe)
            if(lastLoop && e.second == lastLoop && storeId.count(e.first))
                entries.push_back(e.first);
        return verify(lastFed, entries, camera, minInliers);
    }

    // ---- extension: the tracking step on the stored landmarks (mslam_hip_track, mslam_hip_kf_visible) ----
    int initFirstKeyframe(const KeyframePtr& keyframe, const std::vector<OrbKeypoint>& keypoints, const std::uint16_t* depth, int width,
                          int height, const CameraParameters& camera, double zMax)
    {
        const int n = static_cast<int>(keypoints.size());
        gather(keypoints);
        std::vector<double> xyz(3 * keypoints.size() + 3);
        std::vector<std::uint8_t> valid(keypoints.size() + 1);
        const int rb = mslam_hip_backproject(ctx.h, depth, width, height, camera.factor, camera.focal.x(), camera.focal.y(),
                                             camera.principalPoint.x(), camera.principalPoint.y(), xy.data(), n, xyz.data(), valid.data());
        if(rb != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_backproject", rb);
        const int entry = addKeyframe(keyframe, keypoints); // (:176; gathers `desc` again: the same bytes)
        if(entry < 0)
            throw std::runtime_error("initFirstKeyframe: no keypoints");
        std::vector<std::uint8_t> d;
        std::vector<double> world; // identity pose: the camera point is the world point
        for(int i = 0; i < n; ++i)
            if(valid[i] && xyz[3 * i + 2] <= zMax)
            {
                d.insert(d.end(), &desc[32 * (std::size_t)i], &desc[32 * (std::size_t)i] + 32);
                world.insert(world.end(), &xyz[3 * (std::size_t)i], &xyz[3 * (std::size_t)i] + 3);
            }
        const int count = static_cast<int>(world.size() / 3);
        const int rc = mslam_hip_kf_add(ctx.h, entry, d.data(), world.data(), count);
        if(rc != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_kf_add", rc);
        storeId[entry] = entry;
        return count;
    }

    KeyframeTrackResult trackKeyframe(const std::vector<OrbKeypoint>& keypoints, const std::uint16_t* depth, int width, int height,
                                      const CameraParameters& camera, const KeyframePtr& reference,
                                      const std::vector<KeyframePtr>& neighbours, const double* rvecGuess, const double* tvecGuess,
                                      const KeyframePtr& newKeyframe, const KeyframeTrackOptions& o)
    {
        return trackAgainst(storedLandmarksOf(reference), keypoints, depth, width, height, camera, neighbours, rvecGuess, tvecGuess,
                            newKeyframe, o);
    }

    // ---- extension: the local map (mslam_hip_kf_read_ids, mslam_hip_kf_covisible, mslam_hip_kf_union) ----
    std::vector<std::int64_t> landmarkIds(const KeyframePtr& keyframe)
    {
        const int id = storedLandmarksOf(keyframe);
        int n = 0;
        int rc = mslam_hip_kf_read_ids(ctx.h, id, nullptr, 0, &n);
        std::vector<std::int64_t> out(static_cast<std::size_t>(n) + 1);
        if(rc == MSLAM_HIP_OK)
            rc = mslam_hip_kf_read_ids(ctx.h, id, out.data(), n, &n);
        if(rc != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_kf_read_ids", rc);
        out.resize(static_cast<std::size_t>(n));
        return out;
    }

    std::vector<int> covisibleLandmarks(const KeyframePtr& keyframe, const std::vector<KeyframePtr>& others)
    {
        std::vector<std::int32_t> ids(others.size() + 1), counts(others.size() + 1);
        for(std::size_t k = 0; k < others.size(); ++k)
            ids[k] = storedLandmarksOf(others[k]);
        const int rc = mslam_hip_kf_covisible(ctx.h, storedLandmarksOf(keyframe), ids.data(), static_cast<int>(others.size()), counts.data());
        if(rc != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_kf_covisible", rc);
        return std::vector<int>(counts.begin(), counts.begin() + static_cast<std::ptrdiff_t>(others.size()));
    }

    int buildLocalMap(const std::vector<KeyframePtr>& members)
    {
        std::vector<std::int32_t> ids(members.size() + 1);
        for(std::size_t k = 0; k < members.size(); ++k)
            ids[k] = storedLandmarksOf(members[k]);
        int n = 0;
        int rc = mslam_hip_set_union_descriptor(ctx.h, unionDescriptor);
        if(rc != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_set_union_descriptor", rc);
        rc = mslam_hip_kf_union(ctx.h, kLocalMapId, ids.data(), static_cast<int>(members.size()), &n);
        if(rc != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_kf_union", rc);
        haveLocalMap = true;
        return n;
    }

    KeyframeTrackResult trackLocalMap(const std::vector<OrbKeypoint>& keypoints, const std::uint16_t* depth, int width, int height,
                                      const CameraParameters& camera, const std::vector<KeyframePtr>& neighbours,
                                      const double* rvecGuess, const double* tvecGuess, const KeyframePtr& newKeyframe,
                                      const KeyframeTrackOptions& o)
    {
        if(!haveLocalMap)
            throw std::runtime_error("trackLocalMap: no local map has been built");
        return trackAgainst(kLocalMapId, keypoints, depth, width, height, camera, neighbours, rvecGuess, tvecGuess, newKeyframe, o);
    }

    // ---- extension: landmark fusion (mslam_hip_kf_fuse) ----
    LandmarkFusion fuseLandmarks(const KeyframePtr& keepEntry, const KeyframePtr& dropEntry, const double R[9], const double t[3],
                                 const LandmarkFuseParams& p)
    {
        const int keep = storedLandmarksOf(keepEntry), drop = storedLandmarksOf(dropEntry);
        int cap = 0, nDrop = 0;
        int rc = mslam_hip_kf_read_ids(ctx.h, keep, nullptr, 0, &cap);
        if(rc == MSLAM_HIP_OK)
            rc = mslam_hip_kf_read_ids(ctx.h, drop, nullptr, 0, &nDrop);
        if(rc != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_kf_read_ids", rc);
        cap = std::min(cap, nDrop); // one pair per landmark of either entry at most
        const std::size_t rows = static_cast<std::size_t>(cap) + 1;
        std::vector<std::int32_t> keepPos(rows), dropPos(rows), dist(rows);
        std::vector<std::int64_t> keepId(rows), dropId(rows);
        int n = 0;
        LandmarkFusion out;
        rc = mslam_hip_kf_fuse(ctx.h, keep, drop, R, t, p.camera.focal.x(), p.camera.focal.y(), p.camera.principalPoint.x(),
                               p.camera.principalPoint.y(), p.width, p.height, p.radius, p.maxDistance, p.ratio, p.maxWorldDistance,
                               keepPos.data(), dropPos.data(), keepId.data(), dropId.data(), dist.data(), cap, &n, &out.rewritten);
        if(rc != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_kf_fuse", rc);
        for(int k = 0; k < n; ++k)
        {
            FusedLandmarkPair pair;
            pair.keepPosition = keepPos[k], pair.dropPosition = dropPos[k], pair.keepId = keepId[k], pair.dropId = dropId[k];
            pair.distance = dist[k];
            out.pairs.push_back(pair);
        }
        return out;
    }

    // ---- extension: landmark fusion into many keyframes (mslam_hip_kf_fuse_multi) ----
    MultiLandmarkFusion fuseLandmarksMulti(const KeyframePtr& keepEntry, const std::vector<KeyframePtr>& dropEntries,
                                           const std::vector<double>& R, const std::vector<double>& t, const LandmarkFuseParams& p)
    {
        const std::size_t targets = dropEntries.size();
        if(R.size() != 9 * targets || t.size() != 3 * targets)
            throw std::runtime_error("fuseLandmarksMulti: R and t do not hold one pose per target");
        const int keep = storedLandmarksOf(keepEntry);
        std::vector<std::int32_t> drops(targets + 1);
        int cap = 0, nDropAll = 0;
        int rc = mslam_hip_kf_read_ids(ctx.h, keep, nullptr, 0, &cap);
        for(std::size_t m = 0; rc == MSLAM_HIP_OK && m < targets; ++m)
        {
            int n = 0;
            drops[m] = storedLandmarksOf(dropEntries[m]);
            rc = mslam_hip_kf_read_ids(ctx.h, drops[m], nullptr, 0, &n);
            nDropAll += n;
        }
        if(rc != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_kf_read_ids", rc);
        cap = std::min(cap, nDropAll); // one pair per keep id and per drop id at most
        const std::size_t rows = static_cast<std::size_t>(cap) + 1;
        std::vector<std::int32_t> target(rows), keepPos(rows), dropPos(rows), dist(rows);
        std::vector<std::int64_t> keepId(rows), dropId(rows);
        int n = 0;
        MultiLandmarkFusion out;
        rc = mslam_hip_kf_fuse_multi(ctx.h, keep, drops.data(), static_cast<int>(targets), R.data(), t.data(), p.camera.focal.x(),
                                     p.camera.focal.y(), p.camera.principalPoint.x(), p.camera.principalPoint.y(), p.width, p.height,
                                     p.radius, p.maxDistance, p.ratio, p.maxWorldDistance, target.data(), keepPos.data(), dropPos.data(),
                                     keepId.data(), dropId.data(), dist.data(), cap, &n, &out.rewritten);
        if(rc != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_kf_fuse_multi", rc);
        for(int k = 0; k < n; ++k)
        {
            MultiFusedLandmarkPair pair;
            pair.target = target[k], pair.keepPosition = keepPos[k], pair.dropPosition = dropPos[k];
            pair.keepId = keepId[k], pair.dropId = dropId[k], pair.distance = dist[k];
            out.pairs.push_back(pair);
        }
        return out;
    }

    // ---- removeObservation's body (mslam_hip_kf_remove_observations) ----
    std::vector<int> removeObservations(const std::vector<std::pair<KeyframePtr, std::int64_t>>& observations)
    {
        const std::size_t n = observations.size();
        std::vector<std::int32_t> ids(n + 1), removed(n + 1);
        std::vector<std::int64_t> lids(n + 1);
        for(std::size_t p = 0; p < n; ++p)
            ids[p] = storedLandmarksOf(observations[p].first), lids[p] = observations[p].second;
        const int rc = mslam_hip_kf_remove_observations(ctx.h, ids.data(), lids.data(), static_cast<int>(n), removed.data(), nullptr);
        if(rc != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_kf_remove_observations", rc);
        return std::vector<int>(removed.begin(), removed.begin() + static_cast<std::ptrdiff_t>(n));
    }

    // ---- keyframe culling (mslam_hip_kf_cull_search, then this adapter's own removeKeyframe for every culled keyframe: the
    // store id is the BoW entry id, and both entries leave together) ----
    std::vector<KeyframeCullVerdict> cullKeyframes(const std::vector<KeyframePtr>& map, const std::vector<KeyframePtr>& candidates,
                                                   const KeyframeCullParams& p)
    {
        const std::size_t n = map.size(), m = candidates.size();
        std::vector<std::int32_t> ids(n + 1), cand(m + 1), landmarks(m + 1), redundant(m + 1);
        std::vector<std::uint8_t> culled(m + 1);
        for(std::size_t k = 0; k < n; ++k)
            ids[k] = storedLandmarksOf(map[k]);
        for(std::size_t k = 0; k < m; ++k)
            cand[k] = storedLandmarksOf(candidates[k]);
        const int rc = mslam_hip_kf_cull_search(ctx.h, ids.data(), static_cast<int>(n), cand.data(), static_cast<int>(m), p.minObservers,
                                                p.ratio, p.minLandmarks, culled.data(), landmarks.data(), redundant.data(), nullptr);
        if(rc != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_kf_cull_search", rc);
        std::vector<KeyframeCullVerdict> out(m);
        for(std::size_t k = 0; k < m; ++k)
        {
            out[k].keyframe = candidates[k];
            out[k].culled = culled[k] != 0, out[k].landmarks = landmarks[k], out[k].redundant = redundant[k];
            if(out[k].culled)
                removeKeyframe(candidates[k]);
        }
        return out;
    }

    // ---- landmark culling (an extension).  cullLandmarks asks the search for the count first (a NULL list changes nothing
    // and consults no capacity), then runs the fused call with room for exactly that many rows ----
    std::vector<CulledLandmark> cullLandmarks(const std::vector<KeyframePtr>& map, const std::vector<KeyframePtr>& candidates, int minObservers)
    {
        const std::size_t n = map.size(), m = candidates.size();
        std::vector<std::int32_t> ids(n + 1), cand(m + 1);
        for(std::size_t k = 0; k < n; ++k)
            ids[k] = storedLandmarksOf(map[k]);
        for(std::size_t k = 0; k < m; ++k)
            cand[k] = storedLandmarksOf(candidates[k]);
        int found = 0;
        int rc = mslam_hip_kf_cull_landmarks_search(ctx.h, ids.data(), static_cast<int>(n), cand.data(), static_cast<int>(m), minObservers,
                                                    nullptr, nullptr, 0, &found);
        if(rc != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_kf_cull_landmarks_search", rc);
        std::vector<std::int64_t> lids(static_cast<std::size_t>(found) + 1);
        std::vector<std::int32_t> observers(lids.size());
        rc = mslam_hip_kf_cull_landmarks(ctx.h, ids.data(), static_cast<int>(n), cand.data(), static_cast<int>(m), minObservers, lids.data(),
                                         observers.data(), found, &found, nullptr, nullptr);
        if(rc != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_kf_cull_landmarks", rc);
        std::vector<CulledLandmark> out(static_cast<std::size_t>(found));
        for(std::size_t p = 0; p < out.size(); ++p)
            out[p].id = lids[p], out[p].observers = observers[p];
        return out;
    }

    std::vector<int> removeLandmarks(const std::vector<KeyframePtr>& map, const std::vector<std::int64_t>& landmarks)
    {
        const std::size_t n = map.size(), m = landmarks.size();
        std::vector<std::int32_t> ids(n + 1), removed(m + 1);
        for(std::size_t k = 0; k < n; ++k)
            ids[k] = storedLandmarksOf(map[k]);
        const int rc = mslam_hip_kf_remove_landmarks(ctx.h, ids.data(), static_cast<int>(n), landmarks.data(), static_cast<int>(m),
                                                     removed.data(), nullptr, nullptr);
        if(rc != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_kf_remove_landmarks", rc);
        return std::vector<int>(removed.begin(), removed.begin() + static_cast<std::ptrdiff_t>(m));
    }

    KeyframeTrackResult trackAgainst(int refId,const std::vector<OrbKeypoint>& keypoints, const std::uint16_t* depth, int width, int height,
                                     const CameraParameters& camera, const std::vector<KeyframePtr>& neighbours, const double* rvecGuess,
                                     const double* tvecGuess, const KeyframePtr& newKeyframe, const KeyframeTrackOptions& o)
    {
        std::vector<std::int32_t> vote(neighbours.size() + 1), counts(neighbours.size() + 1);
        for(std::size_t k = 0; k < neighbours.size(); ++k)
            vote[k] = storedLandmarksOf(neighbours[k]);
        gather(keypoints);
        const int newId = newKeyframe ? nextTrackedId : -1;
        const int cap = static_cast<int>(keypoints.size());
        std::vector<std::int32_t> src(keypoints.size() + 1), kp(keypoints.size() + 1);
        const bool guess = rvecGuess && tvecGuess;
        if(guidedRadius > 0.0 || guidedSet)
        {
            // the mode's frame extent is this call's
            const int grc = mslam_hip_set_guided_match(ctx.h, guidedRadius, guidedMaxDistance, width, height);
            if(grc != MSLAM_HIP_OK)
                raise(ctx.h, "mslam_hip_set_guided_match", grc);
            guidedSet = guidedRadius > 0.0;
        }
        // setTrackPose: on the context for this call, the default again behind it (relocalizePose shares the context)
        struct PoseScope
        {
            mslam_hip_ctx* h;
            bool on;
            ~PoseScope()
            {
                if(on)
                    mslam_hip_set_track_pose(h, MSLAM_HIP_TRACK_POSE_PNP, 0.0);
            }
        } poseScope{ctx.h, trackPoseKind != MSLAM_HIP_TRACK_POSE_PNP};
        if(poseScope.on)
        {
            const int prc = mslam_hip_set_track_pose(ctx.h, trackPoseKind, trackPoseDistance);
            if(prc != MSLAM_HIP_OK)
                raise(ctx.h, "mslam_hip_set_track_pose", prc);
        }
        mslam_hip_track_result out;
        // the matcher's ratio and OpenCvRansacPnp's operating point, as relocalizePose (orb_feature.cpp:101, cv_ransac_pnp.cpp:56-57)
        const int rc = mslam_hip_track(ctx.h, desc.data(), xy.data(), cap, depth, width, height, camera.factor, camera.focal.x(),
                                       camera.focal.y(), camera.principalPoint.x(), camera.principalPoint.y(), refId, vote.data(),
                                       static_cast<int>(neighbours.size()), 0.7, 100, 5.0, o.seed, guess ? 1 : 0, rvecGuess, tvecGuess,
                                       o.minMatchedPoints, o.newKeyframeMinLandmarks, newId, o.zMax, &out, counts.data(), nullptr,
                                       nullptr, nullptr, 0, src.data(), kp.data(), cap);
        if(rc != MSLAM_HIP_OK && rc != MSLAM_HIP_E_NO_MODEL)
            raise(ctx.h, "mslam_hip_track", rc);
        KeyframeTrackResult r;
        r.tracked = out.tracked != 0, r.keyframeRequired = out.keyframe_required != 0, r.keyframeAdded = out.keyframe_added != 0;
        r.matches = out.n_matches, r.correspondences = out.n_correspondences, r.inliers = out.n_inliers;
        std::memcpy(r.rvec, out.rvec, sizeof(r.rvec));
        std::memcpy(r.tvec, out.tvec, sizeof(r.tvec));
        std::memcpy(r.R, out.R, sizeof(r.R));
        r.visible.assign(counts.begin(), counts.begin() + static_cast<std::ptrdiff_t>(neighbours.size()));
        if(out.vote_best >= 0)
            r.bestReference = neighbours[static_cast<std::size_t>(out.vote_best)];
        if(r.keyframeAdded)
        {
            ++nextTrackedId;
            const int entry = addKeyframe(newKeyframe, keypoints); // (:375 -> :176)
            if(entry < 0)
                throw std::runtime_error("trackKeyframe: the new keyframe could not be fed");
            storeId[entry] = newId;
            r.landmarks = out.n_entry, r.inherited = out.n_inherited;
            r.entrySource.assign(src.begin(), src.begin() + out.n_entry);
            r.entryKeypoint.assign(kp.begin(), kp.begin() + out.n_entry);
        }
        return r;
    }

    std::vector<int> visibleLandmarks(const std::vector<KeyframePtr>& neighbours, const double R[9], const double t[3],
                                      const CameraParameters& camera, int width, int height, int* best)
    {
        std::vector<std::int32_t> ids(neighbours.size() + 1), counts(neighbours.size() + 1);
        for(std::size_t k = 0; k < neighbours.size(); ++k)
            ids[k] = storedLandmarksOf(neighbours[k]);
        int b = -1;
        const int rc = mslam_hip_kf_visible(ctx.h, ids.data(), static_cast<int>(neighbours.size()), R, t, camera.focal.x(), camera.focal.y(),
                                            camera.principalPoint.x(), camera.principalPoint.y(), width, height, counts.data(), &b);
        if(rc != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_kf_visible", rc);
        if(best)
            *best = b;
        return std::vector<int>(counts.begin(), counts.begin() + static_cast<std::ptrdiff_t>(neighbours.size()));
    }

    void setGuidedMatch(double radius, int maxDistance)
    {
        if(!(radius == radius) || maxDistance < 0 || maxDistance > 256)
            throw std::invalid_argument("setGuidedMatch: the radius is NaN or maxDistance lies outside 0..256");
        guidedRadius = radius > 0.0 ? radius : 0.0;
        guidedMaxDistance = maxDistance;
    }

    void setTrackPose(int kind, double maxDistance)
    {
        if((kind != MSLAM_HIP_TRACK_POSE_PNP && kind != MSLAM_HIP_TRACK_POSE_ALIGN) ||
           (kind == MSLAM_HIP_TRACK_POSE_ALIGN && !(maxDistance > 0.0)))
            throw std::invalid_argument("setTrackPose: the kind is neither 0 (PnP) nor 1 (alignment), or alignment without a maxDistance > 0");
        trackPoseKind = kind;
        trackPoseDistance = kind == MSLAM_HIP_TRACK_POSE_ALIGN ? maxDistance : 0.0;
    }

    void setUnionDescriptor(int mode)
    {
        if(mode != MSLAM_HIP_UNION_DESC_RECENT && mode != MSLAM_HIP_UNION_DESC_DISTINCTIVE)
            throw std::invalid_argument("setUnionDescriptor: the mode is neither 0 (recent) nor 1 (distinctive)");
        unionDescriptor = mode;
    }

  private:
    // descriptors into `desc`, coordinates (as float, what the detector produced) into `xy`
    void gather(const std::vector<OrbKeypoint>& keypoints)
    {
        gather_descriptors(keypoints, desc);
        xy.resize(2 * keypoints.size() + 2);
        for(std::size_t i = 0; i < keypoints.size(); ++i)
        {
            xy[2 * i] = static_cast<float>(keypoints[i].keypoint.coordinates.x());
            xy[2 * i + 1] = static_cast<float>(keypoints[i].keypoint.coordinates.y());
        }
    }
    int storedLandmarksOf(const KeyframePtr& keyframe) const
    {
        for(const auto& e : entryToKeyframe)
            if(e.second == keyframe)
            {
                auto it = storeId.find(e.first);
                if(it != storeId.end())
                    return it->second;
            }
        throw std::runtime_error("the keyframe has no stored landmarks");
    }

    VerifiedRelocalization verify(const std::vector<OrbKeypoint>& keypoints, const std::vector<std::int32_t>& entries,
                                  const CameraParameters& camera, int minInliers)
    {
        gather_descriptors(keypoints, desc);
        std::vector<float> xy(2 * keypoints.size());
        for(std::size_t i = 0; i < keypoints.size(); ++i)
        {
            xy[2 * i] = static_cast<float>(keypoints[i].keypoint.coordinates.x());
            xy[2 * i + 1] = static_cast<float>(keypoints[i].keypoint.coordinates.y());
        }
        std::vector<mslam_hip_reloc_candidate> out(entries.size() + 1);
        std::vector<std::int32_t> stored(entries.size());
        for(std::size_t k = 0; k < entries.size(); ++k)
            stored[k] = storeId.at(entries[k]);
        int best = -1;
        const int rc = mslam_hip_relocalize(ctx.h, desc.data(), xy.data(), nullptr, static_cast<int>(keypoints.size()), stored.data(),
                                            static_cast<int>(entries.size()), camera.focal.x(), camera.focal.y(),
                                            camera.principalPoint.x(), camera.principalPoint.y(), 0.7, 100, 5.0, 0, 0, nullptr,
                                            nullptr, minInliers, out.data(), &best, nullptr, nullptr, nullptr, 0);
        if(rc != MSLAM_HIP_OK && rc != MSLAM_HIP_E_NO_MODEL)
            raise(ctx.h, "mslam_hip_relocalize", rc);
        VerifiedRelocalization result;
        for(std::size_t k = 0; k < entries.size(); ++k)
        {
            VerifiedCandidate c;
            c.keyframe = entryToKeyframe[entries[k]];
            c.matches = out[k].n_matches, c.correspondences = out[k].n_correspondences, c.inliers = out[k].n_inliers;
            c.hasModel = out[k].status != 0;
            result.candidates.push_back(c);
        }
        if(best >= 0)
        {
            result.keyframe = result.candidates[static_cast<std::size_t>(best)].keyframe;
            result.inliers = out[best].n_inliers;
            std::memcpy(result.rvec, out[best].rvec, sizeof(result.rvec));
            std::memcpy(result.tvec, out[best].tvec, sizeof(result.tvec));
        }
        return result;
    }

    Ctx ctx;
    std::vector<std::uint8_t> desc;
    std::map<int, KeyframePtr> entryToKeyframe;
    std::map<int, int> storeId; // BoW entry -> id of its landmarks in the keyframe store (entries without landmarks: absent)
    int nextTrackedId = 1 << 30; // store ids of the keyframes trackKeyframe inserts (BoW entry ids count from 0)
    static constexpr int kLocalMapId = 0x7fffffff; // the store id of the local map (above every keyframe's)
    bool haveLocalMap = false;
    double guidedRadius = 0.0; // setGuidedMatch; applied to the context by the next tracking call, with that call's frame size
    int guidedMaxDistance = 256;
    bool guidedSet = false;    // the context's mode is on
    int trackPoseKind = MSLAM_HIP_TRACK_POSE_PNP; // setTrackPose; applied to the context around every tracking call
    double trackPoseDistance = 0.0;
    int unionDescriptor = MSLAM_HIP_UNION_DESC_RECENT; // setUnionDescriptor; applied to the context by every buildLocalMap
    std::vector<float> xy;
    KeyframePtr lastLoop;
    std::vector<OrbKeypoint> lastFed;
};

class HipOrbRelocalizer : public IOrbRelocalizer,
                          public IVerifiedRelocalizer,
                          public IKeyframeTracker,
                          public ILocalMapTracker,
                          public IDistinctiveLocalMap,
                          public IAlignedKeyframeTracker,
                          public ILandmarkFuser,
                          public IMultiLandmarkFuser,
                          public IObservationRemover,
                          public IKeyframeCuller,
                          public ILandmarkCuller
{
  public:
    HipOrbRelocalizer() : db(BowDatabase::shared()) {}
    std::vector<BowDatabase::KeyframePtr> relocalize(const std::vector<OrbKeypoint>& keypoints) override
    {
        return db->relocalize(keypoints);
    }
    void addKeyframe(BowDatabase::KeyframePtr keyframe, const std::vector<OrbKeypoint>& keypoints) override
    {
        db->addKeyframe(std::move(keyframe), keypoints);
    }
    void removeKeyframe(BowDatabase::KeyframePtr keyframe) override { db->removeKeyframe(keyframe); }
    void addKeyframeLandmarks(BowDatabase::KeyframePtr keyframe, const std::vector<OrbKeypoint>& keypoints,
                              const std::vector<Vector3>& worldPoints) override
    {
        db->addKeyframeLandmarks(keyframe, keypoints, worldPoints);
    }
    VerifiedRelocalization relocalizePose(const std::vector<OrbKeypoint>& keypoints, const CameraParameters& camera,
                                          int minInliers) override
    {
        return db->relocalizePose(keypoints, camera, minInliers);
    }
    int initFirstKeyframe(BowDatabase::KeyframePtr keyframe, const std::vector<OrbKeypoint>& keypoints, const std::uint16_t* depth,
                          int width, int height, const CameraParameters& camera, double zMax) override
    {
        return db->initFirstKeyframe(keyframe, keypoints, depth, width, height, camera, zMax);
    }
    KeyframeTrackResult trackKeyframe(const std::vector<OrbKeypoint>& keypoints, const std::uint16_t* depth, int width, int height,
                                      const CameraParameters& camera, BowDatabase::KeyframePtr reference,
                                      const std::vector<BowDatabase::KeyframePtr>& neighbours, const double* rvecGuess,
                                      const double* tvecGuess, BowDatabase::KeyframePtr newKeyframe,
                                      const KeyframeTrackOptions& options) override
    {
        return db->trackKeyframe(keypoints, depth, width, height, camera, reference, neighbours, rvecGuess, tvecGuess, newKeyframe, options);
    }
    std::vector<int> visibleLandmarks(const std::vector<BowDatabase::KeyframePtr>& neighbours, const double R[9], const double t[3],
                                      const CameraParameters& camera, int width, int height, int* best) override
    {
        return db->visibleLandmarks(neighbours, R, t, camera, width, height, best);
    }
    void setGuidedMatch(double radius, int maxDistance) override { db->setGuidedMatch(radius, maxDistance); }
    void addKeyframeLandmarksWithIds(BowDatabase::KeyframePtr keyframe, const std::vector<OrbKeypoint>& keypoints,
                                     const std::vector<Vector3>& worldPoints, const std::vector<std::int64_t>& landmarkIds) override
    {
        db->addKeyframeLandmarks(keyframe, keypoints, worldPoints, &landmarkIds);
    }
    std::vector<std::int64_t> landmarkIds(BowDatabase::KeyframePtr keyframe) override { return db->landmarkIds(keyframe); }
    std::vector<int> covisibleLandmarks(BowDatabase::KeyframePtr keyframe, const std::vector<BowDatabase::KeyframePtr>& others) override
    {
        return db->covisibleLandmarks(keyframe, others);
    }
    int buildLocalMap(const std::vector<BowDatabase::KeyframePtr>& members) override { return db->buildLocalMap(members); }
    void setUnionDescriptor(int mode) override { db->setUnionDescriptor(mode); }
    void setTrackPose(int kind, double maxDistance) override { db->setTrackPose(kind, maxDistance); }
    LandmarkFusion fuseLandmarks(BowDatabase::KeyframePtr keepEntry, BowDatabase::KeyframePtr dropEntry, const double R[9],
                                 const double t[3], const LandmarkFuseParams& params) override
    {
        return db->fuseLandmarks(keepEntry, dropEntry, R, t, params);
    }
    MultiLandmarkFusion fuseLandmarksMulti(BowDatabase::KeyframePtr keepEntry, const std::vector<BowDatabase::KeyframePtr>& dropEntries,
                                           const std::vector<double>& R, const std::vector<double>& t,
                                           const LandmarkFuseParams& params) override
    {
        return db->fuseLandmarksMulti(keepEntry, dropEntries, R, t, params);
    }
    std::vector<int> removeObservations(const std::vector<std::pair<BowDatabase::KeyframePtr, std::int64_t>>& observations) override
    {
        return db->removeObservations(observations);
    }
    std::vector<KeyframeCullVerdict> cullKeyframes(const std::vector<BowDatabase::KeyframePtr>& map,
                                                   const std::vector<BowDatabase::KeyframePtr>& candidates,
                                                   const KeyframeCullParams& params) override
    {
        return db->cullKeyframes(map, candidates, params);
    }
    std::vector<CulledLandmark> cullLandmarks(const std::vector<BowDatabase::KeyframePtr>& map,
                                              const std::vector<BowDatabase::KeyframePtr>& candidates, int minObservers) override
    {
        return db->cullLandmarks(map, candidates, minObservers);
    }
    std::vector<int> removeLandmarks(const std::vector<BowDatabase::KeyframePtr>& map, const std::vector<std::int64_t>& ids) override
    {
        return db->removeLandmarks(map, ids);
    }
    KeyframeTrackResult trackLocalMap(const std::vector<OrbKeypoint>& keypoints, const std::uint16_t* depth, int width, int height,
                                      const CameraParameters& camera, const std::vector<BowDatabase::KeyframePtr>& neighbours,
                                      const double* rvecGuess, const double* tvecGuess, BowDatabase::KeyframePtr newKeyframe,
                                      const KeyframeTrackOptions& options) override
    {
        return db->trackLocalMap(keypoints, depth, width, height, camera, neighbours, rvecGuess, tvecGuess, newKeyframe, options);
    }

  private:
    std::shared_ptr<BowDatabase> db;
};

class HipLoopDetector : public IOrbLoopDetector, public IVerifiedLoopDetector
{
  public:
    HipLoopDetector() : db(BowDatabase::shared()) {}
    BowDatabase::KeyframePtr detectLoop() override { return db->detectLoop(); }
    VerifiedRelocalization detectLoopVerified(const CameraParameters& camera, int minInliers) override
    {
        return db->detectLoopVerified(camera, minInliers);
    }

  private:
    std::shared_ptr<BowDatabase> db;
};

// drop-in for OpenCvRansacPnp (cv_ransac_pnp.cpp:14-85): the same conversions around the solver call — landmark states and
// image points cast to float (:22-40), the initial sensor pose turned into the world -> camera transform and its rotation
// into a Rodrigues vector (:42-50), cv::solvePnPRansac's arguments (useExtrinsicGuess, 100 iterations, 5 px; :56-57), and
// the result inverted back into a sensor pose (:65-78).
class HipRansacPnp : public ISlam3dPnp
{
  public:
    std::optional<PnpResult> solvePnp(const std::vector<std::shared_ptr<Landmark<Vector3>>>& landmarks,
                                      const std::vector<Vector2>& sensorPoints, const slam3d::SensorState& initial) override
    {
        if(landmarks.size() != sensorPoints.size() || landmarks.size() < 4) // cv::solvePnPRansac asserts npoints >= 4
            return std::nullopt;
        const std::size_t n = landmarks.size();
        obj.resize(3 * n);
        img.resize(2 * n);
        for(std::size_t i = 0; i < n; ++i)
        {
            obj[3 * i] = static_cast<float>(landmarks[i]->state.x());
            obj[3 * i + 1] = static_cast<float>(landmarks[i]->state.y());
            obj[3 * i + 2] = static_cast<float>(landmarks[i]->state.z());
            img[2 * i] = static_cast<float>(sensorPoints[i].x());
            img[2 * i + 1] = static_cast<float>(sensorPoints[i].y());
        }
        // toCameraCoordinateSystemProjection (projection.cpp:19-28)
        const auto inverse = initial.orientation.inverse();
        const Vector3 t0 = -(inverse * initial.position);
        double rvec[3], tvec[3] = {t0.x(), t0.y(), t0.z()};
        toRodrigues(inverse.w(), inverse.x(), inverse.y(), inverse.z(), rvec);
        mask.assign(n, 0);
        int nInliers = 0;
        ctx.ensure(0, 0);
        const int rc = mslam_hip_pnp_ransac(ctx.h, obj.data(), img.data(), static_cast<int>(n), cameraParams.focal.x(),
                                            cameraParams.focal.y(), cameraParams.principalPoint.x(),
                                            cameraParams.principalPoint.y(), 1, 100, 5.0, 0, rvec, tvec, mask.data(), &nInliers);
        if(rc == MSLAM_HIP_E_NO_MODEL)
        {
            std::fprintf(stderr, "[error] Didnt find pnp solution\n"); // cv_ransac_pnp.cpp:61
            return std::nullopt;
        }
        if(rc != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_pnp_ransac", rc);
        // :65-78: the camera rotation as angle-axis, inverted = the sensor orientation; position = -(orientation * t)
        const double angle = std::sqrt(rvec[0] * rvec[0] + rvec[1] * rvec[1] + rvec[2] * rvec[2]);
        double w = 1, x = 0, y = 0, z = 0;
        if(angle > 0)
        {
            const double s = std::sin(0.5 * angle) / angle;
            w = std::cos(0.5 * angle), x = rvec[0] * s, y = rvec[1] * s, z = rvec[2] * s;
        }
        PnpResult result;
        result.pose.orientation = Quaternion(w, x, y, z).inverse();
        result.pose.position = -(result.pose.orientation * Vector3(tvec[0], tvec[1], tvec[2]));
        result.inliers.resize(n, false);
        for(std::size_t i = 0; i < n; ++i)
            result.inliers[i] = mask[i] != 0;
        return result;
    }

  private:
    Ctx ctx;
    std::vector<float> obj, img;
    std::vector<std::uint8_t> mask;
};

// RANSAC rigid alignment of two 3-D point sets (mslam_hip_align_ransac): no reference counterpart.  The points are cast to
// float as the PnP adapter casts its landmarks; the rotation comes back from the call's Rodrigues vector.
class HipRigidAligner : public IRigidAligner
{
  public:
    std::optional<RigidAlignment> align(const std::vector<Vector3>& source, const std::vector<Vector3>& target, double maxDistance,
                                        int iterations, std::uint64_t seed) override
    {
        if(source.size() != target.size() || source.size() < 3)
            return std::nullopt;
        const std::size_t n = source.size();
        src.resize(3 * n);
        dst.resize(3 * n);
        for(std::size_t i = 0; i < n; ++i)
        {
            src[3 * i] = static_cast<float>(source[i].x()), src[3 * i + 1] = static_cast<float>(source[i].y());
            src[3 * i + 2] = static_cast<float>(source[i].z());
            dst[3 * i] = static_cast<float>(target[i].x()), dst[3 * i + 1] = static_cast<float>(target[i].y());
            dst[3 * i + 2] = static_cast<float>(target[i].z());
        }
        mask.assign(n, 0);
        double rvec[3] = {0, 0, 0}, tvec[3] = {0, 0, 0};
        int nInliers = 0;
        ctx.ensure(0, 0);
        const int rc = mslam_hip_align_ransac(ctx.h, src.data(), dst.data(), static_cast<int>(n), iterations, maxDistance, seed, rvec,
                                              tvec, mask.data(), &nInliers);
        if(rc == MSLAM_HIP_E_NO_MODEL)
            return std::nullopt;
        if(rc != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_align_ransac", rc);
        RigidAlignment out;
        // Rodrigues: R = I + sin(a) K + (1 - cos(a)) K^2, K the cross-product matrix of the unit axis
        const double a = std::sqrt(rvec[0] * rvec[0] + rvec[1] * rvec[1] + rvec[2] * rvec[2]);
        const double kx = a > 0 ? rvec[0] / a : 0, ky = a > 0 ? rvec[1] / a : 0, kz = a > 0 ? rvec[2] / a : 0;
        const double c = std::cos(a), s = std::sin(a), v = 1 - c;
        const double R[9] = {c + kx * kx * v, kx * ky * v - kz * s, kx * kz * v + ky * s, ky * kx * v + kz * s, c + ky * ky * v,
                             ky * kz * v - kx * s, kz * kx * v - ky * s, kz * ky * v + kx * s, c + kz * kz * v};
        std::copy(R, R + 9, out.R);
        std::copy(tvec, tvec + 3, out.t);
        out.inliers.resize(n);
        for(std::size_t i = 0; i < n; ++i)
            out.inliers[i] = mask[i] != 0;
        return out;
    }

  private:
    Ctx ctx;
    std::vector<float> src, dst;
    std::vector<std::uint8_t> mask;
};

// The dense TSDF map (mslam_hip_tsdf_*): no reference counterpart.  The context has no detector; the volume lives in it.
class HipDenseMap : public IDenseMap, public IDenseMapRenderer, public IDenseAligner
{
  public:
    void create(const DenseMapParams& q) override
    {
        mslam_hip_tsdf_params p{};
        p.nx = q.nx, p.ny = q.ny, p.nz = q.nz, p.max_frames = q.maxFrames;
        p.voxel = q.voxel, p.trunc = q.trunc, p.max_depth = q.maxDepth;
        std::copy(q.origin, q.origin + 3, p.origin);
        p.width = q.width, p.height = q.height, p.factor = q.camera.factor;
        p.fx = q.camera.focal.x(), p.fy = q.camera.focal.y(), p.cx = q.camera.principalPoint.x(), p.cy = q.camera.principalPoint.y();
        ctx.ensure(0, 0);
        check("mslam_hip_tsdf_create", mslam_hip_tsdf_create(ctx.h, &p));
        params = p;
    }
    void addFrame(int id, const std::vector<std::uint16_t>& depth, const DensePose& pose) override
    {
        ctx.ensure(0, 0);
        if(depth.size() != static_cast<std::size_t>(params.width) * static_cast<std::size_t>(params.height))
            throw std::invalid_argument("HipDenseMap::addFrame: the depth image is not width x height of the volume's camera");
        check("mslam_hip_tsdf_add_frame", mslam_hip_tsdf_add_frame(ctx.h, id, depth.data(), pose.R, pose.t));
    }
    int updatePoses(const std::vector<int>& ids, const std::vector<DensePose>& poses) override
    {
        if(ids.size() != poses.size())
            throw std::invalid_argument("HipDenseMap::updatePoses: one pose per id");
        std::vector<std::int32_t> list(ids.begin(), ids.end());
        std::vector<double> R(9 * ids.size()), t(3 * ids.size());
        for(std::size_t i = 0; i < ids.size(); ++i)
        {
            std::copy(poses[i].R, poses[i].R + 9, R.begin() + 9 * i);
            std::copy(poses[i].t, poses[i].t + 3, t.begin() + 3 * i);
        }
        int moved = 0;
        ctx.ensure(0, 0);
        check("mslam_hip_tsdf_update_poses",
              mslam_hip_tsdf_update_poses(ctx.h, list.data(), R.data(), t.data(), static_cast<int>(ids.size()), &moved));
        return moved;
    }
    void removeFrame(int id) override
    {
        ctx.ensure(0, 0);
        check("mslam_hip_tsdf_remove_frame", mslam_hip_tsdf_remove_frame(ctx.h, id));
    }
    int frames() override
    {
        int n = 0;
        ctx.ensure(0, 0);
        check("mslam_hip_tsdf_info", mslam_hip_tsdf_info(ctx.h, nullptr, &n));
        return n;
    }
    void read(std::vector<std::int32_t>& sums, std::vector<std::int32_t>& weights) override
    {
        ctx.ensure(0, 0);
        check("mslam_hip_tsdf_info", mslam_hip_tsdf_info(ctx.h, &params, nullptr));
        const std::size_t n = static_cast<std::size_t>(params.nx) * params.ny * params.nz;
        sums.assign(n, 0);
        weights.assign(n, 0);
        check("mslam_hip_tsdf_read", mslam_hip_tsdf_read(ctx.h, sums.data(), weights.data()));
    }
    DenseSurface extract(int minWeight) override
    {
        DenseSurface out;
        int n = 0;
        ctx.ensure(0, 0);
        int rc = mslam_hip_tsdf_extract(ctx.h, minWeight, nullptr, nullptr, 0, &n); // the count call
        if(rc != MSLAM_HIP_OK && rc != MSLAM_HIP_E_CAPACITY)
            raise(ctx.h, "mslam_hip_tsdf_extract", rc);
        if(n == 0)
            return out;
        out.points.assign(3 * static_cast<std::size_t>(n), 0.f);
        out.normals.assign(3 * static_cast<std::size_t>(n), 0.f);
        check("mslam_hip_tsdf_extract", mslam_hip_tsdf_extract(ctx.h, minWeight, out.points.data(), out.normals.data(), n, &n));
        return out;
    }
    DenseRender render(const DenseRenderParams& q, const DensePose& pose, bool normals) override
    {
        mslam_hip_tsdf_raycast_params p{};
        p.width = q.width, p.height = q.height;
        p.fx = q.camera.focal.x(), p.fy = q.camera.focal.y(), p.cx = q.camera.principalPoint.x(), p.cy = q.camera.principalPoint.y();
        p.z_near = q.zNear, p.z_far = q.zFar, p.step = q.step, p.coarse = q.coarse, p.min_weight = q.minWeight;
        if(q.width < 1 || q.height < 1 || static_cast<long long>(q.width) * q.height > (1 << 30))
            throw std::invalid_argument("HipDenseMap::render: width, height must be >= 1 with at most 2^30 pixels");
        DenseRender out;
        const std::size_t px = static_cast<std::size_t>(q.width) * static_cast<std::size_t>(q.height);
        out.depth.assign(px, 0.f);
        out.points.assign(3 * px, 0.f);
        if(normals)
            out.normals.assign(3 * px, 0.f);
        ctx.ensure(0, 0);
        check("mslam_hip_tsdf_raycast", mslam_hip_tsdf_raycast(ctx.h, &p, pose.R, pose.t, out.depth.data(), out.points.data(),
                                                               normals ? out.normals.data() : nullptr, &out.hits));
        return out;
    }
    DenseAlignResult align(const std::vector<std::uint16_t>& depth, const DensePose& guess, const DenseAlignParams& q,
                           const DenseRenderParams& render) override
    {
        ctx.ensure(0, 0);
        check("mslam_hip_tsdf_info", mslam_hip_tsdf_info(ctx.h, &params, nullptr));
        if(depth.size() != static_cast<std::size_t>(params.width) * static_cast<std::size_t>(params.height))
            throw std::invalid_argument("HipDenseMap::align: the depth image is not width x height of the volume's camera");
        if(q.levels.empty() || q.levels.size() > MSLAM_HIP_ICP_MAX_LEVELS)
            throw std::invalid_argument("HipDenseMap::align: 1..4 levels");
        mslam_hip_icp_params p{};
        p.width = params.width, p.height = params.height, p.factor = params.factor;
        p.fx = params.fx, p.fy = params.fy, p.cx = params.cx, p.cy = params.cy, p.max_depth = params.max_depth;
        p.n_levels = static_cast<std::int32_t>(q.levels.size());
        for(std::size_t l = 0; l < q.levels.size(); ++l)
            p.stride[l] = q.levels[l].first, p.iterations[l] = q.levels[l].second;
        p.dist_max = q.distMax, p.cos_min = q.cosMin, p.min_pairs = q.minPairs, p.rot_tol = q.rotTol, p.trans_tol = q.transTol;
        mslam_hip_tsdf_raycast_params r{};
        r.width = render.width, r.height = render.height;
        r.fx = render.camera.focal.x(), r.fy = render.camera.focal.y();
        r.cx = render.camera.principalPoint.x(), r.cy = render.camera.principalPoint.y();
        r.z_near = render.zNear, r.z_far = render.zFar, r.step = render.step, r.coarse = render.coarse, r.min_weight = render.minWeight;
        DenseAlignResult out;
        mslam_hip_icp_result res{};
        std::vector<mslam_hip_icp_record> rows(MSLAM_HIP_ICP_MAX_ITERATIONS);
        check("mslam_hip_tsdf_icp", mslam_hip_tsdf_icp(ctx.h, &p, &r, depth.data(), guess.R, guess.t, out.pose.R, out.pose.t, &res,
                                                       rows.data(), static_cast<int>(rows.size())));
        out.status = res.status, out.iterations = res.iterations, out.count = res.count, out.level = res.level, out.cost = res.cost;
        std::copy(res.pivots, res.pivots + 6, out.pivots);
        for(int i = 0; i < res.iterations; ++i)
            out.record.push_back(DenseAlignRecord{rows[i].level, rows[i].count, rows[i].cost, rows[i].rot2, rows[i].trans2});
        return out;
    }

  private:
    void check(const char* what, int rc)
    {
        if(rc != MSLAM_HIP_OK)
            raise(ctx.h, what, rc);
    }
    Ctx ctx;
    mslam_hip_tsdf_params params{};
};

// drop-in for MinMseTracker (ceres_reprojection_error_pnp.cpp:64-110), keeping its conventions where they differ from
// OpenCvRansacPnp's: the initial orientation becomes angle-axis as Eigen::AngleAxisd(q) does it and the initial position is
// the translation itself, with no world -> camera inversion (:71-75); the result's angle, axis and position are cast to
// float and the axis is divided by the float angle before the quaternion is built (:99-109); the inlier set stays empty
// (the reference never sizes it).  setLoss (IRobustPnp, an extension) keeps a loss for every later solve: it is set on the
// adapter's own context before each one.  DEVIATES: a result angle of exactly 0 gives the identity quaternion (the reference
// divides by zero and returns NaN).  Ceres's progress printout (minimizer_progress_to_stdout, :91) is not reproduced.
class HipMinMseTracker : public ISlam3dPnp, public IRobustPnp
{
  public:
    void setLoss(int kind, double scale) override
    {
        if(kind < MSLAM_HIP_BA_LOSS_NONE || kind > MSLAM_HIP_BA_LOSS_CAUCHY ||
           (kind != MSLAM_HIP_BA_LOSS_NONE && !(std::isfinite(scale) && scale > 0.0)))
            throw std::invalid_argument("setLoss: kind 0 (none), 1 (Huber) or 2 (Cauchy); their scale finite and > 0");
        lossKind = kind, lossScale = kind == MSLAM_HIP_BA_LOSS_NONE ? 0.0 : scale;
    }
    std::optional<PnpResult> solvePnp(const std::vector<std::shared_ptr<Landmark<Vector3>>>& landmarks,
                                      const std::vector<Vector2>& sensorPoints, const slam3d::SensorState& initial) override
    {
        if(landmarks.size() != sensorPoints.size()) // the reference asserts it (:68)
            return std::nullopt;
        const std::size_t n = landmarks.size();
        obj.resize(3 * n);
        img.resize(2 * n);
        for(std::size_t i = 0; i < n; ++i)
        {
            obj[3 * i] = landmarks[i]->state.x();
            obj[3 * i + 1] = landmarks[i]->state.y();
            obj[3 * i + 2] = landmarks[i]->state.z();
            img[2 * i] = sensorPoints[i].x();
            img[2 * i + 1] = sensorPoints[i].y();
        }
        double rvec[3], tvec[3] = {initial.position.x(), initial.position.y(), initial.position.z()};
        const Quaternion& q = initial.orientation;
        toRodrigues(q.w(), q.x(), q.y(), q.z(), rvec);
        ctx.ensure(0, 0);
        if(const int lrc = mslam_hip_set_pnp_mse_loss(ctx.h, lossKind, lossScale); lrc != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_set_pnp_mse_loss", lrc);
        const int rc = mslam_hip_pnp_min_mse(ctx.h, obj.data(), img.data(), static_cast<int>(n), cameraParams.focal.x(),
                                             cameraParams.focal.y(), cameraParams.principalPoint.x(),
                                             cameraParams.principalPoint.y(), rvec, tvec, nullptr, nullptr, nullptr);
        if(rc == MSLAM_HIP_E_NO_MODEL) // !summary.IsSolutionUsable() (:95-96)
            return std::nullopt;
        if(rc != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_pnp_min_mse", rc);
        const float resultAngle = static_cast<float>(std::sqrt(rvec[0] * rvec[0] + rvec[1] * rvec[1] + rvec[2] * rvec[2]));
        PnpResult result;
        result.pose.position = Vector3(static_cast<float>(tvec[0]), static_cast<float>(tvec[1]), static_cast<float>(tvec[2]));
        if(resultAngle != 0.0f)
        {
            // Vector3 resultAxis = float(r); resultAxis /= resultAngle; Quaternion{AngleAxis(resultAngle, resultAxis)}
            const double angle = resultAngle;
            const double axis[3] = {static_cast<float>(rvec[0]) / angle, static_cast<float>(rvec[1]) / angle,
                                    static_cast<float>(rvec[2]) / angle};
            const double ha = 0.5 * angle, s = std::sin(ha);
            result.pose.orientation = Quaternion(std::cos(ha), s * axis[0], s * axis[1], s * axis[2]);
        }
        return result;
    }

  private:
    Ctx ctx;
    std::vector<double> obj, img;
    int lossKind = MSLAM_HIP_BA_LOSS_NONE;
    double lossScale = 0.0;
};

// drop-in for CeresBackend's solve (ceres_backend.cpp:140-240): the observations become mslam_hip_bundle_adjust's arrays —
// keyframes and landmarks numbered in the order they first appear, the state as (qx qy qz qw px py pz), keyframe id 1
// constant — and the result is written back into keyframe->state and landmark->state, as Ceres writes through the pointers
// the reference hands it.  More than 64 keyframes is an error (the reduced system is dense); FAILURE updates nothing.
// globalBundleAdjustment is the same adapter on mslam_hip_bundle_adjust_global: up to 1024 keyframes.  closeLoop hands the
// keyframes and edges to mslam_hip_pose_graph and writes the corrected states back the same way; setPoseGraphSolver
// (ISparsePoseGraphBackend, an extension) keeps its linear solver, set on the context before each closeLoop.  setLoss (IRobustBackend,
// an extension) keeps a loss for every later solve: it is set on the adapter's own context before each one.  setGlobalSolver
// (ISparseGlobalBackend, an extension) keeps the linear solver of globalBundleAdjustment, set the same way: with kind 1 up to
// 16384 keyframes.  setPoseGraphLoss (IRobustPoseGraphBackend, an extension) keeps a loss for the edges of closeLoop, set the
// same way.  poseGraphCovariance (IPoseGraphCovariance, an extension) hands closeLoop's arrays to
// mslam_hip_pose_graph_covariance and writes nothing back.
class HipBundleAdjustBackend : public ILoopClosingBackend, public IRobustBackend, public ISparsePoseGraphBackend, public ISparseGlobalBackend,
                               public IRobustPoseGraphBackend, public IPoseGraphCovariance, public IIterativeGlobalBackend,
                               public IIterativePoseGraphBackend
{
  public:
    // IIterativePoseGraphBackend (an extension): kept for every later closeLoop, set on the context before each one
    void setPoseGraphPcg(bool enable, int maxIterations, double tolerance) override
    {
        if(maxIterations < 1 || !(tolerance > 0.0 && tolerance < 1.0))
            throw std::invalid_argument("setPoseGraphPcg: maxIterations >= 1 and a tolerance inside (0, 1)");
        pgPcgEnable = enable, pgPcgMaxIterations = maxIterations, pgPcgTolerance = tolerance;
    }
    GlobalPcgStats poseGraphPcgStats() const override { return pgPcgStats; }
    // IIterativeGlobalBackend (an extension): kept for every later globalBundleAdjustment, set on the context before each one
    void setGlobalPcg(bool enable, int maxIterations, double tolerance) override
    {
        if(maxIterations < 1 || !(tolerance > 0.0 && tolerance < 1.0))
            throw std::invalid_argument("setGlobalPcg: maxIterations >= 1 and a tolerance inside (0, 1)");
        pcgEnable = enable, pcgMaxIterations = maxIterations, pcgTolerance = tolerance;
    }
    GlobalPcgStats globalPcgStats() const override { return pcgStats; }
    // IPoseGraphCovariance (an extension): closeLoop's arrays at the keyframes' present states to
    // mslam_hip_pose_graph_covariance, under closeLoop's loss; nothing is written back
    PoseGraphCovariance poseGraphCovariance(const std::vector<KeyframePtr>& keyframes, const std::vector<PoseGraphEdge>& edges,
                                            const std::vector<KeyframePtr>& of,
                                            const std::vector<std::pair<KeyframePtr, KeyframePtr>>& pairs) override
    {
        PoseGraphArrays pg = poseGraphArrays(keyframes, edges, "poseGraphCovariance");
        auto index = [&](const KeyframePtr& kf) {
            const auto at = pg.kfIndex.find(kf.get());
            if(at == pg.kfIndex.end())
                throw std::runtime_error("poseGraphCovariance: a requested keyframe is not listed");
            return static_cast<std::int32_t>(at->second);
        };
        std::vector<std::int32_t> idx, pairA, pairB;
        for(const auto& kf : of)
            idx.push_back(index(kf));
        for(const auto& pr : pairs)
            pairA.push_back(index(pr.first)), pairB.push_back(index(pr.second));
        PoseGraphCovariance out;
        out.blocks.assign(36 * idx.size(), 0.0), out.cross.assign(36 * pairA.size(), 0.0);
        ctx.ensure(0, 0);
        if(const int rs = mslam_hip_set_pose_graph_loss(ctx.h, pgLossKind, pgLossScale); rs != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_set_pose_graph_loss", rs);
        const int rc = mslam_hip_pose_graph_covariance(ctx.h, pg.poses.data(), pg.fixed.data(), static_cast<int>(keyframes.size()),
                                                       pg.edgeA.data(), pg.edgeB.data(), pg.meas.data(), pg.anyInfo ? pg.info.data() : nullptr,
                                                       static_cast<int>(edges.size()), idx.data(), static_cast<int>(idx.size()),
                                                       out.blocks.data(), pairA.data(), pairB.data(), static_cast<int>(pairA.size()),
                                                       out.cross.data());
        if(rc != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_pose_graph_covariance", rc);
        return out;
    }
    void setPoseGraphLoss(int kind, double scale) override
    {
        if(kind < MSLAM_HIP_BA_LOSS_NONE || kind > MSLAM_HIP_BA_LOSS_CAUCHY ||
           (kind != MSLAM_HIP_BA_LOSS_NONE && !(std::isfinite(scale) && scale > 0.0)))
            throw std::invalid_argument("setPoseGraphLoss: kind 0 (none), 1 (Huber) or 2 (Cauchy); their scale finite and > 0");
        pgLossKind = kind, pgLossScale = kind == MSLAM_HIP_BA_LOSS_NONE ? 0.0 : scale;
    }
    void setGlobalSolver(int kind) override
    {
        if(kind != MSLAM_HIP_BA_GLOBAL_SOLVER_DENSE && kind != MSLAM_HIP_BA_GLOBAL_SOLVER_SPARSE)
            throw std::invalid_argument("setGlobalSolver: kind 0 (dense) or 1 (sparse)");
        globalSolver = kind;
    }
    void setPoseGraphSolver(int kind) override
    {
        if(kind != MSLAM_HIP_PG_SOLVER_DENSE && kind != MSLAM_HIP_PG_SOLVER_SPARSE)
            throw std::invalid_argument("setPoseGraphSolver: kind 0 (dense) or 1 (sparse)");
        poseGraphSolver = kind;
    }
    void setLoss(int kind, double scale) override
    {
        if(kind < MSLAM_HIP_BA_LOSS_NONE || kind > MSLAM_HIP_BA_LOSS_CAUCHY ||
           (kind != MSLAM_HIP_BA_LOSS_NONE && !(std::isfinite(scale) && scale > 0.0)))
            throw std::invalid_argument("setLoss: kind 0 (none), 1 (Huber) or 2 (Cauchy); their scale finite and > 0");
        lossKind = kind, lossScale = kind == MSLAM_HIP_BA_LOSS_NONE ? 0.0 : scale;
    }
    BackendOutput bundleAdjustment(const std::vector<BackendObservation>& observations, int maxIterations) override
    {
        return solve(observations, maxIterations, false);
    }
    BackendOutput globalBundleAdjustment(const std::vector<BackendObservation>& observations, int maxIterations) override
    {
        return solve(observations, maxIterations, true);
    }
    BackendOutput closeLoop(const std::vector<std::shared_ptr<Keyframe<slam3d::SensorState>>>& keyframes,
                            const std::vector<PoseGraphEdge>& edges, int maxIterations) override
    {
        PoseGraphArrays pg = poseGraphArrays(keyframes, edges, "closeLoop");
        std::vector<double>&poses = pg.poses, &meas = pg.meas, &info = pg.info;
        std::vector<std::uint8_t>& fixed = pg.fixed;
        std::vector<std::int32_t>&edgeA = pg.edgeA, &edgeB = pg.edgeB;
        const bool anyInfo = pg.anyInfo;
        ctx.ensure(0, 0);
        if(const int rs = mslam_hip_set_pose_graph_solver(ctx.h, poseGraphSolver); rs != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_set_pose_graph_solver", rs);
        if(const int rs = mslam_hip_set_pose_graph_loss(ctx.h, pgLossKind, pgLossScale); rs != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_set_pose_graph_loss", rs);
        if(const int rs = mslam_hip_set_pose_graph_pcg(ctx.h, pgPcgEnable ? 1 : 0, pgPcgMaxIterations, pgPcgTolerance); rs != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_set_pose_graph_pcg", rs);
        pgPcgStats = GlobalPcgStats{};
        mslam_hip_ba_summary summary{};
        const int rc = mslam_hip_pose_graph(ctx.h, poses.data(), fixed.data(), static_cast<int>(keyframes.size()), edgeA.data(),
                                            edgeB.data(), meas.data(), anyInfo ? info.data() : nullptr, static_cast<int>(edges.size()),
                                            maxIterations, &summary);
        if(rc != MSLAM_HIP_OK && rc != MSLAM_HIP_E_NO_MODEL)
            raise(ctx.h, "mslam_hip_pose_graph", rc);
        mslam_hip_pcg_stats st{};
        if(const int rs = mslam_hip_get_pose_graph_pcg_stats(ctx.h, &st); rs != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_get_pose_graph_pcg_stats", rs);
        pgPcgStats = GlobalPcgStats{st.solves, st.iterations, st.longest, st.at_cap, st.breakdowns};
        BackendOutput out;
        out.termination = summary.termination, out.iterations = summary.iterations;
        out.initialCost = summary.initial_cost, out.finalCost = summary.final_cost;
        if(rc == MSLAM_HIP_OK)
            for(std::size_t k = 0; k < keyframes.size(); ++k)
            {
                const double* v = &poses[7 * k];
                keyframes[k]->state.orientation = Quaternion(v[3], v[0], v[1], v[2]);
                keyframes[k]->state.position = Vector3(v[4], v[5], v[6]);
            }
        out.updatedKeyframes = keyframes;
        return out;
    }

  private:
    // closeLoop's problem as mslam_hip_pose_graph's arrays: keyframe id 1 constant, sqrt_info only when an edge carries one
    struct PoseGraphArrays
    {
        std::map<const void*, int> kfIndex;
        std::vector<double> poses, meas, info;
        std::vector<std::uint8_t> fixed;
        std::vector<std::int32_t> edgeA, edgeB;
        bool anyInfo = false;
    };
    static PoseGraphArrays poseGraphArrays(const std::vector<std::shared_ptr<Keyframe<slam3d::SensorState>>>& keyframes,
                                           const std::vector<PoseGraphEdge>& edges, const char* who)
    {
        PoseGraphArrays pg;
        std::map<const void*, int>& kfIndex = pg.kfIndex;
        for(std::size_t k = 0; k < keyframes.size(); ++k)
            kfIndex.emplace(keyframes[k].get(), static_cast<int>(k));
        pg.poses.assign(7 * keyframes.size(), 0.0), pg.meas.assign(7 * edges.size(), 0.0), pg.fixed.assign(keyframes.size(), 0);
        std::vector<double>&poses = pg.poses, &meas = pg.meas, &info = pg.info;
        std::vector<std::uint8_t>& fixed = pg.fixed;
        std::vector<std::int32_t>&edgeA = pg.edgeA, &edgeB = pg.edgeB;
        bool& anyInfo = pg.anyInfo;
        auto put = [](const slam3d::SensorState& st, double* v) {
            v[0] = st.orientation.x(), v[1] = st.orientation.y(), v[2] = st.orientation.z(), v[3] = st.orientation.w();
            v[4] = st.position.x(), v[5] = st.position.y(), v[6] = st.position.z();
        };
        for(std::size_t k = 0; k < keyframes.size(); ++k)
        {
            put(keyframes[k]->state, &poses[7 * k]);
            fixed[k] = keyframes[k]->id == 1 ? 1 : 0;
        }
        for(const auto& e : edges)
            anyInfo = anyInfo || !e.sqrtInformation.empty();
        if(anyInfo)
            info.assign(36 * edges.size(), 0.0);
        for(std::size_t e = 0; e < edges.size(); ++e)
        {
            const auto a = kfIndex.find(edges[e].a.get()), b = kfIndex.find(edges[e].b.get());
            if(a == kfIndex.end() || b == kfIndex.end() || (!edges[e].sqrtInformation.empty() && edges[e].sqrtInformation.size() != 36))
                throw std::runtime_error(std::string(who) + ": an edge names a keyframe that is not listed, or its sqrtInformation is not 6 x 6");
            edgeA.push_back(a->second), edgeB.push_back(b->second);
            put(edges[e].measurement, &meas[7 * e]);
            if(anyInfo)
                for(int j = 0; j < 36; ++j)
                    info[36 * e + j] = edges[e].sqrtInformation.empty() ? (j % 7 == 0 ? 1.0 : 0.0) : edges[e].sqrtInformation[j];
        }
        return pg;
    }
    BackendOutput solve(const std::vector<BackendObservation>& observations, int maxIterations, bool global)
    {
        std::vector<std::shared_ptr<Keyframe<slam3d::SensorState>>> keyframes;
        std::vector<std::shared_ptr<Landmark<Vector3>>> landmarks;
        std::map<const void*, int> kfIndex, lmIndex;
        std::vector<std::int32_t> obsKf, obsLm;
        std::vector<double> obsCam;
        for(const auto& o : observations)
        {
            auto k = kfIndex.emplace(o.keyframe.get(), static_cast<int>(keyframes.size()));
            if(k.second)
                keyframes.push_back(o.keyframe);
            auto l = lmIndex.emplace(o.landmark.get(), static_cast<int>(landmarks.size()));
            if(l.second)
                landmarks.push_back(o.landmark);
            obsKf.push_back(k.first->second);
            obsLm.push_back(l.first->second);
            obsCam.insert(obsCam.end(), {o.cameraPoint.x(), o.cameraPoint.y(), o.cameraPoint.z()});
        }
        std::vector<double> poses(7 * keyframes.size()), points(3 * landmarks.size());
        std::vector<std::uint8_t> fixed(keyframes.size()), outlier(observations.size());
        for(std::size_t k = 0; k < keyframes.size(); ++k)
        {
            const auto& st = keyframes[k]->state;
            const double v[7] = {st.orientation.x(), st.orientation.y(), st.orientation.z(), st.orientation.w(),
                                 st.position.x(),    st.position.y(),    st.position.z()};
            std::copy(v, v + 7, poses.begin() + 7 * k);
            fixed[k] = keyframes[k]->id == 1 ? 1 : 0;
        }
        for(std::size_t l = 0; l < landmarks.size(); ++l)
        {
            const Vector3& x = landmarks[l]->state;
            points[3 * l] = x.x(), points[3 * l + 1] = x.y(), points[3 * l + 2] = x.z();
        }
        ctx.ensure(0, 0);
        mslam_hip_ba_summary summary{};
        const auto entry = global ? mslam_hip_bundle_adjust_global : mslam_hip_bundle_adjust;
        const int lrc = mslam_hip_set_ba_loss(ctx.h, lossKind, lossScale);
        if(lrc != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_set_ba_loss", lrc);
        if(const int rs = mslam_hip_set_ba_global_solver(ctx.h, globalSolver); rs != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_set_ba_global_solver", rs);
        if(const int rs = mslam_hip_set_ba_global_pcg(ctx.h, pcgEnable ? 1 : 0, pcgMaxIterations, pcgTolerance); rs != MSLAM_HIP_OK)
            raise(ctx.h, "mslam_hip_set_ba_global_pcg", rs);
        const int rc = entry(ctx.h, poses.data(), fixed.data(), static_cast<int>(keyframes.size()), points.data(),
                             static_cast<int>(landmarks.size()), obsKf.data(), obsLm.data(), obsCam.data(),
                             static_cast<int>(observations.size()), maxIterations, 0.15, outlier.data(), &summary);
        if(rc != MSLAM_HIP_OK && rc != MSLAM_HIP_E_NO_MODEL)
            raise(ctx.h, global ? "mslam_hip_bundle_adjust_global" : "mslam_hip_bundle_adjust", rc);
        if(global)
        {
            mslam_hip_pcg_stats st{};
            if(const int rs = mslam_hip_get_ba_global_pcg_stats(ctx.h, &st); rs != MSLAM_HIP_OK)
                raise(ctx.h, "mslam_hip_get_ba_global_pcg_stats", rs);
            pcgStats = GlobalPcgStats{st.solves, st.iterations, st.longest, st.at_cap, st.breakdowns};
        }
        BackendOutput out;
        out.termination = summary.termination, out.iterations = summary.iterations;
        out.initialCost = summary.initial_cost, out.finalCost = summary.final_cost;
        if(rc == MSLAM_HIP_OK)
        {
            for(std::size_t k = 0; k < keyframes.size(); ++k)
            {
                const double* v = &poses[7 * k];
                keyframes[k]->state.orientation = Quaternion(v[3], v[0], v[1], v[2]);
                keyframes[k]->state.position = Vector3(v[4], v[5], v[6]);
            }
            for(std::size_t l = 0; l < landmarks.size(); ++l)
                landmarks[l]->state = Vector3(points[3 * l], points[3 * l + 1], points[3 * l + 2]);
        }
        for(std::size_t m = 0; m < observations.size(); ++m)
            if(outlier[m])
                out.outlierObservations.push_back(observations[m]);
        out.updatedKeyframes = std::move(keyframes);
        out.updatedLandmarks = std::move(landmarks);
        return out;
    }

    Ctx ctx;
    int poseGraphSolver = MSLAM_HIP_PG_SOLVER_DENSE;
    int globalSolver = MSLAM_HIP_BA_GLOBAL_SOLVER_DENSE;
    bool pcgEnable = false;
    int pcgMaxIterations = MSLAM_HIP_BA_GLOBAL_PCG_MAX_ITERATIONS;
    double pcgTolerance = MSLAM_HIP_BA_GLOBAL_PCG_TOLERANCE;
    GlobalPcgStats pcgStats;
    bool pgPcgEnable = false;
    int pgPcgMaxIterations = MSLAM_HIP_POSE_GRAPH_PCG_MAX_ITERATIONS;
    double pgPcgTolerance = MSLAM_HIP_POSE_GRAPH_PCG_TOLERANCE;
    GlobalPcgStats pgPcgStats;
    int lossKind = MSLAM_HIP_BA_LOSS_NONE;
    double lossScale = 0.0;
    int pgLossKind = MSLAM_HIP_BA_LOSS_NONE;
    double pgLossScale = 0.0;
};

// ---- factories + aliases (what loadFactoryMethod<T>(lib, name) imports) -------------------------------
std::unique_ptr<IOrbFeatureDetector> createHipOrbDetector() { return std::make_unique<HipOrbDetector>(); }
// drop-in for OrbOpenCvDetector (orb_feature.cpp:25,33-65; wired by src/app/slam/rgbd_slam.cpp:74-76).  The reference leaves
// Keypoint::id uninitialised there (orb_feature.cpp:54-61); the running index is used instead.
std::unique_ptr<IOrbFeatureDetector> createHipCvOrbDetector()
{
    return std::make_unique<HipOrbDetector>(MSLAM_HIP_DETECTOR_CV_ORB);
}
std::unique_ptr<IOrbMatcher> createHipOrbMatcher() { return std::make_unique<HipOrbMatcher>(); }
std::unique_ptr<IOrbRelocalizer> createHipOrbRelocalizer() { return std::make_unique<HipOrbRelocalizer>(); }
std::unique_ptr<IOrbLoopDetector> createHipLoopDetector() { return std::make_unique<HipLoopDetector>(); }
std::unique_ptr<ISlam3dPnp> createHipRansacPnp() { return std::make_unique<HipRansacPnp>(); }
std::unique_ptr<ISlam3dPnp> createHipMinMseTracker() { return std::make_unique<HipMinMseTracker>(); }
std::unique_ptr<IRigidAligner> createHipRigidAligner() { return std::make_unique<HipRigidAligner>(); }
std::unique_ptr<IDenseMap> createHipDenseMap() { return std::make_unique<HipDenseMap>(); }
std::unique_ptr<IBackend> createHipBundleAdjustBackend() { return std::make_unique<HipBundleAdjustBackend>(); }

} // namespace mslam

MSLAM_DLL_ALIAS(mslam::createHipOrbDetector, hipOrbDetectorFactory)
MSLAM_DLL_ALIAS(mslam::createHipCvOrbDetector, hipCvOrbDetectorFactory)
MSLAM_DLL_ALIAS(mslam::createHipOrbMatcher, hipOrbMatcherFactory)
MSLAM_DLL_ALIAS(mslam::createHipOrbRelocalizer, hipOrbRelocalizerFactory)
MSLAM_DLL_ALIAS(mslam::createHipLoopDetector, loopDetection) // key used by test/plugin_config.json
MSLAM_DLL_ALIAS(mslam::createHipRansacPnp, hipRansacPnpFactory)
MSLAM_DLL_ALIAS(mslam::createHipMinMseTracker, hipMinMseTrackerFactory)
MSLAM_DLL_ALIAS(mslam::createHipRigidAligner, hipRigidAlignerFactory)
MSLAM_DLL_ALIAS(mslam::createHipDenseMap, hipDenseMapFactory)
MSLAM_DLL_ALIAS(mslam::createHipBundleAdjustBackend, hipBundleAdjustBackendFactory)
