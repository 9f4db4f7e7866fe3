// harness.cpp — a minimal C++ host that uses the plugin exactly as the reference would:
// loadFactoryMethod<T>(library, alias) (plugin_loader.hpp:20-24, as in test/plugin_loader_test.cpp:17-21),
// then the call order of RgbdFeatureFrontend::processSensorData: detect(frame_t) ->
// match(from = keypoints_t, to = keypoints_{t-1}) (rgbd_feature_frontend.cpp:187,237).
//
// usage: mslam_harness <plugin.so> <width> <height> <frame0.bgr> <frame1.bgr>     raw B,G,R frames
//        mslam_harness <plugin.so> --tum <associations.txt>                       a TUM RGB-D sequence, read the way
//                                                                                 the reference's RgbdFileProvider does
//        mslam_harness <plugin.so> --pnp <scene>                                   hipRansacPnpFactory on one scene
//        mslam_harness <plugin.so> --pnp-mse <scene>                               hipMinMseTrackerFactory on the same
//                                                                                 scene format and output line
//        mslam_harness <plugin.so> --bow <vocabulary.dbow3> <width> <height> <frame.bgr>...
//                                    the BoW boundary: relocalizer + loop detector factories (one shared database),
//                                    fed in the frontend's order: detect -> addKeyframe (rgbd_feature_frontend.cpp:176)
//                                    -> detectLoop (:202); then relocalize / removeKeyframe / relocalize
//        mslam_harness <plugin.so> --reloc <vocabulary.dbow3> <scene>
//                                    the verified relocalisation: addKeyframe + addKeyframeLandmarks per keyframe of the scene,
//                                    relocalizePose(query), then the query fed as a keyframe and detectLoopVerified,
//                                    then removeKeyframe(winner) and relocalizePose again
//        mslam_harness <plugin.so> --track <vocabulary.dbow3> <scene>
//                                    the frontend's loop over a recorded sequence (processSensorData, :185-222) on
//                                    IKeyframeTracker: initFirstKeyframe, then per frame trackKeyframe against the reference
//                                    keyframe with the previous pose as the guess; the vote's winner becomes the reference,
//                                    an inserted keyframe too; relocalizePose when tracking fails.  One line per frame.
//        mslam_harness <plugin.so> --track <vocabulary.dbow3> <scene> --local-map <depth>
//                                    the same loop against the local map, as the reference tracks (:256-277): ILocalMapTracker's
//                                    buildLocalMap over the reference keyframe's covisibility neighbourhood (rebuilt when the
//                                    reference changes or a keyframe is added), trackLocalMap, covisibleLandmarks for the edges
//        mslam_harness <plugin.so> --track <vocabulary.dbow3> <scene> [--local-map <depth>] --guided <radius>
//                                    either loop with IKeyframeTracker::setGuidedMatch(radius): every tracking call matches each
//                                    landmark within <radius> px of its projection under the previous pose
//        mslam_harness <plugin.so> --track <vocabulary.dbow3> <scene> --local-map <depth> --distinct
//                                    the local-map loop with IDistinctiveLocalMap::setUnionDescriptor(1): every landmark of the
//                                    local map carries its most distinctive descriptor instead of the most recent one
//        mslam_harness <plugin.so> --track <vocabulary.dbow3> <scene> [...] --align <max_distance>
//                                    any of the loops above with IAlignedKeyframeTracker::setTrackPose(1, max_distance): the
//                                    tracked pose comes from RANSAC rigid alignment of (landmark, camera-frame point)
//        mslam_harness <plugin.so> --align <scene>
//                                    hipRigidAlignerFactory on one scene (text: `n iterations max_distance seed`, then n lines
//                                    of source xyz and target xyz): prints R, t and the inlier count, or `align none`
//        mslam_harness <plugin.so> --ba <scene>
//        mslam_harness <plugin.so> --ba-global <scene>
//                                    hipBundleAdjustBackendFactory on one bundle-adjustment scene: the summary, then every
//                                    keyframe's and landmark's state and the outlier observations
//        mslam_harness <plugin.so> --ba <scene> --loss huber:<a> | cauchy:<a>
//        mslam_harness <plugin.so> --ba-global <scene> --loss huber:<a> | cauchy:<a>
//                                    the same with IRobustBackend::setLoss(kind, a) first (a in metres, finite and > 0): the
//                                    costs of the summary are then 1/2 sum rho
//        mslam_harness <plugin.so> --ba-global <scene> --sparse
//                                    the global solve with ISparseGlobalBackend::setGlobalSolver(1) first: the reduced camera
//                                    system on its block envelope, up to 16384 keyframes
//        mslam_harness <plugin.so> --ba-global <scene> --pcg [<max_iterations>:<tolerance>]
//                                    the global solve with IIterativeGlobalBackend::setGlobalPcg(true, ...) first (500:1e-6
//                                    without a value): the reduced camera system by preconditioned conjugate gradients; one more
//                                    line, "pcg solves S iterations I longest L at_cap C breakdowns B", follows the summary
//        mslam_harness <plugin.so> --pose-graph <scene>
//                                    ILoopClosingBackend::closeLoop of the same factory's object on one pose-graph scene: the
//                                    summary, then every keyframe's state
//        mslam_harness <plugin.so> --pose-graph <scene> --sparse | --solver <kind>
//                                    the same with ISparsePoseGraphBackend::setPoseGraphSolver(kind) first (--sparse: kind 1,
//                                    the block-envelope factor, up to 16384 keyframes); a kind the backend refuses is its
//                                    std::invalid_argument: "error: ..." and exit code 1; a kind that is no integer is a
//                                    usage error, exit code 2
//        mslam_harness <plugin.so> --pose-graph <scene> [--sparse] --loss huber:<a> | cauchy:<a>
//                                    the same with IRobustPoseGraphBackend::setPoseGraphLoss(kind, a) first (a in the unit of the
//                                    weighted residual, finite and > 0), after --sparse when both are given: the costs of the
//                                    summary are then 1/2 sum rho
//        mslam_harness <plugin.so> --pose-graph <scene> --pcg [<max_iterations>:<tolerance>]
//                                    the same with IIterativePoseGraphBackend::setPoseGraphPcg(true, ...) first (500:1e-6 without
//                                    a value): the normal equations by preconditioned conjugate gradients, up to 16384
//                                    keyframes; one more line, "pcg solves S iterations I longest L at_cap C breakdowns B",
//                                    follows the summary
//        mslam_harness <plugin.so> --pose-graph <scene> --covariance
//                                    no solve: IPoseGraphCovariance::poseGraphCovariance of the same object at the scene's
//                                    states, for every keyframe that is not constant and has an edge: "covariance blocks N",
//                                    then per keyframe "cov <index>" and its 36 entries (row-major, %.17g)
//        mslam_harness <plugin.so> --pnp-mse <scene> --loss huber:<a> | cauchy:<a>
//                                    hipMinMseTrackerFactory with IRobustPnp::setLoss(kind, a) first (a in pixels)
//        mslam_harness <plugin.so> --fuse <scene>
//                                    ILandmarkFuser::fuseLandmarks of the relocalizer adapter (the vocabulary it loads comes
//                                    from MSLAM_ORB_VOCABULARY or ./orbvoc.dbow3) on the scene's first two entries, keep then
//                                    drop: "fuse pairs N rewritten M", one "pair" line per pair, then every entry's landmark
//                                    ids after the replacement
//        mslam_harness <plugin.so> --fuse-multi <scene>
//                                    IMultiLandmarkFuser::fuseLandmarksMulti of the relocalizer adapter on the scene's first
//                                    entry (keep) and its targets, each under its own pose: "fuse-multi pairs N rewritten M",
//                                    one "pair <target> <keep pos> <drop pos> <keep id> <drop id> <distance>" line per pair,
//                                    then every entry's landmark ids after the replacement
//        mslam_harness <plugin.so> --prune <scene>
//                                    IObservationRemover::removeObservations of the relocalizer adapter on the scene's entries
//                                    and rows: "prune removed N", one "row <p> <count>" line per row, then per entry
//                                    "entry <id> n <count> <ids...>" after the removal
//        mslam_harness <plugin.so> --cull <scene>
//                                    IKeyframeCuller::cullKeyframes of the relocalizer adapter on the scene's entries, listed
//                                    keyframes and candidates: "cull culled N", one "cand <p> <id> <culled> <landmarks>
//                                    <redundant>" line per candidate, then "remaining <ids...>": the entries the adapter
//                                    still holds
//        mslam_harness <plugin.so> --cull-landmarks <scene>
//                                    ILandmarkCuller::cullLandmarks of the relocalizer adapter on the scene's entries, listed
//                                    keyframes and candidates: "lmcull found N removed M", one "lm <id> <observers>" line per
//                                    culled landmark id, then "entry <id> <count>" for every entry in scene order
//        mslam_harness <plugin.so> --dense <scene> --icp <frames> [--dump <path>]
//                                    the same, then IDenseAligner (a dynamic_cast of the dense map) aligns every frame of the
//                                    frames file (tests/tsdf_icp_ref.py::write_frames) to the volume: "icp frame F status S
//                                    iterations N pairs C"; --dump: tests/tsdf_icp_ref.py::read_dump
//        mslam_harness <plugin.so> --dense <scene> --raycast <views> [--dump <path>]
//                                    the same, then IDenseMapRenderer (a dynamic_cast of the dense map) renders every view of
//                                    the views file (tests/tsdf_raycast_ref.py::write_views): "raycast view V size W x H hits
//                                    N" per view; the dump holds depth, xyz and normal per view instead of the volume
//        mslam_harness <plugin.so> --dense <scene> [--dump <path>]
//                                    hipDenseMapFactory on one scene file (tests/tsdf_ref.py::write_scene: the volume's
//                                    parameters, the frames with their poses, an optional list of pose updates — one updatePoses
//                                    call — and an optional list of removals): "dense frames F moved M points N sumS S sumW W",
//                                    F the frames retained at the end, S and W the sums over the volume as int64.  --dump writes
//                                    S, W (int32 [nz][ny][nx] each), then the points and the normals (f32, 3 per point), raw
// prints one line per frame/match with an FNV-1a checksum the parity test compares with the oracle's.
#include "mslam_interfaces.hpp"
#include "plugin_loader.hpp"
#include "tum_io.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <map>
#include <set>

static std::uint32_t fnv(const void* p, std::size_t n, std::uint32_t h = 0x811C9DC5u)
{
    const auto* b = static_cast<const unsigned char*>(p);
    for(std::size_t i = 0; i < n; ++i)
        h = (h ^ b[i]) * 0x01000193u;
    return h;
}

// --pcg's value: <whole number>:<number>, all of it: "500", "500:" and "5x:0.1" are not one
static bool parsePcg(const char* text, int& maxIterations, double& tolerance)
{
    char *end = nullptr, *end2 = nullptr;
    const long v = std::strtol(text, &end, 10);
    const double t = end != text && *end == ':' ? std::strtod(end + 1, &end2) : 0.0;
    if(end == text || *end != ':' || end2 == end + 1 || *end2 != '\0' || v < -1000000000 || v > 1000000000)
        return false;
    maxIterations = static_cast<int>(v), tolerance = t;
    return true;
}

int main(int argc, char** argv)
{
    if(argc < 2)
    {
        std::fprintf(stderr, "usage: %s <plugin> [<width> <height> <frame0.bgr> <frame1.bgr>]\n", argv[0]);
        return 2;
    }
    try
    {
        // MSLAM_HARNESS_DETECTOR=cvorb: the factory of the OrbOpenCvDetector drop-in instead of the in-tree extractor's
        const char* det = std::getenv("MSLAM_HARNESS_DETECTOR");
        const bool cvorb = det && std::strcmp(det, "cvorb") == 0;
        auto makeDetector = mslam::loadFactoryMethod<mslam::IOrbFeatureDetector>(
            argv[1], cvorb ? "hipCvOrbDetectorFactory" : "hipOrbDetectorFactory");
        auto makeMatcher = mslam::loadFactoryMethod<mslam::IOrbMatcher>(argv[1], "hipOrbMatcherFactory");
        if(!makeDetector || !makeMatcher)
            return 3;
        std::unique_ptr<mslam::IOrbFeatureDetector> detector = makeDetector();
        std::unique_ptr<mslam::IOrbMatcher> matcher = makeMatcher();
        std::printf("loaded %s\n", detector && matcher ? "ok" : "null");
        const bool pnp_mse_loss = argc == 6 && std::strcmp(argv[2], "--pnp-mse") == 0 && std::strcmp(argv[4], "--loss") == 0;
        const bool pnp_mse = (argc == 4 && std::strcmp(argv[2], "--pnp-mse") == 0) || pnp_mse_loss;
        if((argc == 4 && std::strcmp(argv[2], "--pnp") == 0) || pnp_mse)
        {
            int lossKind = 0;
            double lossScale = 0.0;
            if(pnp_mse_loss && !mslam::parseLoss(argv[5], lossKind, lossScale))
            {
                std::fprintf(stderr, "--loss takes huber:<a> or cauchy:<a> with a finite a > 0, not %s\n", argv[5]);
                return 2;
            }
            // scene file: u32 n, then n x (3 f64 landmark, 2 f64 image point), then the initial sensor pose (3 f64 position,
            // 4 f64 quaternion w x y z) and fx fy cx cy
            std::ifstream in(argv[3], std::ios::binary);
            std::uint32_t n = 0;
            in.read(reinterpret_cast<char*>(&n), 4);
            std::vector<std::shared_ptr<mslam::Landmark<mslam::Vector3>>> landmarks;
            std::vector<mslam::Vector2> points;
            for(std::uint32_t i = 0; i < n; ++i)
            {
                double v[5];
                in.read(reinterpret_cast<char*>(v), sizeof(v));
                auto lm = std::make_shared<mslam::Landmark<mslam::Vector3>>();
                lm->id = i;
                lm->state = mslam::Vector3(v[0], v[1], v[2]);
                landmarks.push_back(lm);
                points.emplace_back(v[3], v[4]);
            }
            double pose[7], cam[4];
            in.read(reinterpret_cast<char*>(pose), sizeof(pose));
            if(!in.read(reinterpret_cast<char*>(cam), sizeof(cam)))
            {
                std::fprintf(stderr, "cannot read %s\n", argv[3]);
                return 5;
            }
            auto makePnp = mslam::loadFactoryMethod<mslam::ISlam3dPnp>(argv[1], pnp_mse ? "hipMinMseTrackerFactory"
                                                                                          : "hipRansacPnpFactory");
            std::unique_ptr<mslam::ISlam3dPnp> pnp = makePnp();
            if(pnp_mse_loss)
            {
                auto* robust = dynamic_cast<mslam::IRobustPnp*>(pnp.get());
                if(!robust)
                {
                    std::fprintf(stderr, "the plugin does not offer setLoss on its min-MSE tracker\n");
                    return 6;
                }
                robust->setLoss(lossKind, lossScale);
            }
            mslam::CameraParameters cp;
            cp.focal = mslam::Vector2(cam[0], cam[1]);
            cp.principalPoint = mslam::Vector2(cam[2], cam[3]);
            cp.factor = 1.0f / 5000.0f;
            pnp->setCameraParameters(cp);
            mslam::slam3d::SensorState initial;
            initial.position = mslam::Vector3(pose[0], pose[1], pose[2]);
            initial.orientation = mslam::Quaternion(pose[3], pose[4], pose[5], pose[6]);
            const auto result = pnp->solvePnp(landmarks, points, initial);
            if(!result)
            {
                std::printf("pnp none\n");
                return 0;
            }
            std::size_t inl = 0;
            for(bool b : result->inliers)
                inl += b ? 1 : 0;
            std::printf("pnp position %.17g %.17g %.17g orientation %.17g %.17g %.17g %.17g inliers %zu\n",
                        result->pose.position.x(), result->pose.position.y(), result->pose.position.z(),
                        result->pose.orientation.w(), result->pose.orientation.x(), result->pose.orientation.y(),
                        result->pose.orientation.z(), inl);
            return 0;
        }
        if(argc == 4 && std::strcmp(argv[2], "--align") == 0)
        {
            std::ifstream in(argv[3]);
            long long n = 0, iterations = 0;
            unsigned long long seed = 0;
            double maxDistance = 0;
            in >> n >> iterations >> maxDistance >> seed;
            std::vector<mslam::Vector3> source, target;
            for(long long i = 0; in && i < n; ++i)
            {
                std::string tok[6];
                double v[6];
                for(int k = 0; k < 6; ++k)
                {
                    in >> tok[k];
                    v[k] = std::strtod(tok[k].c_str(), nullptr); // (reads "nan" too, which operator>> does not)
                }
                source.emplace_back(v[0], v[1], v[2]);
                target.emplace_back(v[3], v[4], v[5]);
            }
            if(!in || n < 0)
            {
                std::fprintf(stderr, "cannot read %s\n", argv[3]);
                return 5;
            }
            auto makeAligner = mslam::loadFactoryMethod<mslam::IRigidAligner>(argv[1], "hipRigidAlignerFactory");
            if(!makeAligner)
                return 3;
            std::unique_ptr<mslam::IRigidAligner> aligner = makeAligner();
            const auto result = aligner->align(source, target, maxDistance, static_cast<int>(iterations), seed);
            if(!result)
            {
                std::printf("align none\n");
                return 0;
            }
            std::size_t inl = 0;
            for(bool b : result->inliers)
                inl += b ? 1 : 0;
            std::printf("align R");
            for(double r : result->R)
                std::printf(" %.17g", r);
            std::printf(" t %.17g %.17g %.17g inliers %zu mask ", result->t[0], result->t[1], result->t[2], inl);
            for(bool b : result->inliers)
                std::putchar(b ? '1' : '0');
            std::printf("\n");
            return 0;
        }
        const bool denseRaycast = (argc == 6 || (argc == 8 && std::strcmp(argv[6], "--dump") == 0)) && std::strcmp(argv[4], "--raycast") == 0;
        const bool denseIcp = (argc == 6 || (argc == 8 && std::strcmp(argv[6], "--dump") == 0)) && std::strcmp(argv[4], "--icp") == 0;
        if((argc == 4 || (argc == 6 && std::strcmp(argv[4], "--dump") == 0) || denseRaycast || denseIcp) && std::strcmp(argv[2], "--dense") == 0)
        {
            // little endian: magic[8]; mslam_hip_tsdf_params' layout (4 i32, 6 f64, 2 i32, f32, i32, 4 f64); i32 F, U, M, min_weight;
            // F x {i32 id, 0; f64 R[9], t[3]; u16 depth[height][width]}; U x {i32 id, 0; f64 R[9], t[3]}; M x i32 id
            std::ifstream in(argv[3], std::ios::binary);
            char magic[8] = {0};
            std::int32_t head[4] = {0}, cam[2] = {0}, pad = 0, counts[4] = {0};
            double vol[6] = {0}, intr[4] = {0};
            float factor = 0;
            in.read(magic, 8);
            in.read(reinterpret_cast<char*>(head), sizeof(head));
            in.read(reinterpret_cast<char*>(vol), sizeof(vol));
            in.read(reinterpret_cast<char*>(cam), sizeof(cam));
            in.read(reinterpret_cast<char*>(&factor), 4);
            in.read(reinterpret_cast<char*>(&pad), 4);
            in.read(reinterpret_cast<char*>(intr), sizeof(intr));
            in.read(reinterpret_cast<char*>(counts), sizeof(counts));
            if(!in || std::memcmp(magic, "MSTSDF1", 8) != 0 || counts[0] < 0 || counts[1] < 0 || counts[2] < 0 || cam[0] < 1 || cam[1] < 1 ||
               static_cast<long long>(cam[0]) * cam[1] > (1 << 26))
            {
                std::fprintf(stderr, "cannot read %s\n", argv[3]);
                return 5;
            }
            // --raycast <views> (tests/tsdf_raycast_ref.py::write_views), little endian: magic[8]; i32 V, 0; V x
            // {mslam_hip_tsdf_raycast_params' layout (2 i32, 7 f64, 2 i32); f64 R[9], t[3]}
            struct View
            {
                mslam::DenseRenderParams params;
                mslam::DensePose pose;
            };
            std::vector<View> views;
            if(denseRaycast)
            {
                std::ifstream vin(argv[5], std::ios::binary);
                char vmagic[8] = {0};
                std::int32_t nViews[2] = {0, 0};
                vin.read(vmagic, 8);
                vin.read(reinterpret_cast<char*>(nViews), sizeof(nViews));
                bool good = vin && std::memcmp(vmagic, "MSTSDFV1", 8) == 0 && nViews[0] >= 0 && nViews[0] <= (1 << 16);
                for(std::int32_t v = 0; good && v < nViews[0]; ++v)
                {
                    std::int32_t size[2] = {0, 0}, march[2] = {0, 0};
                    double real[7] = {0};
                    View view;
                    vin.read(reinterpret_cast<char*>(size), sizeof(size));
                    vin.read(reinterpret_cast<char*>(real), sizeof(real));
                    vin.read(reinterpret_cast<char*>(march), sizeof(march));
                    vin.read(reinterpret_cast<char*>(view.pose.R), sizeof(view.pose.R));
                    vin.read(reinterpret_cast<char*>(view.pose.t), sizeof(view.pose.t));
                    good = static_cast<bool>(vin) && size[0] >= 1 && size[1] >= 1 && static_cast<long long>(size[0]) * size[1] <= (1 << 26);
                    view.params.width = size[0], view.params.height = size[1];
                    view.params.camera.focal = mslam::Vector2(real[0], real[1]);
                    view.params.camera.principalPoint = mslam::Vector2(real[2], real[3]);
                    view.params.zNear = real[4], view.params.zFar = real[5], view.params.step = real[6];
                    view.params.coarse = march[0], view.params.minWeight = march[1];
                    views.push_back(view);
                }
                if(!good)
                {
                    std::fprintf(stderr, "cannot read %s\n", argv[5]);
                    return 5;
                }
            }
            // --icp <frames> (tests/tsdf_icp_ref.py::write_frames), little endian: magic[8]; i32 F, 0; F x {the render as in a views
            // file without its pose (2 i32, 7 f64, 2 i32); i32 n_levels, min_pairs, stride[4], iterations[4]; f64 dist_max, cos_min,
            // rot_tol, trans_tol; f64 R0[9], t0[3]; u16 depth[height][width] of the volume's camera}
            struct IcpFrame
            {
                mslam::DenseRenderParams render;
                mslam::DenseAlignParams params;
                mslam::DensePose guess;
                std::vector<std::uint16_t> depth;
            };
            std::vector<IcpFrame> icpFrames;
            if(denseIcp)
            {
                std::ifstream fin(argv[5], std::ios::binary);
                char fmagic[8] = {0};
                std::int32_t nFrames[2] = {0, 0};
                fin.read(fmagic, 8);
                fin.read(reinterpret_cast<char*>(nFrames), sizeof(nFrames));
                bool good = fin && std::memcmp(fmagic, "MSTSDFI1", 8) == 0 && nFrames[0] >= 0 && nFrames[0] <= (1 << 16);
                for(std::int32_t f = 0; good && f < nFrames[0]; ++f)
                {
                    std::int32_t size[2] = {0, 0}, march[2] = {0, 0}, ints[10] = {0};
                    double real[7] = {0}, gates[4] = {0};
                    IcpFrame fr;
                    fin.read(reinterpret_cast<char*>(size), sizeof(size));
                    fin.read(reinterpret_cast<char*>(real), sizeof(real));
                    fin.read(reinterpret_cast<char*>(march), sizeof(march));
                    fin.read(reinterpret_cast<char*>(ints), sizeof(ints));
                    fin.read(reinterpret_cast<char*>(gates), sizeof(gates));
                    fin.read(reinterpret_cast<char*>(fr.guess.R), sizeof(fr.guess.R));
                    fin.read(reinterpret_cast<char*>(fr.guess.t), sizeof(fr.guess.t));
                    fr.depth.resize(static_cast<std::size_t>(cam[0]) * cam[1]);
                    fin.read(reinterpret_cast<char*>(fr.depth.data()), static_cast<std::streamsize>(fr.depth.size() * 2));
                    good = static_cast<bool>(fin) && ints[0] >= 0 && ints[0] <= 4;
                    fr.render.width = size[0], fr.render.height = size[1];
                    fr.render.camera.focal = mslam::Vector2(real[0], real[1]);
                    fr.render.camera.principalPoint = mslam::Vector2(real[2], real[3]);
                    fr.render.zNear = real[4], fr.render.zFar = real[5], fr.render.step = real[6];
                    fr.render.coarse = march[0], fr.render.minWeight = march[1];
                    fr.params.levels.clear();
                    for(std::int32_t l = 0; good && l < ints[0]; ++l)
                        fr.params.levels.emplace_back(ints[2 + l], ints[6 + l]);
                    fr.params.minPairs = ints[1];
                    fr.params.distMax = gates[0], fr.params.cosMin = gates[1], fr.params.rotTol = gates[2], fr.params.transTol = gates[3];
                    icpFrames.push_back(std::move(fr));
                }
                if(!good)
                {
                    std::fprintf(stderr, "cannot read %s\n", argv[5]);
                    return 5;
                }
            }
            mslam::DenseMapParams dp;
            dp.nx = head[0], dp.ny = head[1], dp.nz = head[2], dp.maxFrames = head[3];
            dp.voxel = vol[0], dp.origin[0] = vol[1], dp.origin[1] = vol[2], dp.origin[2] = vol[3], dp.trunc = vol[4], dp.maxDepth = vol[5];
            dp.width = cam[0], dp.height = cam[1];
            dp.camera.factor = factor;
            dp.camera.focal = mslam::Vector2(intr[0], intr[1]);
            dp.camera.principalPoint = mslam::Vector2(intr[2], intr[3]);
            auto makeDense = mslam::loadFactoryMethod<mslam::IDenseMap>(argv[1], "hipDenseMapFactory");
            if(!makeDense)
                return 3;
            std::unique_ptr<mslam::IDenseMap> dense = makeDense();
            dense->create(dp);
            const auto readPose = [&in](std::int32_t& id, mslam::DensePose& pose) {
                std::int32_t idPad[2] = {0, 0};
                in.read(reinterpret_cast<char*>(idPad), sizeof(idPad));
                in.read(reinterpret_cast<char*>(pose.R), sizeof(pose.R));
                in.read(reinterpret_cast<char*>(pose.t), sizeof(pose.t));
                id = idPad[0];
            };
            std::vector<std::uint16_t> depth(static_cast<std::size_t>(cam[0]) * cam[1]);
            for(std::int32_t f = 0; f < counts[0]; ++f)
            {
                std::int32_t id = 0;
                mslam::DensePose pose;
                readPose(id, pose);
                if(!in.read(reinterpret_cast<char*>(depth.data()), static_cast<std::streamsize>(depth.size() * 2)))
                {
                    std::fprintf(stderr, "cannot read %s\n", argv[3]);
                    return 5;
                }
                dense->addFrame(id, depth, pose);
            }
            std::vector<int> ids;
            std::vector<mslam::DensePose> poses;
            for(std::int32_t u = 0; u < counts[1]; ++u)
            {
                std::int32_t id = 0;
                mslam::DensePose pose;
                readPose(id, pose);
                ids.push_back(id);
                poses.push_back(pose);
            }
            std::vector<std::int32_t> gone(static_cast<std::size_t>(counts[2]));
            in.read(reinterpret_cast<char*>(gone.data()), static_cast<std::streamsize>(gone.size() * 4));
            if(!in)
            {
                std::fprintf(stderr, "cannot read %s\n", argv[3]);
                return 5;
            }
            const int moved = ids.empty() ? 0 : dense->updatePoses(ids, poses);
            for(std::int32_t id : gone)
                dense->removeFrame(id);
            std::vector<std::int32_t> S, W;
            dense->read(S, W);
            const mslam::DenseSurface surface = dense->extract(counts[3]);
            long long sumS = 0, sumW = 0;
            for(std::size_t i = 0; i < S.size(); ++i)
                sumS += S[i], sumW += W[i];
            std::printf("dense frames %d moved %d points %zu sumS %lld sumW %lld\n", dense->frames(), moved, surface.points.size() / 3,
                        sumS, sumW);
            if(denseRaycast)
            {
                // the dump: magic[8]; i32 V, 0; V x {i32 width, height, hits, 0; f32 depth[h][w], xyz[h][w][3], normal[h][w][3]}
                auto* renderer = dynamic_cast<mslam::IDenseMapRenderer*>(dense.get());
                if(!renderer)
                {
                    std::fprintf(stderr, "the dense map offers no IDenseMapRenderer\n");
                    return 3;
                }
                std::ofstream out;
                if(argc == 8)
                {
                    out.open(argv[7], std::ios::binary);
                    const std::int32_t n[2] = {static_cast<std::int32_t>(views.size()), 0};
                    out.write("MSTSDFR1", 8);
                    out.write(reinterpret_cast<const char*>(n), sizeof(n));
                }
                for(std::size_t v = 0; v < views.size(); ++v)
                {
                    const mslam::DenseRender r = renderer->render(views[v].params, views[v].pose);
                    std::printf("raycast view %zu size %d x %d hits %d\n", v, views[v].params.width, views[v].params.height, r.hits);
                    if(argc == 8)
                    {
                        const std::int32_t h[4] = {views[v].params.width, views[v].params.height, r.hits, 0};
                        out.write(reinterpret_cast<const char*>(h), sizeof(h));
                        out.write(reinterpret_cast<const char*>(r.depth.data()), static_cast<std::streamsize>(r.depth.size() * 4));
                        out.write(reinterpret_cast<const char*>(r.points.data()), static_cast<std::streamsize>(r.points.size() * 4));
                        out.write(reinterpret_cast<const char*>(r.normals.data()), static_cast<std::streamsize>(r.normals.size() * 4));
                    }
                }
                if(argc == 8 && !out)
                {
                    std::fprintf(stderr, "cannot write %s\n", argv[7]);
                    return 5;
                }
                return 0;
            }
            if(denseIcp)
            {
                // the dump: magic[8]; i32 F, 0; F x {f64 R[9], t[3]; i32 status, iterations, count, level; f64 cost, pivots[6];
                // i32 rows, 0; rows x {i32 level, count; f64 cost, rot2, trans2}}
                auto* aligner = dynamic_cast<mslam::IDenseAligner*>(dense.get());
                if(!aligner)
                {
                    std::fprintf(stderr, "the dense map offers no IDenseAligner\n");
                    return 3;
                }
                std::ofstream out;
                if(argc == 8)
                {
                    out.open(argv[7], std::ios::binary);
                    const std::int32_t n[2] = {static_cast<std::int32_t>(icpFrames.size()), 0};
                    out.write("MSTSDFA1", 8);
                    out.write(reinterpret_cast<const char*>(n), sizeof(n));
                }
                for(std::size_t f = 0; f < icpFrames.size(); ++f)
                {
                    const mslam::DenseAlignResult r = aligner->align(icpFrames[f].depth, icpFrames[f].guess, icpFrames[f].params, icpFrames[f].render);
                    std::printf("icp frame %zu status %d iterations %d pairs %d\n", f, r.status, r.iterations, r.count);
                    if(argc == 8)
                    {
                        const std::int32_t h[4] = {r.status, r.iterations, r.count, r.level};
                        const std::int32_t rows[2] = {static_cast<std::int32_t>(r.record.size()), 0};
                        out.write(reinterpret_cast<const char*>(r.pose.R), sizeof(r.pose.R));
                        out.write(reinterpret_cast<const char*>(r.pose.t), sizeof(r.pose.t));
                        out.write(reinterpret_cast<const char*>(h), sizeof(h));
                        out.write(reinterpret_cast<const char*>(&r.cost), 8);
                        out.write(reinterpret_cast<const char*>(r.pivots), sizeof(r.pivots));
                        out.write(reinterpret_cast<const char*>(rows), sizeof(rows));
                        static_assert(sizeof(mslam::DenseAlignRecord) == 32, "the dump's row");
                        out.write(reinterpret_cast<const char*>(r.record.data()), static_cast<std::streamsize>(r.record.size() * 32));
                    }
                }
                if(argc == 8 && !out)
                {
                    std::fprintf(stderr, "cannot write %s\n", argv[7]);
                    return 5;
                }
                return 0;
            }
            if(argc == 6)
            {
                std::ofstream out(argv[5], std::ios::binary);
                out.write(reinterpret_cast<const char*>(S.data()), static_cast<std::streamsize>(S.size() * 4));
                out.write(reinterpret_cast<const char*>(W.data()), static_cast<std::streamsize>(W.size() * 4));
                out.write(reinterpret_cast<const char*>(surface.points.data()), static_cast<std::streamsize>(surface.points.size() * 4));
                out.write(reinterpret_cast<const char*>(surface.normals.data()), static_cast<std::streamsize>(surface.normals.size() * 4));
                if(!out)
                {
                    std::fprintf(stderr, "cannot write %s\n", argv[5]);
                    return 5;
                }
            }
            return 0;
        }
        const bool baPcg = (argc == 5 || argc == 6) && std::strcmp(argv[4], "--pcg") == 0 && std::strcmp(argv[2], "--ba-global") == 0;
        if((argc == 4 || (argc == 6 && std::strcmp(argv[4], "--loss") == 0) || baPcg ||
            (argc == 5 && std::strcmp(argv[4], "--sparse") == 0 && std::strcmp(argv[2], "--ba-global") == 0)) &&
           (std::strcmp(argv[2], "--ba") == 0 || std::strcmp(argv[2], "--ba-global") == 0))
        {
            const bool sparseSolver = argc == 5 && !baPcg;
            int pcgIterations = 500;
            double pcgTolerance = 1e-6;
            if(baPcg && argc == 6 && !parsePcg(argv[5], pcgIterations, pcgTolerance))
            {
                std::fprintf(stderr, "--pcg takes <max_iterations>:<tolerance>, not %s\n", argv[5]);
                return 2;
            }
            int lossKind = 0;
            double lossScale = 0.0;
            if(argc == 6 && !baPcg && !mslam::parseLoss(argv[5], lossKind, lossScale))
            {
                std::fprintf(stderr, "--loss takes huber:<a> or cauchy:<a> with a finite a > 0, not %s\n", argv[5]);
                return 2;
            }
            const bool global = std::strcmp(argv[2], "--ba-global") == 0; // IGlobalBackend::globalBundleAdjustment: up to 1024 keyframes (--sparse: 16384)
            // scene file: "MSBA", i32 version (1), K, L, M, max_iterations; K x i32 keyframe id; K x 7 f64 state (qx qy qz qw
            // px py pz); L x 3 f64; M x i32 keyframe index; M x i32 landmark index; M x 3 f64 camera-frame point
            std::ifstream in(argv[3], std::ios::binary);
            char magic[4] = {0, 0, 0, 0};
            std::int32_t head[5] = {0, 0, 0, 0, 0};
            in.read(magic, 4);
            in.read(reinterpret_cast<char*>(head), sizeof(head));
            if(!in || std::memcmp(magic, "MSBA", 4) != 0 || head[0] != 1 || head[1] < 0 || head[2] < 0 || head[3] < 0)
            {
                std::fprintf(stderr, "%s is not a bundle-adjustment scene\n", argv[3]);
                return 5;
            }
            const std::size_t K = head[1], L = head[2], M = head[3];
            std::vector<std::int32_t> ids(K), okf(M), olm(M);
            std::vector<double> poses(7 * K), points(3 * L), cam(3 * M);
            in.read(reinterpret_cast<char*>(ids.data()), K * 4);
            in.read(reinterpret_cast<char*>(poses.data()), K * 56);
            in.read(reinterpret_cast<char*>(points.data()), L * 24);
            in.read(reinterpret_cast<char*>(okf.data()), M * 4);
            in.read(reinterpret_cast<char*>(olm.data()), M * 4);
            in.read(reinterpret_cast<char*>(cam.data()), M * 24);
            if(!in)
            {
                std::fprintf(stderr, "cannot read %s\n", argv[3]);
                return 5;
            }
            std::vector<std::shared_ptr<mslam::Keyframe<mslam::slam3d::SensorState>>> keyframes;
            std::vector<std::shared_ptr<mslam::Landmark<mslam::Vector3>>> landmarks;
            for(std::size_t k = 0; k < K; ++k)
            {
                auto kf = std::make_shared<mslam::Keyframe<mslam::slam3d::SensorState>>();
                const double* v = &poses[7 * k];
                kf->id = static_cast<mslam::Id>(ids[k]);
                kf->state.orientation = mslam::Quaternion(v[3], v[0], v[1], v[2]);
                kf->state.position = mslam::Vector3(v[4], v[5], v[6]);
                keyframes.push_back(kf);
            }
            for(std::size_t l = 0; l < L; ++l)
            {
                auto lm = std::make_shared<mslam::Landmark<mslam::Vector3>>();
                lm->id = l;
                lm->state = mslam::Vector3(points[3 * l], points[3 * l + 1], points[3 * l + 2]);
                landmarks.push_back(lm);
            }
            std::vector<mslam::BackendObservation> observations;
            for(std::size_t m = 0; m < M; ++m)
            {
                if(okf[m] < 0 || static_cast<std::size_t>(okf[m]) >= K || olm[m] < 0 || static_cast<std::size_t>(olm[m]) >= L)
                {
                    std::fprintf(stderr, "observation %zu of %s is out of range\n", m, argv[3]);
                    return 5;
                }
                observations.push_back({keyframes[okf[m]], landmarks[olm[m]], mslam::Vector3(cam[3 * m], cam[3 * m + 1], cam[3 * m + 2])});
            }
            auto makeBackend = mslam::loadFactoryMethod<mslam::IBackend>(argv[1], "hipBundleAdjustBackendFactory");
            if(!makeBackend)
                return 3;
            std::unique_ptr<mslam::IBackend> backend = makeBackend();
            auto* globalBackend = dynamic_cast<mslam::IGlobalBackend*>(backend.get());
            if(global && !globalBackend)
            {
                std::fprintf(stderr, "the plugin does not offer the global bundle adjustment\n");
                return 6;
            }
            if(lossKind != 0)
            {
                auto* robust = dynamic_cast<mslam::IRobustBackend*>(backend.get());
                if(!robust)
                {
                    std::fprintf(stderr, "the plugin does not offer a loss function\n");
                    return 6;
                }
                robust->setLoss(lossKind, lossScale);
            }
            if(sparseSolver)
            {
                auto* sparseBackend = dynamic_cast<mslam::ISparseGlobalBackend*>(backend.get());
                if(!sparseBackend)
                {
                    std::fprintf(stderr, "the plugin does not offer setGlobalSolver\n");
                    return 6;
                }
                sparseBackend->setGlobalSolver(1);
            }
            auto* pcgBackend = baPcg ? dynamic_cast<mslam::IIterativeGlobalBackend*>(backend.get()) : nullptr;
            if(baPcg)
            {
                if(!pcgBackend)
                {
                    std::fprintf(stderr, "the plugin does not offer setGlobalPcg\n");
                    return 6;
                }
                pcgBackend->setGlobalPcg(true, pcgIterations, pcgTolerance); // bad values: its std::invalid_argument, exit code 1
            }
            const mslam::BackendOutput out =
                global ? globalBackend->globalBundleAdjustment(observations, head[4]) : backend->bundleAdjustment(observations, head[4]);
            std::printf("ba termination %d iterations %d initial %.17g final %.17g keyframes %zu landmarks %zu outliers %zu\n", out.termination,
                        out.iterations, out.initialCost, out.finalCost, out.updatedKeyframes.size(), out.updatedLandmarks.size(),
                        out.outlierObservations.size());
            if(pcgBackend)
            {
                const mslam::GlobalPcgStats st = pcgBackend->globalPcgStats();
                std::printf("pcg solves %lld iterations %lld longest %lld at_cap %lld breakdowns %lld\n", st.solves, st.iterations, st.longest,
                            st.atCap, st.breakdowns);
            }
            for(std::size_t k = 0; k < K; ++k)
            {
                const auto& st = keyframes[k]->state;
                std::printf("keyframe %zu %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", k, st.orientation.x(), st.orientation.y(),
                            st.orientation.z(), st.orientation.w(), st.position.x(), st.position.y(), st.position.z());
            }
            for(std::size_t l = 0; l < L; ++l)
                std::printf("landmark %zu %.17g %.17g %.17g\n", l, landmarks[l]->state.x(), landmarks[l]->state.y(), landmarks[l]->state.z());
            for(const auto& o : out.outlierObservations)
                std::printf("outlier %llu %llu\n", static_cast<unsigned long long>(o.keyframe->id), static_cast<unsigned long long>(o.landmark->id));
            return 0;
        }
        // --pose-graph <scene>, then nothing, --sparse, --solver <kind>, --loss <spec>, --sparse --loss <spec>, --covariance or
        // --pcg [<spec>]
        const bool pgPcg = (argc == 5 || argc == 6) && std::strcmp(argv[4], "--pcg") == 0;
        const bool pgCovariance = argc == 5 && std::strcmp(argv[4], "--covariance") == 0;
        const bool pgLossOnly = argc == 6 && std::strcmp(argv[4], "--loss") == 0;
        const bool pgSparseLoss = argc == 7 && std::strcmp(argv[4], "--sparse") == 0 && std::strcmp(argv[5], "--loss") == 0;
        if((argc == 4 || (argc == 5 && std::strcmp(argv[4], "--sparse") == 0) || (argc == 6 && std::strcmp(argv[4], "--solver") == 0) ||
            pgLossOnly || pgSparseLoss || pgCovariance || pgPcg) &&
           std::strcmp(argv[2], "--pose-graph") == 0)
        {
            const bool setSolver = argc > 4 && !pgLossOnly && !pgCovariance && !pgPcg;
            int pcgIterations = 500;
            double pcgTolerance = 1e-6;
            if(pgPcg && argc == 6 && !parsePcg(argv[5], pcgIterations, pcgTolerance))
            {
                std::fprintf(stderr, "--pcg takes <max_iterations>:<tolerance>, not %s\n", argv[5]);
                return 2;
            }
            int solverKind = 1;
            int lossKind = 0;
            double lossScale = 0.0;
            if((pgLossOnly || pgSparseLoss) && !mslam::parseLoss(argv[argc - 1], lossKind, lossScale))
            {
                std::fprintf(stderr, "--loss takes huber:<a> or cauchy:<a> with a finite a > 0, not %s\n", argv[argc - 1]);
                return 2;
            }
            if(argc == 6 && !pgLossOnly && !pgPcg)
            {
                // a whole integer or nothing: "abc" and "1x" are usage errors, not kind 0 or 1
                char* end = nullptr;
                const long v = std::strtol(argv[5], &end, 10);
                if(end == argv[5] || *end != '\0' || v < -1000 || v > 1000)
                {
                    std::fprintf(stderr, "--solver takes an integer kind (0 dense, 1 sparse), not %s\n", argv[5]);
                    return 2;
                }
                solverKind = static_cast<int>(v);
            }
            // scene file: "MSPG", i32 version (1), K, E, max_iterations, has_info; K x i32 keyframe id; K x 7 f64 state (qx qy qz
            // qw px py pz); E x i32 a; E x i32 b; E x 7 f64 measurement (q then p of b in a's frame); has_info: E x 36 f64
            std::ifstream in(argv[3], std::ios::binary);
            char magic[4] = {0, 0, 0, 0};
            std::int32_t head[5] = {0, 0, 0, 0, 0};
            in.read(magic, 4);
            in.read(reinterpret_cast<char*>(head), sizeof(head));
            if(!in || std::memcmp(magic, "MSPG", 4) != 0 || head[0] != 1 || head[1] < 0 || head[2] < 0)
            {
                std::fprintf(stderr, "%s is not a pose-graph scene\n", argv[3]);
                return 5;
            }
            const std::size_t K = head[1], E = head[2];
            std::vector<std::int32_t> ids(K), ea(E), eb(E);
            std::vector<double> poses(7 * K), meas(7 * E), info(head[4] ? 36 * E : 0);
            in.read(reinterpret_cast<char*>(ids.data()), K * 4);
            in.read(reinterpret_cast<char*>(poses.data()), K * 56);
            in.read(reinterpret_cast<char*>(ea.data()), E * 4);
            in.read(reinterpret_cast<char*>(eb.data()), E * 4);
            in.read(reinterpret_cast<char*>(meas.data()), E * 56);
            in.read(reinterpret_cast<char*>(info.data()), info.size() * 8);
            if(!in)
            {
                std::fprintf(stderr, "cannot read %s\n", argv[3]);
                return 5;
            }
            using Kf = mslam::Keyframe<mslam::slam3d::SensorState>;
            std::vector<std::shared_ptr<Kf>> keyframes;
            for(std::size_t k = 0; k < K; ++k)
            {
                auto kf = std::make_shared<Kf>();
                const double* v = &poses[7 * k];
                kf->id = static_cast<mslam::Id>(ids[k]);
                kf->state.orientation = mslam::Quaternion(v[3], v[0], v[1], v[2]);
                kf->state.position = mslam::Vector3(v[4], v[5], v[6]);
                keyframes.push_back(kf);
            }
            std::vector<mslam::PoseGraphEdge> edges;
            for(std::size_t e = 0; e < E; ++e)
            {
                if(ea[e] < 0 || static_cast<std::size_t>(ea[e]) >= K || eb[e] < 0 || static_cast<std::size_t>(eb[e]) >= K)
                {
                    std::fprintf(stderr, "edge %zu of %s is out of range\n", e, argv[3]);
                    return 5;
                }
                mslam::PoseGraphEdge edge;
                const double* v = &meas[7 * e];
                edge.a = keyframes[ea[e]], edge.b = keyframes[eb[e]];
                edge.measurement.orientation = mslam::Quaternion(v[3], v[0], v[1], v[2]);
                edge.measurement.position = mslam::Vector3(v[4], v[5], v[6]);
                if(head[4])
                    edge.sqrtInformation.assign(info.begin() + 36 * e, info.begin() + 36 * (e + 1));
                edges.push_back(edge);
            }
            auto makeBackend = mslam::loadFactoryMethod<mslam::IBackend>(argv[1], "hipBundleAdjustBackendFactory");
            if(!makeBackend)
                return 3;
            std::unique_ptr<mslam::IBackend> backend = makeBackend();
            auto* loopBackend = dynamic_cast<mslam::ILoopClosingBackend*>(backend.get());
            if(!loopBackend)
            {
                std::fprintf(stderr, "the plugin does not offer closeLoop\n");
                return 6;
            }
            if(setSolver)
            {
                auto* sparseBackend = dynamic_cast<mslam::ISparsePoseGraphBackend*>(backend.get());
                if(!sparseBackend)
                {
                    std::fprintf(stderr, "the plugin does not offer setPoseGraphSolver\n");
                    return 6;
                }
                sparseBackend->setPoseGraphSolver(solverKind);
            }
            if(pgLossOnly || pgSparseLoss)
            {
                auto* robust = dynamic_cast<mslam::IRobustPoseGraphBackend*>(backend.get());
                if(!robust)
                {
                    std::fprintf(stderr, "the plugin does not offer setPoseGraphLoss\n");
                    return 6;
                }
                robust->setPoseGraphLoss(lossKind, lossScale);
            }
            if(pgCovariance)
            {
                auto* covBackend = dynamic_cast<mslam::IPoseGraphCovariance*>(backend.get());
                if(!covBackend)
                {
                    std::fprintf(stderr, "the plugin does not offer poseGraphCovariance\n");
                    return 6;
                }
                std::vector<bool> hasEdge(K, false);
                for(std::size_t e = 0; e < E; ++e)
                    hasEdge[ea[e]] = hasEdge[eb[e]] = true;
                std::vector<std::shared_ptr<Kf>> of;
                std::vector<std::size_t> ofIndex;
                for(std::size_t k = 0; k < K; ++k)
                    if(hasEdge[k] && keyframes[k]->id != 1)
                        of.push_back(keyframes[k]), ofIndex.push_back(k);
                const mslam::PoseGraphCovariance cov = covBackend->poseGraphCovariance(keyframes, edges, of, {});
                std::printf("covariance blocks %zu\n", of.size());
                for(std::size_t p = 0; p < of.size(); ++p)
                {
                    std::printf("cov %zu", ofIndex[p]);
                    for(int j = 0; j < 36; ++j)
                        std::printf(" %.17g", cov.blocks[36 * p + j]);
                    std::printf("\n");
                }
                return 0;
            }
            auto* pcgBackend = pgPcg ? dynamic_cast<mslam::IIterativePoseGraphBackend*>(backend.get()) : nullptr;
            if(pgPcg)
            {
                if(!pcgBackend)
                {
                    std::fprintf(stderr, "the plugin does not offer setPoseGraphPcg\n");
                    return 6;
                }
                pcgBackend->setPoseGraphPcg(true, pcgIterations, pcgTolerance); // bad values: its std::invalid_argument, exit code 1
            }
            const mslam::BackendOutput out = loopBackend->closeLoop(keyframes, edges, head[3]);
            std::printf("pose_graph termination %d iterations %d initial %.17g final %.17g keyframes %zu edges %zu\n", out.termination,
                        out.iterations, out.initialCost, out.finalCost, out.updatedKeyframes.size(), E);
            if(pcgBackend)
            {
                const mslam::GlobalPcgStats st = pcgBackend->poseGraphPcgStats();
                std::printf("pcg solves %lld iterations %lld longest %lld at_cap %lld breakdowns %lld\n", st.solves, st.iterations, st.longest,
                            st.atCap, st.breakdowns);
            }
            for(std::size_t k = 0; k < K; ++k)
            {
                const auto& st = keyframes[k]->state;
                std::printf("keyframe %zu %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", k, st.orientation.x(), st.orientation.y(),
                            st.orientation.z(), st.orientation.w(), st.position.x(), st.position.y(), st.position.z());
            }
            return 0;
        }
        if(argc == 4 && std::strcmp(argv[2], "--fuse") == 0)
        {
            // scene file: "MSFU", i32 version (1), width, height, max_distance; f64 fx fy cx cy radius ratio max_world_distance;
            // R (9 f64), t (3 f64); i32 number of entries (>= 2: keep, drop, others); per entry i32 n (>= 1), n x 32 descriptor
            // bytes, n x 3 f64 world points, n x i64 landmark ids
            std::ifstream in(argv[3], std::ios::binary);
            char magic[4] = {0, 0, 0, 0};
            std::int32_t head[4] = {0, 0, 0, 0}, nEntries = 0;
            double par[7], R[9], t[3];
            in.read(magic, 4);
            in.read(reinterpret_cast<char*>(head), sizeof(head));
            in.read(reinterpret_cast<char*>(par), sizeof(par));
            in.read(reinterpret_cast<char*>(R), sizeof(R));
            in.read(reinterpret_cast<char*>(t), sizeof(t));
            in.read(reinterpret_cast<char*>(&nEntries), 4);
            if(!in || std::memcmp(magic, "MSFU", 4) != 0 || head[0] != 1 || nEntries < 2)
            {
                std::fprintf(stderr, "%s is not a fusion scene\n", argv[3]);
                return 5;
            }
            auto makeReloc = mslam::loadFactoryMethod<mslam::IOrbRelocalizer>(argv[1], "hipOrbRelocalizerFactory");
            if(!makeReloc)
                return 3;
            std::unique_ptr<mslam::IOrbRelocalizer> relocalizer = makeReloc();
            auto* fuser = dynamic_cast<mslam::ILandmarkFuser*>(relocalizer.get());
            auto* localMap = dynamic_cast<mslam::ILocalMapTracker*>(relocalizer.get());
            if(!fuser || !localMap)
            {
                std::fprintf(stderr, "the plugin does not offer landmark fusion\n");
                return 6;
            }
            using Kf = mslam::Keyframe<mslam::slam3d::SensorState>;
            std::vector<std::shared_ptr<Kf>> entries;
            for(std::int32_t e = 0; e < nEntries; ++e)
            {
                std::int32_t n = 0;
                in.read(reinterpret_cast<char*>(&n), 4);
                if(!in || n < 1 || n > 65535)
                {
                    std::fprintf(stderr, "entry %d of %s is malformed\n", e, argv[3]);
                    return 5;
                }
                std::vector<mslam::OrbKeypoint> kps(static_cast<std::size_t>(n));
                std::vector<mslam::Vector3> world(kps.size());
                std::vector<std::int64_t> ids(kps.size());
                for(std::size_t i = 0; i < kps.size(); ++i)
                {
                    kps[i].keypoint.id = i;
                    in.read(reinterpret_cast<char*>(kps[i].descriptor.data()), 32);
                }
                for(auto& w : world)
                    in.read(reinterpret_cast<char*>(w.v), sizeof(w.v));
                in.read(reinterpret_cast<char*>(ids.data()), static_cast<std::streamsize>(ids.size() * 8));
                if(!in)
                {
                    std::fprintf(stderr, "cannot read %s\n", argv[3]);
                    return 5;
                }
                auto kf = std::make_shared<Kf>();
                kf->id = static_cast<mslam::Id>(100 + e);
                relocalizer->addKeyframe(kf, kps);
                localMap->addKeyframeLandmarksWithIds(kf, kps, world, ids);
                entries.push_back(kf);
            }
            mslam::LandmarkFuseParams fp;
            fp.camera.focal = mslam::Vector2(par[0], par[1]);
            fp.camera.principalPoint = mslam::Vector2(par[2], par[3]);
            fp.width = head[1], fp.height = head[2], fp.maxDistance = head[3];
            fp.radius = par[4], fp.ratio = par[5], fp.maxWorldDistance = par[6];
            const mslam::LandmarkFusion fused = fuser->fuseLandmarks(entries[0], entries[1], R, t, fp);
            std::printf("fuse pairs %zu rewritten %d\n", fused.pairs.size(), fused.rewritten);
            for(const auto& p : fused.pairs)
                std::printf("pair %d %d %lld %lld %d\n", p.keepPosition, p.dropPosition, static_cast<long long>(p.keepId),
                            static_cast<long long>(p.dropId), p.distance);
            for(std::size_t e = 0; e < entries.size(); ++e)
            {
                std::printf("entry %zu ids", e);
                for(const std::int64_t id : localMap->landmarkIds(entries[e]))
                    std::printf(" %lld", static_cast<long long>(id));
                std::printf("\n");
            }
            return 0;
        }
        if(argc == 4 && std::strcmp(argv[2], "--fuse-multi") == 0)
        {
            // scene file: "MSFM", i32 version (1), width, height, max_distance, number of targets (1..64); f64 fx fy cx cy
            // radius ratio max_world_distance; per target R (9 f64), t (3 f64); i32 number of entries (>= 1 + targets: keep,
            // the targets, others); per entry i32 n (>= 1), n x 32 descriptor bytes, n x 3 f64 world points, n x i64 landmark ids
            std::ifstream in(argv[3], std::ios::binary);
            char magic[4] = {0, 0, 0, 0};
            std::int32_t head[5] = {0, 0, 0, 0, 0}, nEntries = 0;
            double par[7];
            in.read(magic, 4);
            in.read(reinterpret_cast<char*>(head), sizeof(head));
            in.read(reinterpret_cast<char*>(par), sizeof(par));
            if(!in || std::memcmp(magic, "MSFM", 4) != 0 || head[0] != 1 || head[4] < 1 || head[4] > 64)
            {
                std::fprintf(stderr, "%s is not a multi-target fusion scene\n", argv[3]);
                return 5;
            }
            const std::size_t targets = static_cast<std::size_t>(head[4]);
            std::vector<double> R(9 * targets), t(3 * targets);
            for(std::size_t m = 0; m < targets; ++m)
            {
                in.read(reinterpret_cast<char*>(&R[9 * m]), 9 * sizeof(double));
                in.read(reinterpret_cast<char*>(&t[3 * m]), 3 * sizeof(double));
            }
            in.read(reinterpret_cast<char*>(&nEntries), 4);
            if(!in || nEntries < head[4] + 1)
            {
                std::fprintf(stderr, "%s is not a multi-target fusion scene\n", argv[3]);
                return 5;
            }
            auto makeReloc = mslam::loadFactoryMethod<mslam::IOrbRelocalizer>(argv[1], "hipOrbRelocalizerFactory");
            if(!makeReloc)
                return 3;
            std::unique_ptr<mslam::IOrbRelocalizer> relocalizer = makeReloc();
            auto* fuser = dynamic_cast<mslam::IMultiLandmarkFuser*>(relocalizer.get());
            auto* localMap = dynamic_cast<mslam::ILocalMapTracker*>(relocalizer.get());
            if(!fuser || !localMap)
            {
                std::fprintf(stderr, "the plugin does not offer multi-target landmark fusion\n");
                return 6;
            }
            using Kf = mslam::Keyframe<mslam::slam3d::SensorState>;
            std::vector<std::shared_ptr<Kf>> entries;
            for(std::int32_t e = 0; e < nEntries; ++e)
            {
                std::int32_t n = 0;
                in.read(reinterpret_cast<char*>(&n), 4);
                if(!in || n < 1 || n > 65535)
                {
                    std::fprintf(stderr, "entry %d of %s is malformed\n", e, argv[3]);
                    return 5;
                }
                std::vector<mslam::OrbKeypoint> kps(static_cast<std::size_t>(n));
                std::vector<mslam::Vector3> world(kps.size());
                std::vector<std::int64_t> ids(kps.size());
                for(std::size_t i = 0; i < kps.size(); ++i)
                {
                    kps[i].keypoint.id = i;
                    in.read(reinterpret_cast<char*>(kps[i].descriptor.data()), 32);
                }
                for(auto& w : world)
                    in.read(reinterpret_cast<char*>(w.v), sizeof(w.v));
                in.read(reinterpret_cast<char*>(ids.data()), static_cast<std::streamsize>(ids.size() * 8));
                if(!in)
                {
                    std::fprintf(stderr, "cannot read %s\n", argv[3]);
                    return 5;
                }
                auto kf = std::make_shared<Kf>();
                kf->id = static_cast<mslam::Id>(100 + e);
                relocalizer->addKeyframe(kf, kps);
                localMap->addKeyframeLandmarksWithIds(kf, kps, world, ids);
                entries.push_back(kf);
            }
            mslam::LandmarkFuseParams fp;
            fp.camera.focal = mslam::Vector2(par[0], par[1]);
            fp.camera.principalPoint = mslam::Vector2(par[2], par[3]);
            fp.width = head[1], fp.height = head[2], fp.maxDistance = head[3];
            fp.radius = par[4], fp.ratio = par[5], fp.maxWorldDistance = par[6];
            const std::vector<std::shared_ptr<Kf>> drops(entries.begin() + 1, entries.begin() + 1 + static_cast<std::ptrdiff_t>(targets));
            const mslam::MultiLandmarkFusion fused = fuser->fuseLandmarksMulti(entries[0], drops, R, t, fp);
            std::printf("fuse-multi pairs %zu rewritten %d\n", fused.pairs.size(), fused.rewritten);
            for(const auto& p : fused.pairs)
                std::printf("pair %d %d %d %lld %lld %d\n", p.target, p.keepPosition, p.dropPosition, static_cast<long long>(p.keepId),
                            static_cast<long long>(p.dropId), p.distance);
            for(std::size_t e = 0; e < entries.size(); ++e)
            {
                std::printf("entry %zu ids", e);
                for(const std::int64_t id : localMap->landmarkIds(entries[e]))
                    std::printf(" %lld", static_cast<long long>(id));
                std::printf("\n");
            }
            return 0;
        }
        if(argc == 4 && std::strcmp(argv[2], "--prune") == 0)
        {
            // scene file: "MSPR", i32 version (1), i32 number of entries, i32 number of rows; per entry i32 id, i32 n (>= 1),
            // n x 32 descriptor bytes, n x 3 f64 world points, n x i64 landmark ids; then rows x i32 entry id, rows x i64
            // landmark id
            std::ifstream in(argv[3], std::ios::binary);
            char magic[4] = {0, 0, 0, 0};
            std::int32_t head[3] = {0, 0, 0};
            in.read(magic, 4);
            in.read(reinterpret_cast<char*>(head), sizeof(head));
            if(!in || std::memcmp(magic, "MSPR", 4) != 0 || head[0] != 1 || head[1] < 1 || head[2] < 0)
            {
                std::fprintf(stderr, "%s is not a pruning scene\n", argv[3]);
                return 5;
            }
            auto makeReloc = mslam::loadFactoryMethod<mslam::IOrbRelocalizer>(argv[1], "hipOrbRelocalizerFactory");
            if(!makeReloc)
                return 3;
            std::unique_ptr<mslam::IOrbRelocalizer> relocalizer = makeReloc();
            auto* remover = dynamic_cast<mslam::IObservationRemover*>(relocalizer.get());
            auto* localMap = dynamic_cast<mslam::ILocalMapTracker*>(relocalizer.get());
            if(!remover || !localMap)
            {
                std::fprintf(stderr, "the plugin does not offer the removal of observations\n");
                return 6;
            }
            using Kf = mslam::Keyframe<mslam::slam3d::SensorState>;
            std::vector<std::shared_ptr<Kf>> entries;
            std::map<std::int32_t, std::shared_ptr<Kf>> byId;
            std::size_t before = 0;
            for(std::int32_t e = 0; e < head[1]; ++e)
            {
                std::int32_t eh[2] = {0, 0};
                in.read(reinterpret_cast<char*>(eh), sizeof(eh));
                if(!in || eh[1] < 1 || eh[1] > 65535 || byId.count(eh[0]))
                {
                    std::fprintf(stderr, "entry %d of %s is malformed\n", e, argv[3]);
                    return 5;
                }
                std::vector<mslam::OrbKeypoint> kps(static_cast<std::size_t>(eh[1]));
                std::vector<mslam::Vector3> world(kps.size());
                std::vector<std::int64_t> ids(kps.size());
                for(std::size_t i = 0; i < kps.size(); ++i)
                {
                    kps[i].keypoint.id = i;
                    in.read(reinterpret_cast<char*>(kps[i].descriptor.data()), 32);
                }
                for(auto& w : world)
                    in.read(reinterpret_cast<char*>(w.v), sizeof(w.v));
                in.read(reinterpret_cast<char*>(ids.data()), static_cast<std::streamsize>(ids.size() * 8));
                if(!in)
                {
                    std::fprintf(stderr, "cannot read %s\n", argv[3]);
                    return 5;
                }
                auto kf = std::make_shared<Kf>();
                kf->id = static_cast<mslam::Id>(eh[0]);
                relocalizer->addKeyframe(kf, kps);
                localMap->addKeyframeLandmarksWithIds(kf, kps, world, ids);
                entries.push_back(kf);
                byId[eh[0]] = kf;
                before += kps.size();
            }
            const std::size_t nRows = static_cast<std::size_t>(head[2]);
            std::vector<std::int32_t> rowKf(nRows + 1);
            std::vector<std::int64_t> rowLid(nRows + 1);
            in.read(reinterpret_cast<char*>(rowKf.data()), static_cast<std::streamsize>(nRows * 4));
            in.read(reinterpret_cast<char*>(rowLid.data()), static_cast<std::streamsize>(nRows * 8));
            if(!in)
            {
                std::fprintf(stderr, "cannot read the rows of %s\n", argv[3]);
                return 5;
            }
            std::vector<std::pair<std::shared_ptr<Kf>, std::int64_t>> rows;
            for(std::size_t p = 0; p < nRows; ++p)
            {
                const auto it = byId.find(rowKf[p]);
                if(it == byId.end())
                {
                    std::fprintf(stderr, "row %zu of %s names no entry\n", p, argv[3]);
                    return 5;
                }
                rows.emplace_back(it->second, rowLid[p]);
            }
            const std::vector<int> removed = remover->removeObservations(rows);
            // the store's own account: what the entries lost
            std::vector<std::vector<std::int64_t>> after;
            std::size_t left = 0;
            for(const auto& kf : entries)
            {
                after.push_back(localMap->landmarkIds(kf));
                left += after.back().size();
            }
            std::printf("prune removed %zu\n", before - left);
            for(std::size_t p = 0; p < removed.size(); ++p)
                std::printf("row %zu %d\n", p, removed[p]);
            for(std::size_t e = 0; e < entries.size(); ++e)
            {
                std::printf("entry %lld n %zu", static_cast<long long>(entries[e]->id), after[e].size());
                for(const std::int64_t id : after[e])
                    std::printf(" %lld", static_cast<long long>(id));
                std::printf("\n");
            }
            return 0;
        }
        if(argc == 4 && (std::strcmp(argv[2], "--cull") == 0 || std::strcmp(argv[2], "--cull-landmarks") == 0))
        {
            // scene file: "MSCL", i32 version (1), i32 entries, i32 listed, i32 candidates, i32 min_observers, i32
            // min_landmarks, f64 ratio; per entry i32 id, i32 n (>= 1), n x 32 descriptor bytes, n x 3 f64 world points,
            // n x i64 landmark ids; then the listed ids and the candidates as i32.  --cull-landmarks: the same layout under
            // the magic "MSLC", with min_observers as the only parameter (no min_landmarks, no ratio)
            const bool landmarks = std::strcmp(argv[2], "--cull-landmarks") == 0;
            std::ifstream in(argv[3], std::ios::binary);
            char magic[4] = {0, 0, 0, 0};
            std::int32_t head[6] = {0, 0, 0, 0, 0, 0};
            mslam::KeyframeCullParams params;
            in.read(magic, 4);
            in.read(reinterpret_cast<char*>(head), landmarks ? 5 * sizeof(head[0]) : sizeof(head));
            if(!landmarks)
                in.read(reinterpret_cast<char*>(&params.ratio), sizeof(params.ratio));
            if(!in || std::memcmp(magic, landmarks ? "MSLC" : "MSCL", 4) != 0 || head[0] != 1 || head[1] < 1 || head[2] < 0 || head[3] < 0)
            {
                std::fprintf(stderr, "%s is not a %s scene\n", argv[3], landmarks ? "landmark-culling" : "culling");
                return 5;
            }
            params.minObservers = head[4], params.minLandmarks = head[5];
            auto makeReloc = mslam::loadFactoryMethod<mslam::IOrbRelocalizer>(argv[1], "hipOrbRelocalizerFactory");
            if(!makeReloc)
                return 3;
            std::unique_ptr<mslam::IOrbRelocalizer> relocalizer = makeReloc();
            auto* culler = dynamic_cast<mslam::IKeyframeCuller*>(relocalizer.get());
            auto* landmarkCuller = dynamic_cast<mslam::ILandmarkCuller*>(relocalizer.get());
            auto* localMap = dynamic_cast<mslam::ILocalMapTracker*>(relocalizer.get());
            if((landmarks ? !landmarkCuller : !culler) || !localMap)
            {
                std::fprintf(stderr, "the plugin does not offer %s culling\n", landmarks ? "landmark" : "keyframe");
                return 6;
            }
            using Kf = mslam::Keyframe<mslam::slam3d::SensorState>;
            std::vector<std::shared_ptr<Kf>> entries;
            std::map<std::int32_t, std::shared_ptr<Kf>> byId;
            for(std::int32_t e = 0; e < head[1]; ++e)
            {
                std::int32_t eh[2] = {0, 0};
                in.read(reinterpret_cast<char*>(eh), sizeof(eh));
                if(!in || eh[1] < 1 || eh[1] > 65535 || byId.count(eh[0]))
                {
                    std::fprintf(stderr, "entry %d of %s is malformed\n", e, argv[3]);
                    return 5;
                }
                std::vector<mslam::OrbKeypoint> kps(static_cast<std::size_t>(eh[1]));
                std::vector<mslam::Vector3> world(kps.size());
                std::vector<std::int64_t> ids(kps.size());
                for(std::size_t i = 0; i < kps.size(); ++i)
                {
                    kps[i].keypoint.id = i;
                    in.read(reinterpret_cast<char*>(kps[i].descriptor.data()), 32);
                }
                for(auto& w : world)
                    in.read(reinterpret_cast<char*>(w.v), sizeof(w.v));
                in.read(reinterpret_cast<char*>(ids.data()), static_cast<std::streamsize>(ids.size() * 8));
                if(!in)
                {
                    std::fprintf(stderr, "cannot read %s\n", argv[3]);
                    return 5;
                }
                auto kf = std::make_shared<Kf>();
                kf->id = static_cast<mslam::Id>(eh[0]);
                relocalizer->addKeyframe(kf, kps);
                localMap->addKeyframeLandmarksWithIds(kf, kps, world, ids);
                entries.push_back(kf);
                byId[eh[0]] = kf;
            }
            std::vector<std::shared_ptr<Kf>> lists[2];
            for(int which = 0; which < 2; ++which)
            {
                std::vector<std::int32_t> named(static_cast<std::size_t>(head[2 + which]) + 1);
                in.read(reinterpret_cast<char*>(named.data()), static_cast<std::streamsize>(head[2 + which]) * 4);
                for(std::int32_t p = 0; in && p < head[2 + which]; ++p)
                {
                    const auto it = byId.find(named[static_cast<std::size_t>(p)]);
                    if(it == byId.end())
                    {
                        std::fprintf(stderr, "%s names an entry it does not hold\n", argv[3]);
                        return 5;
                    }
                    lists[which].push_back(it->second);
                }
                if(!in)
                {
                    std::fprintf(stderr, "cannot read the lists of %s\n", argv[3]);
                    return 5;
                }
            }
            if(landmarks)
            {
                // "lmcull found N removed M", one "lm <id> <observers>" line per culled id (ascending), then
                // "entry <id> <count>" for every entry in scene order: the landmarks it holds afterwards
                std::size_t before = 0, after = 0;
                for(const auto& kf : entries)
                    before += localMap->landmarkIds(kf).size();
                const std::vector<mslam::CulledLandmark> culled = landmarkCuller->cullLandmarks(lists[0], lists[1], params.minObservers);
                std::vector<std::size_t> counts;
                for(const auto& kf : entries)
                {
                    counts.push_back(localMap->landmarkIds(kf).size());
                    after += counts.back();
                }
                std::printf("lmcull found %zu removed %zu\n", culled.size(), before - after);
                for(const auto& l : culled)
                    std::printf("lm %lld %d\n", static_cast<long long>(l.id), l.observers);
                for(std::size_t e = 0; e < entries.size(); ++e)
                    std::printf("entry %lld %zu\n", static_cast<long long>(entries[e]->id), counts[e]);
                return 0;
            }
            const std::vector<mslam::KeyframeCullVerdict> verdicts = culler->cullKeyframes(lists[0], lists[1], params);
            std::size_t gone = 0;
            for(const auto& v : verdicts)
                gone += v.culled ? 1 : 0;
            std::printf("cull culled %zu\n", gone);
            for(std::size_t p = 0; p < verdicts.size(); ++p)
                std::printf("cand %zu %lld %d %d %d\n", p, static_cast<long long>(verdicts[p].keyframe->id), verdicts[p].culled ? 1 : 0,
                            verdicts[p].landmarks, verdicts[p].redundant);
            // the adapter's own account: an entry it no longer holds has no landmark ids to give
            std::printf("remaining");
            for(const auto& kf : entries)
            {
                try
                {
                    (void)localMap->landmarkIds(kf);
                    std::printf(" %lld", static_cast<long long>(kf->id));
                }
                catch(const std::exception&)
                {
                }
            }
            std::printf("\n");
            return 0;
        }
        if(argc == 5 && std::strcmp(argv[2], "--reloc") == 0)
        {
            // scene file: u32 n_keyframes, per keyframe u32 n, n x 32 descriptor bytes, n x 3 f64 world points; then the
            // query: u32 n, n x 32 descriptor bytes, n x 2 f64 keypoint coordinates; then fx fy cx cy (f64)
            setenv("MSLAM_ORB_VOCABULARY", argv[3], 1);
            auto makeReloc = mslam::loadFactoryMethod<mslam::IOrbRelocalizer>(argv[1], "hipOrbRelocalizerFactory");
            auto makeLoop = mslam::loadFactoryMethod<mslam::IOrbLoopDetector>(argv[1], "loopDetection");
            std::unique_ptr<mslam::IOrbRelocalizer> relocalizer = makeReloc();
            std::unique_ptr<mslam::IOrbLoopDetector> loopDetector = makeLoop();
            auto* verified = dynamic_cast<mslam::IVerifiedRelocalizer*>(relocalizer.get());
            auto* verifiedLoop = dynamic_cast<mslam::IVerifiedLoopDetector*>(loopDetector.get());
            if(!verified || !verifiedLoop)
            {
                std::fprintf(stderr, "the plugin does not offer the verified relocalisation\n");
                return 6;
            }
            std::ifstream in(argv[4], std::ios::binary);
            auto readKeypoints = [&in](std::vector<mslam::OrbKeypoint>& kps) {
                std::uint32_t n = 0;
                in.read(reinterpret_cast<char*>(&n), 4);
                kps.resize(n);
                for(std::uint32_t i = 0; i < n; ++i)
                {
                    kps[i].keypoint.id = i;
                    in.read(reinterpret_cast<char*>(kps[i].descriptor.data()), 32);
                }
            };
            using Kf = mslam::Keyframe<mslam::slam3d::SensorState>;
            std::uint32_t nKeyframes = 0;
            in.read(reinterpret_cast<char*>(&nKeyframes), 4);
            std::vector<std::shared_ptr<Kf>> keyframes;
            for(std::uint32_t f = 0; f < nKeyframes; ++f)
            {
                std::vector<mslam::OrbKeypoint> kps;
                readKeypoints(kps);
                std::vector<mslam::Vector3> world(kps.size());
                for(auto& w : world)
                    in.read(reinterpret_cast<char*>(w.v), sizeof(w.v));
                auto kf = std::make_shared<Kf>();
                kf->id = 100 + f;
                relocalizer->addKeyframe(kf, kps);
                verified->addKeyframeLandmarks(kf, kps, world);
                keyframes.push_back(kf);
            }
            std::vector<mslam::OrbKeypoint> query;
            readKeypoints(query);
            for(auto& k : query)
            {
                double xy[2];
                in.read(reinterpret_cast<char*>(xy), sizeof(xy));
                k.keypoint.coordinates = mslam::Vector2(xy[0], xy[1]);
            }
            double cam[4];
            if(!in.read(reinterpret_cast<char*>(cam), sizeof(cam)))
            {
                std::fprintf(stderr, "cannot read %s\n", argv[4]);
                return 5;
            }
            mslam::CameraParameters cp;
            cp.focal = mslam::Vector2(cam[0], cam[1]);
            cp.principalPoint = mslam::Vector2(cam[2], cam[3]);
            cp.factor = 1.0f / 5000.0f;
            auto print = [](const char* what, const mslam::VerifiedRelocalization& r) {
                std::printf("%s keyframe %lld inliers %d rvec %.17g %.17g %.17g tvec %.17g %.17g %.17g\n", what,
                            r.keyframe ? (long long)r.keyframe->id : -1LL, r.inliers, r.rvec[0], r.rvec[1], r.rvec[2], r.tvec[0],
                            r.tvec[1], r.tvec[2]);
                for(const auto& c : r.candidates)
                    std::printf("%s candidate %llu matches %d correspondences %d inliers %d model %d\n", what,
                                (unsigned long long)c.keyframe->id, c.matches, c.correspondences, c.inliers, c.hasModel ? 1 : 0);
            };
            const auto first = verified->relocalizePose(query, cp);
            print("reloc", first);
            auto kf = std::make_shared<Kf>();
            kf->id = 100 + nKeyframes;
            relocalizer->addKeyframe(kf, query);
            const auto loop = loopDetector->detectLoop();
            std::printf("loop %lld\n", loop ? (long long)loop->id : -1LL);
            print("loop-verified", verifiedLoop->detectLoopVerified(cp));
            if(first.keyframe)
            {
                relocalizer->removeKeyframe(first.keyframe);
                print("after-remove", verified->relocalizePose(query, cp));
            }
            return 0;
        }
        // --track <vocabulary> <scene> followed by any of: --local-map <depth>, --guided <radius>, --distinct, --align <max_distance>
        bool trackArgs = argc >= 5 && std::strcmp(argv[2], "--track") == 0;
        int mapDepthArg = -1;
        double guidedRadius = 0.0;
        bool distinct = false;
        double alignDistance = 0.0;
        for(int k = 5; trackArgs && k < argc;)
        {
            if(k + 1 < argc && std::strcmp(argv[k], "--align") == 0)
            {
                alignDistance = std::atof(argv[k + 1]), k += 2;
                if(!(alignDistance > 0.0))
                {
                    std::fprintf(stderr, "--align takes a max_distance > 0, not %s\n", argv[k - 1]);
                    return 2;
                }
                continue;
            }
            if(std::strcmp(argv[k], "--distinct") == 0)
                distinct = true, k += 1;
            else if(k + 1 < argc && std::strcmp(argv[k], "--local-map") == 0)
                mapDepthArg = std::atoi(argv[k + 1]), k += 2;
            else if(k + 1 < argc && std::strcmp(argv[k], "--guided") == 0)
                guidedRadius = std::atof(argv[k + 1]), k += 2;
            else
                trackArgs = false;
        }
        if(trackArgs)
        {
            // --local-map <depth>: track against the union of the reference keyframe's covisibility neighbourhood
            // (ILocalMapTracker) instead of the reference keyframe's own landmarks; the reference uses depth 2
            const int mapDepth = mapDepthArg;
            // scene file, little-endian: 'MSTK', i32 version = 1, n_frames, width, height; f64 fx, fy, cx, cy; f32 factor; i32 seed,
            // min_matched_points, new_keyframe_min_landmarks; f64 z_max; per frame: i32 n, n x 32 descriptor bytes, n x 2 f32
            // keypoint coordinates, height x width u16 depth
            setenv("MSLAM_ORB_VOCABULARY", argv[3], 1);
            auto makeReloc = mslam::loadFactoryMethod<mslam::IOrbRelocalizer>(argv[1], "hipOrbRelocalizerFactory");
            std::unique_ptr<mslam::IOrbRelocalizer> relocalizer = makeReloc();
            auto* tracker = dynamic_cast<mslam::IKeyframeTracker*>(relocalizer.get());
            auto* verified = dynamic_cast<mslam::IVerifiedRelocalizer*>(relocalizer.get());
            auto* localMap = dynamic_cast<mslam::ILocalMapTracker*>(relocalizer.get());
            if(!tracker || !verified || (mapDepth >= 0 && !localMap))
            {
                std::fprintf(stderr, "the plugin does not offer the keyframe tracking step\n");
                return 6;
            }
            if(guidedRadius > 0.0)
                tracker->setGuidedMatch(guidedRadius);
            if(alignDistance > 0.0)
            {
                auto* aligned = dynamic_cast<mslam::IAlignedKeyframeTracker*>(relocalizer.get());
                if(!aligned)
                {
                    std::fprintf(stderr, "--align needs a plugin that offers IAlignedKeyframeTracker\n");
                    return 6;
                }
                aligned->setTrackPose(1, alignDistance);
            }
            if(distinct)
            {
                // --distinct (needs --local-map): the local map carries the most distinctive descriptor of every landmark
                auto* distinctive = dynamic_cast<mslam::IDistinctiveLocalMap*>(relocalizer.get());
                if(!distinctive || mapDepth < 0)
                {
                    std::fprintf(stderr, "--distinct needs --local-map and a plugin that offers IDistinctiveLocalMap\n");
                    return 6;
                }
                distinctive->setUnionDescriptor(1);
            }
            std::ifstream in(argv[4], std::ios::binary);
            char magic[4] = {0, 0, 0, 0};
            std::int32_t head[4] = {0, 0, 0, 0}, par[3] = {0, 0, 0};
            double cam[4], zMax = 0;
            float factor = 0;
            in.read(magic, 4);
            in.read(reinterpret_cast<char*>(head), sizeof(head));
            in.read(reinterpret_cast<char*>(cam), sizeof(cam));
            in.read(reinterpret_cast<char*>(&factor), 4);
            in.read(reinterpret_cast<char*>(par), sizeof(par));
            if(!in.read(reinterpret_cast<char*>(&zMax), 8) || std::memcmp(magic, "MSTK", 4) != 0 || head[0] != 1 || head[2] <= 0 || head[3] <= 0)
            {
                std::fprintf(stderr, "%s is not a tracking scene\n", argv[4]);
                return 5;
            }
            const int nFrames = head[1], width = head[2], height = head[3];
            mslam::CameraParameters cp;
            cp.focal = mslam::Vector2(cam[0], cam[1]);
            cp.principalPoint = mslam::Vector2(cam[2], cam[3]);
            cp.factor = factor;
            mslam::KeyframeTrackOptions opt;
            opt.minMatchedPoints = par[1], opt.newKeyframeMinLandmarks = par[2], opt.zMax = zMax;
            using Kf = mslam::Keyframe<mslam::slam3d::SensorState>;
            std::vector<std::shared_ptr<Kf>> keyframes; // in insertion order: the vote's list (its most recent 64)
            std::shared_ptr<Kf> reference;
            // the local map: the covisibility graph over keyframe ids (updateCovisibility, basic_map.cpp:141-164), the members of
            // the union built last and the reference keyframe it was built for (null: rebuild)
            std::map<mslam::Id, std::set<mslam::Id>> graph;
            std::vector<std::shared_ptr<Kf>> members;
            std::shared_ptr<Kf> mapOf;
            double rvec[3] = {0, 0, 0}, tvec[3] = {0, 0, 0};
            std::vector<std::uint16_t> depth(static_cast<std::size_t>(width) * height);
            for(int f = 0; f < nFrames; ++f)
            {
                std::int32_t n = 0;
                in.read(reinterpret_cast<char*>(&n), 4);
                std::vector<mslam::OrbKeypoint> kps(static_cast<std::size_t>(n > 0 ? n : 0));
                for(std::size_t i = 0; i < kps.size(); ++i)
                {
                    kps[i].keypoint.id = i;
                    in.read(reinterpret_cast<char*>(kps[i].descriptor.data()), 32);
                }
                for(auto& k : kps)
                {
                    float xy[2];
                    in.read(reinterpret_cast<char*>(xy), sizeof(xy));
                    k.keypoint.coordinates = mslam::Vector2(xy[0], xy[1]);
                }
                if(!in.read(reinterpret_cast<char*>(depth.data()), static_cast<std::streamsize>(depth.size() * 2)))
                {
                    std::fprintf(stderr, "cannot read frame %d of %s\n", f, argv[4]);
                    return 5;
                }
                int tracked = 1, inliers = 0, relocalized = 0;
                long long added = -1;
                if(!reference)
                {
                    auto kf = std::make_shared<Kf>();
                    kf->id = 0;
                    tracker->initFirstKeyframe(kf, kps, depth.data(), width, height, cp, zMax);
                    keyframes.push_back(kf);
                    reference = kf;
                    added = 0;
                    graph[kf->id];
                }
                else
                {
                    const std::size_t first = keyframes.size() > 64 ? keyframes.size() - 64 : 0;
                    const std::vector<std::shared_ptr<Kf>> neighbours(keyframes.begin() + static_cast<std::ptrdiff_t>(first), keyframes.end());
                    auto kf = std::make_shared<Kf>();
                    kf->id = keyframes.back()->id + 1;
                    opt.seed = static_cast<std::uint64_t>(par[0]) + static_cast<std::uint64_t>(f);
                    if(mapDepth >= 0 && mapOf != reference)
                    {
                        // getNeighbourKeyframes (basic_map.cpp:209-237) as written: `level <= deepLevel` still expands the nodes
                        // at level mapDepth, so the walk reaches mapDepth + 1 hops; more than 64 keyframes: the 64 largest ids
                        std::set<mslam::Id> result;
                        std::deque<std::pair<mslam::Id, int>> queue{{reference->id, 0}};
                        while(!queue.empty())
                        {
                            const auto [cur, level] = queue.front();
                            queue.pop_front();
                            result.insert(cur);
                            if(level <= mapDepth)
                                for(const mslam::Id nb : graph[cur])
                                    if(!result.count(nb))
                                        queue.emplace_back(nb, level + 1);
                        }
                        members.clear();
                        for(const auto& k : keyframes) // (ascending ids)
                            if(result.count(k->id))
                                members.push_back(k);
                        if(members.size() > 64)
                            members.erase(members.begin(), members.end() - 64);
                        localMap->buildLocalMap(members);
                        mapOf = reference;
                    }
                    const auto r = mapDepth >= 0 ? localMap->trackLocalMap(kps, depth.data(), width, height, cp, neighbours, rvec, tvec, kf, opt)
                                                 : tracker->trackKeyframe(kps, depth.data(), width, height, cp, reference, neighbours, rvec, tvec, kf, opt);
                    tracked = r.tracked ? 1 : 0, inliers = r.inliers;
                    if(r.tracked)
                    {
                        std::memcpy(rvec, r.rvec, sizeof(rvec));
                        std::memcpy(tvec, r.tvec, sizeof(tvec));
                        if(r.bestReference)
                            reference = r.bestReference; // (:366-371)
                        if(r.keyframeAdded)
                        {
                            keyframes.push_back(kf);
                            reference = kf; // (:395-396)
                            added = static_cast<long long>(kf->id);
                            if(mapDepth >= 0)
                            {
                                // part A of the new entry inherits from the union: only its members can share landmarks with it
                                const auto shared = localMap->covisibleLandmarks(kf, members);
                                graph[kf->id];
                                for(std::size_t k = 0; k < members.size(); ++k)
                                    if(shared[k] > 0 && members[k]->id != kf->id)
                                    {
                                        graph[kf->id].insert(members[k]->id);
                                        graph[members[k]->id].insert(kf->id);
                                    }
                                mapOf = nullptr; // a keyframe was added: the local map is rebuilt
                            }
                        }
                    }
                    else if(auto found = verified->relocalizePose(kps, cp).keyframe) // (:210-217)
                    {
                        reference = found;
                        relocalized = 1;
                    }
                }
                std::printf("track frame %d tracked %d inliers %d rvec %.17g %.17g %.17g tvec %.17g %.17g %.17g reference %llu keyframe %lld "
                            "relocalized %d\n",
                            f, tracked, inliers, rvec[0], rvec[1], rvec[2], tvec[0], tvec[1], tvec[2],
                            (unsigned long long)reference->id, added, relocalized);
            }
            return 0;
        }
        if(argc >= 7 && std::strcmp(argv[2], "--bow") == 0)
        {
            setenv("MSLAM_ORB_VOCABULARY", argv[3], 1); // the reference hard-codes "orbvoc.dbow3" in the working directory
            auto makeReloc = mslam::loadFactoryMethod<mslam::IOrbRelocalizer>(argv[1], "hipOrbRelocalizerFactory");
            auto makeLoop = mslam::loadFactoryMethod<mslam::IOrbLoopDetector>(argv[1], "loopDetection");
            std::unique_ptr<mslam::IOrbRelocalizer> relocalizer = makeReloc();
            std::unique_ptr<mslam::IOrbLoopDetector> loopDetector = makeLoop();
            const int w = std::atoi(argv[4]), h = std::atoi(argv[5]);
            using Kf = mslam::Keyframe<mslam::slam3d::SensorState>;
            std::vector<std::shared_ptr<Kf>> keyframes;
            std::vector<std::vector<mslam::OrbKeypoint>> all;
            for(int f = 0; f + 6 < argc; ++f)
            {
                mslam::RgbFrame frame;
                frame.size = {w, h};
                frame.data.resize(static_cast<std::size_t>(w) * h * 3);
                std::ifstream in(argv[6 + f], std::ios::binary);
                if(!in.read(reinterpret_cast<char*>(frame.data.data()), static_cast<std::streamsize>(frame.data.size())))
                {
                    std::fprintf(stderr, "cannot read %s\n", argv[6 + f]);
                    return 5;
                }
                auto kps = detector->detect(frame);
                auto kf = std::make_shared<Kf>();
                kf->id = 100 + static_cast<mslam::Id>(f);
                relocalizer->addKeyframe(kf, kps);
                const auto loop = loopDetector->detectLoop();
                std::printf("keyframe %d keypoints %zu loop %lld\n", f, kps.size(), loop ? (long long)loop->id : -1LL);
                keyframes.push_back(kf);
                all.push_back(std::move(kps));
            }
            for(std::size_t f = 0; f < all.size(); ++f)
            {
                std::printf("relocalize %zu:", f);
                for(const auto& k : relocalizer->relocalize(all[f]))
                    std::printf(" %llu", (unsigned long long)k->id);
                std::printf("\n");
            }
            relocalizer->removeKeyframe(keyframes[0]);
            std::printf("after remove 0:");
            for(const auto& k : relocalizer->relocalize(all[0]))
                std::printf(" %llu", (unsigned long long)k->id);
            std::printf("\n");
            return 0;
        }
        const bool tum = argc == 4 && std::strcmp(argv[2], "--tum") == 0;
        if(argc < 6 && !tum)
            return detector && matcher ? 0 : 4;
        const int w = tum ? 0 : std::atoi(argv[2]), h = tum ? 0 : std::atoi(argv[3]);
        mslam::RgbdFileProvider provider(tum ? mslam::readTumRgbdDataset(argv[3]) : mslam::RgbdFilePaths{},
                                         mslam::tumRgbdCameraParams());
        if(tum && !provider.init())
        {
            std::fprintf(stderr, "no frames listed in %s\n", argv[3]);
            return 5;
        }
        std::vector<mslam::OrbKeypoint> prev;
        for(int f = 0; tum ? provider.fetch() : f < 2; ++f)
        {
            mslam::RgbFrame frame;
            if(tum)
            {
                const auto data = provider.recentData();
                frame.size = {data->width, data->height};
                frame.data = data->rgb;
            }
            else
            {
                frame.size = {w, h};
                frame.data.resize(static_cast<std::size_t>(w) * h * 3);
                std::ifstream in(argv[4 + f], std::ios::binary);
                if(!in.read(reinterpret_cast<char*>(frame.data.data()), static_cast<std::streamsize>(frame.data.size())))
                {
                    std::fprintf(stderr, "cannot read %s\n", argv[4 + f]);
                    return 5;
                }
            }
            auto kps = detector->detect(frame);
            std::uint32_t hc = 0x811C9DC5u;
            for(const auto& k : kps)
            {
                const double xy[2] = {k.keypoint.coordinates.x(), k.keypoint.coordinates.y()};
                hc = fnv(&k.keypoint.id, 8, hc);
                hc = fnv(xy, 16, hc);
                hc = fnv(k.descriptor.data(), 32, hc);
            }
            std::printf("frame %d keypoints %zu fnv %08x\n", f, kps.size(), hc);
            if(f > 0)
            {
                auto m = matcher->match(kps, prev);
                std::uint32_t hm = 0x811C9DC5u;
                for(const auto& d : m)
                {
                    const std::uint64_t ft[2] = {d.fromIndex, d.toIndex};
                    hm = fnv(ft, 16, hm);
                }
                std::printf("match %d pairs %zu fnv %08x\n", f, m.size(), hm);
            }
            prev = std::move(kps);
        }
    }
    catch(const std::exception& e)
    {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
