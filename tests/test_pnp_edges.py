"""RANSAC PnP (k_pnp.hip) at its edges: the consensus floor (5 inliers, RANSACPointSetRegistrator::run's
goodCount > max(maxGoodCount, modelPoints - 1) with modelPoints = 5), problems above the LDS staging limits (2048 points,
256 hypotheses), the single-problem scratch growing between calls, 4 - 6 points and degenerate inputs, points behind the
camera, and the batched form's no-model frames and large frames.

Every test first checks its precondition on the oracle, so that it cannot pass on a scene that misses its edge."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import mslam_cv_pnp_oracle as cvo  # noqa: E402
import mslam_pnp_oracle as po  # noqa: E402
from test_pnp import CAM, rot_err, scene  # noqa: E402
from test_oracle_cv_pnp import scene as cv_scene  # noqa: E402


def group_scene(seed, sizes, n_out=2, far=25.0, first=None):
    """Groups of points, group g exact (up to float32 rounding) under its own pose, the poses far apart (rotation angles
    0.5, 1.5, 2.5 ... rad about random axes), plus n_out outliers moved at least `far` pixels off group 0's projection.
    -> obj, img, label (group index, -1 = outlier), poses [(rvec, t)].  The points are shuffled; `first` = the indices
    group 0 takes instead."""
    rng = np.random.default_rng(seed)
    obj, img, lab, poses = [], [], [], []
    for g, m in enumerate(sizes):
        rvec = rng.normal(size=3)
        rvec *= (0.5 + g) / np.linalg.norm(rvec)
        t = rng.normal(size=3) * 0.3
        X = np.stack([rng.uniform(-2, 2, m), rng.uniform(-1.5, 1.5, m), rng.uniform(2, 7, m)], 1)
        P = ((X - t) @ cvo.rodrigues(rvec)).astype(np.float32)
        obj.append(P)
        img.append(cvo.project_points(P, rvec, t, CAM))
        lab += [g] * m
        poses.append((rvec, t))
    rvec, t = poses[0]
    X = np.stack([rng.uniform(-2, 2, n_out), rng.uniform(-1.5, 1.5, n_out), rng.uniform(2, 7, n_out)], 1)
    P = ((X - t) @ cvo.rodrigues(rvec)).astype(np.float32)
    ang = rng.uniform(0, 2 * np.pi, n_out)
    uv = cvo.project_points(P, rvec, t, CAM) + (far + rng.uniform(0, 200, n_out))[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
    obj.append(P)
    img.append(uv)
    lab += [-1] * n_out
    obj, img, lab = np.concatenate(obj), np.concatenate(img), np.array(lab)
    n = len(obj)
    perm = rng.permutation(n)
    if first is not None:
        perm = np.empty(n, int)
        perm[list(first)] = np.nonzero(lab == 0)[0]
        perm[[i for i in range(n) if i not in first]] = rng.permutation(np.nonzero(lab != 0)[0])
    return obj[perm], img[perm].astype(np.float32), lab[perm], poses


def four_inlier_scene():
    """two groups of 4 + 2 far outliers (n = 10): with sampler seed 0, several of the kernel's hypotheses explain one whole
    group (4 inliers) and none explains more"""
    return group_scene(11, (4, 4))


def five_inlier_scene():
    """a group of 5, a group of 4, 2 far outliers (n = 11).  The group of 5 sits at the indices of cv::RNG's first 5-point
    subset for n = 11, so the OpenCV-algorithm oracle draws it in its first hypothesis; the kernel's sampler (seed 0)
    reaches it on its own"""
    first = cvo.get_subset(cvo.CvRNG(cvo.M64), 11, 5)
    return group_scene(0, (5, 4), first=first)


def mirrored_scene(n=400, n_mirror=20, seed=51):
    """a clean, noise-free scene plus n_mirror points whose camera coordinates are the negatives of inlier points: their
    pixels are exactly the ones a projection that divides by a negative depth gives them"""
    obj, img, rvec, t, good = cv_scene(seed, n=n, outliers=0.0, noise=0.0)
    R = cvo.rodrigues(rvec)
    src = np.arange(0, n, n // n_mirror)[:n_mirror]
    X = obj[src].astype(np.float64) @ R.T + t
    mirrored = ((-X - t) @ R).astype(np.float32)
    assert (mirrored.astype(np.float64) @ R.T + t)[:, 2].max() < -1.0          # well behind the camera
    obj2 = np.concatenate([obj, mirrored])
    img2 = np.concatenate([img, cvo.project_points(mirrored, rvec, t, CAM).astype(np.float32)])
    assert np.abs(img2[n:] - img[src]).max() < 1e-3                            # the pixels of the points they mirror
    return obj2, img2, rvec, t, n


def rvec_of(R):
    return cvo.rodrigues_inv(R)


# ---- CPU: the oracles at the consensus floor -----------------------------------------------------------------------------

def test_oracles_reject_a_best_hypothesis_of_exactly_four_inliers():
    obj, img, lab, _ = four_inlier_scene()
    assert len(obj) == 10 and (lab >= 0).sum() == 8
    run = po.consensus(obj, img, CAM, seed=0)
    c = np.array(run["counts"])
    assert c.max() == 4 and (c == 4).sum() >= 2 and run["best"] == -1 and run["looked_at"] == 100
    # the 4-inlier hypotheses explain one whole group each
    for h in np.nonzero(c == 4)[0]:
        m = po.inliers_of(run["hyps"][h][0], run["hyps"][h][1], obj, img, CAM, 5.0)
        assert len(set(lab[m])) == 1 and lab[m][0] >= 0
    assert po.pnp_ransac(obj, img, CAM, seed=0) is None
    ref = cvo.solve_pnp_ransac(obj, img, CAM)
    assert not ref["ok"] and not ref["mask"].any()


def test_oracles_accept_a_best_hypothesis_of_exactly_five_inliers():
    obj, img, lab, poses = five_inlier_scene()
    assert len(obj) == 11 and (lab == 0).sum() == 5
    res = po.pnp_ransac(obj, img, CAM, seed=0)
    assert res is not None and max(res["counts"]) == 5 and res["counts"][res["best"]] == 5
    assert np.array_equal(res["mask"], lab == 0)
    ref = cvo.solve_pnp_ransac(obj, img, CAM)
    assert ref["ok"] and np.array_equal(ref["mask"], lab == 0)
    # both refine on the same five points: the same pose, which is group 0's
    assert np.abs(rvec_of(res["R"]) - ref["rvec"]).max() < 1e-9 and np.abs(res["t"] - ref["tvec"]).max() < 1e-9
    assert np.abs(ref["rvec"] - poses[0][0]).max() < 1e-5 and np.abs(ref["tvec"] - poses[0][1]).max() < 1e-5


def test_oracles_disagree_on_points_behind_the_camera():
    """cv::projectPoints divides by a negative depth, so OpenCV counts a point behind the camera whose mirrored projection
    lands within 5 px; the library (and its same-sample oracle) never counts a point with depth <= 1e-9"""
    obj, img, rvec, t, n = mirrored_scene()
    ref = cvo.solve_pnp_ransac(obj, img, CAM)
    res = po.pnp_ransac(obj, img, CAM, seed=5)
    assert ref["ok"] and ref["mask"][n:].all() and ref["mask"][:n].all()
    assert res is not None and not res["mask"][n:].any() and np.array_equal(res["mask"][:n], ref["mask"][:n])
    assert np.abs(rvec_of(res["R"]) - ref["rvec"]).max() < 1e-7 and np.abs(res["t"] - ref["tvec"]).max() < 1e-7


def test_oracle_small_and_degenerate_problems():
    for n in (5, 6):
        obj, img, R, t, good = scene(60 + n, n=n, outliers=0.0, noise=0.0)
        res = po.pnp_ransac(obj, img, CAM, seed=0)
        assert res is not None and res["mask"].all() and rot_err(res["R"], R) < 1e-3
    obj, img, R, t, good = scene(64, n=4, outliers=0.0, noise=0.0)
    assert max(po.consensus(obj, img, CAM, seed=0)["counts"]) == 4 and po.pnp_ransac(obj, img, CAM, seed=0) is None
    with np.errstate(all="ignore"):
        obj, img = collinear_scene()
        assert max(po.consensus(obj, img, CAM, seed=0)["counts"]) == -1 and po.pnp_ransac(obj, img, CAM, seed=0) is None
        obj, img = one_pixel_scene()
        assert po.pnp_ransac(obj, img, CAM, seed=0) is None


def collinear_scene(n=40):
    """object points exactly on a line (y, z constant, x on a dyadic grid: every cross product of their differences is 0
    in floating point too) and their exact projections under a real pose"""
    x = np.arange(n, dtype=np.float64) * 0.0625 - 1.25
    obj = np.stack([x, np.full(n, 0.375), np.zeros(n)], 1).astype(np.float32)
    rvec, t = np.array([0.1, -0.2, 0.05]), np.array([0.1, -0.1, 4.0])
    return obj, cvo.project_points(obj, rvec, t, CAM).astype(np.float32)


def one_pixel_scene(n=50):
    """generic object points, every image point the same pixel"""
    rng = np.random.default_rng(70)
    obj = (rng.normal(size=(n, 3)) + [0, 0, 5]).astype(np.float32)
    return obj, np.tile(np.float32([320.0, 240.0]), (n, 1))


# ---- GPU -----------------------------------------------------------------------------------------------------------------

def _same_result(got, ref, ctx=""):
    """kernel result vs the same-sample oracle: same best hypothesis (mask), same optimum"""
    assert got is not None and ref is not None, (ctx, got is None, ref is None)
    r, tv, mask = got
    assert np.array_equal(mask, ref["mask"]), (ctx, mask.sum(), ref["mask"].sum())
    assert small_angle(po.rodrigues(r), ref["R"]) < 1e-6 and np.linalg.norm(tv - ref["t"]) < 1e-7, (ctx, tv - ref["t"])


def small_angle(Ra, Rb):
    """degrees between two nearby rotations: ||Ra - Rb||_F = 2 sqrt(2) sin(angle / 2) (no arccos of a trace next to 3,
    whose resolution is ~1e-6 degrees)"""
    return np.degrees(2 * np.arcsin(min(1.0, np.linalg.norm(Ra - Rb) / (2 * np.sqrt(2)))))


@pytest.mark.gpu
def test_gpu_pnp_consensus_floor(pkg):
    """a best hypothesis of exactly 4 inliers is no model (solvePnPRansac returns false); exactly 5 is one"""
    c = pkg.Context(width=0, height=0)
    obj, img, lab, _ = four_inlier_scene()
    assert max(po.consensus(obj, img, CAM, seed=0)["counts"]) == 4
    assert c.pnp_ransac(obj, img, CAM[:2], CAM[2:], seed=0) is None
    obj, img, lab, _ = five_inlier_scene()
    ref = po.pnp_ransac(obj, img, CAM, seed=0)
    assert max(ref["counts"]) == 5 and np.array_equal(ref["mask"], lab == 0)
    _same_result(c.pnp_ransac(obj, img, CAM[:2], CAM[2:], seed=0), ref, "five")
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2047, 2048, 2049, 5000, 20000])
def test_gpu_pnp_large_problems(pkg, n):
    """above kPnpLdsPts = 2048 points the scoring loop and the refinement read the points from global memory"""
    c = pkg.Context(width=0, height=0)
    obj, img, R, t, good = scene(100 + n, n=n, outliers=0.3, noise=0.4)
    assert len(obj) == n
    ref = po.pnp_ransac(obj, img, CAM, seed=n)
    assert ref is not None and rot_err(ref["R"], R) < 0.1
    _same_result(c.pnp_ransac(obj, img, CAM[:2], CAM[2:], seed=n), ref, n)
    if n == 5000:
        obj, img, rvec, t, good = cv_scene(105, n=n, outliers=0.3, noise=0.0)
        assert len(obj) > 2048
        ref = cvo.solve_pnp_ransac(obj, img, CAM)
        r, tv, mask = c.pnp_ransac(obj, img, CAM[:2], CAM[2:], seed=7)
        assert ref["ok"] and np.array_equal(ref["mask"], good) and np.array_equal(mask, good)
        assert np.abs(r - ref["rvec"]).max() < 1e-6 and np.abs(tv - ref["tvec"]).max() < 1e-6
    c.close()


@pytest.mark.gpu
def test_gpu_pnp_iteration_counts(pkg):
    """above kPnpLdsHyp = 256 iterations the hypotheses and their counts live in the caller's global arrays; the loop ends
    at the same hypothesis as the oracle's sequential one with and without the confidence bound"""
    c = pkg.Context(width=0, height=0)
    obj, img, R, t, good = scene(22, outliers=0.6)
    assert po.consensus(obj, img, CAM, seed=2)["looked_at"] == 100     # no early exit in the first round (60 % outliers)
    for conf in (0.99, 1.0):
        c.pnp_set_confidence(conf)
        for it in (1, 3, 255, 256, 257, 1000, 4096):
            ref = po.pnp_ransac(obj, img, CAM, iterations=it, seed=2, confidence=conf)
            got = c.pnp_ransac(obj, img, CAM[:2], CAM[2:], iterations=it, seed=2)
            if it <= 3 and ref is None:        # a handful of samples at 60 % outliers may hold no all-inlier one
                assert got is None, (conf, it)
                continue
            if it >= 255:
                assert ref["looked_at"] > 4 * 2 and (conf < 1 or ref["looked_at"] == it)
            _same_result(got, ref, (conf, it))
    c.pnp_set_confidence(0.99)
    for it in (0, 4097):
        with pytest.raises(pkg.MslamHipError):
            c.pnp_ransac(obj, img, CAM[:2], CAM[2:], iterations=it)
    c.close()


@pytest.mark.gpu
def test_gpu_pnp_scratch_regrowth(pkg):
    """the single-problem scratch grows with n (above 1024) and with the iterations (above 128) and is reused in between:
    every call on one context is bit-identical to the same call on a fresh one"""
    scenes = {500: scene(80, n=500, outliers=0.3), 5000: scene(81, n=5000, outliers=0.3)}
    shared = pkg.Context(width=0, height=0)
    for n, it in ((500, 100), (5000, 100), (500, 2000), (500, 100), (5000, 100)):
        obj, img = scenes[n][:2]
        got = shared.pnp_ransac(obj, img, CAM[:2], CAM[2:], iterations=it, seed=3)
        fresh = pkg.Context(width=0, height=0)
        ref = fresh.pnp_ransac(obj, img, CAM[:2], CAM[2:], iterations=it, seed=3)
        fresh.close()
        assert got is not None and ref is not None
        for a, b in zip(got, ref):
            assert np.array_equal(a, b), (n, it)
    shared.close()


@pytest.mark.gpu
def test_gpu_pnp_small_and_degenerate_problems(pkg):
    """n = 4: at most 4 inliers, so no model (OpenCV solves 4 points with P3P and returns all of them: the header's
    'n <= 5' DEVIATES item); n = 5, 6 exact: every point an inlier; n = 3: invalid; collinear object points and a single
    image pixel: P3P fails or explains too few points, no model"""
    c = pkg.Context(width=0, height=0)
    obj, img, R, t, good = scene(64, n=4, outliers=0.0, noise=0.0)
    assert max(po.consensus(obj, img, CAM, seed=0)["counts"]) == 4
    assert c.pnp_ransac(obj, img, CAM[:2], CAM[2:], seed=0) is None
    for n in (5, 6):
        obj, img, R, t, good = scene(60 + n, n=n, outliers=0.0, noise=0.0)
        ref = po.pnp_ransac(obj, img, CAM, seed=0)
        assert ref["mask"].all()
        _same_result(c.pnp_ransac(obj, img, CAM[:2], CAM[2:], seed=0), ref, n)
    with pytest.raises(pkg.MslamHipError):
        c.pnp_ransac(obj[:3], img[:3], CAM[:2], CAM[2:])
    with np.errstate(all="ignore"):
        for obj, img in (collinear_scene(), one_pixel_scene()):
            assert po.pnp_ransac(obj, img, CAM, seed=0) is None
            assert c.pnp_ransac(obj, img, CAM[:2], CAM[2:], seed=0) is None
    c.close()


@pytest.mark.gpu
def test_gpu_pnp_never_counts_points_behind_the_camera(pkg):
    """the kernel keeps its cheirality test where OpenCV counts mirrored points (header: DEVIATES item)"""
    obj, img, rvec, t, n = mirrored_scene()
    ref = cvo.solve_pnp_ransac(obj, img, CAM)
    assert ref["ok"] and ref["mask"][n:].all()
    c = pkg.Context(width=0, height=0)
    r, tv, mask = c.pnp_ransac(obj, img, CAM[:2], CAM[2:], seed=5)
    c.close()
    assert not mask[n:].any() and np.array_equal(mask[:n], ref["mask"][:n])
    assert np.abs(r - ref["rvec"]).max() < 1e-6 and np.abs(tv - ref["tvec"]).max() < 1e-6


def _run_batch(pkg, frames, Z, ctx_kw, seed):
    """detect, match, back-project (a plane at Z metres) and PnP one batch on the device -> the host copies"""
    import torch
    B, H, W = frames.shape[:3]
    K = ctx_kw["max_keypoints"]
    c = pkg.Context(width=W, height=H, max_batch=B, **ctx_kw)
    c.detect_batch_dev(torch.from_numpy(frames).cuda().data_ptr(), B)
    c.match_batch_dev(0.7, False)
    d_depth = torch.from_numpy(np.full((B, H, W), int(Z * 5000), np.uint16).view(np.int16)).cuda()
    c.backproject_batch_dev(d_depth.data_ptr(), focal=CAM[:2], principal=CAM[2:])
    c.pnp_batch_dev(CAM[:2], CAM[2:], seed=seed)
    c.sync()
    nv = c.pnp_view()
    out = dict(pose=pkg.read_device(c, nv.pose, (B, 16), np.float64), n=pkg.read_device(c, nv.n_points, (B,), np.int32),
               obj=pkg.read_device(c, nv.object_points, (B, K, 3), np.float32),
               img=pkg.read_device(c, nv.image_points, (B, K, 2), np.float32),
               inl=pkg.read_device(c, nv.inliers, (B, K), np.uint8))
    c.close()
    return out


def _check_frame_against_single(single, out, t, seed):
    n = int(out["n"][t])
    r1, t1, m1 = single.pnp_ransac(out["obj"][t, :n], out["img"][t, :n], CAM[:2], CAM[2:], seed=seed + t)
    pose = out["pose"][t]
    assert pose[14] == 1.0 and np.array_equal(m1, out["inl"][t, :n]) and int(pose[12]) == int(m1.sum())
    # (the single-problem call returns a Rodrigues vector: the matrices are compared at its round-trip resolution)
    assert np.abs(po.rodrigues(r1) - pose[:9].reshape(3, 3)).max() < 1e-9 and np.array_equal(t1, pose[9:12])


@pytest.mark.gpu
def test_gpu_pnp_batch_no_model_frames_and_recovery(pkg):
    """a flat frame in the middle of a batch: it has no keypoints, so it and the frame after it have no correspondences
    (status 0, an all-zero pose); the frame after those recovers and equals the single-problem call"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth
    B, Z, flat = 6, 2.0, 3
    base = synth.make_stream(1, 640 + 64, 480 + 48, seed=11)[0]
    shifts = [(3 * t, 2 * t) for t in range(B)]
    frames = np.stack([np.ascontiguousarray(base[dy:dy + 480, dx:dx + 640]) for dx, dy in shifts])
    frames[flat] = 128
    out = _run_batch(pkg, frames, Z, dict(max_keypoints=4096), seed=40)
    single = pkg.Context(width=0, height=0)
    for t in range(B):
        pose = out["pose"][t]
        if t in (0, flat, flat + 1):
            assert out["n"][t] == 0 and pose[14] == 0.0 and not pose[:13].any() and pose[13] == -1.0, (t, pose)
        else:
            assert out["n"][t] > 300
            _check_frame_against_single(single, out, t, 40)
    single.close()


@pytest.mark.gpu
def test_gpu_pnp_batch_large_frames(pkg):
    """cfg5 geometry (1920x1080, 3 levels, up to 32768 keypoints): frames with more than 2048 correspondences run the
    global-memory paths of the batched kernel; every frame equals the single-problem call with seed + t"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth
    B, Z, W, H = 4, 2.0, 1920, 1080
    base = synth.make_stream(1, W + 64, H + 48, seed=12)[0]
    shifts = [(3 * t, 2 * t) for t in range(B)]
    frames = np.stack([np.ascontiguousarray(base[dy:dy + H, dx:dx + W]) for dx, dy in shifts])
    area = -(-W * H // (640 * 480))
    out = _run_batch(pkg, frames, Z, dict(n_levels=3, min_node_area=370, max_keypoints=32768, max_candidates=16384 * area),
                     seed=90)
    assert out["n"][0] == 0 and out["pose"][0, 14] == 0.0
    assert out["n"][1:].max() > 2048, out["n"]
    single = pkg.Context(width=0, height=0)
    for t in range(1, B):
        assert out["n"][t] > 300
        _check_frame_against_single(single, out, t, 90)
    single.close()
