"""RANSAC rigid alignment on the GPU (k_align.hip) against the numpy reference tests/align_ref.py: same samples by
construction (the same splitmix64 rule), so masks, inlier counts and the best hypothesis are equal and the two closed forms
(Horn's quaternion in the kernel, SVD in the reference) agree to rounding.  tests/test_align.py checks on the CPU that no
point of these scenes lies within 1e-6 of the inlier bound."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_ref as ar  # noqa: E402

pytestmark = pytest.mark.gpu

CAM = (525.0, 525.0, 319.5, 239.5)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(width=0, height=0)
    yield c
    c.close()


def agree(pkg, got, ref, name):
    """the agreement the comparison asks for: mask, n_inliers and best hypothesis equal, R and t within 1e-9, a proper R"""
    if ref["best"] < 0:
        assert got is None, name
        return
    assert got is not None, name
    rvec, t, mask, rec = got
    R = rec[:9].reshape(3, 3)
    assert np.array_equal(mask, ref["mask"]), (name, mask.sum(), ref["mask"].sum())
    assert int(rec[12]) == int(ref["mask"].sum()) and int(rec[13]) == ref["best"] and rec[14] == 1.0, (name, rec[12:15], ref["best"])
    print("%s: |dR| %.3g |dt| %.3g |det - 1| %.3g" % (name, np.abs(R - ref["R"]).max(), np.abs(t - ref["t"]).max(),
                                                      abs(np.linalg.det(R) - 1)))
    assert np.abs(R - ref["R"]).max() <= 1e-9 and np.abs(t - ref["t"]).max() <= 1e-9, name
    assert abs(np.linalg.det(R) - 1) <= 1e-12, name
    assert np.array_equal(t, rec[9:12])
    # the Rodrigues vector the C ABI returns is that rotation
    assert np.abs(ar.rodrigues(rvec) - R).max() <= 1e-9, name


@pytest.mark.parametrize("case", ar.shape_cases(), ids=lambda c: c[0])
def test_gpu_align_agrees_with_the_reference(pkg, ctx, case):
    name, kw, iterations, confidence = case
    src, dst, R, t, good = ar.scene(**kw)
    ctx.pnp_set_confidence(confidence)
    try:
        got = ctx.align_ransac(src, dst, ar.MAX_DISTANCE, iterations, kw["seed"], record=True)
    finally:
        ctx.pnp_set_confidence(0.99)
    ref = ar.align_ransac(src, dst, ar.MAX_DISTANCE, iterations, kw["seed"], confidence)
    agree(pkg, got, ref, name)
    if kw["n"] >= 63 and iterations >= 100:
        # ... and with ground truth: noise of at most 10 mm on >= 25 inliers
        assert ref["best"] >= 0 and np.abs(got[3][:9].reshape(3, 3) - R).max() < 0.02 and np.abs(got[1] - t).max() < 0.05


@pytest.mark.parametrize("confidence", (0.99, 1.0))
def test_gpu_align_edge_scenes(pkg, ctx, confidence):
    ctx.pnp_set_confidence(confidence)
    try:
        for name, (src, dst, dist, expect) in ar.edge_scenes().items():
            got = ctx.align_ransac(src, dst, dist, 100, 5, record=True)
            ref = ar.align_ransac(src, dst, dist, 100, 5, confidence)
            agree(pkg, got, ref, name)
            if expect == "no_model":
                assert got is None, name
            elif expect != "reference":
                assert got is not None and np.abs(got[3][:9].reshape(3, 3) - expect[1]).max() < 1e-5, name
                assert np.abs(got[1] - expect[2]).max() < 1e-4, name
            if got is not None:
                assert abs(np.linalg.det(got[3][:9].reshape(3, 3)) - 1) <= 1e-12, name   # never a reflection
            if name == "nan_point":
                assert not got[2][7] and not got[2][31] and got[2].sum() == len(src) - 2
    finally:
        ctx.pnp_set_confidence(0.99)


def test_gpu_align_no_model_leaves_the_outputs(pkg, ctx):
    """E_NO_MODEL: rvec, tvec and the mask as they were, *n_inliers = 0 (as mslam_hip_pnp_ransac)"""
    src, dst, dist, _ = ar.edge_scenes()["collinear"]
    r, t = np.full(3, 7.0), np.full(3, -3.0)
    mask = np.full(len(src), 9, np.uint8)
    n_in = C.c_int(55)
    rc = ctx.L.mslam_hip_align_ransac(ctx._h, pkg._p(src), pkg._p(dst), len(src), 100, C.c_double(dist), C.c_uint64(5), pkg._p(r),
                                      pkg._p(t), pkg._p(mask), C.byref(n_in))
    assert rc == pkg.E_NO_MODEL and n_in.value == 0
    assert (r == 7.0).all() and (t == -3.0).all() and (mask == 9).all()


def test_gpu_align_invalid_arguments(pkg, ctx):
    src, dst = ar.scene(1, 50, 0.0, 0.0)[:2]
    r, t = np.zeros(3), np.zeros(3)

    def call(s=src, d=dst, n=50, it=100, dist=0.05, rv=r, tv=t, h=None):
        return ctx.L.mslam_hip_align_ransac(ctx._h if h is None else h, pkg._p(s), pkg._p(d), n, it, C.c_double(dist), C.c_uint64(0),
                                            pkg._p(rv), pkg._p(tv), None, None)
    assert call() == pkg.OK
    for kw in (dict(n=2), dict(n=0), dict(n=-1), dict(it=0), dict(it=4097), dict(dist=0.0), dict(dist=-1.0), dict(dist=float("nan")),
               dict(s=None), dict(d=None), dict(rv=None), dict(tv=None)):
        assert call(**kw) == pkg.E_INVALID, kw
    assert ctx.L.mslam_hip_align_ransac(None, pkg._p(src), pkg._p(dst), 50, 100, C.c_double(0.05), C.c_uint64(0), pkg._p(r), pkg._p(t),
                                        None, None) == pkg.E_INVALID
    assert call(it=1) in (pkg.OK, pkg.E_NO_MODEL) and call(it=4096) == pkg.OK and call(n=3) == pkg.E_NO_MODEL
    # the tracking setting
    assert ctx.get_track_pose() == (pkg.TRACK_POSE_PNP, 0.0)
    for kind, dist in ((2, 0.05), (-1, 0.05), (pkg.TRACK_POSE_ALIGN, 0.0), (pkg.TRACK_POSE_ALIGN, -0.1), (pkg.TRACK_POSE_ALIGN, float("nan"))):
        assert ctx.L.mslam_hip_set_track_pose(ctx._h, kind, C.c_double(dist)) == pkg.E_INVALID
        assert ctx.get_track_pose() == (pkg.TRACK_POSE_PNP, 0.0)
    ctx.set_track_pose("align", 0.05)
    assert ctx.get_track_pose() == (pkg.TRACK_POSE_ALIGN, 0.05)
    ctx.set_track_pose("pnp")
    assert ctx.get_track_pose() == (pkg.TRACK_POSE_PNP, 0.0)
    assert ctx.L.mslam_hip_set_track_pose(None, 0, C.c_double(0.0)) == pkg.E_INVALID
    fresh = pkg.Context(width=0, height=0)
    with pytest.raises(pkg.MslamHipError):
        fresh.align_view()                     # neither alignment call has run
    with pytest.raises(pkg.MslamHipError):
        fresh.align_batch_dev(0.05)            # no detect batch
    fresh.close()


def test_gpu_align_two_calls_give_equal_bits(pkg, ctx):
    for n, it in ((400, 100), (ar.LDS_POINTS + 77, ar.LDS_HYPOTHESES + 9)):
        src, dst = ar.scene(31, n, 0.3, 0.005)[:2]
        a = ctx.align_ransac(src, dst, ar.MAX_DISTANCE, it, 8, record=True)
        other = pkg.Context(width=0, height=0)
        b = other.align_ransac(src, dst, ar.MAX_DISTANCE, it, 8, record=True)
        other.close()
        c = ctx.align_ransac(src, dst, ar.MAX_DISTANCE, it, 8, record=True)
        for x in (b, c):
            assert all(np.array_equal(p, q) for p, q in zip(a, x))


def _shifted_batch(pkg, B, K, Z, depth_edit=None):
    """the six shifted frames of tests/test_pnp.py's batch test: detected, matched and back-projected on the device"""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth
    base = synth.make_stream(1, 640 + 64, 480 + 48, seed=11)[0]
    shifts = [(3 * t, 2 * t) for t in range(B)]
    frames = np.stack([np.ascontiguousarray(base[dy:dy + 480, dx:dx + 640]) for dx, dy in shifts])
    depth = np.full((B, 480, 640), int(Z * 5000), np.uint16)
    c = pkg.Context(width=640, height=480, max_batch=B, max_keypoints=K)
    c.detect_batch_dev(torch.from_numpy(frames).cuda().data_ptr(), B)
    c.match_batch_dev(0.7, False)
    c.sync()
    v = c.batch_view()
    xy = pkg.read_device(c, v.xy, (B, K, 2), np.float32)
    mc = pkg.read_device(c, v.match_count, (B,), np.int32)
    mf = pkg.read_device(c, v.match_from, (B, K), np.int32)
    mt = pkg.read_device(c, v.match_to, (B, K), np.int32)
    if depth_edit is not None:
        depth_edit(depth, xy, mc, mf, mt)
    d_depth = torch.from_numpy(depth.view(np.int16)).cuda()
    c.backproject_batch_dev(d_depth.data_ptr(), focal=CAM[:2], principal=CAM[2:])
    c.sync()
    pv = c.points_view()
    xyz = pkg.read_device(c, pv.xyz, (B, K, 3), np.float64)
    ok = pkg.read_device(c, pv.valid, (B, K), np.uint8)
    return c, shifts, (mc, mf, mt, xyz, ok), d_depth


def _align_view(pkg, c, B, K):
    av = c.align_view()
    return (pkg.read_device(c, av.pose, (B, 16), np.float64), pkg.read_device(c, av.n_points, (B,), np.int32),
            pkg.read_device(c, av.src_points, (B, K, 3), np.float32), pkg.read_device(c, av.dst_points, (B, K, 3), np.float32),
            pkg.read_device(c, av.inliers, (B, K), np.uint8))


def _host_gather(t, mc, mf, mt, xyz, ok):
    f, to = mf[t, :mc[t]], mt[t, :mc[t]]
    keep = (ok[t - 1, to] != 0) & (ok[t, f] != 0)
    return xyz[t - 1, to[keep]].astype(np.float32), xyz[t, f[keep]].astype(np.float32)


def test_gpu_align_batch_on_device_results(pkg):
    B, K, Z = 6, 4096, 2.0
    c, shifts, (mc, mf, mt, xyz, ok), keep_alive = _shifted_batch(pkg, B, K, Z)
    c.align_batch_dev(ar.MAX_DISTANCE, seed=40)
    c.sync()
    pose, npts, src, dst, inl = _align_view(pkg, c, B, K)
    assert c.align_view().capacity == K
    assert npts[0] == 0 and pose[0, 14] == 0.0                       # no predecessor inside the batch
    single = pkg.Context(width=0, height=0)
    for t in range(1, B):
        ref_src, ref_dst = _host_gather(t, mc, mf, mt, xyz, ok)
        n = int(npts[t])
        assert n == len(ref_src) and n > 300
        assert np.array_equal(src[t, :n], ref_src) and np.array_equal(dst[t, :n], ref_dst)
        assert pose[t, 14] == 1.0
        r1, t1, m1, rec = single.align_ransac(ref_src, ref_dst, ar.MAX_DISTANCE, seed=40 + t, record=True)
        assert np.array_equal(m1, inl[t, :n]) and np.array_equal(rec, pose[t])        # the same problem body: the same bits
        R, tv = pose[t, :9].reshape(3, 3), pose[t, 9:12]
        dx, dy = shifts[t][0] - shifts[t - 1][0], shifts[t][1] - shifts[t - 1][1]
        cos = np.clip((np.trace(R) - 1) / 2, -1, 1)
        assert np.degrees(np.arccos(cos)) < 0.2 and np.linalg.norm(tv - [-dx * Z / CAM[0], -dy * Z / CAM[1], 0]) < 0.01
        assert m1.sum() > 0.9 * n
    single.close()
    c.close()


def test_gpu_align_batch_frames_with_few_correspondences(pkg):
    """frames 1..4 keep 0, 1, 2 and 3 correspondences: the depth images of frames 0..4 are holes but for the pixels under
    both ends of the first few matches of each frame.  Status 0 on each — below 3 there is no problem, and 3 points never
    reach the floor of 4 inliers.  Frame 5 (full depth against frame 4's few valid pixels) is whatever the gather finds."""
    B, K, Z = 6, 4096, 2.0
    keep = {1: 0, 2: 1, 3: 2, 4: 3}

    def holes(depth, xy, mc, mf, mt):
        px = xy.astype(int)                                            # the depth lookup truncates

        def counts():
            out = [0]
            for t in range(1, 5):
                f, to = px[t, mf[t, :mc[t]]], px[t - 1, mt[t, :mc[t]]]
                out.append(int(((depth[t, f[:, 1], f[:, 0]] != 0) & (depth[t - 1, to[:, 1], to[:, 0]] != 0)).sum()))
            return out
        depth[:5] = 0
        target = [0] + [keep[t] for t in range(1, 5)]
        for t in range(1, 5):
            for j in range(mc[t]):                                     # matches in order, each kept only if it adds exactly itself
                if counts()[t] == keep[t]:
                    break
                f, to = px[t, mf[t, j]], px[t - 1, mt[t, j]]
                before = depth[t, f[1], f[0]], depth[t - 1, to[1], to[0]]
                depth[t, f[1], f[0]] = depth[t - 1, to[1], to[0]] = int(Z * 5000)
                now = counts()
                if any(n > w for n, w in zip(now, target)):
                    depth[t, f[1], f[0]], depth[t - 1, to[1], to[0]] = before
        assert counts() == target
    c, shifts, (mc, mf, mt, xyz, ok), keep_alive = _shifted_batch(pkg, B, K, Z, holes)
    c.align_batch_dev(ar.MAX_DISTANCE, seed=40)
    c.sync()
    pose, npts, src, dst, inl = _align_view(pkg, c, B, K)
    want = [len(_host_gather(t, mc, mf, mt, xyz, ok)[0]) if t else 0 for t in range(B)]
    print("correspondences per frame:", want)
    assert list(npts) == want and want[1:5] == [0, 1, 2, 3]
    for t in range(B):
        if want[t] <= 3:
            assert pose[t, 14] == 0.0 and pose[t, 12] == 0.0 and pose[t, 13] == -1.0 and not pose[t, :12].any(), t
            assert not inl[t, :want[t]].any()
    c.close()
