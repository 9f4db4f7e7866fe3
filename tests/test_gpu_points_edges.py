"""The RGB-D point path at its edges: k_backproject, k_pack_plan, k_pack_copy (csrc/k_points.hip) and k_pnp_gather
(csrc/k_pnp.hip) against tests/points_ref.py and host-side restatements of the gather and of the packed layout.

Everything here is exact (bit-equal or integer-equal).  The only numeric bounds are conditions on the INPUTS (the share of
valid points, the share of holes), which tests/test_points_ref.py also checks on the CPU for the shared inputs."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import points_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import mslam_pnp_oracle as po  # noqa: E402

pytestmark = pytest.mark.gpu

TUM = (525.0, 525.0, 319.5, 239.5)
SENTINEL = 0xA5


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(width=0, height=0)
    yield c
    c.close()


def _raw(ctx, depth, xy, n, factor, focal, principal, xyz, valid):
    """the raw C call on the caller's own output arrays (Context.backproject allocates exact-size ones)"""
    depth = np.ascontiguousarray(depth, np.uint16)
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    h, w = depth.shape
    return ctx.L.mslam_hip_backproject(ctx._h, _ptr(depth), w, h, C.c_float(factor), C.c_double(focal[0]), C.c_double(focal[1]),
                                       C.c_double(principal[0]), C.c_double(principal[1]), _ptr(xy), int(n), _ptr(xyz), _ptr(valid))


# ---- 2. back-projection: single call ----------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", pr.SIZES)
def test_backproject_coordinate_edges(ctx, w, h):
    """random coordinates reaching 3 px outside every border + the edge list (NaN, +-inf, the truncation boundary, values no
    int holds) on depth images whose row 0 and column 0 have depth everywhere, non-TUM intrinsics, four factors"""
    depth = pr.make_depth(w, h, seed=w + h)
    xy = pr.make_coordinates(w, h, 3000, seed=3 * w + h)
    none = pr.has_no_depth(xy, w, h)
    assert none[3000:3003].all() and np.isnan(xy[3000:3003]).any(1).all()
    for factor in pr.FACTORS:
        ref_xyz, ref_ok = pr.backproject(depth, xy, factor, pr.FOCAL, pr.PRINCIPAL)
        if (w, h) != (1, 1):
            assert 0.05 < ref_ok.mean() < 0.95, ref_ok.mean()
        got_xyz, got_ok = ctx.backproject(depth, xy, factor, pr.FOCAL, pr.PRINCIPAL)
        bad = np.nonzero(got_ok != ref_ok)[0]
        assert len(bad) == 0, (factor, bad[:8], xy[bad[:8]])
        assert np.array_equal(_bits(got_xyz), _bits(ref_xyz)), factor
        # every coordinate without a depth pixel: invalid, and the point is +0.0 three times
        assert not got_ok[none].any() and not _bits(got_xyz[none]).any()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_backproject_block_edge_writes_n_rows_only(ctx, n):
    """n across the 256-lane block edge; rows >= n of a larger output buffer keep their sentinel"""
    w, h = 37, 23
    depth = pr.make_depth(w, h, seed=5)
    full = pr.make_coordinates(w, h, 600, seed=6)
    xy = np.concatenate([full[600:], full[:600]])[:n + 300]         # the edge list first
    xyz = np.full((n + 300, 3), np.nan, np.float64)
    xyz.view(np.uint8)[:] = SENTINEL
    valid = np.full(n + 300, SENTINEL, np.uint8)
    assert _raw(ctx, depth, xy, n, 1.0 / 5000.0, pr.FOCAL, pr.PRINCIPAL, xyz, valid) == 0
    ref_xyz, ref_ok = pr.backproject(depth, xy[:n], 1.0 / 5000.0, pr.FOCAL, pr.PRINCIPAL)
    assert np.array_equal(valid[:n], ref_ok.astype(np.uint8)) and np.array_equal(_bits(xyz[:n]), _bits(ref_xyz))
    assert (valid[n:] == SENTINEL).all() and (xyz[n:].view(np.uint8) == SENTINEL).all()


def test_backproject_factor_edges(ctx):
    """depth * factor exactly at FLT_EPSILON (invalid), one ulp above (valid), negative, NaN, +inf (z = inf; 0 * inf is
    NaN: invalid) and a denormal factor.  (x - cx and y - cy are nonzero here, so no valid point holds a NaN.)"""
    xy = np.array([(0.5, 0), (1.5, 0), (2.5, 0), (3.5, 0)], np.float32)
    for factor, want in zip(pr.FACTOR_EDGES, pr.FACTOR_EDGES_VALID):
        ref_xyz, ref_ok = pr.backproject(pr.FACTOR_EDGE_DEPTH, xy, factor, pr.FOCAL, pr.PRINCIPAL)
        assert list(ref_ok) == want and not np.isnan(ref_xyz).any()
        got_xyz, got_ok = ctx.backproject(pr.FACTOR_EDGE_DEPTH, xy, factor, pr.FOCAL, pr.PRINCIPAL)
        assert list(got_ok) == want, (factor, got_ok)
        assert np.array_equal(_bits(got_xyz), _bits(ref_xyz)), (factor, got_xyz, ref_xyz)


def test_backproject_argument_errors_and_empty_call(pkg, ctx):
    depth = pr.make_depth(37, 23, seed=5)
    xy = pr.make_coordinates(37, 23, 10, seed=6)
    for focal in ((0.0, 500.0), (500.0, 0.0), (float("nan"), 500.0), (500.0, float("nan"))):
        with pytest.raises(pkg.MslamHipError) as e:
            ctx.backproject(depth, xy, focal=focal)
        assert e.value.code == pkg.E_INVALID
    xyz = np.full((4, 3), np.nan, np.float64)
    xyz.view(np.uint8)[:] = SENTINEL
    valid = np.full(4, SENTINEL, np.uint8)
    assert _raw(ctx, depth, xy, 0, 1.0 / 5000.0, pr.FOCAL, pr.PRINCIPAL, xyz, valid) == 0      # n == 0: OK, nothing written
    assert (valid == SENTINEL).all() and (xyz.view(np.uint8) == SENTINEL).all()
    assert _raw(ctx, depth, xy, -1, 1.0 / 5000.0, pr.FOCAL, pr.PRINCIPAL, xyz, valid) == pkg.E_INVALID
    got_xyz, got_ok = ctx.backproject(depth, xy, focal=pr.FOCAL, principal=pr.PRINCIPAL)      # the context still works
    ref_xyz, ref_ok = pr.backproject(depth, xy, focal=pr.FOCAL, principal=pr.PRINCIPAL)
    assert np.array_equal(got_ok, ref_ok) and np.array_equal(_bits(got_xyz), _bits(ref_xyz))


# ---- 2. back-projection: the batch entry --------------------------------------------------------------------------------
def test_backproject_batch_odd_size_partial_batch_and_empty_frame(pkg, orc):
    """333 x 207 (no multiple of anything), max_keypoints = 1000 (no multiple of the 256-lane block), 3 frames of a 4-frame
    context, a flat frame in the middle: rows [:count[t]] equal the reference on the oracle's keypoints; rows beyond
    count[t] and the unused frame slot keep what they held"""
    import torch
    import synth
    W, H, B, K = 333, 207, 4, 1000
    frames = synth.make_stream(3, W, H, seed=99)
    frames[1] = 128
    depth = synth.make_depth(3, W, H)
    assert 0.03 < (depth == 0).mean() < 0.08
    c = pkg.Context(width=W, height=H, max_batch=B, max_keypoints=K, max_candidates=65536)
    c.detect_batch_dev(torch.from_numpy(frames).cuda().data_ptr(), 3)
    fill = torch.from_numpy(np.full((3, H, W), 7000, np.uint16).view(np.int16)).cuda()
    c.backproject_batch_dev(fill.data_ptr(), focal=pr.FOCAL, principal=pr.PRINCIPAL)
    c.sync()
    v, pv = c.batch_view(), c.points_view()
    assert pv.capacity == K
    cnt = pkg.read_device(c, v.count, (3,), np.int32)
    xy = pkg.read_device(c, v.xy, (3, K, 2), np.float32)
    before_xyz = pkg.read_device(c, pv.xyz, (B, K, 3), np.float64)
    before_ok = pkg.read_device(c, pv.valid, (B, K), np.uint8)
    for t in (0, 2):                                     # the fill itself: every point valid at z = 7000 / 5000
        assert cnt[t] > 100 and (before_ok[t, :cnt[t]] == 1).all() and (before_xyz[t, :cnt[t], 2] == float(np.float32(7000) * np.float32(1.0 / 5000.0))).all()
    d_depth = torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).cuda()
    c.backproject_batch_dev(d_depth.data_ptr(), focal=pr.FOCAL, principal=pr.PRINCIPAL)
    c.sync()
    xyz = pkg.read_device(c, pv.xyz, (B, K, 3), np.float64)
    ok = pkg.read_device(c, pv.valid, (B, K), np.uint8)
    assert cnt[1] == 0
    holes = 0
    for t in range(3):
        det = orc.detect(frames[t], orc.params())
        n = int(cnt[t])
        assert n == len(det["xy"]) and np.array_equal(xy[t, :n], det["xy"])
        ref_xyz, ref_ok = pr.backproject(depth[t], det["xy"], 1.0 / 5000.0, pr.FOCAL, pr.PRINCIPAL)
        assert np.array_equal(ok[t, :n], ref_ok.astype(np.uint8)) and np.array_equal(_bits(xyz[t, :n]), _bits(ref_xyz)), t
        holes += int((~ref_ok).sum())
        assert np.array_equal(ok[t, n:], before_ok[t, n:]) and np.array_equal(_bits(xyz[t, n:]), _bits(before_xyz[t, n:])), t
    assert holes > 0
    assert np.array_equal(ok[3], before_ok[3]) and np.array_equal(_bits(xyz[3]), _bits(before_xyz[3]))
    for focal in ((0.0, 500.0), (500.0, float("nan"))):      # refused before anything is launched
        with pytest.raises(pkg.MslamHipError) as e:
            c.backproject_batch_dev(d_depth.data_ptr(), focal=focal)
        assert e.value.code == pkg.E_INVALID
    c.close()


# ---- 4. holes through the PnP gather -----------------------------------------------------------------------------------
def _rot_err(Ra, Rb):
    return np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))


def _plane_batch(pkg, depth, seed):
    """the geometry of test_pnp.py's batched test (a plane at 2 m, whole-pixel shifts, B = 4) on `depth`: detect, match,
    back-project and PnP on the device -> host copies of everything the checks need"""
    import torch
    import synth
    B, K = 4, 4096
    base = synth.make_stream(1, 640 + 64, 480 + 48, seed=11)[0]
    shifts = [(3 * t, 2 * t) for t in range(B)]
    frames = np.stack([np.ascontiguousarray(base[dy:dy + 480, dx:dx + 640]) for dx, dy in shifts])
    c = pkg.Context(width=640, height=480, max_batch=B, max_keypoints=K)
    c.detect_batch_dev(torch.from_numpy(frames).cuda().data_ptr(), B)
    c.match_batch_dev(0.7, False)
    d_depth = torch.from_numpy(depth.view(np.int16)).cuda()
    c.backproject_batch_dev(d_depth.data_ptr(), focal=TUM[:2], principal=TUM[2:])
    c.pnp_batch_dev(TUM[:2], TUM[2:], seed=seed)
    c.sync()
    v, pv, nv = c.batch_view(), c.points_view(), c.pnp_view()
    out = dict(shifts=shifts,
               cnt=pkg.read_device(c, v.count, (B,), np.int32), xy=pkg.read_device(c, v.xy, (B, K, 2), np.float32),
               mc=pkg.read_device(c, v.match_count, (B,), np.int32), mf=pkg.read_device(c, v.match_from, (B, K), np.int32),
               mt=pkg.read_device(c, v.match_to, (B, K), np.int32),
               xyz=pkg.read_device(c, pv.xyz, (B, K, 3), np.float64), ok=pkg.read_device(c, pv.valid, (B, K), np.uint8),
               pose=pkg.read_device(c, nv.pose, (B, 16), np.float64), npts=pkg.read_device(c, nv.n_points, (B,), np.int32),
               obj=pkg.read_device(c, nv.object_points, (B, K, 3), np.float32),
               img=pkg.read_device(c, nv.image_points, (B, K, 2), np.float32), inl=pkg.read_device(c, nv.inliers, (B, K), np.uint8))
    c.close()
    return out


def _host_gather(o, depth, t):
    """frame t's correspondences in match order, from the REFERENCE back-projection of the device's keypoints of frame t-1
    (not from the device's own valid flags)"""
    n_prev = int(o["cnt"][t - 1])
    ref_xyz, ref_ok = pr.backproject(depth[t - 1], o["xy"][t - 1, :n_prev], 1.0 / 5000.0, TUM[:2], TUM[2:])
    assert np.array_equal(o["ok"][t - 1, :n_prev], ref_ok.astype(np.uint8)) and np.array_equal(_bits(o["xyz"][t - 1, :n_prev]), _bits(ref_xyz))
    mf, mt = o["mf"][t, :o["mc"][t]], o["mt"][t, :o["mc"][t]]
    assert mt.max(initial=-1) < n_prev and mf.max(initial=-1) < o["cnt"][t]
    keep = ref_ok[mt]
    return keep, ref_xyz[mt[keep]].astype(np.float32), o["xy"][t, mf[keep]]


def _check_pose(single, o, t, seed, ref_obj, ref_img, Z=2.0):
    n = int(o["npts"][t])
    pose = o["pose"][t]
    assert pose[14] == 1.0
    R, tv = pose[:9].reshape(3, 3), pose[9:12]
    r1, t1, m1 = single.pnp_ransac(ref_obj, ref_img, TUM[:2], TUM[2:], seed=seed + t)
    assert np.array_equal(m1, o["inl"][t, :n]) and int(pose[12]) == int(m1.sum())
    assert np.abs(po.rodrigues(r1) - R).max() < 1e-9 and np.array_equal(t1, tv)
    dx, dy = o["shifts"][t][0] - o["shifts"][t - 1][0], o["shifts"][t][1] - o["shifts"][t - 1][1]
    assert _rot_err(R, np.eye(3)) < 0.2 and np.linalg.norm(tv - [-dx * Z / TUM[0], -dy * Z / TUM[1], 0]) < 0.01
    assert m1.sum() > 0.9 * n


def test_pnp_gather_drops_holes_in_match_order(pkg):
    """30 % of the depth pixels are 0: about 30 % of every frame's matches have no 3-D point and the compaction (ballot,
    four-wave prefix, `running` across 256-match chunks) has to close the gaps.  The plane is unchanged where it has
    depth, so the ground-truth pose is too."""
    B, Z = 4, 2.0
    depth = np.full((B, 480, 640), int(Z * 5000), np.uint16)
    depth[np.random.default_rng(5).random(depth.shape) < 0.3] = 0
    o = _plane_batch(pkg, depth, seed=40)
    assert o["npts"][0] == 0 and o["pose"][0, 14] == 0.0
    single = pkg.Context(width=0, height=0)
    for t in range(1, B):
        keep, ref_obj, ref_img = _host_gather(o, depth, t)
        assert o["mc"][t] > 512                                           # `running` carries over at least two chunks
        assert 0.15 < 1.0 - keep.mean() < 0.5, (t, keep.mean())           # a condition on the input
        assert (~keep[:256]).any() and (~keep[256:512]).any()             # holes in each of the first two chunks
        n = int(o["npts"][t])
        assert n == len(ref_obj) and n > 300
        assert np.array_equal(o["obj"][t, :n], ref_obj) and np.array_equal(o["img"][t, :n], ref_img), t
        _check_pose(single, o, t, 40, ref_obj, ref_img)
    single.close()


def test_pnp_gather_frame_without_any_depth(pkg):
    """frame 1 has no depth at all (its keypoints and matches are all there): frame 2 gathers nothing — n_points 0, status
    0 and the all-zero pose of a frame without a model — and frame 3 recovers"""
    B, Z = 4, 2.0
    depth = np.full((B, 480, 640), int(Z * 5000), np.uint16)
    depth[np.random.default_rng(6).random(depth.shape) < 0.3] = 0
    depth[1] = 0
    o = _plane_batch(pkg, depth, seed=40)
    single = pkg.Context(width=0, height=0)
    assert o["cnt"].min() > 1000 and o["mc"][1:].min() > 512
    assert not o["ok"][1, :o["cnt"][1]].any() and not _bits(o["xyz"][1, :o["cnt"][1]]).any()
    for t in (0, 2):
        pose = o["pose"][t]
        assert o["npts"][t] == 0 and pose[14] == 0.0 and not pose[:13].any() and pose[13] == -1.0, (t, pose)
    for t in (1, 3):
        keep, ref_obj, ref_img = _host_gather(o, depth, t)
        n = int(o["npts"][t])
        assert n == len(ref_obj) and n > 300
        assert np.array_equal(o["obj"][t, :n], ref_obj) and np.array_equal(o["img"][t, :n], ref_img), t
        _check_pose(single, o, t, 40, ref_obj, ref_img)
    single.close()


# ---- 5. packed results --------------------------------------------------------------------------------------------------
def _al(x):
    return (x + 15) & ~15


def _layout(pkg, cnt, mc, with_points):
    """the packed layout recomputed on the host from the counts (include/mslam_hip.h: header, two offset tables, then the
    sections in header order, each starting on a 16-byte boundary)"""
    n = len(cnt)
    nk, nm = int(cnt.sum()), int(mc.sum())
    hdr, tab = _al(C.sizeof(pkg.PackedHeader)), _al((n + 1) * 4)
    L = dict(hdr=hdr, tab=tab, n_frames=n, total_keypoints=nk, total_matches=nm, with_points=int(with_points),
             off_kp_offset=hdr, off_match_offset=hdr + tab)
    o = hdr + 2 * tab
    for name, size in (("off_xy", nk * 8), ("off_desc", nk * 32), ("off_octave", nk * 4), ("off_angle", nk * 4),
                       ("off_response", nk * 4), ("off_xyz", nk * 24 if with_points else 0), ("off_valid", nk if with_points else 0),
                       ("off_match_from", nm * 4), ("off_match_to", nm * 4)):
        L[name] = o
        o = _al(o + size)
    L["bytes"] = o
    return L


def _header(pkg, buf):
    return pkg.PackedHeader.from_buffer_copy(bytes(buf[:C.sizeof(pkg.PackedHeader)]))


def _assert_header(pkg, buf, L, fits):
    h = _header(pkg, buf)
    for k, want in L.items():
        if k not in ("hdr", "tab"):
            assert getattr(h, k) == want, (k, getattr(h, k), want)
    assert h.fits == fits and h.pad == 0
    return h


def test_packed_batch_beyond_1024_frames_and_capacity_boundaries(pkg, orc):
    """1500 frames in one batch: k_pack_plan's scan runs two 1024-frame chunks and carries the totals between them; frames
    without keypoints at both ends, on both sides of the chunk boundary and inside; then the capacity boundaries"""
    import torch
    import synth
    W, H, B, K = 100, 80, 1500, 256
    kw = dict(n_levels=3, ini_fast_thr=10, min_fast_thr=3, min_node_area=10)
    src = synth.make_stream(6, W, H, seed=99).astype(np.int16) + np.random.default_rng(7).integers(-25, 26, (6, H, W, 3))
    src = np.concatenate([np.clip(src, 0, 255).astype(np.uint8), np.full((1, H, W, 3), 128, np.uint8)])
    FLAT = 6
    idx = (np.arange(B) * 5 + np.arange(B) // 7) % 6
    flat_at = [0, 17, 500, 501, 1023, 1024, 1100, 1499]
    idx[flat_at] = FLAT
    idx[[300, 301, 1200, 1201]] = [2, 2, 4, 4]                       # identical consecutive frames: every keypoint matches
    refs = [orc.detect(f, orc.params(n_levels=3, ini_fast_thr=10, min_fast_thr=3, min_size=10)) for f in src]
    ref_cnt = np.array([len(r["xy"]) for r in refs], np.int32)
    assert ref_cnt[FLAT] == 0 and ref_cnt[:6].min() > 100 and ref_cnt.max() <= K and len(set(ref_cnt)) >= 5
    frames = torch.from_numpy(np.ascontiguousarray(src[idx])).cuda()
    depth = synth.make_depth(1, W, H)[0]
    d_depth = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(depth, (B, H, W))).view(np.int16)).cuda()

    c = pkg.Context(width=W, height=H, max_batch=B, max_keypoints=K, max_candidates=2048, **kw)
    c.detect_batch_dev(frames.data_ptr(), B)
    c.match_batch_dev(0.7, True)
    c.backproject_batch_dev(d_depth.data_ptr(), focal=pr.FOCAL, principal=pr.PRINCIPAL)
    cap = c.packed_capacity(B)
    buf = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    c.pack_batch_dev(buf.data_ptr(), cap, True)
    c.sync()
    host = buf.cpu().numpy()
    p = pkg.unpack_batch(host)
    v, pv = c.batch_view(), c.points_view()
    cnt = pkg.read_device(c, v.count, (B,), np.int32)
    mc = pkg.read_device(c, v.match_count, (B,), np.int32)
    # detection above 1024 frames: every frame has its source frame's count and keypoints
    assert np.array_equal(cnt, ref_cnt[idx])
    assert mc[0] == 0 and mc[301] > 0.9 * cnt[301] and mc[1201] > 0.9 * cnt[1201] and mc.sum() > 10000
    for t in flat_at:
        assert mc[t] == 0 and (t + 1 == B or mc[t + 1] == 0)
    pair_kinds = {}
    for t in range(1, B):                                # the pair (t, t-1) depends on (idx[t], idx[t-1]) only
        key = (idx[t], idx[t - 1])
        if key not in pair_kinds:
            pair_kinds[key] = len(orc.match(refs[key[0]]["desc"], refs[key[1]]["desc"])[0])
        assert mc[t] == pair_kinds[key], (t, key)

    # offsets: exclusive sums of the counts, across the 1024-frame chunk boundary
    kp_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    m_off = np.concatenate([[0], np.cumsum(mc)]).astype(np.int32)
    assert p["kp_offset"].dtype == np.int32 and np.array_equal(p["kp_offset"], kp_off) and np.array_equal(p["match_offset"], m_off)
    for t in (1023, 1024, 1025, 1500):
        assert p["kp_offset"][t] == kp_off[t] and p["match_offset"][t] == m_off[t], t
    assert kp_off[1024] > 100000 and m_off[1024] > 5000
    for t in flat_at:
        assert p["kp_offset"][t] == p["kp_offset"][t + 1] and p["match_offset"][t] == p["match_offset"][t + 1]
    L = _layout(pkg, cnt, mc, True)
    h = _assert_header(pkg, host, L, fits=1)
    assert p["n_frames"] == B and h.bytes == L["bytes"] <= cap and L["bytes"] % 16 == 0

    # records: byte-identical to the capacity-strided views, frame by frame
    full = {"xy": pkg.read_device(c, v.xy, (B, K, 2), np.float32), "desc": pkg.read_device(c, v.desc, (B, K, 32), np.uint8),
            "octave": pkg.read_device(c, v.octave, (B, K), np.int32), "angle": pkg.read_device(c, v.angle, (B, K), np.float32),
            "response": pkg.read_device(c, v.response, (B, K), np.float32), "xyz": pkg.read_device(c, pv.xyz, (B, K, 3), np.float64),
            "valid": pkg.read_device(c, pv.valid, (B, K), np.uint8)}
    mf = pkg.read_device(c, v.match_from, (B, K), np.int32)
    mt = pkg.read_device(c, v.match_to, (B, K), np.int32)

    def assert_records(p, with_points=True):
        for t in range(B):
            a, b = kp_off[t], kp_off[t + 1]
            for k, arr in full.items():
                if with_points or k not in ("xyz", "valid"):
                    assert np.array_equal(p[k][a:b].view(np.uint8), arr[t, :cnt[t]].view(np.uint8)), (t, k)
            a, b = m_off[t], m_off[t + 1]
            assert np.array_equal(p["match_from"][a:b], mf[t, :mc[t]]) and np.array_equal(p["match_to"][a:b], mt[t, :mc[t]]), t
    assert_records(p)
    for r in range(6):                                   # and the views themselves: the oracle's keypoints, the reference's points
        t = int(np.nonzero(idx == r)[0][-1])             # (the last frame of each kind: five of the six lie beyond frame 1024)
        n = int(cnt[t])
        assert np.array_equal(full["xy"][t, :n], refs[r]["xy"]) and np.array_equal(full["desc"][t, :n], refs[r]["desc"])
        ref_xyz, ref_ok = pr.backproject(depth, refs[r]["xy"], 1.0 / 5000.0, pr.FOCAL, pr.PRINCIPAL)
        assert np.array_equal(full["valid"][t, :n], ref_ok.astype(np.uint8)) and np.array_equal(_bits(full["xyz"][t, :n]), _bits(ref_xyz))
    assert 0 < full["valid"][idx != FLAT, :100].mean() < 1

    def pack(capacity, with_points, size):
        """pack into a fresh sentinel-filled buffer of `size` bytes with `capacity` declared -> (host copy, sync() error code)"""
        b = torch.full((size,), SENTINEL, dtype=torch.uint8, device="cuda")
        c.pack_batch_dev(b.data_ptr(), capacity, with_points)
        try:
            c.sync()
            code = 0
        except pkg.MslamHipError as e:
            code = e.code
        return b.cpu().numpy(), code

    # with_points = 0: the two point sections are empty
    L0 = _layout(pkg, cnt, mc, False)
    got, code = pack(L0["bytes"], False, L0["bytes"] + 64)
    assert code == 0
    h0 = _assert_header(pkg, got, L0, fits=1)
    assert h0.off_xyz == h0.off_valid == h0.off_match_from and L0["bytes"] < L["bytes"]
    p0 = pkg.unpack_batch(got)
    assert "xyz" not in p0 and "valid" not in p0
    assert_records(p0, with_points=False)
    assert (got[L0["bytes"]:] == SENTINEL).all()

    # capacity == bytes: fits, the same records, nothing behind them
    need = L["bytes"]
    got, code = pack(need, True, need + 64)
    assert code == 0
    _assert_header(pkg, got, L, fits=1)
    assert_records(pkg.unpack_batch(got))
    assert (got[need:] == SENTINEL).all()

    def assert_packs_again():
        got, code = pack(cap, True, cap)
        assert code == 0
        _assert_header(pkg, got, L, fits=1)
        q = pkg.unpack_batch(got)
        for k in p:
            assert np.array_equal(q[k], p[k]), k

    # capacity == bytes - 1: refused; the header still says what is needed, the tables are written, no record is
    got, code = pack(need - 1, True, need + 64)
    assert code == pkg.E_CAPACITY
    _assert_header(pkg, got, L, fits=0)
    with pytest.raises(pkg.MslamHipError):
        pkg.unpack_batch(got)
    assert np.array_equal(np.frombuffer(got, np.int32, B + 1, L["off_kp_offset"]), kp_off)
    assert np.array_equal(np.frombuffer(got, np.int32, B + 1, L["off_match_offset"]), m_off)
    assert (got[L["hdr"] + 2 * L["tab"]:] == SENTINEL).all()
    assert_packs_again()

    # the header fits, the two tables do not (by one byte): only the header is written
    got, code = pack(L["hdr"] + 2 * L["tab"] - 1, True, need + 64)
    assert code == pkg.E_CAPACITY
    _assert_header(pkg, got, L, fits=0)
    assert (got[C.sizeof(pkg.PackedHeader):] == SENTINEL).all()
    assert_packs_again()

    # exactly the header: the smallest capacity the call takes; one byte less is an argument error
    got, code = pack(C.sizeof(pkg.PackedHeader), True, 4096)
    assert code == pkg.E_CAPACITY
    _assert_header(pkg, got, L, fits=0)
    assert (got[C.sizeof(pkg.PackedHeader):] == SENTINEL).all()
    with pytest.raises(pkg.MslamHipError) as e:
        c.pack_batch_dev(buf.data_ptr(), C.sizeof(pkg.PackedHeader) - 1, True)
    assert e.value.code == pkg.E_INVALID
    assert_packs_again()
    c.close()
