"""HipKeyframeTracker(dense_icp=...) and dense_align on the GPU.  The sequence of tests/test_gpu_tsdf_tracker.py slides along a
sloping plane, which leaves an in-plane translation free, so this file has its own: a camera that moves a little in front of
the room corner of tests/tsdf_icp_ref.py (the "fine" volume and camera), landmarks on the corner's three planes, every tracked
frame a keyframe.  The numpy reference shows on the CPU that the frame the test blanks is constrained in all six degrees of
freedom by the volume of the keyframes before it.  One middle frame is given no keypoints: without the option the pose stays,
with it the pose is Context.tsdf_icp's, byte for byte, and nearer the true one.  A run in which every frame tracks is the same
with and without the option, and dense_align is the direct call."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_ref as tr  # noqa: E402
import tsdf_raycast_ref as rr  # noqa: E402
import tsdf_icp_ref as ir  # noqa: E402

pytestmark = pytest.mark.gpu

N_FRAMES, BLANK = 6, 3
EVERY_FRAME_A_KEYFRAME = dict(new_keyframe_min_landmarks=1 << 20)


def pose_of(f):
    return tr.rot(1, 0.012 * f) @ tr.rot(0, -0.008 * f) @ tr.rot(2, 0.01 * f), np.array([0.008 * f, -0.004 * f, 0.006 * f])


@pytest.fixture(scope="module")
def sequence():
    """-> dict(p, frames = [dict(desc, xy, depth, R, t)]): frame 0 is the world frame"""
    p, _ = ir.corner_scene("fine")
    fx, fy = p["focal"]
    cx, cy = p["principal"]
    rng = np.random.default_rng(7)
    N = ir.corner_normals()
    # landmarks: where random rays of the first camera meet the corner (the nearest of the three planes in front of it)
    uv = rng.uniform([2, 2], [p["width"] - 3, p["height"] - 3], (500, 2))
    d = np.stack([(uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy, np.ones(len(uv))], axis=1)
    s = (N.T @ ir.APEX)[None, :] / (d @ N)
    s = np.where(s > 0, s, np.inf).min(axis=1)
    L = d * s[:, None]
    ldesc = rng.integers(0, 256, (len(L), 32), dtype=np.uint8)
    frames = []
    for f in range(N_FRAMES):
        R, t = pose_of(f)
        c = L @ R.T + t
        img = np.stack([c[:, 0] / c[:, 2] * fx + cx, c[:, 1] / c[:, 2] * fy + cy], axis=1).astype(np.float32)
        inside = (c[:, 2] > 0) & (img[:, 0] >= 1) & (img[:, 0] < p["width"] - 2) & (img[:, 1] >= 1) & (img[:, 1] < p["height"] - 2)
        frames.append(dict(desc=ldesc[inside].copy(), xy=img[inside].copy(), depth=ir.render_corner(p, R, t), R=R, t=t))
    return dict(p=p, frames=frames)


def dense_of(p):
    return dict(dims=p["dims"], voxel=p["voxel"], origin=p["origin"], trunc=p["trunc"], max_depth=p["max_depth"], max_frames=64)


def run(pkg, seq, n, blank=None, window=None, **kw):
    p = seq["p"]
    c = pkg.Context(width=0, height=0, max_keypoints=4096)
    t = pkg.HipKeyframeTracker(c, focal=p["focal"], principal=p["principal"], factor=float(p["factor"]), dense_map=dense_of(p),
                               **dict(EVERY_FRAME_A_KEYFRAME, **kw))
    fr = [dict(f) for f in seq["frames"][:n]]
    if blank is not None and blank < n:
        fr[blank]["desc"], fr[blank]["xy"] = np.zeros((0, 32), np.uint8), np.zeros((0, 2), np.float32)
    if window is None:
        rows = [t.processSensorData(f["desc"], f["xy"], f["depth"]) for f in fr]
    else:
        rows = t.process_window([f["desc"] for f in fr], [f["xy"] for f in fr], [f["depth"] for f in fr], window=window)
    return c, t, rows


def err(row, f):
    return ir.pose_error(row["R"], row["tvec"], *pose_of(f))


def test_the_sequence_constrains_six_degrees_of_freedom(sequence):
    """on the CPU: the blanked frame against the volume of the keyframes before it, from the pose of the frame before it"""
    p, fr = sequence["p"], sequence["frames"]
    S, W = tr.fresh(p, [(f["depth"], f["R"], f["t"]) for f in fr[:BLANK]])
    guess = pose_of(BLANK - 1)
    _, xyz, nrm = rr.raycast(S, W, p, *guess)
    out = ir.solve(fr[BLANK]["depth"], ir.frame_camera(p), (xyz, nrm), rr.camera_of(p), *guess, *guess)
    e0, e1 = ir.pose_error(*guess, *pose_of(BLANK)), ir.pose_error(out["R"], out["t"], *pose_of(BLANK))
    print("reference: status %d, %d pairs, pivots %s; error %.2f mm / %.2f mrad -> %.2f mm / %.2f mrad"
          % (out["status"], out["count"], np.array2string(out["pivots"], precision=3), 1e3 * e0[0], 1e3 * e0[1], 1e3 * e1[0], 1e3 * e1[1]))
    assert out["status"] != ir.DEGENERATE and out["count"] > ir.MIN_PAIRS and np.all(out["pivots"] > 0)
    assert out["pivots"].min() / out["pivots"].max() > 1e-2    # the room corner of the issue's prototype: 2e-2
    assert e1[0] < e0[0] and e1[1] < e0[1]


@pytest.fixture(scope="module")
def runs(pkg, sequence):
    r = dict(plain=run(pkg, sequence, N_FRAMES, BLANK), icp=run(pkg, sequence, N_FRAMES, BLANK, dense_icp={}),
             before=run(pkg, sequence, BLANK), all_plain=run(pkg, sequence, N_FRAMES), all_icp=run(pkg, sequence, N_FRAMES, dense_icp={}))
    yield r
    for c, _, _ in r.values():
        c.close()


def test_a_frame_without_keypoints_is_aligned_to_the_model(pkg, runs, sequence):
    (_, _, plain), (_, _, icp), (cb, tb, before) = runs["plain"], runs["icp"], runs["before"]
    assert all(r["tracked"] for f, r in enumerate(plain) if f != BLANK) and not plain[BLANK]["tracked"]
    assert [r["keyframe"] for r in plain[:BLANK]] == list(range(BLANK))
    # without the option the pose stays
    assert plain[BLANK]["R"].tobytes() == plain[BLANK - 1]["R"].tobytes() and plain[BLANK]["tvec"].tobytes() == plain[BLANK - 1]["tvec"].tobytes()
    assert "dense_tracked" not in plain[BLANK] and "dense" not in plain[BLANK]
    # with it the frames before are the same, and the pose is the direct call's on the same volume from the same pose
    for f in range(BLANK):
        assert icp[f]["R"].tobytes() == plain[f]["R"].tobytes() and icp[f]["tvec"].tobytes() == plain[f]["tvec"].tobytes()
        assert "dense_tracked" not in icp[f]
    row = icp[BLANK]
    assert not row["tracked"] and row["dense_tracked"] is True and row["keyframe"] == -1
    direct = cb.tsdf_icp(sequence["frames"][BLANK]["depth"], before[-1]["R"], before[-1]["tvec"])
    assert direct["status"] != pkg.ICP_DEGENERATE
    assert row["R"].tobytes() == direct["R"].tobytes() and row["tvec"].tobytes() == direct["t"].tobytes()
    assert row["dense"]["R"].tobytes() == direct["R"].tobytes() and bytes(row["dense"]["result"]) == bytes(direct["result"])
    assert row["dense"]["record"].tobytes() == direct["record"].tobytes()
    assert np.allclose(pkg.rvec_to_rotation(row["rvec"]), row["R"], atol=1e-12)
    rms = math.sqrt(direct["cost"] / direct["count"])
    kept, aligned = err(plain[BLANK], BLANK), err(row, BLANK)
    print("blank frame: kept pose %.2f mm / %.2f mrad from the truth, aligned %.2f mm / %.2f mrad; rms %.2f mm over %d pairs"
          % (1e3 * kept[0], 1e3 * kept[1], 1e3 * aligned[0], 1e3 * aligned[1], 1e3 * rms, direct["count"]))
    assert rms <= sequence["p"]["voxel"]
    assert aligned[0] < kept[0] and aligned[1] < kept[1]
    # the store never saw the frame, and the frames after it track again
    assert runs["icp"][1].ids == runs["plain"][1].ids and all(r["tracked"] for r in icp[BLANK + 1:])


def test_a_rejected_alignment_keeps_the_pose(pkg, sequence):
    c, t, rows = run(pkg, sequence, BLANK + 1, BLANK, dense_icp=dict(max_rms=1e-9))
    row = rows[BLANK]
    assert row["dense_tracked"] is False and row["dense"]["status"] != pkg.ICP_DEGENERATE
    assert row["R"].tobytes() == rows[BLANK - 1]["R"].tobytes() and row["tvec"].tobytes() == rows[BLANK - 1]["tvec"].tobytes()
    c.close()


def test_windows_take_the_same_branch(pkg, runs, sequence):
    c, t, rows = run(pkg, sequence, N_FRAMES, BLANK, window=4, dense_icp={})
    assert rows[BLANK]["dense_tracked"] is True and not rows[BLANK]["tracked"]
    direct = c.tsdf_icp(sequence["frames"][BLANK]["depth"], rows[BLANK - 1]["R"], rows[BLANK - 1]["tvec"])
    # (the volume has gained keyframes since: only the run without them is byte-equal, the one of test_a_frame_...)
    assert direct["status"] != pkg.ICP_DEGENERATE
    assert all(r["tracked"] for f, r in enumerate(rows) if f != BLANK)
    c.close()


def test_the_option_changes_nothing_when_every_frame_tracks(runs):
    (c0, t0, a), (c1, t1, b) = runs["all_plain"], runs["all_icp"]
    assert all(r["tracked"] for r in a) and t0.ids == t1.ids and len(t0.ids) == N_FRAMES
    for f, (x, y) in enumerate(zip(a, b)):
        assert sorted(x) == sorted(y), f
        assert (x["tracked"], x["n_inliers"], x["keyframe"], x["reference"], x["relocalized"]) == \
               (y["tracked"], y["n_inliers"], y["keyframe"], y["reference"], y["relocalized"]), f
        assert x["R"].tobytes() == y["R"].tobytes() and x["tvec"].tobytes() == y["tvec"].tobytes() and x["rvec"].tobytes() == y["rvec"].tobytes(), f
    for k in t0.ids:
        assert c0.kf_read(k)[1].tobytes() == c1.kf_read(k)[1].tobytes()
    S0, W0 = c0.tsdf_read()
    S1, W1 = c1.tsdf_read()
    assert np.array_equal(S0, S1) and np.array_equal(W0, W1) and W0.any()


def test_dense_align_is_the_direct_call(pkg, runs, sequence):
    c, t, rows = runs["before"]
    depth = sequence["frames"][BLANK]["depth"]
    got = t.dense_align(depth)
    want = c.tsdf_icp(depth, rows[-1]["R"], rows[-1]["tvec"])
    assert got["R"].tobytes() == want["R"].tobytes() and got["t"].tobytes() == want["t"].tobytes()
    assert bytes(got["result"]) == bytes(want["result"]) and got["record"].tobytes() == want["record"].tobytes()
    assert t.R.tobytes() == rows[-1]["R"].tobytes()    # no state of the tracker changes
    other = t.dense_align(depth, np.eye(3), np.zeros(3), levels=((2, 3),), raycast=dict(coarse=1))
    want = c.tsdf_icp(depth, np.eye(3), np.zeros(3), levels=((2, 3),), raycast=dict(coarse=1))
    assert other["iterations"] == 3 and other["R"].tobytes() == want["R"].tobytes() and other["t"].tobytes() == want["t"].tobytes()
    with pytest.raises(pkg.MslamHipError) as e:
        t.dense_align(depth, R=np.eye(3))
    assert e.value.code == pkg.E_INVALID


def test_the_options_need_the_dense_map(pkg, sequence):
    p = sequence["p"]
    c = pkg.Context(width=0, height=0, max_keypoints=4096)
    with pytest.raises(pkg.MslamHipError) as e:
        pkg.HipKeyframeTracker(c, focal=p["focal"], principal=p["principal"], dense_icp={})
    assert e.value.code == pkg.E_INVALID
    with pytest.raises(pkg.MslamHipError) as e:
        pkg.HipKeyframeTracker(c, focal=p["focal"], principal=p["principal"], dense_map=dense_of(p), dense_icp=dict(rms=1.0))
    assert e.value.code == pkg.E_INVALID
    t = pkg.HipKeyframeTracker(c, focal=p["focal"], principal=p["principal"])
    f = sequence["frames"][0]
    t.processSensorData(f["desc"], f["xy"], f["depth"])
    with pytest.raises(pkg.MslamHipError) as e:
        t.dense_align(f["depth"])
    assert e.value.code == pkg.E_INVALID
    t2 = pkg.HipKeyframeTracker(c, focal=p["focal"], principal=p["principal"], dense_map=dense_of(p))
    with pytest.raises(pkg.MslamHipError) as e:
        t2.dense_align(f["depth"])    # before the first keyframe there is no volume yet
    assert e.value.code == pkg.E_INVALID
    c.close()
