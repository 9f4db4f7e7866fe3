"""Tracking with the pose from RANSAC rigid alignment (mslam_hip_set_track_pose(ALIGN)) on the GPU, on
track_ref.make_sequence(): mslam_hip_track against tests/track_align_ref.py — equal pairs, counts, masks, flags and votes,
poses within 1e-9 (two closed forms of one optimum, no iteration between them), the new entry bit for bit once the
device's own pose is fed to the reference's construction — the loop through HipKeyframeTracker(track_pose=...), the window
forms against the per-frame calls, and the PNP setting giving back the bits of a context that never left it."""
import numpy as np
import pytest

import reloc_ref as rr
import track_align_ref as tar
import track_ref as tr
from reloc_ref import po

CAM = tr.CAM
DIST = 0.05
KF_MIN = tr.SEQ_PARAMS["new_keyframe_min_landmarks"]
pytestmark = pytest.mark.gpu
KINDS = pytest.mark.parametrize("kind", [0, 1], ids=["auto", "popcount"])
FIELDS = ("n_matches", "n_correspondences", "n_inliers", "status", "tracked", "keyframe_required", "vote_best", "vote_best_count")


def _ctx(pkg, kind=0, max_keypoints=1024, align=True):
    c = pkg.Context(width=0, height=0, max_keypoints=max_keypoints)
    c.set_matcher(kind)
    if align:
        c.set_track_pose("align", DIST)
    return c


def _rvec(R):
    th = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    if th < 1e-12:
        return np.zeros(3)
    return th / (2 * np.sin(th)) * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])


@pytest.fixture(scope="module")
def sequence(orc):
    seq = tr.make_sequence(seed=0)
    rows, trk = tar.run_reference(seq, DIST)
    # a condition of every comparison below: no point of any hypothesis the reference loop looked at lies within 1e-6 of the bound
    assert trk.margin >= 1e-6, trk.margin
    return seq, rows, trk


def _fill(c, store):
    for cid, (d, w) in store.items():
        c.kf_add(cid, d, w)


def _state(rows, trk, f):
    """the reference loop's state before frame f: the store, the reference, the vote list, the previous pose"""
    ids = [i for i in trk.ids if i <= max(r["keyframe"] for r in rows[:f])]
    return {i: trk.store[i] for i in ids}, rows[f - 1]["reference"], ids, (rows[f - 1]["R"], rows[f - 1]["t"])


def _compare_step(got, ref, what=""):
    assert np.array_equal(got["pairs"][0], ref["pairs"][0]) and np.array_equal(got["pairs"][1], ref["pairs"][1]), what
    assert (got["n_matches"], got["n_correspondences"]) == (ref["n_matches"], ref["n_correspondences"]), what
    assert got["status"] == ref["status"] and got["n_inliers"] == ref["n_inliers"], (what, got["n_inliers"], ref["n_inliers"])
    assert np.array_equal(got["inliers"], ref["mask"]), what
    if ref["status"]:
        dR, dt = np.abs(got["R"] - ref["R"]).max(), np.abs(got["tvec"] - ref["t"]).max()
        dr = np.abs(po.rodrigues(got["rvec"]) - ref["R"]).max()
        print(what, "inliers", got["n_inliers"], "pose difference", dR, dr, dt)
        assert dR <= 1e-9 and dt <= 1e-9, (what, dR, dt)
        assert dr <= 1e-9, (what, dr)
        assert abs(np.linalg.det(got["R"]) - 1) <= 1e-12
    else:
        assert not got["R"].any() and not got["rvec"].any() and not got["tvec"].any()
    assert bool(got["tracked"]) == ref["tracked"] and bool(got["keyframe_required"]) == ref["keyframe_required"], what
    assert np.array_equal(got["vote_counts"], ref["vote_counts"]), (what, got["vote_counts"], ref["vote_counts"])
    assert (got["vote_best"], got["vote_best_count"]) == (ref["vote_best"], ref["vote_best_count"]), what


def _compare_entry(c, got, ref, fr, store, ref_id, new_id, z_max=3.0):
    """the reference's construction fed with the device's own R, t: everything equal, world points bit for bit"""
    e = tr.build_entry(fr["desc"], ref["xyz"], ref["valid"], got["pairs"], got["inliers"], store[ref_id][1], got["R"],
                       got["tvec"], z_max)
    gd, gw = c.kf_read(new_id)
    assert (got["n_entry"], got["n_inherited"]) == (len(e["kp"]), e["n_inherited"]) and len(gd) == len(e["kp"])
    assert np.array_equal(got["entry_src"], e["src"]) and np.array_equal(got["entry_kp"], e["kp"])
    assert np.array_equal(gd, e["desc"])
    assert np.array_equal(gw.view(np.uint64), e["world"].view(np.uint64))
    assert 0 < e["n_inherited"] < len(e["kp"])


def _same_record(a, b, what):
    for k in FIELDS:
        assert a[k] == b[k], (what, k, a[k], b[k])
    for k in ("R", "rvec", "tvec"):
        assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), (what, k, np.abs(a[k] - b[k]).max())
    assert np.array_equal(a["vote_counts"], b["vote_counts"]), what


def test_reference_loop_tracks_the_sequence(sequence):
    """the reference loop itself: every frame tracked close to ground truth, keyframes on the way out, an older keyframe
    preferred on the way back"""
    seq, rows, trk = sequence
    tracked, inserted, switched = tr.summarize(rows)
    print("inserted", inserted, "switched", switched, "worst", max(r["err_deg"] for r in rows), max(r["err_m"] for r in rows))
    assert all(tracked) and len(inserted) >= 3 and len(switched) >= 1
    # depth quantised to 0.2 mm and f32 points: far inside a millimetre and a hundredth of a degree
    assert max(r["err_deg"] for r in rows) < 0.01 and max(r["err_m"] for r in rows) < 0.001


@KINDS
def test_align_single_steps_equal_the_reference(pkg, sequence, kind):
    """steps taken from the reference loop's state: one that only tracks, the ones that insert a keyframe, the one where the
    vote prefers an older keyframe"""
    seq, rows, trk = sequence
    tracked, inserted, switched = tr.summarize(rows)
    c = _ctx(pkg, kind)
    for f in [3] + inserted[1:3] + switched[:1]:
        fr = seq["frames"][f]
        store, ref_id, ids, guess = _state(rows, trk, f)
        c.kf_clear()
        _fill(c, store)
        new_id = 40 + f
        ref = tar.track(fr["desc"], fr["xy"], fr["depth"], store, ref_id, ids, max_distance=DIST, seed=f,
                        new_keyframe_min_landmarks=KF_MIN)
        assert ref["margin"] >= 1e-6
        got = c.track(fr["desc"], fr["xy"], fr["depth"], ref_id, ids, new_id, seed=f, rvec=_rvec(guess[0]), tvec=guess[1],
                      new_keyframe_min_landmarks=KF_MIN, with_pairs=True, with_entry=True)
        _compare_step(got, ref, (kind, f))
        assert c.last_match_kernel() == ("matrix", "popcount")[kind]
        assert got["tracked"] and got["n_correspondences"] < got["n_matches"]         # the depth filter cuts
        assert rr.rot_err(got["R"], fr["R"]) < 0.01 and np.linalg.norm(got["tvec"] - fr["t"]) < 0.001
        assert bool(got["keyframe_added"]) == (f in inserted)
        if got["keyframe_added"]:
            _compare_entry(c, got, ref, fr, store, ref_id, new_id)
            assert c.kf_size() == len(ids) + 1
        else:
            assert c.kf_size() == len(ids) and got["n_entry"] == 0
        if f in switched:
            assert ids[got["vote_best"]] != ref_id
        # the guess takes no part in the estimate, and reprojection_error is unused
        other = c.track(fr["desc"], fr["xy"], fr["depth"], ref_id, ids, -1, seed=f, reprojection_error=0.001,
                        new_keyframe_min_landmarks=KF_MIN, with_pairs=True)
        _same_record(other, got, "no guess")
        if got["keyframe_added"]:
            c.kf_remove(new_id)
    c.close()


@KINDS
def test_align_sequence_through_the_tracker_equals_the_reference_loop(pkg, sequence, kind):
    seq, rows, trk = sequence
    c = _ctx(pkg, kind, align=False)
    t = pkg.HipKeyframeTracker(c, focal=CAM[:2], principal=CAM[2:], track_pose=("align", DIST), **tr.SEQ_PARAMS)
    got = []
    for f, fr in enumerate(seq["frames"]):
        o = t.processSensorData(fr["desc"], fr["xy"], fr["depth"])
        assert c.get_track_pose() == (pkg.TRACK_POSE_PNP, 0.0)          # the tracker restores the context's setting
        o["err_deg"], o["err_m"] = rr.rot_err(o["R"], fr["R"]), float(np.linalg.norm(o["tvec"] - fr["t"]))
        print(f, "tracked", o["tracked"], "inliers", o["n_inliers"], "reference", o["reference"], "keyframe", o["keyframe"],
              "error %.5f deg %.6f m" % (o["err_deg"], o["err_m"]))
        got.append(o)
    assert tr.summarize(got) == tr.summarize(rows)
    assert [o["reference"] for o in got] == [r["reference"] for r in rows]
    assert [o["n_inliers"] for o in got] == [r["n_inliers"] for r in rows]
    for o, r in zip(got, rows):
        assert np.abs(o["R"] - r["R"]).max() <= 1e-9 and np.abs(o["tvec"] - r["t"]).max() <= 1e-9
    assert t.ids == trk.ids and c.kf_size() == len(trk.ids)
    c.close()
    with pytest.raises(pkg.MslamHipError):
        pkg.HipKeyframeTracker(c, track_pose=("align", 0.0))
    with pytest.raises(pkg.MslamHipError):
        pkg.HipKeyframeTracker(c, track_pose=("horn", 0.05))


@KINDS
def test_align_track_window_equals_the_per_frame_calls(pkg, sequence, kind):
    seq, rows, trk = sequence
    store, ref_id, ids, guess = _state(rows, trk, 1)
    frames = seq["frames"][1:9]                                  # frame 6 requires the keyframe: an event inside the window
    c = _ctx(pkg, kind)
    _fill(c, store)
    kw = dict(focal=CAM[:2], principal=CAM[2:], seed=1, rvec=_rvec(guess[0]), tvec=guess[1], new_keyframe_min_landmarks=KF_MIN)
    recs, first = c.track_window([x["desc"] for x in frames], [x["xy"] for x in frames], [x["depth"] for x in frames], ref_id, ids, 77,
                                 0, with_entry=True, **kw)
    assert len(recs) == len(frames)
    for s, fr in enumerate(frames):
        one = c.track(fr["desc"], fr["xy"], fr["depth"], ref_id, ids, -1, focal=CAM[:2], principal=CAM[2:], seed=1 + s,
                      rvec=kw["rvec"], tvec=kw["tvec"], new_keyframe_min_landmarks=KF_MIN)
        _same_record(recs[s], one, s)
    events = [s for s, r in enumerate(recs) if not r["tracked"] or r["keyframe_required"] or (r["vote_best"] not in (-1, 0))]
    assert first == (events[0] if events else len(frames)) and first < len(frames)
    assert recs[first]["keyframe_added"] and c.kf_size() == len(ids) + 1
    # the entry is the one the single call builds
    d_w, w_w = c.kf_read(77)
    c.kf_remove(77)
    fr = frames[first]
    one = c.track(fr["desc"], fr["xy"], fr["depth"], ref_id, ids, 78, focal=CAM[:2], principal=CAM[2:], seed=1 + first,
                  rvec=kw["rvec"], tvec=kw["tvec"], new_keyframe_min_landmarks=KF_MIN, with_entry=True)
    d_1, w_1 = c.kf_read(78)
    assert np.array_equal(d_w, d_1) and np.array_equal(w_w.view(np.uint64), w_1.view(np.uint64))
    assert np.array_equal(recs[first]["entry_src"], one["entry_src"]) and np.array_equal(recs[first]["entry_kp"], one["entry_kp"])
    c.close()


@KINDS
def test_align_track_window_dev_equals_the_host_form(pkg, kind):
    import torch
    import synth
    B, K = 8, 2048
    stream = synth.make_stream(B, 640, 480, seed=1234)
    depth = np.ascontiguousarray(synth.make_depth(B, 640, 480))
    c = pkg.Context(width=640, height=480, max_batch=B, max_keypoints=K)
    c.set_matcher(kind)
    c.set_track_pose("align", DIST)
    d_frames = torch.from_numpy(stream).cuda()
    d_depth = torch.from_numpy(depth.view(np.int16)).cuda()
    c.detect_batch_dev(d_frames.data_ptr(), B)
    c.backproject_batch_dev(d_depth.data_ptr(), focal=CAM[:2], principal=CAM[2:])
    c.kf_add_from_batch_dev(0, 0, np.eye(3), np.zeros(3), 3.0)
    c.sync()
    v = c.batch_view()
    cnt = pkg.read_device(c, v.count, (B,), np.int32)
    desc = pkg.read_device(c, v.desc, (B, K, 32), np.uint8)
    xy = pkg.read_device(c, v.xy, (B, K, 2), np.float32)
    kw = dict(focal=CAM[:2], principal=CAM[2:], seed=7, rvec=np.zeros(3), tvec=np.zeros(3), new_keyframe_min_landmarks=30)
    dev, dev_first = c.track_window_dev(1, 7, 0, [0], -1, 0, **kw)
    host, host_first = c.track_window([desc[f, :cnt[f]] for f in range(1, 8)], [xy[f, :cnt[f]] for f in range(1, 8)],
                                      [depth[f] for f in range(1, 8)], 0, [0], -1, 0, **kw)
    print("first", dev_first, [(r["n_matches"], r["n_correspondences"], r["n_inliers"], r["tracked"]) for r in dev])
    assert dev_first == host_first and len(dev) == len(host) == 7
    for s, (a, b) in enumerate(zip(dev, host)):
        _same_record(a, b, ("dev", s))
        one = c.track(desc[1 + s, :cnt[1 + s]], xy[1 + s, :cnt[1 + s]], depth[1 + s], 0, [0], -1, focal=CAM[:2], principal=CAM[2:],
                      seed=7 + s, rvec=np.zeros(3), tvec=np.zeros(3), new_keyframe_min_landmarks=30)
        _same_record(a, one, ("single", s))
    assert any(r["status"] for r in dev)
    c.close()


def test_align_outlier_depths_are_not_tracked(pkg, sequence):
    """every landmark keypoint's depth is off by 0.3 .. 1 m, each by its own amount: the correspondences are all there, no
    rigid transform explains four of them, the step is not tracked and the store stays as it was"""
    seq, rows, trk = sequence
    f = 6
    fr = seq["frames"][f]
    store, ref_id, ids, guess = _state(rows, trk, f)
    rng = np.random.default_rng(3)
    depth = fr["depth"].copy()
    lm = np.flatnonzero(fr["landmark"] >= 0)
    px = fr["xy"][lm].astype(np.float64).astype(np.int64)
    z = depth[px[:, 1], px[:, 0]].astype(np.int64)
    off = (rng.uniform(0.3, 1.0, len(lm)) * 5000).astype(np.int64) * rng.choice([-1, 1], len(lm))
    depth[px[:, 1], px[:, 0]] = np.where(z > 0, np.clip(z + off, 500, 20000), 0).astype(np.uint16)
    ref = tar.track(fr["desc"], fr["xy"], depth, store, ref_id, ids, max_distance=DIST, seed=f, new_keyframe_min_landmarks=KF_MIN)
    assert ref["n_correspondences"] > 50 and not ref["status"] and not ref["tracked"] and ref["margin"] >= 1e-6
    c = _ctx(pkg)
    _fill(c, store)
    snap = {i: c.kf_read(i) for i in ids}
    got = c.track(fr["desc"], fr["xy"], depth, ref_id, ids, 9, seed=f, rvec=_rvec(guess[0]), tvec=guess[1],
                  new_keyframe_min_landmarks=KF_MIN, with_pairs=True, with_entry=True)
    _compare_step(got, ref, "outlier depths")
    assert not got["tracked"] and not got["status"] and not got["keyframe_added"] and got["vote_best"] == -1 and got["n_inliers"] == 0
    assert c.kf_size() == len(snap)
    for i, (d, w) in snap.items():
        gd, gw = c.kf_read(i)
        assert np.array_equal(gd, d) and np.array_equal(gw, w), i
    c.close()


@KINDS
def test_back_to_pnp_gives_the_bits_of_a_fresh_context(pkg, sequence, kind):
    seq, rows, trk = sequence
    store, ref_id, ids, guess = _state(rows, trk, 1)
    frames = seq["frames"][1:5]
    kw = dict(focal=CAM[:2], principal=CAM[2:], seed=1, rvec=_rvec(guess[0]), tvec=guess[1], new_keyframe_min_landmarks=KF_MIN)

    def run(c):
        one = c.track(frames[2]["desc"], frames[2]["xy"], frames[2]["depth"], ref_id, ids, -1, with_pairs=True, **kw)
        win = c.track_window([x["desc"] for x in frames], [x["xy"] for x in frames], [x["depth"] for x in frames], ref_id, ids, -1, 0, **kw)
        return one, win
    fresh = _ctx(pkg, kind, align=False)
    _fill(fresh, store)
    want_one, (want_recs, want_first) = run(fresh)
    fresh.close()
    c = _ctx(pkg, kind, align=True)
    _fill(c, store)
    a_one, (a_recs, a_first) = run(c)                                   # under ALIGN: another estimate of the same pose
    assert a_one["status"] and not np.array_equal(a_one["R"], want_one["R"])
    assert np.abs(a_one["R"] - want_one["R"]).max() < 1e-3
    c.set_track_pose("pnp")
    got_one, (got_recs, got_first) = run(c)
    _same_record(got_one, want_one, "track")
    assert np.array_equal(got_one["inliers"], want_one["inliers"])
    assert got_first == want_first
    for s, (a, b) in enumerate(zip(got_recs, want_recs)):
        _same_record(a, b, ("window", s))
    c.close()


def test_relocalize_is_pnp_under_either_setting(pkg, sequence):
    seq, rows, trk = sequence
    store, ref_id, ids, guess = _state(rows, trk, 12)
    fr = seq["frames"][12]
    c = _ctx(pkg, align=False)
    _fill(c, store)
    want = c.relocalize(fr["desc"], fr["xy"], ids, CAM[:2], CAM[2:], seed=4, min_inliers=20, with_pairs=True)
    c.set_track_pose("align", DIST)
    got = c.relocalize(fr["desc"], fr["xy"], ids, CAM[:2], CAM[2:], seed=4, min_inliers=20, with_pairs=True)
    assert got["best"] == want["best"] >= 0
    for a, b in zip(got["candidates"], want["candidates"]):
        assert (a["n_matches"], a["n_correspondences"], a["n_inliers"], a["status"]) == (b["n_matches"], b["n_correspondences"],
                                                                                        b["n_inliers"], b["status"])
        assert np.array_equal(a["rvec"].view(np.uint64), b["rvec"].view(np.uint64))
        assert np.array_equal(a["tvec"].view(np.uint64), b["tvec"].view(np.uint64))
    for a, b in zip(got["inliers"], want["inliers"]):
        assert np.array_equal(a, b)
    c.close()
