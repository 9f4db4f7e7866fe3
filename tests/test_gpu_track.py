"""The keyframe tracking step on the GPU, through the C ABI: mslam_hip_kf_visible and mslam_hip_track against the numpy
composition of tests/track_ref.py — equal pairs, counts, masks, flags and votes, poses within 1e-7 (the PnP kernel against
its hypothesis-sequence oracle, the bound tests/test_gpu_reloc.py uses), the new entry bit for bit once the device's own
pose is fed to the reference's construction — with both matcher kinds where matching is involved."""
import numpy as np
import pytest

import reloc_ref as rr
import track_ref as tr
from reloc_ref import po

CAM = tr.CAM
pytestmark = pytest.mark.gpu
KINDS = pytest.mark.parametrize("kind", [0, 1], ids=["auto", "popcount"])


def _ctx(pkg, kind=0, max_keypoints=1024):
    c = pkg.Context(width=0, height=0, max_keypoints=max_keypoints)
    c.set_matcher(kind)
    return c


def _rvec(R):
    th = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    if th < 1e-12:
        return np.zeros(3)
    return th / (2 * np.sin(th)) * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])


@pytest.fixture(scope="module")
def sequence(orc):
    seq = tr.make_sequence(seed=0)
    rows, trk = tr.run_reference(seq)
    return seq, rows, trk


def _fill(c, store):
    for cid, (d, w) in store.items():
        c.kf_add(cid, d, w)


def _snapshot(c, ids):
    return {i: c.kf_read(i) for i in ids}


def _same_store(c, snap):
    assert c.kf_size() == len(snap)
    for i, (d, w) in snap.items():
        gd, gw = c.kf_read(i)
        assert np.array_equal(gd, d) and np.array_equal(gw, w), i


def _compare_step(got, ref, what=""):
    assert np.array_equal(got["pairs"][0], ref["pairs"][0]) and np.array_equal(got["pairs"][1], ref["pairs"][1]), what
    assert (got["n_matches"], got["n_correspondences"]) == (ref["n_matches"], ref["n_correspondences"]), what
    assert got["status"] == ref["status"] and got["n_inliers"] == ref["n_inliers"], (what, got["n_inliers"], ref["n_inliers"])
    assert np.array_equal(got["inliers"], ref["mask"]), what
    if ref["status"]:
        dR, dt = np.abs(got["R"] - ref["R"]).max(), np.abs(got["tvec"] - ref["t"]).max()
        dr = np.abs(po.rodrigues(got["rvec"]) - ref["R"]).max()
        print(what, "inliers", got["n_inliers"], "pose difference", dR, dr, dt)
        assert dR < 1e-7 and dr < 1e-7 and dt < 1e-7, (what, dR, dr, dt)
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
    na = e["n_inherited"]
    assert np.array_equal(gw[:na].view(np.uint64), e["world"][:na].view(np.uint64))       # inherited
    assert np.array_equal(gw[na:].view(np.uint64), e["world"][na:].view(np.uint64))       # lifted
    assert 0 < na < len(e["kp"])
    return e


def test_kf_visible_equals_the_reference(pkg):
    rng = np.random.default_rng(11)
    c = _ctx(pkg, max_keypoints=2048)
    store = {}
    for i in range(70):
        n = (0, 1, 2048, 63, 64, 65, 255, 256, 257)[i] if i < 9 else int(rng.integers(0, 900))
        store[100 + i] = (rng.integers(0, 256, (n, 32), dtype=np.uint8),
                          np.stack([rng.uniform(-4, 4, n), rng.uniform(-3, 3, n), rng.uniform(-1, 6, n)], 1))
    # the boundary cases of tests/test_track.py::test_vote_hand_cases, with the camera they are exact for
    hand_cam = (500.0, 500.0, 320.0, 240.0)
    pts = np.array([[0.0, 0.0, 2.0], [0.0, 0.0, -2.0], [-1.28, 0.0, 2.0], [1.28, 0.0, 2.0], [0.0, -0.96, 2.0], [0.0, 0.96, 2.0],
                    [0.0, 0.0, 0.0]])
    store[7] = (np.zeros((len(pts), 32), np.uint8), pts)
    for k, p in enumerate(pts):
        store[10 + k] = (np.zeros((1, 32), np.uint8), p[None].copy())
    _fill(c, store)
    counts, best = c.kf_visible([7] + [10 + k for k in range(len(pts))], np.eye(3), np.zeros(3), hand_cam[:2], hand_cam[2:])
    assert counts.tolist() == [3, 1, 0, 1, 0, 1, 0, 0] and best == 0
    rc, rb = tr.vote(store, [7] + [10 + k for k in range(len(pts))], np.eye(3), np.zeros(3), hand_cam)
    assert counts.tolist() == rc.tolist() and best == rb
    # random poses, lists of 1, 8 and 64 ids (entries of 0 landmarks among them)
    ids = sorted(i for i in store if i >= 100)
    for trial in range(6):
        R = po.rodrigues(rng.normal(size=3) * 0.4)
        t = rng.normal(size=3) * 0.5
        for lst in (ids[:1], ids[:8], ids[:64], ids[6:70], [ids[0]], [ids[0], ids[0]]):
            counts, best = c.kf_visible(lst, R, t, CAM[:2], CAM[2:], 640, 480)
            rc, rb = tr.vote(store, lst, R, t, CAM, 640, 480)
            assert counts.tolist() == rc.tolist() and best == rb, (trial, len(lst))
            assert len(lst) < 64 or rc.max() > 50
    # ties: the first maximum; an empty list; a frame of another size
    counts, best = c.kf_visible([ids[3], ids[3], ids[3]], np.eye(3), np.zeros(3))
    assert best == 0 and counts[0] == counts[2]
    counts, best = c.kf_visible([], np.eye(3), np.zeros(3))
    assert best == -1 and len(counts) == 0
    counts, best = c.kf_visible(ids[:8], np.eye(3), np.zeros(3), CAM[:2], CAM[2:], 320, 200)
    rc, rb = tr.vote(store, ids[:8], np.eye(3), np.zeros(3), CAM, 320, 200)
    assert counts.tolist() == rc.tolist() and best == rb
    for bad in ([ids[0], 99999], ids[:64] + [ids[0]]):
        with pytest.raises(pkg.MslamHipError) as e:
            c.kf_visible(bad, np.eye(3), np.zeros(3))
        assert e.value.code == pkg.E_INVALID
    c.close()


@KINDS
def test_track_single_steps_equal_the_reference(pkg, sequence, kind):
    """steps of the sequence taken from the reference loop's state: one that only tracks, the two that insert a keyframe,
    one on the way back where the vote prefers an older keyframe"""
    seq, rows, trk = sequence
    c = _ctx(pkg, kind)
    kf_min = tr.SEQ_PARAMS["new_keyframe_min_landmarks"]
    for f in (3, 6, 11, 25):
        fr = seq["frames"][f]
        ref_id = rows[f - 1]["reference"]
        ids = [i for i in trk.ids if i <= max(r["keyframe"] for r in rows[:f])]
        store = {i: trk.store[i] for i in ids}
        c.kf_clear()
        _fill(c, store)
        guess = (rows[f - 1]["R"], rows[f - 1]["t"])
        new_id = 40 + f
        ref = tr.track(fr["desc"], fr["xy"], fr["depth"], store, ref_id, ids, seed=f, guess=guess, new_keyframe_min_landmarks=kf_min)
        got = c.track(fr["desc"], fr["xy"], fr["depth"], ref_id, ids, new_id, seed=f, rvec=_rvec(guess[0]), tvec=guess[1],
                      new_keyframe_min_landmarks=kf_min, with_pairs=True, with_entry=True)
        _compare_step(got, ref, (kind, f))
        assert c.last_match_kernel() == ("matrix", "popcount")[kind]
        assert got["tracked"] and got["n_correspondences"] < got["n_matches"]         # the depth filter cuts
        assert rr.rot_err(got["R"], fr["R"]) < 0.1 and np.linalg.norm(got["tvec"] - fr["t"]) < 0.02
        assert bool(got["keyframe_added"]) == (f in (6, 11))
        if got["keyframe_added"]:
            e = _compare_entry(c, got, ref, fr, store, ref_id, new_id)
            assert c.kf_size() == len(ids) + 1
            print("frame", f, "entry", len(e["kp"]), "inherited", e["n_inherited"])
        else:
            assert c.kf_size() == len(ids) and got["n_entry"] == 0 and len(got["entry_src"]) == 0
        if f == 25:
            assert ids[got["vote_best"]] != ref_id
        # the same call without the optional outputs gives the same record
        if not got["keyframe_added"]:
            bare = c.track(fr["desc"], fr["xy"], fr["depth"], ref_id, ids, new_id, seed=f, rvec=_rvec(guess[0]), tvec=guess[1],
                           new_keyframe_min_landmarks=kf_min)
            for k in ("n_matches", "n_correspondences", "n_inliers", "tracked", "vote_best", "vote_best_count"):
                assert bare[k] == got[k], k
            assert np.array_equal(bare["R"], got["R"]) and np.array_equal(bare["vote_counts"], got["vote_counts"])
    c.close()


@KINDS
def test_track_edges(pkg, sequence, kind):
    seq, rows, trk = sequence
    f = 6                                                     # a step that requires a keyframe
    fr = seq["frames"][f]
    store = {0: trk.store[0], 5: trk.store[1]}                # (5: an unrelated second entry)
    guess = (rows[f - 1]["R"], rows[f - 1]["t"])
    kw = dict(seed=f, rvec=_rvec(guess[0]), tvec=guess[1], new_keyframe_min_landmarks=100)
    c = _ctx(pkg, kind)
    _fill(c, store)
    snap = _snapshot(c, [0, 5])
    ref = tr.track(fr["desc"], fr["xy"], fr["depth"], store, 0, [0, 5], seed=f, guess=guess, new_keyframe_min_landmarks=100)
    assert ref["keyframe_required"]
    # fewer than min_matched_points correspondences: not tracked, nothing added, a failed call leaves every entry as it was
    ref_few = tr.track(fr["desc"], fr["xy"], fr["depth"], store, 0, [0, 5], seed=f, guess=guess, new_keyframe_min_landmarks=100,
                       min_matched_points=ref["n_correspondences"] + 1)
    got = c.track(fr["desc"], fr["xy"], fr["depth"], 0, [0, 5], 9, min_matched_points=ref["n_correspondences"] + 1,
                  with_pairs=True, with_entry=True, **kw)
    _compare_step(got, ref_few, "few")
    assert not got["tracked"] and got["status"] == 1 and not got["keyframe_added"] and got["vote_best"] == -1
    _same_store(c, snap)
    got = c.track(fr["desc"], fr["xy"], fr["depth"], 0, [0, 5], 9, min_matched_points=ref["n_correspondences"], **kw)
    assert got["tracked"] and got["keyframe_added"]
    c.kf_remove(9)
    # no model: a query of distractors only (no correspondences), and a query of one keypoint
    lone = fr["landmark"] < 0
    ref_none = tr.track(fr["desc"][lone], fr["xy"][lone], fr["depth"], store, 0, [0, 5], seed=f, guess=guess)
    got = c.track(fr["desc"][lone], fr["xy"][lone], fr["depth"], 0, [0, 5], 9, with_pairs=True, with_entry=True, **kw)
    _compare_step(got, ref_none, "no model")
    assert not got["tracked"]
    got = c.track(fr["desc"][:1], fr["xy"][:1], fr["depth"], 0, [0, 5], 9, with_pairs=True, **kw)
    assert not got["tracked"] and got["n_matches"] == 0 and got["vote_best"] == -1 and not got["vote_counts"].any()
    _same_store(c, snap)
    # new_id < 0: required, never inserted
    got = c.track(fr["desc"], fr["xy"], fr["depth"], 0, [0, 5], -1, with_pairs=True, with_entry=True, **kw)
    _compare_step(got, ref, "no insert")
    assert got["keyframe_required"] and not got["keyframe_added"] and got["n_entry"] == 0
    _same_store(c, snap)
    # new_id colliding with the reference id or a vote id; unknown reference / vote ids; too many vote ids
    for call in (lambda: c.track(fr["desc"], fr["xy"], fr["depth"], 0, [5], 0, **kw),
                 lambda: c.track(fr["desc"], fr["xy"], fr["depth"], 0, [0, 5], 5, **kw),
                 lambda: c.track(fr["desc"], fr["xy"], fr["depth"], 77, [0], 9, **kw),
                 lambda: c.track(fr["desc"], fr["xy"], fr["depth"], 0, [0, 77], 9, **kw),
                 lambda: c.track(fr["desc"], fr["xy"], fr["depth"], 0, [0] * 65, 9, **kw)):
        with pytest.raises(pkg.MslamHipError) as e:
            call()
        assert e.value.code == pkg.E_INVALID
    _same_store(c, snap)
    # pair_stride / entry_capacity too small
    with pytest.raises(pkg.MslamHipError) as e:
        c.track(fr["desc"], fr["xy"], fr["depth"], 0, [0, 5], -1, with_pairs=True, pair_stride=ref["n_matches"] - 1, **kw)
    assert e.value.code == pkg.E_CAPACITY
    _same_store(c, snap)
    with pytest.raises(pkg.MslamHipError) as e:
        c.track(fr["desc"], fr["xy"], fr["depth"], 0, [0, 5], 9, with_entry=True, entry_capacity=10, **kw)
    assert e.value.code == pkg.E_CAPACITY
    c.kf_remove(9)                                            # (the step ran: the entry is in the store, only the rows are not copied)
    _same_store(c, snap)
    # more query keypoints than an entry holds
    small = _ctx(pkg, kind, max_keypoints=600)
    small.kf_add(0, store[0][0][:500], store[0][1][:500])
    with pytest.raises(pkg.MslamHipError) as e:
        small.track(fr["desc"], fr["xy"], fr["depth"], 0, [0], 9, **kw)
    assert e.value.code == pkg.E_CAPACITY and small.kf_size() == 1
    small.close()
    # an empty vote list
    got = c.track(fr["desc"], fr["xy"], fr["depth"], 0, [], 9, with_pairs=True, with_entry=True, **kw)
    ref_nv = tr.track(fr["desc"], fr["xy"], fr["depth"], store, 0, [], seed=f, guess=guess, new_keyframe_min_landmarks=100)
    _compare_step(got, ref_nv, "grow")
    assert got["keyframe_added"] and got["vote_best"] == -1 and c.kf_size() == 3
    _compare_entry(c, got, ref_nv, fr, store, 0, 9)
    for i, (d, w) in snap.items():
        gd, gw = c.kf_read(i)
        assert np.array_equal(gd, d) and np.array_equal(gw, w), i
    # the store grows during a call: its first allocation holds 16 entries, track alone fills it and goes past it
    for new_id in range(20, 40):
        got = c.track(fr["desc"], fr["xy"], fr["depth"], 0, [0, 5], new_id, **kw)
        assert got["keyframe_added"]
    assert c.kf_size() == 23
    a, b = c.kf_read(9), c.kf_read(39)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # an existing new_id is replaced when a keyframe is added, left alone when not
    before = c.kf_read(5)
    got = c.track(fr["desc"][lone], fr["xy"][lone], fr["depth"], 0, [0], 5, **kw)
    after = c.kf_read(5)
    assert not got["tracked"] and np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and c.kf_size() == 23
    got = c.track(fr["desc"], fr["xy"], fr["depth"], 0, [0], 5, **kw)
    after = c.kf_read(5)
    assert got["keyframe_added"] and c.kf_size() == 23 and np.array_equal(after[0], a[0]) and np.array_equal(after[1], a[1])
    c.close()


@KINDS
def test_sequence_through_the_tracker_equals_the_reference_loop(pkg, sequence, kind):
    seq, rows, trk = sequence
    c = _ctx(pkg, kind)
    t = pkg.HipKeyframeTracker(c, focal=CAM[:2], principal=CAM[2:], **tr.SEQ_PARAMS)
    got = []
    for f, fr in enumerate(seq["frames"]):
        o = t.processSensorData(fr["desc"], fr["xy"], fr["depth"])
        o["err_deg"], o["err_m"] = rr.rot_err(o["R"], fr["R"]), float(np.linalg.norm(o["tvec"] - fr["t"]))
        print(f, "tracked", o["tracked"], "inliers", o["n_inliers"], "reference", o["reference"], "keyframe", o["keyframe"],
              "error %.5f deg %.6f m" % (o["err_deg"], o["err_m"]))
        got.append(o)
    assert tr.summarize(got) == tr.summarize(rows)
    assert [o["reference"] for o in got] == [r["reference"] for r in rows]
    assert max(o["err_deg"] for o in got) < 0.1 and max(o["err_m"] for o in got) < 0.02
    assert t.ids == trk.ids and c.kf_size() == len(trk.ids)
    gd, gw = c.kf_read(0)                                            # initFirstKeyframe: the same entry, bit for bit
    assert np.array_equal(gd, trk.store[0][0]) and np.array_equal(gw, trk.store[0][1])
    c.close()


@KINDS
def test_track_failure_falls_back_to_relocalize(pkg, sequence, kind):
    """a frame the reference keyframe does not see: track fails, the loop's relocalize names the keyframe that does"""
    seq, rows, trk = sequence
    c = _ctx(pkg, kind)
    t = pkg.HipKeyframeTracker(c, focal=CAM[:2], principal=CAM[2:], **tr.SEQ_PARAMS)
    r = tr.KeyframeTracker(cam=CAM, **tr.SEQ_PARAMS)
    flags = []
    for f in list(range(13)) + [1, 2]:                       # out to keyframe 2, then a jump home: keyframe 2 sees nothing of it
        fr = seq["frames"][f]
        a, b = t.processSensorData(fr["desc"], fr["xy"], fr["depth"]), r.process(fr["desc"], fr["xy"], fr["depth"])
        print(f, a["tracked"], a["relocalized"], a["reference"], a["keyframe"], "|", b["tracked"], b["relocalized"], b["reference"])
        assert (a["tracked"], a["relocalized"], a["reference"], a["keyframe"]) == (b["tracked"], b["relocalized"], b["reference"], b["keyframe"]), f
        flags.append((a["tracked"], a["relocalized"]))
    assert flags[13] == (False, True) and flags[14] == (True, False) and t.ids == [0, 1, 2]
    c.close()


def test_track_leaves_its_neighbours_results_alone(pkg, sequence):
    """relocalize, kf_add_from_batch_dev and backproject share the context's scratch with track: the same results before
    and after a track call"""
    import torch
    import synth
    seq, rows, trk = sequence
    K = 2048
    c = pkg.Context(width=640, height=480, max_batch=1, max_keypoints=K)
    frame = synth.make_stream(1, 640, 480, seed=21)[0]
    depth = np.tile((np.linspace(1.0, 4.2, 640) * 5000).astype(np.uint16), (480, 1))
    d_depth = torch.from_numpy(depth.view(np.int16)).cuda()
    d_frame = torch.from_numpy(frame[None]).cuda()
    store = {0: trk.store[0], 1: trk.store[1], 2: trk.store[2]}
    _fill(c, store)
    R, t = po.rodrigues([0.1, -0.2, 0.05]), np.array([0.3, -0.1, 1.5])
    q = seq["frames"][9]

    def others(tag):
        c.detect_batch_dev(d_frame.data_ptr(), 1)
        c.backproject_batch_dev(d_depth.data_ptr(), focal=CAM[:2], principal=CAM[2:])
        c.kf_add_from_batch_dev(50, 0, R, t, 3.0)
        lifted = c.kf_read(50)
        reloc = c.relocalize(q["desc"], q["xy"], [0, 1, 2], seed=3, with_pairs=True)
        bp = c.backproject(q["depth"], q["xy"], focal=CAM[:2], principal=CAM[2:])
        return lifted, reloc, bp

    before = others("before")
    fr = seq["frames"][6]
    got = c.track(fr["desc"], fr["xy"], fr["depth"], 0, [0, 1, 2], 60, seed=6, rvec=_rvec(rows[5]["R"]), tvec=rows[5]["t"],
                  new_keyframe_min_landmarks=100, with_pairs=True, with_entry=True)
    assert got["tracked"] and got["keyframe_added"]
    after = others("after")
    assert np.array_equal(before[0][0], after[0][0]) and np.array_equal(before[0][1], after[0][1]) and len(before[0][0]) > 50
    assert before[1]["best"] == after[1]["best"] >= 0
    for a, b in zip(before[1]["candidates"], after[1]["candidates"]):
        assert all(np.array_equal(a[k], b[k]) for k in a)
    for k in range(3):
        assert np.array_equal(before[1]["pairs"][k][0], after[1]["pairs"][k][0]) and np.array_equal(before[1]["inliers"][k], after[1]["inliers"][k])
    assert np.array_equal(before[2][0], after[2][0]) and np.array_equal(before[2][1], after[2][1])
    # and against the references
    xyz, valid = tr._oracle().backproject(q["depth"], q["xy"], tr.FACTOR, CAM[:2], CAM[2:])
    assert np.array_equal(after[2][0], xyz) and np.array_equal(after[2][1], valid)
    ref = rr.relocalize(q["desc"], q["xy"], store, [0, 1, 2], seed=3)
    assert ref["best"] == after[1]["best"] and [x["n_inliers"] for x in ref["candidates"]] == [x["n_inliers"] for x in after[1]["candidates"]]
    c.close()


def _bits_equal(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_bits_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_bits_equal(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, float):
        return np.float64(a).tobytes() == np.float64(b).tobytes()
    return a == b


@KINDS
def test_calls_sharing_the_scratch_equal_a_fresh_context(pkg, sequence, kind):
    """kf_visible, relocalize, track and track_window stage their upload, their device arrays and their results in the same
    three blocks of the context.  One context makes five such calls in a row — the blocks grow between them, and the row
    stride of the per-row arrays goes from 256 (relocalize on entries of 200 and 250 landmarks) to 512 (the full entry 0)
    — and every result equals, field for field and bit for bit, what a fresh context holding the same store returns for
    the same call as its first."""
    seq, rows, trk = sequence
    rng = np.random.default_rng(5)
    fr, q, win = seq["frames"][6], seq["frames"][9], seq["frames"][6:8]
    R, t = rows[5]["R"], rows[5]["t"]
    store = {0: trk.store[0], 1: tuple(x[:200] for x in trk.store[1]), 2: tuple(x[:250] for x in trk.store[2])}
    assert 256 < len(store[0][0]) <= 512 and 290 <= len(fr["desc"]) and len(q["desc"]) > 256
    for i, n in enumerate([1, 255, 256, 257] + [int(v) for v in rng.integers(40, 301, 57)]):
        store[100 + i] = (rng.integers(0, 256, (n, 32), dtype=np.uint8),
                          np.stack([rng.uniform(-4, 4, n), rng.uniform(-3, 3, n), rng.uniform(-1, 6, n)], 1))
    ids64 = [0, 1, 60] + [100 + i for i in range(61)]
    kw = dict(seed=6, rvec=_rvec(R), tvec=t, new_keyframe_min_landmarks=100)

    def track(c):
        got = c.track(fr["desc"], fr["xy"], fr["depth"], 0, [0, 1, 2], 60, with_pairs=True, with_entry=True, **kw)
        assert got["tracked"] and got["keyframe_added"]
        return got, c.kf_read(60)

    def window(c):
        recs, first = c.track_window([x["desc"] for x in win], [x["xy"] for x in win], [x["depth"] for x in win], 0, [0, 1, 2], 61, 0,
                                     focal=CAM[:2], principal=CAM[2:], with_entry=True, **kw)
        assert first == 0 and recs[0]["keyframe_added"] and recs[1]["tracked"]
        return recs, first, c.kf_read(61)

    calls = [("kf_visible, 3 ids", lambda c: c.kf_visible([0, 1, 2], R, t, CAM[:2], CAM[2:])),
             ("relocalize", lambda c: c.relocalize(q["desc"], q["xy"], [1, 2], seed=3, with_pairs=True)),
             ("track", track),
             ("kf_visible, 64 ids", lambda c: c.kf_visible(ids64, R, t, CAM[:2], CAM[2:])),
             ("track_window", window)]
    c = _ctx(pkg, kind)
    _fill(c, store)
    for what, call in calls:
        fresh = _ctx(pkg, kind)
        _fill(fresh, store)
        want = call(fresh)
        fresh.close()
        got = call(c)
        assert _bits_equal(got, want), what
        if what == "relocalize":
            assert max(x["n_inliers"] for x in got["candidates"]) >= 60 and len(got["pairs"][1][0]) > 60
        if what == "track":
            store[60] = got[1]                     # the keyframe the step made: part of the store from here on
        if what == "kf_visible, 64 ids":
            assert got[0][:3].min() > 0 and np.count_nonzero(got[0]) > 32
    c.close()
