"""Window tracking on the GPU, through the C ABI: mslam_hip_track_window / _dev and HipKeyframeTracker.process_window.
Every record of a window equals Context.track of that frame alone (same guess, seed + s) field for field — bit for bit,
poses included: both run the same kernels — and tests/track_window_ref.py as tests/test_gpu_track.py::_compare_step judges
a single step (poses within its 1e-7); the entry a window builds equals _compare_entry's reference bit for bit.  The inputs
are tests/track_window_cases.py's, which tests/test_track_window.py proves to produce the events they claim.  Both matcher
kinds throughout."""
import numpy as np
import pytest

import reloc_ref as rr
import track_ref as tr
import track_window_cases as cases
import track_window_ref as twr
from test_gpu_track import KINDS, _compare_entry, _compare_step, _ctx, _fill, _rvec, _same_store, _snapshot

CAM = tr.CAM
pytestmark = pytest.mark.gpu
KF_MIN = cases.KF_MIN
FIELDS = ("n_matches", "n_correspondences", "n_inliers", "status", "tracked", "keyframe_required", "vote_best", "vote_best_count")


@pytest.fixture(scope="module")
def sequence(orc):
    seq = tr.make_sequence(seed=0)
    rows, trk = tr.run_reference(seq)
    return seq, rows, trk


_REF = {}


def _ref_window(key, frames, store, ref, ids, pos, **kw):
    """the reference window, computed once per input and shared by both matcher kinds"""
    if key not in _REF:
        _REF[key] = twr.track_window([x["desc"] for x in frames], [x["xy"] for x in frames], [x["depth"] for x in frames], store, ref,
                                     ids, pos, **kw)
    return _REF[key]


def _window(c, frames, ref, ids, new_id, pos, seed, guess, cam=CAM, kf_min=KF_MIN, **kw):
    return c.track_window([x["desc"] for x in frames], [x["xy"] for x in frames], [x["depth"] for x in frames], ref, ids, new_id, pos,
                          focal=cam[:2], principal=cam[2:], seed=seed, rvec=_rvec(guess[0]), tvec=guess[1],
                          new_keyframe_min_landmarks=kf_min, with_entry=True, **kw)


def _single(c, fr, ref, ids, seed, guess, cam=CAM, kf_min=KF_MIN):
    return c.track(fr["desc"], fr["xy"], fr["depth"], ref, ids, -1, focal=cam[:2], principal=cam[2:], seed=seed, rvec=_rvec(guess[0]),
                   tvec=guess[1], new_keyframe_min_landmarks=kf_min, with_pairs=True)


def _same_record(win, one, what):
    """a window's record against Context.track of the frame alone: every field, poses bit for bit"""
    for k in FIELDS:
        assert win[k] == one[k], (what, k, win[k], one[k])
    for k in ("R", "rvec", "tvec"):
        assert np.array_equal(win[k].view(np.uint64), one[k].view(np.uint64)), (what, k, np.abs(win[k] - one[k]).max())
    assert np.array_equal(win["vote_counts"], one["vote_counts"]), what


def _check_window(c, recs, first, frames, store, ref, ids, pos, seed, guess, steps, ref_first, cam=CAM, kf_min=KF_MIN, singles=None):
    """records == single calls == the reference; the event position == the reference's"""
    assert len(recs) == len(frames) == len(steps)
    for s in (range(len(frames)) if singles is None else singles):
        one = _single(c, frames[s], ref, ids, seed + s, guess, cam, kf_min)
        _same_record(recs[s], one, s)
        _compare_step(one, steps[s], ("single", s))
    for s, (r, st) in enumerate(zip(recs, steps)):
        for k in FIELDS:
            assert r[k] == st[k], (s, k, r[k], st[k])
        assert np.array_equal(r["vote_counts"], st["vote_counts"]), s
        if st["status"]:
            assert np.abs(r["R"] - st["R"]).max() < 1e-7 and np.abs(r["tvec"] - st["t"]).max() < 1e-7, s
        else:
            assert not r["R"].any() and not r["rvec"].any() and not r["tvec"].any()
    assert first == ref_first
    assert first == next((s for s, st in enumerate(steps) if twr.is_event(st, len(ids), pos)), len(steps))


def _check_entry(c, recs, first, frames, store, ref, ids, new_id, seed, guess, steps, cam=CAM, kf_min=KF_MIN):
    """the entry the window built for its event frame: _compare_entry's reference, fed with that frame's pairs and mask
    (from the single call, whose record the window's equals) and the device's own pose"""
    one = _single(c, frames[first], ref, ids, seed + first, guess, cam, kf_min)
    _same_record(recs[first], one, "event frame")
    got = dict(one, n_entry=recs[first]["n_entry"], n_inherited=recs[first]["n_inherited"], entry_src=recs[first]["entry_src"],
               entry_kp=recs[first]["entry_kp"])
    return _compare_entry(c, got, steps[first], frames[first], store, ref, new_id)


@KINDS
@pytest.mark.parametrize("S", [1, 2, 7, 32])
def test_every_record_equals_the_single_frame_call(pkg, sequence, kind, S):
    seq, rows, trk = sequence
    st = cases.state(rows, trk, 1)
    frames = (seq["frames"][1:] + seq["frames"][:1])[:S]       # from frame 1 on; 32 frames: out of keyframe 0's sight and back
    steps, ref_first, _ = _ref_window(("seq", S), frames, st["store"], 0, [0], 0, seed=1, guess=st["guess"],
                                      new_keyframe_min_landmarks=KF_MIN)
    c = _ctx(pkg, kind)
    _fill(c, st["store"])
    recs, first = _window(c, frames, 0, [0], -1, 0, 1, st["guess"])
    _check_window(c, recs, first, frames, st["store"], 0, [0], 0, 1, st["guess"], steps, ref_first)
    assert c.last_match_kernel() == ("matrix", "popcount")[kind]
    assert c.kf_size() == 1 and not any(r["keyframe_added"] for r in recs)
    print("S", S, "first_event", first, "tracked", [r["tracked"] for r in recs])
    assert S < 7 or first == 5                                   # frame 6 requires the keyframe
    c.close()


@KINDS
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_event_position_kind_and_keyframe(pkg, sequence, kind, name):
    seq, rows, trk = sequence
    inp = cases.case_inputs(seq, rows, trk, name)
    frames, store, ref, ids, pos, seed, guess = (inp[k] for k in ("frames", "store", "ref", "ids", "pos", "seed", "guess"))
    steps, ref_first, ref_entry = _ref_window(("case", name), frames, store, ref, ids, pos, seed=seed, guess=guess,
                                              new_keyframe_min_landmarks=KF_MIN)
    c = _ctx(pkg, kind)
    _fill(c, store)
    snap = _snapshot(c, list(store))
    new_id = 50
    recs, first = _window(c, frames, ref, ids, new_id, pos, seed, guess)
    _check_window(c, recs, first, frames, store, ref, ids, pos, seed, guess, steps, ref_first)
    assert first == inp["first"]
    kinds = {s: cases.kind(r, len(ids), pos) for s, r in enumerate(recs)}
    assert {s: k for s, k in kinds.items() if k} == inp["kinds"], kinds
    added = [s for s, r in enumerate(recs) if r["keyframe_added"]]
    if inp["kinds"].get(first) == "keyframe":
        assert added == [first] and c.kf_size() == len(store) + 1            # later keyframe-requiring frames insert nothing
        e = _check_entry(c, recs, first, frames, store, ref, ids, new_id, seed, guess, steps)
        assert np.array_equal(e["desc"], ref_entry["desc"]) and np.array_equal(e["src"], ref_entry["src"])
        lids, ref_lids = c.kf_read_ids(new_id), c.kf_read_ids(ref)
        na = recs[first]["n_inherited"]
        assert np.array_equal(lids[:na], ref_lids[recs[first]["entry_src"][:na]])      # part A inherits the ids
        assert len(set(lids[na:].tolist())) == len(lids) - na and (lids[na:] >> 62 == 1).all()
        c.kf_remove(new_id)
        # new_id = -1: required, never inserted
        recs2, first2 = _window(c, frames, ref, ids, -1, pos, seed, guess)
        assert first2 == first and recs2[first]["keyframe_required"] and not any(r["keyframe_added"] for r in recs2)
        assert recs2[first]["n_entry"] == 0 and len(recs2[first]["entry_src"]) == 0
    else:
        assert added == [] and all(r["n_entry"] == 0 and len(r["entry_src"]) == 0 for r in recs)
    _same_store(c, snap)                                                          # unchanged, the slot released
    c.close()


@KINDS
def test_ragged_windows(pkg, sequence, kind):
    seq, rows, trk = sequence
    st = cases.state(rows, trk, 1)
    f = seq["frames"]

    def cut(fr, n, depth=None):
        return dict(desc=fr["desc"][:n].copy(), xy=fr["xy"][:n].copy(), depth=fr["depth"] if depth is None else depth)
    frames = [f[1], cut(f[2], 0), f[2], cut(f[3], 1), cut(f[4], 2), dict(f[3], depth=np.zeros_like(f[3]["depth"])), f[4]]
    stride = max(len(x["desc"]) for x in frames) + 37
    c = _ctx(pkg, kind)
    for L in (None, 255, 256, 257):
        store = st["store"] if L is None else {0: (st["store"][0][0][:L], st["store"][0][1][:L])}
        fr = frames if L is None else frames[:3]
        c.kf_clear()
        _fill(c, store)
        steps, ref_first, _ = _ref_window(("ragged", L), fr, store, 0, [0], 0, seed=1, guess=st["guess"], new_keyframe_min_landmarks=KF_MIN)
        recs, first = _window(c, fr, 0, [0], -1, 0, 1, st["guess"], stride=stride, pad_value=0xA5)   # sentinel-filled padding rows
        _check_window(c, recs, first, fr, store, 0, [0], 0, 1, st["guess"], steps, ref_first)
        tight, first_t = _window(c, fr, 0, [0], -1, 0, 1, st["guess"])                               # stride = the largest n
        assert first_t == first
        for s, (a, b) in enumerate(zip(recs, tight)):
            _same_record(a, b, ("stride", s))
        print("landmarks", L, "first", first, [(r["n_matches"], r["n_correspondences"], r["n_inliers"]) for r in recs])
        if L is None:
            assert first == 1 and [r["tracked"] for r in recs] == [1, 0, 1, 0, 0, 0, 1]
            assert recs[5]["n_matches"] > 0 and recs[5]["n_correspondences"] == 0                     # no depth anywhere
            assert [r["n_matches"] for r in recs[3:5]] == [0, steps[4]["n_matches"]]
    c.close()


@KINDS
@pytest.mark.parametrize("S,at", [(65, 64), (256, 255)])
def test_scan_width(pkg, orc, kind, S, at):
    sc = cases.small_scene(S, at)
    frames, store, cam, guess = sc["frames"], sc["store"], sc["cam"], sc["guess"]
    steps, ref_first, _ = _ref_window(("small", S), frames, store, 0, [0], 0, cam=cam, guess=guess)
    c = _ctx(pkg, kind, max_keypoints=256)
    _fill(c, store)
    recs, first = _window(c, frames, 0, [0], 1, 0, 0, guess, cam=cam, kf_min=30)
    _check_window(c, recs, first, frames, store, 0, [0], 0, 0, guess, steps, ref_first, cam=cam, kf_min=30,
                  singles=sorted({0, 1, 63, 64, at - 1, at} & set(range(S))))
    assert first == at and [s for s, r in enumerate(recs) if r["keyframe_added"]] == [at] and c.kf_size() == 2
    _check_entry(c, recs, first, frames, store, 0, [0], 1, 0, guess, steps, cam=cam, kf_min=30)
    if S == 256:
        with pytest.raises(pkg.MslamHipError) as e:
            _window(c, frames + frames[:1], 0, [0], 2, 0, 0, guess, cam=cam, kf_min=30)
        assert e.value.code == pkg.E_INVALID and c.kf_size() == 2
    c.close()


@KINDS
def test_errors_leave_the_context_usable(pkg, sequence, kind):
    """the vote list [0, 5] with ref_vote_pos = -1: keyframe 5 sees more of these frames than the reference does, so with a
    position the vote would be the event; without one the window's event is the keyframe frame 6 requires"""
    seq, rows, trk = sequence
    inp = cases.case_inputs(seq, rows, trk, "at_last")
    frames, guess = inp["frames"], inp["guess"]
    store = {0: trk.store[0], 5: trk.store[1]}
    steps, ref_first, _ = _ref_window(("errors",), frames, store, 0, [0, 5], -1, seed=3, guess=guess, new_keyframe_min_landmarks=KF_MIN)
    voted, voted_first, _ = _ref_window(("errors", "voted"), frames, store, 0, [0, 5], 0, seed=3, guess=guess,
                                        new_keyframe_min_landmarks=KF_MIN)
    assert ref_first == 3 and voted_first == 0 and voted[0]["vote_best"] == 1
    c = _ctx(pkg, kind)
    _fill(c, store)
    snap = _snapshot(c, [0, 5])
    base, base_first = _window(c, frames, 0, [0, 5], -1, -1, 3, guess)
    _check_window(c, base, base_first, frames, store, 0, [0, 5], -1, 3, guess, steps, ref_first, singles=[0, 3])
    recs, first = _window(c, frames, 0, [0, 5], -1, 0, 3, guess)
    assert first == voted_first and base_first == 3

    def clean():
        recs, first = _window(c, frames, 0, [0, 5], -1, -1, 3, guess)
        assert first == base_first
        for s, (a, b) in enumerate(zip(recs, base)):
            _same_record(a, b, ("clean", s))
        _same_store(c, snap)
    for args in (dict(ref=77, ids=[0], new_id=9, pos=-1), dict(ref=0, ids=[0, 77], new_id=9, pos=-1),
                 dict(ref=0, ids=[5], new_id=0, pos=-1), dict(ref=0, ids=[0, 5], new_id=5, pos=-1),
                 dict(ref=0, ids=[0] * 65, new_id=9, pos=-1), dict(ref=0, ids=[0, 5], new_id=9, pos=2),
                 dict(ref=0, ids=[0, 5], new_id=9, pos=-2), dict(ref=0, ids=[], new_id=9, pos=0)):
        with pytest.raises(pkg.MslamHipError) as e:
            _window(c, frames, args["ref"], args["ids"], args["new_id"], args["pos"], 3, guess)
        assert e.value.code == pkg.E_INVALID, args
        clean()
    with pytest.raises(pkg.MslamHipError) as e:
        _window(c, [], 0, [0, 5], 9, -1, 3, guess)
    assert e.value.code == pkg.E_INVALID
    clean()
    # entry_capacity too small: the window has run and the keyframe is in the store, only the rows are not copied
    with pytest.raises(pkg.MslamHipError) as e:
        _window(c, frames, 0, [0, 5], 9, -1, 3, guess, entry_capacity=10)
    assert e.value.code == pkg.E_CAPACITY and c.kf_size() == 3
    c.kf_remove(9)
    clean()
    # a frame with more keypoints than an entry holds
    small = _ctx(pkg, kind, max_keypoints=600)
    small.kf_add(0, store[0][0][:500], store[0][1][:500])
    with pytest.raises(pkg.MslamHipError) as e:
        _window(small, frames, 0, [0], 9, 0, 3, guess)
    assert e.value.code == pkg.E_CAPACITY and small.kf_size() == 1
    cut = [dict(fr, desc=fr["desc"][:600], xy=fr["xy"][:600]) for fr in frames]
    recs, first = _window(small, cut, 0, [0], 9, 0, 3, guess)
    assert len(recs) == 4 and small.kf_size() == 1 + int(any(r["keyframe_added"] for r in recs))
    small.close()
    c.close()


@KINDS
def test_the_dev_form_equals_the_host_form_on_the_batch_arrays(pkg, kind):
    import torch
    import synth
    B, K = 8, 2048
    stream = synth.make_stream(B, 640, 480, seed=1234)
    depth = np.ascontiguousarray(synth.make_depth(B, 640, 480))
    c = pkg.Context(width=640, height=480, max_batch=B, max_keypoints=K)
    c.set_matcher(kind)
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
    kw = dict(focal=CAM[:2], principal=CAM[2:], seed=7, rvec=np.zeros(3), tvec=np.zeros(3), with_entry=True)
    for kf_min in (30, 100000):                               # as the sequence goes; and every frame a keyframe candidate
        dev, dev_first = c.track_window_dev(1, 7, 0, [0], 70, 0, new_keyframe_min_landmarks=kf_min, **kw)
        dev_entry = c.kf_read(70) + (c.kf_read_ids(70),) if c.kf_size() == 2 else None
        if dev_entry:
            c.kf_remove(70)
        host, host_first = c.track_window([desc[f, :cnt[f]] for f in range(1, 8)], [xy[f, :cnt[f]] for f in range(1, 8)],
                                          [depth[f] for f in range(1, 8)], 0, [0], 71, 0, new_keyframe_min_landmarks=kf_min, **kw)
        host_entry = c.kf_read(71) + (c.kf_read_ids(71),) if c.kf_size() == 2 else None
        if host_entry:
            c.kf_remove(71)
        print("kf_min", kf_min, "first", dev_first, [(r["n_matches"], r["n_correspondences"], r["n_inliers"], r["tracked"]) for r in dev])
        assert dev_first == host_first and len(dev) == len(host) == 7
        for s, (a, b) in enumerate(zip(dev, host)):
            _same_record(a, b, ("dev", s))
            assert (a["keyframe_added"], a["n_entry"], a["n_inherited"]) == (b["keyframe_added"], b["n_entry"], b["n_inherited"])
            assert np.array_equal(a["entry_src"], b["entry_src"]) and np.array_equal(a["entry_kp"], b["entry_kp"])
        assert (dev_entry is None) == (host_entry is None)
        if dev_entry:
            na = dev[dev_first]["n_inherited"]
            assert np.array_equal(dev_entry[0], host_entry[0])
            assert np.array_equal(dev_entry[1].view(np.uint64), host_entry[1].view(np.uint64))
            assert np.array_equal(dev_entry[2][:na], host_entry[2][:na])                       # inherited ids; fresh ones differ
            assert np.array_equal(dev_entry[2][na:] & 0xFFFF, host_entry[2][na:] & 0xFFFF)     # in the serial alone
        if kf_min == 100000:                                  # frame 1 is the event whatever it does: a keyframe if it is tracked
            assert dev_first == 0 and (dev_entry is not None) == bool(dev[0]["tracked"])
    for bad in ((0, 9), (8, 1), (-1, 2), (0, 0)):
        with pytest.raises(pkg.MslamHipError) as e:
            c.track_window_dev(bad[0], bad[1], 0, [0], -1, 0, **kw)
        assert e.value.code == pkg.E_INVALID
    c.close()


@KINDS
def test_process_window_equals_the_reference_loop(pkg, sequence, kind):
    seq, rows, trk = sequence
    fr = seq["frames"]
    args = ([x["desc"] for x in fr], [x["xy"] for x in fr], [x["depth"] for x in fr])
    for window in (1, 5, 16):
        w = twr.WindowTracker(cam=CAM, **tr.SEQ_PARAMS)
        ref = w.process_window(*args, window=window)
        c = _ctx(pkg, kind)
        t = pkg.HipKeyframeTracker(c, focal=CAM[:2], principal=CAM[2:], **tr.SEQ_PARAMS)
        got = t.process_window(*args, window=window)
        assert len(got) == len(ref) == len(fr)
        for k in ("tracked", "keyframe", "reference", "relocalized", "n_inliers"):
            assert [o[k] for o in got] == [o[k] for o in ref], (window, k)
        for f, (a, b) in enumerate(zip(got, ref)):
            # a loop's poses: the existing tracker tests' tolerance (0.1 degrees, 2 cm), against the reference loop and ground truth
            assert rr.rot_err(a["R"], b["R"]) < 0.1 and np.linalg.norm(a["tvec"] - b["t"]) < 0.02, (window, f)
            assert rr.rot_err(a["R"], fr[f]["R"]) < 0.1 and np.linalg.norm(a["tvec"] - fr[f]["t"]) < 0.02, (window, f)
        assert t.ids == w.ids and c.kf_size() == len(w.ids)
        assert (t.window_calls, t.window_computed, t.window_discarded) == (w.window_calls, w.computed, w.discarded)
        print("window", window, "calls", t.window_calls, "computed", t.window_computed, "discarded", t.window_discarded)
        c.close()


@KINDS
@pytest.mark.parametrize("depth", [None, 2])
def test_process_window_of_one_is_process_sensor_data(pkg, sequence, kind, depth):
    seq, rows, trk = sequence
    fr = seq["frames"]
    K = 1024 if depth is None else 4096
    ca, cb = _ctx(pkg, kind, K), _ctx(pkg, kind, K)
    ta = pkg.HipKeyframeTracker(ca, focal=CAM[:2], principal=CAM[2:], local_map_depth=depth, **tr.SEQ_PARAMS)
    tb = pkg.HipKeyframeTracker(cb, focal=CAM[:2], principal=CAM[2:], local_map_depth=depth, **tr.SEQ_PARAMS)
    a = [ta.processSensorData(x["desc"], x["xy"], x["depth"]) for x in fr]
    b = tb.process_window([x["desc"] for x in fr], [x["xy"] for x in fr], [x["depth"] for x in fr], window=1)
    for f, (x, y) in enumerate(zip(a, b)):
        assert (x["tracked"], x["keyframe"], x["reference"], x["relocalized"], x["n_inliers"]) == \
               (y["tracked"], y["keyframe"], y["reference"], y["relocalized"], y["n_inliers"]), f
        for k in ("R", "rvec", "tvec"):
            assert np.array_equal(x[k].view(np.uint64), y[k].view(np.uint64)), (f, k)
    assert ta.ids == tb.ids and ta.graph == tb.graph and ta.local_map == tb.local_map
    for i in ta.ids:
        assert all(np.array_equal(p, q) for p, q in zip(ca.kf_read(i), cb.kf_read(i))) and np.array_equal(ca.kf_read_ids(i), cb.kf_read_ids(i))
    ca.close()
    cb.close()
