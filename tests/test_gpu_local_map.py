"""Local-map tracking on the GPU, through the C ABI: landmark ids in the keyframe store, mslam_hip_kf_union[_dev] bit for
bit against tests/local_map_ref.py::union, mslam_hip_kf_covisible against its covisible, mslam_hip_track on a union judged
as tests/test_gpu_track.py judges a single-entry step, and HipKeyframeTracker(local_map_depth=2) row for row against
LocalMapTracker — also through `harness --track --local-map 2`."""
import os
import subprocess
import sys

import numpy as np
import pytest

import local_map_ref as lm
import reloc_ref as rr
import track_ref as tr
from reloc_ref import po
from test_gpu_track import _compare_entry, _compare_step, _rvec

CAM = tr.CAM
pytestmark = pytest.mark.gpu
KINDS = pytest.mark.parametrize("kind", [0, 1], ids=["auto", "popcount"])
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 320


def _ctx(pkg, kind=0, max_keypoints=K):
    c = pkg.Context(width=0, height=0, max_keypoints=max_keypoints)
    c.set_matcher(kind)
    return c


def _entry(rng, lids):
    n = len(lids)
    return (rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.normal(size=(n, 3)) * 3.0), np.asarray(lids, np.int64)


def _fill(c, store, lids):
    for i, (d, w) in store.items():
        c.kf_add(i, d, w, lids=lids[i])


def _read(c, i):
    d, w = c.kf_read(i)
    return d, w, c.kf_read_ids(i)


def _same(got, ref, what=""):
    """descriptors, world points (as bytes), ids and count"""
    assert len(got[0]) == len(got[1]) == len(got[2]) == len(ref[2]), (what, len(got[2]), len(ref[2]))
    assert np.array_equal(got[2], ref[2]), what
    assert np.array_equal(got[0], ref[0]), what
    assert np.array_equal(got[1].view(np.uint64), np.ascontiguousarray(ref[1]).view(np.uint64)), what


def _check_union(c, store, lids, ids, dst=900, what=""):
    ref = lm.union(store, lids, ids)
    n = c.kf_union(dst, ids)
    assert n == len(ref[2]), (what, n, len(ref[2]))
    _same(_read(c, dst), ref, what)
    return ref


# ---- ids --------------------------------------------------------------------------------------------------------------------

def test_fresh_and_caller_ids(pkg):
    rng = np.random.default_rng(1)
    c = _ctx(pkg)
    (d1, w1), _ = _entry(rng, range(65))
    (d2, w2), _ = _entry(rng, range(320))
    c.kf_add(1, d1, w1)                                   # serial 1
    c.kf_add(2, d2, w2)                                   # serial 2
    a, b = c.kf_read_ids(1), c.kf_read_ids(2)
    assert a.dtype == np.int64 and np.array_equal(a, lm.fresh_ids(1, 65)) and np.array_equal(b, lm.fresh_ids(2, 320))
    c.kf_add(1, d2[:64], w2[:64])                          # a replace: serial 3
    a2 = c.kf_read_ids(1)
    assert np.array_equal(a2, lm.fresh_ids(3, 64))
    assert len(np.unique(np.concatenate([a, b, a2]))) == 65 + 320 + 64
    gd, gw = c.kf_read(1)                                  # kf_read gives what it always gave
    assert np.array_equal(gd, d2[:64]) and np.array_equal(gw, w2[:64])
    c.kf_add(4, d1[:0], w1[:0])                            # an empty entry: serial 4
    assert len(c.kf_read_ids(4)) == 0
    # caller ids round-trip, extremes included; a repeat is the caller's business
    mine = np.array([0, (1 << 62) - 1, 7, 7, 123456789012345], np.int64)
    c.kf_add(5, d1[:5], w1[:5], lids=mine)                 # serial 5
    assert np.array_equal(c.kf_read_ids(5), mine)
    gd, gw = c.kf_read(5)
    assert np.array_equal(gd, d1[:5]) and np.array_equal(gw, w1[:5])
    snap = {i: _read(c, i) for i in (1, 2, 4, 5)}
    for bad in ([1 << 62], [-1], [3, (1 << 62) + 5], [np.iinfo(np.int64).min], [np.iinfo(np.int64).max]):
        with pytest.raises(pkg.MslamHipError) as e:
            c.kf_add(6, d1[:len(bad)], w1[:len(bad)], lids=np.array(bad, np.int64))
        assert e.value.code == pkg.E_INVALID
        with pytest.raises(pkg.MslamHipError) as e:
            c.kf_add(5, d1[:len(bad)], w1[:len(bad)], lids=np.array(bad, np.int64))
        assert e.value.code == pkg.E_INVALID
    assert c.kf_size() == 4
    for i, s in snap.items():
        _same(_read(c, i), s, i)
    with pytest.raises(pkg.MslamHipError) as e:
        c.kf_read_ids(77)
    assert e.value.code == pkg.E_INVALID
    c.kf_add(6, d1, w1)                                    # the rejected calls took no serial: 6
    assert np.array_equal(c.kf_read_ids(6), lm.fresh_ids(6, 65))
    c.close()


def test_device_lift_gives_fresh_ids_in_kept_order(pkg, bundled_frames, bundled_depth):
    import torch
    Kd = 4096
    c = pkg.Context(width=640, height=480, max_batch=1, max_keypoints=Kd)
    c.detect_batch_dev(torch.from_numpy(bundled_frames[0][None].copy()).cuda().data_ptr(), 1)
    d_depth = torch.from_numpy(np.ascontiguousarray(bundled_depth[0]).view(np.int16)[None].copy()).cuda()
    c.backproject_batch_dev(d_depth.data_ptr(), focal=CAM[:2], principal=CAM[2:])
    R, t = po.rodrigues([0.1, -0.2, 0.05]), np.array([0.3, -0.1, 1.5])
    c.kf_add_from_batch_dev(3, 0, R, t, 3.0)               # serial 1
    c.kf_add_from_batch_dev(4, 0, R, t, 2.0)               # serial 2
    c.sync()
    v, pv = c.batch_view(), c.points_view()
    n = int(pkg.read_device(c, v.count, (1,), np.int32)[0])
    desc = pkg.read_device(c, v.desc, (1, Kd, 32), np.uint8)[0, :n]
    xyz = pkg.read_device(c, pv.xyz, (1, Kd, 3), np.float64)[0, :n]
    ok = pkg.read_device(c, pv.valid, (1, Kd), np.uint8)[0, :n]
    for i, (serial, z_max) in ((3, (1, 3.0)), (4, (2, 2.0))):
        rd, rw = rr.lift(desc, xyz, ok, R, t, z_max)
        gd, gw, gl = _read(c, i)
        print("keypoints", n, "landmarks", len(rd))
        assert 50 < len(rd) <= n and np.array_equal(gd, rd) and np.array_equal(gw, rw)
        assert np.array_equal(gl, lm.fresh_ids(serial, len(rd)))
    assert len(c.kf_read_ids(4)) <= len(c.kf_read_ids(3))
    c.close()


# ---- union ------------------------------------------------------------------------------------------------------------------

SIZES = (0, 1, 63, 64, 65, 256, 257, 320)


@pytest.fixture(scope="module")
def sized():
    """entries 10 .. 17 of the sizes that cover the wave, block and capacity edges, their landmark ids drawn from one pool
    of 320 (the entry of 320 holds them all, so every union of these fits exactly)"""
    rng = np.random.default_rng(2)
    store, lids = {}, {}
    for k, n in enumerate(SIZES):
        store[10 + k], lids[10 + k] = _entry(rng, 1000 + rng.permutation(320)[:n])
    return store, lids


def test_union_entry_sizes_and_list_orders(pkg, sized):
    store, lids = sized
    rng = np.random.default_rng(3)
    c = _ctx(pkg)
    _fill(c, store, lids)
    ids = sorted(store)
    for what, order in (("ascending", ids), ("descending", ids[::-1]), ("shuffled", [int(i) for i in rng.permutation(ids)])):
        ref = _check_union(c, store, lids, order, what=what)
        assert len(ref[2]) == 320                                     # exactly the capacity: it fits
    for i in ids:                                                     # n_ids = 1: the entry itself, empty and full included
        ref = _check_union(c, store, lids, [i], what=("single", i))
        assert np.array_equal(ref[2], lids[i])
    for pair in ([10, 11], [11, 10], [12, 13, 14], [16, 15, 10, 11], [15, 16], [16, 15]):
        _check_union(c, store, lids, pair, what=pair)
    # the sources are untouched, and dst is an ordinary entry: the union of a union
    for i in ids:
        _same(_read(c, i), (store[i][0], store[i][1], lids[i]), i)
    ref = lm.union(store, lids, [14, 13])
    assert c.kf_union(901, [14, 13]) == len(ref[2])
    store2, lids2 = dict(store), dict(lids)
    store2[901], lids2[901] = ref[:2], ref[2]
    _check_union(c, store2, lids2, [901, 12, 16], dst=902, what="of a union")
    c.close()


def test_union_overlaps_and_many_entries(pkg):
    rng = np.random.default_rng(4)
    c = _ctx(pkg)
    # two entries of 160 with 0 %, 25 %, 50 % and 100 % of their ids in common
    for share in (0, 40, 80, 160):
        store, lids = {}, {}
        store[1], lids[1] = _entry(rng, np.arange(160))
        store[2], lids[2] = _entry(rng, np.arange(160 - share, 320 - share))
        c.kf_clear()
        _fill(c, store, lids)
        for order in ([1, 2], [2, 1]):
            ref = _check_union(c, store, lids, order, what=(share, order))
            assert len(ref[2]) == 320 - share
        assert c.kf_covisible(1, [1, 2]).tolist() == [160, share]
    # every entry the same landmarks (other observations of them): the largest id's observation of each, wherever it is listed
    store, lids = {}, {}
    same = 500 + rng.permutation(100)
    for i in (3, 9, 5, 7, 4):
        store[i], lids[i] = _entry(rng, same)
    c.kf_clear()
    _fill(c, store, lids)
    for order in ([3, 9, 5, 7, 4], [9, 3, 5, 7, 4], [3, 5, 7, 4, 9]):
        ref = _check_union(c, store, lids, order, what=order)
        assert np.array_equal(ref[0], store[9][0]) and np.array_equal(ref[2], same)
    # bit-identical entries too
    for i in (3, 5):
        store[i] = store[9]
    _fill(c, store, lids)
    _check_union(c, store, lids, [3, 9, 5])
    # 64 entries of 0 .. 40 landmarks from a pool of 300, with repeats inside some of them; fresh-id entries among them
    store, lids = {}, {}
    for k in range(64):
        n = int(rng.integers(0, 41))
        l = 2000 + rng.permutation(300)[:n]
        if k % 7 == 3 and n > 3:
            l[n - 1] = l[0]                                           # a repeat inside the entry: the higher position wins
        store[100 + 3 * k], lids[100 + 3 * k] = _entry(rng, l)
    c.kf_clear()
    _fill(c, store, lids)
    (fd, fw), _ = _entry(rng, range(12))
    c.kf_add(50, fd, fw)                                              # fresh ids: shared with nobody
    store[50], lids[50] = (fd, fw), c.kf_read_ids(50)
    assert np.all(lids[50] >= 1 << 62)
    ids = sorted(i for i in store if i >= 100)
    for order in (ids, ids[::-1], [int(i) for i in rng.permutation(ids)], [50] + ids[:63], ids[:30] + [50] + ids[31:64]):
        assert len(order) == 64
        ref = _check_union(c, store, lids, order, what="64")
        assert len(ref[2]) < sum(len(lids[i]) for i in order)         # the lists overlap
    got = c.kf_covisible(ids[5], ids)                                 # n_ids = 64, self included
    assert np.array_equal(got, lm.covisible(lids, ids[5], ids)) and got.max() > 0
    rep = next(i for i in ids if len(np.unique(lids[i])) < len(lids[i]))
    assert np.array_equal(c.kf_covisible(rep, ids + []), lm.covisible(lids, rep, ids))
    assert np.array_equal(c.kf_covisible(ids[5], [rep, rep, 50]), lm.covisible(lids, ids[5], [rep, rep, 50]))
    c.close()


def test_union_capacity_and_errors(pkg, sized):
    store, lids = dict(sized[0]), dict(sized[1])
    rng = np.random.default_rng(5)
    store[30], lids[30] = _entry(rng, [5000])                          # one landmark nobody else has
    c = _ctx(pkg)
    _fill(c, store, lids)
    assert c.kf_union(900, [17, 15]) == 320
    # 321 distinct landmarks: E_CAPACITY, the count that was needed, an entry of 0 landmarks
    with pytest.raises(pkg.MslamHipError) as e:
        c.kf_union(900, [17, 30])
    assert e.value.code == pkg.E_CAPACITY and e.value.needed == 321
    assert len(c.kf_read_ids(900)) == 0 and len(c.kf_read(900)[0]) == 0
    with pytest.raises(pkg.MslamHipError) as e:
        c.kf_union(901, [30, 16, 17, 10])                              # a dst that did not exist
    assert e.value.code == pkg.E_CAPACITY and e.value.needed == 321 and len(c.kf_read_ids(901)) == 0
    c.sync()                                                           # the synchronous form left nothing behind
    # the _dev form reports it through sync, once
    assert c.kf_union(902, [17, 30], sync=False) is None
    with pytest.raises(pkg.MslamHipError) as e:
        c.sync()
    assert e.value.code == pkg.E_CAPACITY
    c.sync()
    assert len(c.kf_read_ids(902)) == 0
    c.kf_union(902, [16, 30], sync=False)                              # and one that fits: nothing to report
    c.sync()
    _same(_read(c, 902), lm.union(store, lids, [16, 30]))
    # dst replaced by a second union
    _check_union(c, store, lids, [12, 13], dst=900)
    _check_union(c, store, lids, [16, 14], dst=900)
    _check_union(c, store, lids, [10], dst=900)
    # dst among the ids, a repeated id, an unknown id, an empty or too long list: E_INVALID, the store unchanged
    before = {i: _read(c, i) for i in list(store) + [900, 901, 902]}
    for dst, bad in ((900, [12, 900]), (12, [12, 13]), (903, [12, 13, 12]), (903, [12, 777]), (777, [777]), (903, []),
                     (903, list(range(10, 18)) * 8 + [30])):
        with pytest.raises(pkg.MslamHipError) as e:
            c.kf_union(dst, bad)
        assert e.value.code == pkg.E_INVALID, (dst, bad)
        with pytest.raises(pkg.MslamHipError) as e:
            c.kf_union(dst, bad, sync=False)
        assert e.value.code == pkg.E_INVALID, (dst, bad)
    c.sync()
    assert c.kf_size() == len(before)
    for i, s in before.items():
        _same(_read(c, i), s, i)
    for bad in ((777, [12]), (12, [777]), (12, [12] * 65)):
        with pytest.raises(pkg.MslamHipError) as e:
            c.kf_covisible(*bad)
        assert e.value.code == pkg.E_INVALID
    assert len(c.kf_covisible(12, [])) == 0
    c.close()


def test_covisible_equals_the_reference(pkg, sized):
    store, lids = sized
    c = _ctx(pkg)
    _fill(c, store, lids)
    ids = sorted(store)
    for i in ids:                                                      # self, the empty entry and the full one on both sides
        got = c.kf_covisible(i, ids)
        assert np.array_equal(got, lm.covisible(lids, i, ids)), i
        assert got[ids.index(i)] == len(lids[i])
    assert np.array_equal(c.kf_covisible(16, [17, 10, 16, 11][::-1]), lm.covisible(lids, 16, [11, 16, 10, 17]))
    c.close()


# ---- track on a union ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sequence(orc):
    seq = tr.make_sequence(seed=0)
    rows, trk = lm.run(seq, None)
    # the loop's fresh ids as caller ids: the same identities, numbered 0 ..
    every = np.unique(np.concatenate([trk.lids[i] for i in trk.ids]))
    lids = {i: np.searchsorted(every, trk.lids[i]).astype(np.int64) for i in trk.ids}
    return seq, rows, trk, lids


@KINDS
def test_track_on_a_union_equals_the_reference(pkg, sequence, kind):
    """frame 7 of the sequence, the one after keyframe 1's, against the union of keyframes 0 and 1 in both list orders,
    with a threshold that makes the step insert a keyframe"""
    seq, rows, trk, all_lids = sequence
    f, kf_min, U = 7, 1 << 20, 900
    fr = seq["frames"][f]
    assert rows[f - 1]["keyframe"] == 1 and rows[f - 1]["reference"] == 1
    store, lids = {i: trk.store[i] for i in (0, 1)}, {i: all_lids[i] for i in (0, 1)}
    shared = lm.covisible(lids, 1, [0])[0]
    assert 0 < shared < len(lids[0])
    guess = (rows[f - 1]["R"], rows[f - 1]["t"])
    single = tr.track(fr["desc"], fr["xy"], fr["depth"], store, 1, [0, 1], seed=f, guess=guess, new_keyframe_min_landmarks=kf_min)
    for order in ([0, 1], [1, 0]):
        c = _ctx(pkg, kind, max_keypoints=2048)
        _fill(c, store, lids)                                          # serials 1, 2
        ud, uw, ul = lm.union(store, lids, order)
        assert c.kf_union(U, order) == len(ul) == len(lids[0]) + len(lids[1]) - shared          # serial 3
        ustore = dict(store)
        ustore[U] = (ud, uw)
        ref = tr.track(fr["desc"], fr["xy"], fr["depth"], ustore, U, [0, 1], seed=f, guess=guess, new_keyframe_min_landmarks=kf_min)
        got = c.track(fr["desc"], fr["xy"], fr["depth"], U, [0, 1], 7, seed=f, rvec=_rvec(guess[0]), tvec=guess[1],
                      new_keyframe_min_landmarks=kf_min, with_pairs=True, with_entry=True)      # serial 4
        _compare_step(got, ref, (kind, order))
        assert c.last_match_kernel() == ("matrix", "popcount")[kind]
        assert got["tracked"] and got["keyframe_added"] and got["n_correspondences"] > single["n_correspondences"]
        e = _compare_entry(c, got, ref, fr, ustore, U, 7)
        na = e["n_inherited"]
        gl = c.kf_read_ids(7)
        assert np.array_equal(gl[:na], ul[e["src"][:na]])              # part A: the union's ids at entry_src
        assert np.array_equal(gl[na:], lm.fresh_ids(4, len(gl) - na, na))   # part B: fresh under the new serial
        assert len(np.unique(gl)) == len(gl)
        new_lids = dict(lids)
        new_lids[7], new_lids[U] = gl, ul
        assert np.array_equal(c.kf_covisible(7, [0, 1, U, 7]), lm.covisible(new_lids, 7, [0, 1, U, 7]))
        assert lm.covisible(new_lids, 7, [0])[0] > 0 and lm.covisible(new_lids, 7, [U])[0] == na
        _same(_read(c, U), (ud, uw, ul), "the union after the step")
        # relocalize runs on the union as on any entry
        q = c.relocalize(fr["desc"], fr["xy"], [U, 0], CAM[:2], CAM[2:], seed=3, min_inliers=0)
        r = rr.relocalize(fr["desc"], fr["xy"], ustore, [U, 0], CAM, seed=3, min_inliers=0)
        assert q["best"] == r["best"] and [x["n_inliers"] for x in q["candidates"]] == [x["n_inliers"] for x in r["candidates"]]
        c.close()


# ---- the tracker ----------------------------------------------------------------------------------------------------------

def _run_tracker(pkg, seq, depth, max_keypoints):
    c = _ctx(pkg, 0, max_keypoints)
    t = pkg.HipKeyframeTracker(c, focal=CAM[:2], principal=CAM[2:], local_map_depth=depth, **tr.SEQ_PARAMS)
    got = [t.processSensorData(fr["desc"], fr["xy"], fr["depth"]) for fr in seq["frames"]]
    return c, t, got


def _compare_rows(seq, got, rows):
    for f, (a, b, fr) in enumerate(zip(got, rows, seq["frames"])):
        nc = a["step"]["n_correspondences"] if a["step"] else 0
        print(f, "tracked", a["tracked"], "correspondences", nc, "inliers", a["n_inliers"], "reference", a["reference"],
              "keyframe", a["keyframe"], "| pose difference", rr.rot_err(a["R"], b["R"]), float(np.linalg.norm(a["tvec"] - b["t"])))
        assert (a["tracked"], a["keyframe"], a["reference"], nc, a["n_inliers"], a["relocalized"]) == \
               (b["tracked"], b["keyframe"], b["reference"], b["n_correspondences"], b["n_inliers"], b["relocalized"]), f
        # the existing tracker test's tolerance (0.1 degrees, 2 cm), against the reference loop and against ground truth
        assert rr.rot_err(a["R"], b["R"]) < 0.1 and np.linalg.norm(a["tvec"] - b["t"]) < 0.02, f
        assert rr.rot_err(a["R"], fr["R"]) < 0.1 and np.linalg.norm(a["tvec"] - fr["t"]) < 0.02, f


@pytest.mark.parametrize("which", ["scene", "sequence"])
def test_tracker_with_a_local_map_equals_the_reference_loop(pkg, orc, which):
    seq = lm.make_scene() if which == "scene" else tr.make_sequence(seed=0)
    rows, trk = lm.run(seq, 2)
    assert max(len(trk.store[i][0]) for i in trk.ids) < 4096
    c, t, got = _run_tracker(pkg, seq, 2, 4096)
    _compare_rows(seq, got, rows)
    assert t.ids == trk.ids and t.graph == trk.graph and t.local_map == trk.local
    assert c.kf_size() == len(trk.ids) + 1 and t.LOCAL_MAP_ID not in t.ids      # the keyframes and the reserved union entry
    for i in trk.ids:                                                 # the same identities, serials included
        assert np.array_equal(c.kf_read_ids(i), trk.lids[i]), i
        assert np.array_equal(c.kf_read(i)[0], trk.store[i][0])
    assert np.array_equal(c.kf_read_ids(t.LOCAL_MAP_ID), trk.map[2])
    if which == "scene":
        single, _ = lm.run(seq, None)
        k1 = next(f for f, r in enumerate(rows) if r["keyframe"] == 1)
        assert got[k1 + 1]["step"]["n_correspondences"] > single[k1 + 1]["n_correspondences"]
    c.close()


def test_tracker_without_a_local_map_is_todays_tracker(pkg, orc):
    seq = lm.make_scene()
    rows, trk = tr.run_reference(seq)
    c, t, got = _run_tracker(pkg, seq, None, 1024)
    c0 = _ctx(pkg, 0, 1024)
    t0 = pkg.HipKeyframeTracker(c0, focal=CAM[:2], principal=CAM[2:], **tr.SEQ_PARAMS)       # as every caller of today builds it
    for f, (fr, a, b) in enumerate(zip(seq["frames"], got, rows)):
        o = t0.processSensorData(fr["desc"], fr["xy"], fr["depth"])
        assert (a["tracked"], a["n_inliers"], a["keyframe"], a["reference"], a["relocalized"]) == \
               (o["tracked"], o["n_inliers"], o["keyframe"], o["reference"], o["relocalized"]), f
        assert (a["tracked"], a["keyframe"], a["reference"], a["relocalized"]) == (b["tracked"], b["keyframe"], b["reference"], b["relocalized"]), f
        assert np.array_equal(a["R"], o["R"]) and np.array_equal(a["tvec"], o["tvec"]), f
    assert t.ids == t0.ids == trk.ids and c.kf_size() == len(trk.ids) and t.graph == {0: set()}
    for i in trk.ids:
        assert np.array_equal(c.kf_read(i)[1], c0.kf_read(i)[1])
    c.close()
    c0.close()


def test_harness_tracks_with_a_local_map_as_the_python_tracker(pkg, orc, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth
    host = os.path.join(ROOT, "modular-slam_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    seq = lm.make_scene()
    c, t, got = _run_tracker(pkg, seq, 2, 4096)
    voc = tmp_path / "orbvoc.dbow3"
    voc.write_bytes(synth.make_vocabulary(10, 4, seed=5))
    path = tmp_path / "scene.bin"
    tr.write_scene(str(path), seq, seed=0)
    r = subprocess.run([os.path.join(host, "mslam_harness"), os.path.join(host, "libmslam_hip_plugin.so"), "--track", str(voc),
                        str(path), "--local-map", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("track frame ")]
    print("\n".join(lines))
    assert len(lines) == len(got)
    for f, (line, a) in enumerate(zip(lines, got)):
        tok = line.split()
        assert int(tok[2]) == f
        rv, tv = np.array([float(x) for x in tok[8:11]]), np.array([float(x) for x in tok[12:15]])
        assert (bool(int(tok[4])), int(tok[6]), int(tok[16]), int(tok[18]), bool(int(tok[20]))) == \
               (a["tracked"], a["n_inliers"], a["reference"], a["keyframe"], a["relocalized"]), f
        assert np.abs(rv - a["rvec"]).max() < 1e-9 and np.abs(tv - a["tvec"]).max() < 1e-9, f      # the same library, the same calls
    assert [int(l.split()[18]) for l in lines if int(l.split()[18]) >= 0] == t.ids
    c.close()
