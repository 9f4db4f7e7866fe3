"""The union's DISTINCTIVE descriptor mode on the GPU, through the C ABI: mslam_hip_kf_union[_dev] with
mslam_hip_set_union_descriptor(DISTINCTIVE) byte for byte against tests/distinct_ref.py::union on the cases of
tests/distinct_cases.py (tests/test_distinct_union.py shows on the CPU that each case is what it is named after), the mode
as context state, mslam_hip_track on such a union, and HipKeyframeTracker(union_descriptor="distinctive") row for row
against DistinctLocalMapTracker — also through `harness --track --local-map 2 --distinct`."""
import os
import subprocess
import sys

import numpy as np
import pytest

import distinct_cases as dc
import distinct_ref as dr
import local_map_ref as lm
import track_ref as tr
from test_gpu_local_map import _compare_rows, _fill, _read, _same
from test_gpu_track import _compare_step, _rvec

CAM = tr.CAM
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 900


def _ctx(pkg, mode="distinctive", max_keypoints=dc.K):
    c = pkg.Context(width=0, height=0, max_keypoints=max_keypoints)
    if mode is not None:
        c.set_union_descriptor(mode)
    return c


def _check(c, store, lids, ids, dst=U, what="", ref_union=dr.union):
    ref = ref_union(store, lids, ids)
    n = c.kf_union(dst, ids)
    assert n == len(ref[2]), (what, n, len(ref[2]))
    _same(_read(c, dst), ref, what)
    return ref


# ---- the cases -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ladder():
    store, lids, order = dc.ladder()
    return store, lids, order, dr.union(store, lids, order)


def test_n_ladder(pkg, ladder):
    store, lids, order, ref = ladder
    c = _ctx(pkg)
    _fill(c, store, lids)
    assert c.kf_union(U, order) == len(ref[2]) == 192
    got = _read(c, U)
    _same(got, ref, "ladder")
    recent = lm.union(store, lids, order)
    n = dr.counts(lids, order, ref[2])
    differ = (got[0] != recent[0]).any(axis=1)
    print("rows whose descriptor is not the most recent one:", int(differ.sum()), "of", len(n))
    assert differ.sum() > 100 and differ[n >= 63].any()
    for other in (sorted(order), sorted(order)[::-1], order[:33], order[40:43]):
        _check(c, store, lids, other, what=len(other))
    for i in order:                                                       # the listed entries are not written
        _same(_read(c, i), (store[i][0], store[i][1], lids[i]), i)
    c.close()


def test_ties_and_extremes(pkg):
    store, lids, order, winners = dc.ties()
    c = _ctx(pkg)
    _fill(c, store, lids)
    for o in (order, sorted(order), sorted(order)[::-1]):
        d, _, l = _check(c, store, lids, o, what=o)
        gd = c.kf_read(U)[0]
        for landmark, kf in winners.items():
            assert np.array_equal(gd[np.flatnonzero(l == landmark)[0]], store[kf][0][np.flatnonzero(lids[kf] == landmark)[0]]), landmark
        assert np.array_equal(gd[np.flatnonzero(l == dc.EXTREME)[0]], dc.ONES)          # a nine-bit median
    _check(c, store, lids, [30, 40, 50], what="N = 3 everywhere")
    c.close()


def test_repeats_count_once_at_the_highest_position(pkg):
    store, lids, order, ideal = dc.repeats()
    c = _ctx(pkg)
    _fill(c, store, lids)
    for o in (order, sorted(order), [4, 3, 2, 1]):
        d, _, l = _check(c, store, lids, o, what=o)
        assert not np.array_equal(c.kf_read(U)[0][np.flatnonzero(l == dc.REPEATED)[0]], ideal)
    c.close()


def test_sizes(pkg):
    store, lids, orders = dc.sizes()
    c = _ctx(pkg)
    _fill(c, store, lids)
    for o in orders:
        _check(c, store, lids, o, what=o)
    for i in sorted(store):                                               # n_ids = 1: the entry itself, as in the recent mode
        ref = _check(c, store, lids, [i], what=("single", i))
        _same(ref, lm.union(store, lids, [i]))
    for pair in ([12, 13], [14, 10]):                                     # n_ids = 2: the recent union
        _same(_check(c, store, lids, pair, what=pair), lm.union(store, lids, pair))
    c.close()


def test_probe_chains(pkg):
    store, lids, order = dc.chains()
    c = _ctx(pkg)
    _fill(c, store, lids)
    for o in (order, sorted(order), order[:3]):
        ref = _check(c, store, lids, o, what=o)
        assert (ref[0] != lm.union(store, lids, o)[0]).any()
    c.close()


def test_capacity_in_both_forms(pkg):
    store, lids, too_many, needed, fits = dc.capacity()
    c = _ctx(pkg)
    _fill(c, store, lids)
    _check(c, store, lids, fits)
    with pytest.raises(pkg.MslamHipError) as e:
        c.kf_union(U, too_many)
    assert e.value.code == pkg.E_CAPACITY and e.value.needed == needed
    assert len(c.kf_read_ids(U)) == 0 and len(c.kf_read(U)[0]) == 0
    c.sync()                                                              # the synchronous form left nothing behind
    _check(c, store, lids, fits, what="after E_CAPACITY")                 # the scratch is not poisoned
    assert c.kf_union(U + 1, too_many, sync=False) is None
    with pytest.raises(pkg.MslamHipError) as e:
        c.sync()
    assert e.value.code == pkg.E_CAPACITY
    c.sync()
    assert len(c.kf_read_ids(U + 1)) == 0
    c.kf_union(U + 1, fits[::-1], sync=False)
    c.sync()
    _same(_read(c, U + 1), dr.union(store, lids, fits[::-1]), "the _dev form after its overflow")
    for i in sorted(store):
        _same(_read(c, i), (store[i][0], store[i][1], lids[i]), i)
    c.close()


def test_mode_is_context_state(pkg):
    store, lids, order = dc.chains()
    c = _ctx(pkg, mode=None)
    assert c.get_union_descriptor() == pkg.UNION_DESC_RECENT               # the default
    for i, (d, w) in store.items():                                       # fresh ids for one more entry below: serials 1 .. 5
        c.kf_add(i, d, w, lids=lids[i])
    recent = _check(c, store, lids, order, ref_union=lm.union)            # serial 6
    c.set_union_descriptor(pkg.UNION_DESC_DISTINCTIVE)
    assert c.get_union_descriptor() == pkg.UNION_DESC_DISTINCTIVE
    assert np.array_equal(c.kf_covisible(3, order), lm.covisible(lids, 3, order))       # shares the table scratch
    distinct = _check(c, store, lids, order)                              # serial 7
    assert (distinct[0] != recent[0]).any()
    for bad in (2, -1, 7):
        with pytest.raises(pkg.MslamHipError) as e:
            c.set_union_descriptor(bad)
        assert e.value.code == pkg.E_INVALID and c.get_union_descriptor() == pkg.UNION_DESC_DISTINCTIVE
    with pytest.raises(pkg.MslamHipError) as e:
        c.set_union_descriptor("median")
    assert e.value.code == pkg.E_INVALID
    _check(c, store, lids, order, what="after the rejected modes")        # serial 8
    c.set_union_descriptor("recent")
    assert c.get_union_descriptor() == pkg.UNION_DESC_RECENT
    assert np.array_equal(c.kf_covisible(5, order), lm.covisible(lids, 5, order))
    _check(c, store, lids, order, ref_union=lm.union, what="recent again")               # serial 9
    # serials and fresh ids do not depend on the mode: a context that stayed in the recent mode made the same calls
    c0 = _ctx(pkg, mode=None)
    for i, (d, w) in store.items():
        c0.kf_add(i, d, w, lids=lids[i])
    for _ in range(4):
        c0.kf_union(U, order)
    rng = np.random.default_rng(9)
    fd, fw = rng.integers(0, 256, (12, 32), dtype=np.uint8), rng.normal(size=(12, 3))
    c.kf_add(77, fd, fw)
    c0.kf_add(77, fd, fw)
    assert np.array_equal(c.kf_read_ids(77), c0.kf_read_ids(77)) and np.array_equal(c.kf_read_ids(77), lm.fresh_ids(10, 12))
    c.close()
    c0.close()


def test_the_same_bytes_every_time(pkg, ladder):
    store, lids, order, ref = ladder
    c = _ctx(pkg)
    _fill(c, store, lids)
    c.kf_union(U, order)
    first = _read(c, U)
    c.kf_union(U + 1, order)
    _same(_read(c, U + 1), first, "twice in one context")
    c.close()
    c = _ctx(pkg)
    _fill(c, store, lids)
    c.kf_union(U, order)
    _same(_read(c, U), first, "a fresh context")
    _same(first, ref)
    c.close()


# ---- tracking ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def loop(orc):
    """the reference loop on the distinctive union, once for the tests below"""
    seq = tr.make_sequence(seed=3, n_frames=24, n_landmarks=400, n_distractors=60)
    rows, trk = dr.run(seq, 2)
    return seq, rows, trk


def test_track_on_a_distinctive_union_equals_the_reference(pkg, loop):
    """the last frame of the sequence against the distinctive union of the last six keyframes: an ordinary entry"""
    seq, rows, trk = loop
    members = trk.ids[-7:-1]
    every = np.unique(np.concatenate([trk.lids[i] for i in members]))          # the loop's fresh ids as caller ids
    store = {i: trk.store[i] for i in members}
    lids = {i: np.searchsorted(every, trk.lids[i]).astype(np.int64) for i in members}
    order = members[::-1]
    ud, uw, ul = dr.union(store, lids, order)
    assert (ud != lm.union(store, lids, order)[0]).any()
    f = len(seq["frames"]) - 1
    fr, guess = seq["frames"][f], (rows[f - 1]["R"], rows[f - 1]["t"])
    c = _ctx(pkg, max_keypoints=1024)
    _fill(c, store, lids)
    assert c.kf_union(U, order) == len(ul)
    ustore = dict(store)
    ustore[U] = (ud, uw)
    ref = tr.track(fr["desc"], fr["xy"], fr["depth"], ustore, U, members, seed=f, guess=guess, new_keyframe_min_landmarks=1 << 20)
    got = c.track(fr["desc"], fr["xy"], fr["depth"], U, members, 77, seed=f, rvec=_rvec(guess[0]), tvec=guess[1],
                  new_keyframe_min_landmarks=1 << 20, with_pairs=True, with_entry=True)
    _compare_step(got, ref, "distinctive union")
    assert got["tracked"] and got["keyframe_added"]
    na = got["n_inherited"]
    assert na > 0 and np.array_equal(c.kf_read_ids(77)[:na], ul[got["entry_src"][:na]])    # part A inherits the union's ids
    _same(_read(c, U), (ud, uw, ul), "the union after the step")
    c.close()


def test_tracker_with_a_distinctive_local_map_equals_the_reference_loop(pkg, loop):
    seq, rows, trk = loop
    print("unions (rows, rows that differ from the recent mode, largest N):", trk.unions)
    assert len(trk.unions) >= 10 and max(u[1] for u in trk.unions) >= 1 and max(u[2] for u in trk.unions) >= 3    # not vacuous
    assert max(u[0] for u in trk.unions) <= 1024 and max(len(trk.store[i][0]) for i in trk.ids) <= 1024
    c = _ctx(pkg, mode=None, max_keypoints=1024)
    t = pkg.HipKeyframeTracker(c, focal=CAM[:2], principal=CAM[2:], local_map_depth=2, union_descriptor="distinctive", **tr.SEQ_PARAMS)
    assert c.get_union_descriptor() == pkg.UNION_DESC_DISTINCTIVE
    got = [t.processSensorData(fr["desc"], fr["xy"], fr["depth"]) for fr in seq["frames"]]
    _compare_rows(seq, got, rows)
    assert t.ids == trk.ids and t.graph == trk.graph and t.local_map == trk.local
    for i in trk.ids:
        assert np.array_equal(c.kf_read_ids(i), trk.lids[i]), i
        assert np.array_equal(c.kf_read(i)[0], trk.store[i][0])
    # the final local map: descriptors and ids are the reference loop's; world points are the device's own (the lift on the
    # device and in numpy agree to rounding only, which is why the rows above carry a tolerance), so all three are compared
    # with the distinctive union of the store as the device holds it
    gd, gw, gl = _read(c, t.LOCAL_MAP_ID)
    assert np.array_equal(gl, trk.map[2]) and np.array_equal(gd, trk.map[0])
    held = {i: c.kf_read(i) for i in trk.local}
    _same((gd, gw, gl), dr.union(held, trk.lids, trk.local), "the final local map")
    recent = lm.union(trk.store, trk.lids, trk.local)
    assert np.array_equal(recent[2], trk.map[2]) and (recent[0] != trk.map[0]).any()
    c.close()


def test_harness_distinct_flag_tracks_as_the_python_tracker(pkg, loop, tmp_path):
    import synth
    seq, rows, trk = loop
    host = os.path.join(ROOT, "modular-slam_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    c = _ctx(pkg, mode=None, max_keypoints=4096)
    t = pkg.HipKeyframeTracker(c, focal=CAM[:2], principal=CAM[2:], local_map_depth=2, union_descriptor="distinctive", **tr.SEQ_PARAMS)
    got = [t.processSensorData(fr["desc"], fr["xy"], fr["depth"]) for fr in seq["frames"]]
    voc = tmp_path / "orbvoc.dbow3"
    voc.write_bytes(synth.make_vocabulary(10, 4, seed=5))
    path = tmp_path / "scene.bin"
    tr.write_scene(str(path), seq, seed=0)
    exe, plugin = os.path.join(host, "mslam_harness"), os.path.join(host, "libmslam_hip_plugin.so")
    r = subprocess.run([exe, plugin, "--track", str(voc), str(path), "--local-map", "2", "--distinct"], capture_output=True, text=True,
                       timeout=300)
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
    # the flag needs the local map
    r = subprocess.run([exe, plugin, "--track", str(voc), str(path), "--distinct"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 6 and "--distinct" in r.stderr
    c.close()
