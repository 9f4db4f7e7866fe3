"""The match-to-PnP sequence's row, correspondence, entry and lift edges on the GPU, through the C ABI: seq_enqueue
(k_reloc_gather_desc, matcher, k_reloc_corr, PnP, k_reloc_rank), track_keyframe_block through mslam_hip_track and
mslam_hip_track_window, and k_kf_lift, on the inputs of tests/seq_edge_cases.py (which tests/test_seq_edge_cases.py proves
to meet their conditions) against tests/reloc_ref.py, tests/track_ref.py and tests/track_window_ref.py.  The rules are
those of tests/test_gpu_reloc.py::_compare and tests/test_gpu_track.py::_compare_entry: pairs, counts, status, masks, best,
entry_src and entry_kp equal, descriptors and world points bit for bit, poses within 1e-7.  Both matcher kinds throughout."""
import numpy as np
import pytest

import reloc_ref as rr
import seq_edge_cases as sec
import track_ref as tr
from test_gpu_reloc import _compare
from test_gpu_track import KINDS, _bits_equal, _compare_step, _ctx, _fill, _same_store, _snapshot
from test_gpu_track_window import _same_record

pytestmark = pytest.mark.gpu
ZERO = dict(rvec=np.zeros(3), tvec=np.zeros(3))          # the identity guess
SMALL_CAM, SMALL_W, SMALL_H = (330.0, 330.0, 199.5, 149.5), 400, 300


def _entry_equals(c, got, ref, fr, ref_world, ref_lids, new_id, K, z_max=3.0):
    """test_gpu_track.py::_compare_entry with the store's capacity and the landmark ids: the reference's construction fed with
    the device's own pairs, mask and pose and cut at K; part A inherits the reference entry's ids at entry_src, part B gets
    lid_base | o with o continuing behind part A"""
    e = tr.build_entry(fr["desc"], ref["xyz"], ref["valid"], got["pairs"], got["inliers"], ref_world, got["R"], got["tvec"], z_max,
                       capacity=K)
    gd, gw = c.kf_read(new_id)
    lids = c.kf_read_ids(new_id)
    n, na = len(e["kp"]), e["n_inherited"]
    assert (got["n_entry"], got["n_inherited"]) == (n, na) and len(gd) == len(gw) == len(lids) == n <= K
    assert np.array_equal(got["entry_src"], e["src"]) and np.array_equal(got["entry_kp"], e["kp"])
    assert np.array_equal(gd, e["desc"])
    assert np.array_equal(gw.view(np.uint64), e["world"].view(np.uint64))
    assert np.array_equal(lids[:na], np.asarray(ref_lids)[e["src"][:na]])
    fresh = lids[na:]
    assert (fresh >> 62 == 1).all() and np.array_equal(fresh & 0xFFFF, np.arange(na, n)) and len(set((fresh >> 16).tolist())) <= 1
    return e


# ---- A: twins and the cut at cap ------------------------------------------------------------------------------------------

@KINDS
@pytest.mark.parametrize("copies", [2, 3])
def test_twins_and_the_cut_at_capacity(pkg, orc, kind, copies):
    tc, ref = sec.twin_case(copies), sec.twin_track(copies)
    K, fr = tc["K"], tc["frame"]
    c = _ctx(pkg, kind, K)
    c.kf_add(0, *tc["store"][0], lids=tc["lids"])
    got = c.track(fr["desc"], fr["xy"], fr["depth"], 0, [0], 7, seed=tc["seed"], new_keyframe_min_landmarks=sec.BIG, with_pairs=True,
                  with_entry=True, **ZERO)
    _compare_step(got, ref, ("twins", copies))
    assert got["keyframe_added"]
    e = _entry_equals(c, got, ref, fr, tc["store"][0][1], tc["lids"], 7, K)
    na = e["n_inherited"]
    print("copies", copies, "K", K, "entry", len(e["kp"]), "inherited", na, "distinct", len(set(e["kp"][:na].tolist())))
    assert (len(e["kp"]), na) == ((220, 102), (K, 153))[copies - 2] and len(set(e["kp"][:na].tolist())) == 51
    assert np.array_equal(got["entry_kp"], ref["entry"]["kp"]) and np.array_equal(got["entry_src"], ref["entry"]["src"])
    if copies == 3:
        # the next frame against the cut entry, whose size the host now knows exactly
        store, nx = {7: c.kf_read(7), 0: tc["store"][0]}, tc["next"]
        ref2 = tr.track(nx["desc"], nx["xy"], nx["depth"], store, 7, [7, 0], seed=2, guess=sec.IDENTITY)
        got2 = c.track(nx["desc"], nx["xy"], nx["depth"], 7, [7, 0], -1, seed=2, with_pairs=True, **ZERO)
        _compare_step(got2, ref2, "next")
        assert got2["tracked"] and got2["n_inliers"] >= 30
    c.close()


# ---- B: the same through track_window, the event at frame 1 -----------------------------------------------------------------

@KINDS
def test_twins_through_a_window_whose_event_is_frame_1(pkg, orc, kind):
    tc, w = sec.twin_case(3), sec.twin_window()
    K, frames, seed = tc["K"], w["frames"], w["seed"]
    c = _ctx(pkg, kind, K)
    c.kf_add(0, *tc["store"][0], lids=tc["lids"])
    recs, first = c.track_window([x["desc"] for x in frames], [x["xy"] for x in frames], [x["depth"] for x in frames], 0, [0], 7, 0,
                                 seed=seed, new_keyframe_min_landmarks=w["kf_min"], with_entry=True, **ZERO)
    assert first == w["first"] == 1 and [r["keyframe_added"] for r in recs] == [0, 1, 0]
    singles = []
    for s, fr in enumerate(frames):
        one = c.track(fr["desc"], fr["xy"], fr["depth"], 0, [0], -1, seed=seed + s, new_keyframe_min_landmarks=w["kf_min"],
                      with_pairs=True, **ZERO)
        _same_record(recs[s], one, s)
        _compare_step(one, w["steps"][s], ("window", s))
        singles.append(one)
    got = dict(singles[1], n_entry=recs[1]["n_entry"], n_inherited=recs[1]["n_inherited"], entry_src=recs[1]["entry_src"],
               entry_kp=recs[1]["entry_kp"])
    e = _entry_equals(c, got, w["steps"][1], frames[1], tc["store"][0][1], tc["lids"], 7, K)
    assert (len(e["kp"]), e["n_inherited"]) == (K, 153)
    # and the single-frame call's entry: the same bytes, the same ids but for the serial of the fresh ones
    one = c.track(frames[1]["desc"], frames[1]["xy"], frames[1]["depth"], 0, [0], 8, seed=seed + 1, new_keyframe_min_landmarks=w["kf_min"],
                  with_entry=True, **ZERO)
    assert one["keyframe_added"] and (one["n_entry"], one["n_inherited"]) == (recs[1]["n_entry"], recs[1]["n_inherited"])
    assert np.array_equal(one["entry_src"], recs[1]["entry_src"]) and np.array_equal(one["entry_kp"], recs[1]["entry_kp"])
    (da, wa), (db, wb), la, lb = c.kf_read(7), c.kf_read(8), c.kf_read_ids(7), c.kf_read_ids(8)
    assert np.array_equal(da, db) and np.array_equal(wa.view(np.uint64), wb.view(np.uint64))
    assert np.array_equal(la[:153], lb[:153]) and np.array_equal(la[153:] & 0xFFFF, lb[153:] & 0xFFFF)
    c.close()


# ---- C: k correspondences on dirty scratch -------------------------------------------------------------------------------

@KINDS
def test_k_correspondences_after_a_larger_call(pkg, orc, kind):
    sc = sec.few_scene()
    tid = sc["target_id"]
    c = _ctx(pkg, kind)
    _fill(c, sc["store"])
    for k in range(8):
        full = c.relocalize(sc["desc"], sc["xy"], [tid], seed=1, with_pairs=True)       # leaves ones in the mask row
        _compare(full, sec.few_full(), "full")
        assert full["inliers"][0].all() and len(full["inliers"][0]) == 538
        ref = sec.few_ref(k)
        got = c.relocalize(sc["desc"], sc["xy"], [tid], valid=sec.few_valid(k), seed=1, with_pairs=True)
        _compare(got, ref, ("k", k))
        g = got["candidates"][0]
        assert (g["n_matches"], g["n_correspondences"], g["status"]) == (538, k, int(k >= 5)) and len(got["inliers"][0]) == k
        assert got["inliers"][0].all() if k >= 5 else not got["inliers"][0].any()
        assert got["best"] == -1                                                            # (min_inliers = 60)
    c.close()


@KINDS
def test_track_with_k_valid_depths(pkg, orc, kind):
    base = sec.zmax_case()
    c = _ctx(pkg, kind)
    _fill(c, base["store"])
    snap = _snapshot(c, [0])
    for k in range(8):
        fr = base["frame"]                                                                  # an ordinary step first
        full = c.track(fr["desc"], fr["xy"], fr["depth"], 0, [0], -1, seed=1, new_keyframe_min_landmarks=sec.BIG, with_pairs=True, **ZERO)
        _compare_step(full, base["ref"], "full")
        assert full["tracked"] and full["inliers"].sum() > 30
        fd = sec.few_depth(k)
        fr = fd["frame"]
        got = c.track(fr["desc"], fr["xy"], fr["depth"], 0, [0], 9, seed=1, new_keyframe_min_landmarks=sec.BIG, with_pairs=True,
                      with_entry=True, **ZERO)
        _compare_step(got, fd["ref"], ("depth", k))
        assert got["n_correspondences"] == k and got["status"] == int(k >= 5) and not got["tracked"] and not got["keyframe_added"]
        assert got["n_entry"] == 0 and len(got["entry_src"]) == 0 and not got["vote_counts"].any() and got["vote_best"] == -1
        assert got["inliers"].all() if k >= 5 else not got["inliers"].any()
        _same_store(c, snap)
    c.close()


# ---- D: full and adjacent rows -----------------------------------------------------------------------------------------------

@KINDS
@pytest.mark.parametrize("n_cand", [2, 64])
@pytest.mark.parametrize("n", sec.FULL_SIZES)
def test_full_and_adjacent_rows(pkg, orc, kind, n, n_cand):
    case, ref = sec.full_rows(n, n_cand), sec.full_ref(n, n_cand)
    c = _ctx(pkg, kind)
    _fill(c, case["store"])
    got = c.relocalize(case["desc"], case["xy"], case["ids"], seed=3, with_pairs=True)
    _compare(got, ref, (n, n_cand))
    assert all(g["n_matches"] == g["n_correspondences"] == n for g in got["candidates"])
    c.close()


@KINDS
def test_valid_patterns_that_empty_waves_and_chunks(pkg, orc, kind):
    n = 512
    case = sec.full_rows(n, 2)
    c = _ctx(pkg, kind)
    _fill(c, case["store"])
    for pattern in sec.VALID_PATTERNS:
        _compare(c.relocalize(case["desc"], case["xy"], case["ids"], seed=3, with_pairs=True), sec.full_ref(n, 2), "unmasked")
        got = c.relocalize(case["desc"], case["xy"], case["ids"], valid=sec.pattern_valid(n, pattern), seed=3, with_pairs=True)
        _compare(got, sec.full_ref(n, 2, pattern), pattern)
        want = {"wave0": n - 64, "chunk_64_319": n - 256, "alternate": n // 2, "none": 0, "last_only": 1}[pattern]
        assert got["candidates"][0]["n_matches"] == n and got["candidates"][0]["n_correspondences"] == want
    c.close()


# ---- E / F: entries lifted on the device ---------------------------------------------------------------------------------

def _detected(pkg, kind):
    """a context holding one detected 3-frame batch (400 x 300: two to four 256-chunks of keypoints per frame, K = 1024)
    -> (context, counts, descriptors, coordinates, a function that back-projects a depth stack and returns xyz, valid)"""
    import torch
    import synth
    B, K = 3, 1024
    c = pkg.Context(width=SMALL_W, height=SMALL_H, max_batch=B, max_keypoints=K)
    c.set_matcher(kind)
    d_frames = torch.from_numpy(np.stack(synth.make_stream(B, SMALL_W, SMALL_H, seed=21))).cuda()
    c.detect_batch_dev(d_frames.data_ptr(), B)
    c.sync()
    v = c.batch_view()
    cnt = pkg.read_device(c, v.count, (B,), np.int32)
    desc = pkg.read_device(c, v.desc, (B, K, 32), np.uint8)
    xy = pkg.read_device(c, v.xy, (B, K, 2), np.float32)
    print("detected keypoints per frame", cnt.tolist())
    assert cnt.min() > 256 and cnt.max() <= K                     # more than one 256-chunk in play

    def backproject(depth):
        d_depth = torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).cuda()
        c.backproject_batch_dev(d_depth.data_ptr(), focal=SMALL_CAM[:2], principal=SMALL_CAM[2:])
        c.sync()
        pv = c.points_view()
        return pkg.read_device(c, pv.xyz, (B, K, 3), np.float64), pkg.read_device(c, pv.valid, (B, K), np.uint8)
    return c, cnt, desc, xy, backproject


def _ramp(lo, hi, B=3):
    return np.tile((np.linspace(lo, hi, SMALL_W) * 5000).astype(np.uint16), (B, SMALL_H, 1))


@KINDS
def test_row_stride_slack_changes_nothing(pkg, orc, kind):
    """n_upper is K after a device lift and the sum of the members after an enqueued union, and exact after a read or a host
    add: the row stride of the same landmarks is 1024 at first and 512 or 768 afterwards, and nothing may change with it"""
    c, cnt, desc, xy, backproject = _detected(pkg, kind)
    xyz, ok = backproject(_ramp(1.0, 2.8))
    f = int(np.argmin(cnt))                                      # the frame with the fewest keypoints
    n = int(cnt[f])
    assert n <= 768                                              # al256(n) < K: the strides really differ
    ld, lw = rr.lift(desc[f, :n], xyz[f, :n], ok[f, :n], np.eye(3), np.zeros(3), 3.0)      # (known without reading the entry)
    qd, qxy = sec.query_of_entry(ld, lw, seed=3, n_distractors=100, width=SMALL_W, height=SMALL_H, cam=SMALL_CAM)
    depth = _ramp(1.0, 4.0)[0]
    cam = dict(focal=SMALL_CAM[:2], principal=SMALL_CAM[2:])
    assert len(ld) == n and len(qd) <= 1024

    def calls(entry):
        a = c.relocalize(qd, qxy, [entry], seed=4, with_pairs=True, **cam)
        t = c.track(qd, qxy, depth, entry, [entry], -1, seed=4, with_pairs=True, **cam)
        return a, t

    def against_reference(a, t, d, w):
        _compare(a, rr.relocalize(qd, qxy, {0: (d, w)}, [0], SMALL_CAM, seed=4), "lifted")
        _compare_step(t, tr.track(qd, qxy, depth, {0: (d, w)}, 0, [0], SMALL_CAM, seed=4), "lifted")
        assert a["best"] == 0 and a["candidates"][0]["n_inliers"] > 100 and t["tracked"]

    c.kf_add_from_batch_dev(1, f, np.eye(3), np.zeros(3), 3.0)   # n_upper = K = 1024
    before = calls(1)
    gd, gw = c.kf_read(1)                                        # n_upper = n
    after = calls(1)
    c.kf_add(2, gd, gw)
    copy = calls(2)
    assert np.array_equal(gd, ld) and np.array_equal(gw.view(np.uint64), lw.view(np.uint64))
    assert _bits_equal(before, after) and _bits_equal(before, copy)
    against_reference(before[0], before[1], gd, gw)
    # a union whose members overlap: 900 landmarks by the sum of its members, 500 distinct ones
    lids = np.arange(n, dtype=np.int64)
    for j, lo in enumerate((0, 100, 200)):
        c.kf_add(10 + j, gd[lo:lo + 300], gw[lo:lo + 300], lids=lids[lo:lo + 300])
    c.kf_union(20, [10, 11, 12], sync=False)                     # n_upper = 900: stride 1024
    before = calls(20)
    ud, uw = c.kf_read(20)                                       # n_upper = 500: stride 512
    ul = c.kf_read_ids(20)
    after = calls(20)
    c.kf_add(21, ud, uw, lids=ul)
    copy = calls(21)
    assert len(ud) == 500 and sorted(ul.tolist()) == list(range(500))
    assert _bits_equal(before, after) and _bits_equal(before, copy)
    against_reference(before[0], before[1], ud, uw)
    c.close()


def _lift_all(c, cnt, desc, xyz, ok, z_max, first_id, poses):
    """every frame of the batch lifted on the device against rr.lift: bytes and ids -> landmark counts"""
    out, serials = [], []
    for f, (R, t) in enumerate(poses):
        c.kf_add_from_batch_dev(first_id + f, f, R, t, z_max)
    c.sync()
    for f, (R, t) in enumerate(poses):
        n = int(cnt[f])
        rd, rw = rr.lift(desc[f, :n], xyz[f, :n], ok[f, :n], R, t, z_max)
        gd, gw = c.kf_read(first_id + f)
        lids = c.kf_read_ids(first_id + f)
        assert np.array_equal(gd, rd) and np.array_equal(gw.view(np.uint64), rw.view(np.uint64)), (f, z_max)
        assert (lids >> 62 == 1).all() and np.array_equal(lids & 0xFFFF, np.arange(len(rd))) and len(set((lids >> 16).tolist())) <= 1
        serials += list(set((lids >> 16).tolist()))
        out.append(len(rd))
    assert len(set(serials)) == len(serials)                     # every entry has a serial of its own
    return out


@KINDS
def test_lift_edges(pkg, orc, kind):
    c, cnt, desc, xy, backproject = _detected(pkg, kind)
    poses = [(rr.po.rodrigues([0.1 * f, -0.2, 0.05]), np.array([0.3, -0.1 * f, 1.5])) for f in range(3)]
    sc = sec.few_scene()
    # no depth anywhere: entries of 0 landmarks, and a query against one
    xyz, ok = backproject(np.zeros((3, SMALL_H, SMALL_W), np.uint16))
    assert _lift_all(c, cnt, desc, xyz, ok, 3.0, 100, poses) == [0, 0, 0]
    got = c.relocalize(sc["desc"][:500], sc["xy"][:500], [100, 101], seed=1, with_pairs=True)
    _compare(got, rr.relocalize(sc["desc"][:500], sc["xy"][:500], {0: (np.empty((0, 32), np.uint8), np.empty((0, 3)))}, [0, 0], seed=1), "empty")
    assert got["best"] == -1 and got["candidates"][0]["n_matches"] == 0
    # every depth valid and below z_max: every keypoint a landmark
    xyz, ok = backproject(_ramp(1.0, 2.8))
    assert _lift_all(c, cnt, desc, xyz, ok, 3.0, 110, poses) == cnt.tolist()
    # z == z_max: kept; the next double below: dropped (the ramp gives every column one depth: several keypoints share it)
    z = float(xyz[0, int(cnt[0]) // 2, 2])
    at = _lift_all(c, cnt, desc, xyz, ok, z, 120, poses)
    under = _lift_all(c, cnt, desc, xyz, ok, float(np.nextafter(z, 0)), 130, poses)
    n_eq = int((xyz[0, :cnt[0], 2] == z).sum())
    print("z_max", z, "landmarks at", at, "just below", under, "keypoints of frame 0 at that depth", n_eq)
    assert n_eq >= 1 and at[0] - under[0] == n_eq and 0 < under[0] < at[0] < cnt[0]
    # runs of 64 and of 256 consecutive keypoints without depth, the rest with
    depth = _ramp(1.0, 4.0)
    for f in range(3):
        px = xy[f, :cnt[f]].astype(np.float64).astype(np.int64)             # the pixel back-projection reads: truncation
        for a, b in ((10, 74), (int(cnt[f]) - 256 - 5, int(cnt[f]) - 5)):
            depth[f, px[a:b, 1], px[a:b, 0]] = 0
    xyz, ok = backproject(depth)
    for f in range(3):
        n = int(cnt[f])
        assert not ok[f, 10:74].any() and not ok[f, n - 261:n - 5].any() and ok[f, :10].any() and ok[f, n - 5:n].any()
    runs = _lift_all(c, cnt, desc, xyz, ok, 3.0, 140, poses)
    every = _lift_all(c, cnt, desc, xyz, ok, np.inf, 150, poses)            # z_max = inf keeps every valid keypoint
    print("landmarks with the runs cut out", runs, "and with z_max = inf", every)
    assert every == [int(ok[f, :cnt[f]].sum()) for f in range(3)] and all(0 < a < b for a, b in zip(runs, every))
    c.close()


@KINDS
def test_part_b_keeps_z_equal_to_z_max(pkg, orc, kind):
    zc = sec.zmax_case()
    fr, i, z = zc["frame"], zc["i"], zc["z"]
    c = _ctx(pkg, kind)
    _fill(c, zc["store"])
    ref_lids = c.kf_read_ids(0)
    sizes = []
    for z_max in (z, float(np.nextafter(z, 0)), np.inf):
        got = c.track(fr["desc"], fr["xy"], fr["depth"], 0, [0], 9, seed=1, new_keyframe_min_landmarks=sec.BIG, z_max=z_max,
                      with_pairs=True, with_entry=True, **ZERO)
        _compare_step(got, zc["ref"], z_max)
        e = _entry_equals(c, got, zc["ref"], fr, zc["store"][0][1], ref_lids, 9, 1024, z_max)
        assert np.array_equal(e["kp"], sec.zmax_entry(z_max)["kp"])
        assert (i in got["entry_kp"][got["n_inherited"]:]) == (z_max >= z)
        sizes.append(got["n_entry"])
    assert sizes[1] < sizes[0] < sizes[2]
    c.close()


# ---- G: the upper half of `used` ------------------------------------------------------------------------------------------

@KINDS
def test_matched_keypoints_above_32768(pkg, orc, kind):
    g = sec.upper_used()
    c = _ctx(pkg, kind, g["K"])
    _fill(c, g["store"])
    got = c.track(g["desc"], g["xy"], g["depth"], 0, [0], 5, seed=2, new_keyframe_min_landmarks=sec.BIG, with_pairs=True, with_entry=True)
    _compare_step(got, g["ref"], "33000 keypoints")
    e = _entry_equals(c, got, g["ref"], g, g["store"][0][1], c.kf_read_ids(0), 5, g["K"])
    na = e["n_inherited"]
    assert got["keyframe_added"] and na > 100 and e["kp"][:na].min() >= 32768 and not np.isin(e["kp"][na:], got["pairs"][0]).any()
    assert np.array_equal(got["entry_kp"], g["ref"]["entry"]["kp"])
    c.close()


# ---- H: ranking ---------------------------------------------------------------------------------------------------------------

@KINDS
def test_rankings_without_a_winner_and_at_the_threshold(pkg, orc, kind):
    sc, store = sec.few_scene(), sec.ranking_store()
    c = _ctx(pkg, kind)
    _fill(c, store)
    for name in ("no_model", "last", "at_min", "below_min"):
        cand, min_inliers, ref = sec.ranking_ref(name)
        got = c.relocalize(sc["desc"], sc["xy"], cand, seed=5, min_inliers=min_inliers, with_pairs=True)
        _compare(got, ref, name)
        assert got["best"] == {"no_model": -1, "last": 63, "at_min": 63, "below_min": -1}[name]
        if got["best"] < 0:                                       # MSLAM_HIP_E_NO_MODEL, the ranking's own message
            assert b"no candidate reached min_inliers" in c.L.mslam_hip_last_error(c._h)
        if name == "no_model":
            for g in got["candidates"]:
                assert (g["n_inliers"], g["status"]) == (0, 0) and not g["rvec"].any() and not g["tvec"].any()
        else:
            assert got["candidates"][63]["n_inliers"] == min_inliers - (name == "below_min") or name == "last"
    c.close()
