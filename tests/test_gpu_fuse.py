"""Landmark fusion on the MI355X: mslam_hip_kf_fuse_search, mslam_hip_kf_replace_ids and mslam_hip_kf_fuse against
tests/fuse_ref.py — pairs, ids and counts exactly, stores read back and compared as bytes — and HipKeyframeTracker with
loop_fusion on the ring walk of tests/loop_walk.py against the CPU tracker."""
import numpy as np
import pytest

import fuse_ref as fr
import loop_walk
import pose_graph_ref as pg
import reloc_ref as rr
import synth
import track_ref as tr

pytestmark = pytest.mark.gpu

K = 4608
KEYS = ("keep_pos", "drop_pos", "keep_lid", "drop_lid", "dist")


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(width=640, height=480, max_keypoints=K)
    yield c
    c.close()


def _fill(c, store):
    c.kf_clear()
    for id, e in store.items():
        d, w, l = fr.entry(*e)
        c.kf_add(id, d, w, l)


def _read(c, id):
    d, w = c.kf_read(id)
    return d, w, c.kf_read_ids(id)


def _same_store(c, ref, what=""):
    assert c.kf_size() == len(ref), what
    for id, e in ref.items():
        for got, want, name in zip(_read(c, id), fr.entry(*e), ("desc", "world", "ids")):
            assert got.tobytes() == want.tobytes(), (what, id, name)


def _args(case):
    kw = case["kw"]
    return dict(R=kw["R"], t=kw["t"], radius=case["radius"], max_distance=kw["max_distance"], ratio=kw["ratio"],
                max_world_distance=kw["max_world_distance"], focal=kw["cam"][:2], principal=kw["cam"][2:], width=kw["width"],
                height=kw["height"])


def _same_pairs(got, ref, what=""):
    for k in KEYS:
        assert got[k].dtype == ref[k].dtype and got[k].tobytes() == ref[k].tobytes(), (what, k, got[k][:8], ref[k][:8])


@pytest.mark.parametrize("nk,nd", fr.SIZES)
def test_entry_sizes(ctx, nk, nd):
    """search, then fuse, at every size at which a kernel takes another path; a few ids are shared between the sides"""
    case = fr.sized_case(nk, nd)
    store = {1: case["keep"], 2: case["drop"]}
    _fill(ctx, store)
    ref = fr.search(case["keep"], case["drop"], radius=case["radius"], **case["kw"])
    got = ctx.kf_fuse_search(1, 2, **_args(case))
    print("sizes %d / %d: %d pairs" % (nk, nd, len(ref["keep_pos"])))
    _same_pairs(got, ref, "search")
    _same_store(ctx, store, "search changes nothing")
    assert min(nk, nd) == 0 or len(ref["keep_pos"]) > 0
    pairs, new, n = fr.fuse(store, 1, 2, radius=case["radius"], **case["kw"])
    fused = ctx.kf_fuse(1, 2, **_args(case))
    _same_pairs(fused, ref, "fuse")
    assert fused["n_rewritten"] == n
    _same_store(ctx, new, "fuse")


@pytest.mark.parametrize("name", fr.HAND_CASES)
def test_hand_cases(ctx, name):
    case = fr.hand_case(name)
    _fill(ctx, {1: case["keep"], 2: case["drop"]})
    got = ctx.kf_fuse_search(1, 2, **_args(case))
    assert list(zip(got["keep_pos"].tolist(), got["drop_pos"].tolist(), got["dist"].tolist())) == case["expect"]
    _same_pairs(got, fr.search(case["keep"], case["drop"], radius=case["radius"], **case["kw"]))


def _five(seed=5):
    """keep (300) and drop (280) with more entries of other sizes (520, 1, 257) that hold drop ids (some twice), keep ids and
    strangers; the slot of id 40 is freed before the call"""
    case = fr.random_case(seed, 300, 280)
    rng = np.random.default_rng(seed)
    dl, kl = case["drop"][2], case["keep"][2]

    def other(ids):
        return (rng.integers(0, 256, (len(ids), 32), dtype=np.uint8), rng.normal(size=(len(ids), 3)), ids)

    store = {10: case["keep"], 20: case["drop"], 30: other(np.concatenate([dl[::2], kl[:250], dl[:130]])),      # 520
             40: other(dl[:33]), 50: other(dl[5:6]), 60: other(np.concatenate([dl[100:], 9000000 + np.arange(77)]))}   # 33, 1, 257
    return case, store


def _fill_five(c, store):
    _fill(c, store)
    c.kf_remove(40)
    return {k: v for k, v in store.items() if k != 40}


def test_store_of_five_with_a_freed_slot_and_covisibility(ctx):
    case, store = _five()
    live = _fill_five(ctx, store)
    assert ctx.kf_covisible(10, [20]).tolist() == [0]
    pairs, new, n = fr.fuse(live, 10, 20, radius=case["radius"], **case["kw"])
    got = ctx.kf_fuse(10, 20, **_args(case))
    _same_pairs(got, pairs)
    assert got["n_rewritten"] == n > len(pairs["keep_pos"]) > 50
    _same_store(ctx, new)
    assert ctx.kf_covisible(10, [20]).tolist() == [len(pairs["keep_pos"])]
    # the two steps on their own give the same store, and a second search the same bytes
    live = _fill_five(ctx, store)
    a = ctx.kf_fuse_search(10, 20, **_args(case))
    b = ctx.kf_fuse_search(10, 20, **_args(case))
    _same_pairs(a, pairs), _same_pairs(b, pairs)
    assert ctx.kf_replace_ids(a["drop_lid"], a["keep_lid"], fr.entry(*store[10])[1][a["keep_pos"]]) == n
    _same_store(ctx, new, "search + replace")
    # nothing left to fuse: every former pair is shared now
    again = ctx.kf_fuse(10, 20, **_args(case))
    assert set(again["drop_lid"].tolist()).isdisjoint(pairs["drop_lid"].tolist()) and set(again["keep_lid"].tolist()).isdisjoint(pairs["keep_lid"].tolist())


def test_replacement_rules(ctx):
    case, store = _five(6)
    live = _fill_five(ctx, store)
    dl, kl = case["drop"][2], case["keep"][2]
    rng = np.random.default_rng(1)
    # simultaneous (a swap), no points
    f, t = np.concatenate([dl[:50], kl[:50]]), np.concatenate([kl[:50], dl[:50]])
    ref, n = fr.replace_ids(live, f, t)
    assert ctx.kf_replace_ids(f, t) == n > 100
    _same_store(ctx, ref, "swap")
    # a `from` listed twice (the later wins), from == to (the point alone changes), ids the store does not hold
    f = np.concatenate([dl[60:90], dl[60:90][::-1], kl[100:110], [7777777, 2 ** 62 + 5]])
    t = np.concatenate([kl[200:230], kl[230:260], kl[100:110], [1, 2]])
    xyz = rng.normal(size=(len(f), 3))
    live, n = fr.replace_ids(ref, f, t, xyz)
    assert ctx.kf_replace_ids(f, t, xyz) == n > 40
    _same_store(ctx, live, "twice / same / unknown")
    assert ctx.kf_replace_ids([], []) == 0
    _same_store(ctx, live, "empty list")


def test_errors_leave_the_store_alone(pkg, ctx):
    """(an entry above 65535 landmarks cannot be made: mslam_hip_create bounds max_keypoints by 65535, so that error is
    checked on the host only and has no case here)"""
    case, store = _five(7)
    live = _fill_five(ctx, store)
    ok = _args(case)
    ref = fr.search(case["keep"], case["drop"], radius=case["radius"], **case["kw"])

    def bad(code, fn, *a, **kw):
        with pytest.raises(pkg.MslamHipError) as e:
            fn(*a, **kw)
        assert e.value.code == code, (a, kw)
        return e.value

    for fn in (ctx.kf_fuse_search, ctx.kf_fuse):
        bad(pkg.E_INVALID, fn, 10, 10, **ok)
        bad(pkg.E_INVALID, fn, 10, 40, **ok)                       # removed
        bad(pkg.E_INVALID, fn, 999, 20, **ok)
        for k, vals in (("radius", (0.0, -1.0, np.nan)), ("max_distance", (-1, 257)), ("width", (0, 8193)), ("height", (0, 8193)),
                        ("max_world_distance", (0.0, -1.0, np.nan)), ("focal", ((0.0, 1.0), (1.0, np.nan)))):
            for v in vals:
                bad(pkg.E_INVALID, fn, 10, 20, **dict(ok, **{k: v}))
        e = bad(pkg.E_CAPACITY, fn, 10, 20, capacity=len(ref["keep_pos"]) - 1, **ok)
        assert e.needed == len(ref["keep_pos"])
        _same_store(ctx, live, fn.__name__)                        # kf_fuse: nothing was rewritten
    bad(pkg.E_INVALID, ctx.kf_replace_ids, [-1], [5])
    bad(pkg.E_INVALID, ctx.kf_replace_ids, [5], [-(2 ** 63)])
    bad(pkg.E_INVALID, ctx.kf_replace_ids, [5, 6], [5])
    _same_store(ctx, live, "replace_ids")
    _same_pairs(ctx.kf_fuse_search(10, 20, capacity=len(ref["keep_pos"]), **ok), ref, "a clean call after the errors")


# ---- the tracker ----------------------------------------------------------------------------------------------------------------

RING = dict(local_map_depth=2, local_ba=True, new_keyframe_min_landmarks=200, loop_closure=True, loop_min_gap=5)


def _run_ring(pkg, seq, **kw):
    c = pkg.Context(width=0, height=0, max_keypoints=4096)
    c.bow_load(synth.make_vocabulary(10, 3))
    t = pkg.HipKeyframeTracker(c, focal=tr.CAM[:2], principal=tr.CAM[2:], **dict(RING, **kw))
    return c, t, [t.processSensorData(fr_["desc"], fr_["xy"], fr_["depth"]) for fr_ in seq["frames"]]


@pytest.fixture(scope="module")
def ring():
    seq = loop_walk.ring_sequence()
    rows, trk = fr.run_ring(seq, True)
    return seq, rows, trk


@pytest.mark.parametrize("global_ba", [False, True])
def test_tracker_fuses_the_ring_walk_loop_as_the_cpu_tracker(pkg, ring, global_ba):
    seq, cpu_rows, cpu = ring
    c, t, rows = _run_ring(pkg, seq, loop_fusion=True, loop_global_ba=global_ba)
    want = cpu.loops[0]
    fired = [(f, r["loop"]) for f, r in enumerate(rows) if r["loop"] is not None]
    closed = [a for a in t.loop_results if a["loop"] is not None]
    print("ring walk with fusion: loop events %s, fusion %s, CPU %s" % (
        fired, [a.get("fusion") for a in closed], {k: v for k, v in want["fusion"].items() if k != "pairs"}))
    assert len(cpu.loops) == 1 and fired == [(want["frame"], (want["keyframe"], want["loop"]))] and len(closed) == 1
    fu = closed[0]["fusion"]
    assert (fu["n_pairs"], fu["n_rewritten"], fu["edges"]) == (want["fusion"]["n_pairs"], want["fusion"]["n_rewritten"], want["fusion"]["edges"])
    assert {k: sorted(v) for k, v in t.graph.items()} == {k: sorted(v) for k, v in cpu.graph.items()}
    assert t.ids == cpu.ids and all(r["tracked"] for r in rows)
    for id in (t.LOCAL_MAP_ID, t.FUSE_KEEP_ID, t.FUSE_DROP_ID):
        assert id not in t.ids
    assert c.kf_size() == len(t.ids) + 1                                   # the keyframes and the local map: the unions are gone
    # the backend renamed its observations: the two keyframes of the loop share landmarks now, the dropped ones are gone
    cur, loop = want["keyframe"], want["loop"]
    assert len(set(t.backend.obs[cur][0].tolist()) & set(t.backend.obs[loop][0].tolist())) > 0
    assert int(c.kf_covisible(cur, [loop])[0]) > 0
    assert ("global_ba" in closed[0]) == global_ba
    if global_ba:
        ba = closed[0]["global_ba"]
        print("global BA after the fusion: termination %d, cost %.6g -> %.6g" % (ba["termination"], ba["initial_cost"], ba["final_cost"]))
        assert ba["termination"] in (0, 1) and ba["final_cost"] <= ba["initial_cost"]
    kf_frame = {r["keyframe"]: f for f, r in enumerate(rows) if r["keyframe"] >= 0}
    for k in t.ids:                                                        # 0.1 degree / 0.02 m, the ring test's bound
        q, p = t.backend.poses[k][:4], t.backend.poses[k][4:]
        R = pg.q_matrix(q).T
        f = seq["frames"][kf_frame[k]]
        assert rr.rot_err(R, f["R"]) < 0.1 and float(np.linalg.norm(-R @ p - f["t"])) < 0.02, k
    for f, r in enumerate(rows):
        assert rr.rot_err(r["R"], seq["frames"][f]["R"]) < 0.1 and np.linalg.norm(r["tvec"] - seq["frames"][f]["t"]) < 0.02, f
    c.close()


def test_tracker_loop_fusion_false_is_the_default(pkg):
    """loop_fusion named and omitted: rows, store and backend poses are byte-identical, no union is built (the serials, and
    so the fresh ids of later entries, are unchanged) and no attempt carries a fusion"""
    seq = loop_walk.ring_sequence()
    c0, t0, a = _run_ring(pkg, seq)
    c1, t1, b = _run_ring(pkg, seq, loop_fusion=False)
    assert t0.ids == t1.ids and len(t0.loop_results) == len(t1.loop_results) > 0
    assert all("fusion" not in r for r in t0.loop_results + t1.loop_results)
    for f, (x, y) in enumerate(zip(a, b)):
        assert sorted(x) == sorted(y)
        assert (x["tracked"], x["n_inliers"], x["keyframe"], x["reference"], x["relocalized"], x["loop"]) == \
               (y["tracked"], y["n_inliers"], y["keyframe"], y["reference"], y["relocalized"], y["loop"]), f
        assert x["R"].tobytes() == y["R"].tobytes() and x["tvec"].tobytes() == y["tvec"].tobytes() and x["rvec"].tobytes() == y["rvec"].tobytes(), f
    for k in t0.ids:
        for u, v in zip(_read(c0, k), _read(c1, k)):
            assert u.tobytes() == v.tobytes(), k
        assert t0.backend.poses[k].tobytes() == t1.backend.poses[k].tobytes()
    c0.close()
    c1.close()
