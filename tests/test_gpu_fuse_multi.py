"""Landmark fusion into many target entries on the MI355X: mslam_hip_kf_fuse_search_multi and mslam_hip_kf_fuse_multi against
tests/fuse_multi_ref.py — pairs, ids and counts exactly, stores read back and compared as bytes — and HipKeyframeTracker with
loop_fusion_keyframes on the ring walk of tests/loop_walk.py against the CPU tracker."""
import numpy as np
import pytest

import fuse_multi_ref as fm
import fuse_ref as fr
import local_map_ref as lm
import loop_walk
import synth
import track_ref as tr

pytestmark = pytest.mark.gpu

K = 2048
KEEP = 1


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(width=640, height=480, max_keypoints=K)
    yield c
    c.close()


def _store(case, others=None):
    """keep under id 1, target m under id 10 + m"""
    store = {KEEP: case["keep"]}
    store.update({10 + m: d for m, d in enumerate(case["drops"])})
    store.update(others or {})
    return store, [10 + m for m in range(len(case["drops"]))]


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
    return dict(R=case["Rs"], t=case["ts"], radius=case["radius"], max_distance=kw["max_distance"], ratio=kw["ratio"],
                max_world_distance=kw["max_world_distance"], focal=kw["cam"][:2], principal=kw["cam"][2:], width=kw["width"],
                height=kw["height"])


def _same_pairs(got, ref, what=""):
    for k in fm.KEYS:
        assert got[k].dtype == ref[k].dtype and got[k].tobytes() == ref[k].tobytes(), (what, k, got[k][:8], ref[k][:8])


def _ref(case, stages=None):
    return fm.search_multi(case["keep"], case["drops"], case["Rs"], case["ts"], case["radius"], stages=stages, **case["kw"])


@pytest.mark.parametrize("name", fm.HAND_CASES)
def test_hand_cases(ctx, name):
    case = fm.hand_case(name)
    store, drops = _store(case)
    _fill(ctx, store)
    got = ctx.kf_fuse_search_multi(KEEP, drops, **_args(case))
    assert fm.rows_of(got) == case["expect"]
    _same_pairs(got, _ref(case))
    _same_store(ctx, store, "the search changes nothing")


def test_two_pose_scene(ctx):
    case = fm.two_pose_scene()
    store, drops = _store(case)
    _fill(ctx, store)
    ref = _ref(case)
    assert (ref["target"] == 1).sum() > 10
    _same_pairs(ctx.kf_fuse_search_multi(KEEP, drops, **_args(case)), ref)


@pytest.mark.parametrize("n_drop,nk", fm.RANDOM_CASES)
def test_posed_random_cases(ctx, n_drop, nk):
    """search, then fuse; the restatement alone shows that step A and step B each drop a row of the case"""
    case = fm.random_case(n_drop, nk)
    store, drops = _store(case)
    _fill(ctx, store)
    st = {}
    ref = _ref(case, st)
    print("n_drop %d, keep %d: %d rows, A drops %d, B drops %d -> %d pairs" % (
        n_drop, nk, len(st["rows"]), len(st["dropped_a"]), len(st["dropped_b"]), len(ref["dist"])))
    assert len(st["dropped_a"]) > 0 and len(st["dropped_b"]) > 0 and len(ref["dist"]) > 0
    _same_pairs(ctx.kf_fuse_search_multi(KEEP, drops, **_args(case)), ref, "search")
    _same_store(ctx, store, "the search changes nothing")
    pairs, new, n = fm.fuse_multi(store, KEEP, drops, case["Rs"], case["ts"], case["radius"], **case["kw"])
    fused = ctx.kf_fuse_multi(KEEP, drops, **_args(case))
    _same_pairs(fused, ref, "fuse")
    assert fused["n_rewritten"] == n
    _same_store(ctx, new, "fuse")


def _wide(seed=3):
    """random_case(3, 1024) with further entries (520, 33, 1, 257 landmarks) that hold drop ids (some twice), keep ids and
    strangers; the slot of id 40 is freed before the call"""
    case = fm.random_case(3, 1024, seed=seed)
    rng = np.random.default_rng(seed)
    dl, kl = np.concatenate([d[2] for d in case["drops"]]), case["keep"][2]

    def other(ids):
        return (rng.integers(0, 256, (len(ids), 32), dtype=np.uint8), rng.normal(size=(len(ids), 3)), ids)

    others = {30: other(np.concatenate([dl[::2], kl[:256], dl[:130]])), 40: other(dl[:33]), 50: other(dl[5:6]),
              60: other(np.concatenate([dl[100:280], 9000000 + np.arange(77)]))}
    store, drops = _store(case, others)
    return case, store, drops


def _fill_wide(c, store):
    _fill(c, store)
    c.kf_remove(40)
    return {k: v for k, v in store.items() if k != 40}


def test_store_wide_rewrite_with_a_freed_slot_and_covisibility(ctx):
    case, store, drops = _wide()
    live = _fill_wide(ctx, store)
    before = ctx.kf_covisible(KEEP, drops).tolist()
    pairs, new, n = fm.fuse_multi(live, KEEP, drops, case["Rs"], case["ts"], case["radius"], **case["kw"])
    got = ctx.kf_fuse_multi(KEEP, drops, **_args(case))
    _same_pairs(got, pairs)
    assert got["n_rewritten"] == n > len(pairs["keep_pos"]) > 50
    _same_store(ctx, new)
    after = ctx.kf_covisible(KEEP, drops).tolist()
    print("covisibility of the keep entry with the targets: %s -> %s" % (before, after))
    # (a drop id that two targets hold counts in both, so the gain over the targets is at least the number of pairs)
    assert after == lm.covisible({k: fr.entry(*e)[2] for k, e in new.items()}, KEEP, drops).tolist()
    assert all(a > 0 for a in after) and after[0] > before[0] and sum(after) - sum(before) >= len(pairs["keep_pos"])
    # search + kf_replace_ids give the same store
    _fill_wide(ctx, store)
    a = ctx.kf_fuse_search_multi(KEEP, drops, **_args(case))
    _same_pairs(a, pairs)
    assert ctx.kf_replace_ids(a["drop_lid"], a["keep_lid"], fr.entry(*store[KEEP])[1][a["keep_pos"]]) == n
    _same_store(ctx, new, "search + replace")


def test_the_same_call_twice_gives_the_same_bytes(ctx):
    case, store, drops = _wide(4)
    outs = []
    for _ in range(2):
        _fill_wide(ctx, store)
        s = ctx.kf_fuse_search_multi(KEEP, drops, **_args(case))
        f = ctx.kf_fuse_multi(KEEP, drops, **_args(case))
        outs.append([s[k].tobytes() for k in fm.KEYS] + [f[k].tobytes() for k in fm.KEYS] + [f["n_rewritten"]] +
                    [x.tobytes() for id in sorted(store) if id != 40 for x in _read(ctx, id)])
    assert outs[0] == outs[1] and len(outs[0][0]) > 0


def _stages(c, fn, *a, **kw):
    c.set_profiling(1)                                                 # (starts a new list)
    try:
        fn(*a, **kw)
        return [name for name, _ in c.stage_times()]
    finally:
        c.set_profiling(0)


SEARCH_STAGES = ["fusem_clear", "fusem_ids", "fusem_project", "fusem_bin", "fusem_search", "fusem_claim_a", "fusem_claim_b",
                 "fusem_count", "fusem_compact"]


def test_the_launches_do_not_grow_with_the_targets(ctx):
    case = fm.random_case(64, 1025)
    store, drops = _store(case)
    _fill(ctx, store)
    for n in (1, 2, 64):
        a = dict(_args(case), R=case["Rs"][:n], t=case["ts"][:n])
        assert _stages(ctx, ctx.kf_fuse_search_multi, KEEP, drops[:n], **a) == SEARCH_STAGES, n
    assert _stages(ctx, ctx.kf_fuse_multi, KEEP, drops, **_args(case)) == SEARCH_STAGES + ["fusem_table", "fusem_replace"]


def test_errors_leave_the_store_alone(pkg, ctx):
    """(an entry above 65535 landmarks cannot be made: mslam_hip_create bounds max_keypoints by 65535, so that error is
    checked on the host only and has no case here)"""
    case, store, drops = _wide(5)
    live = _fill_wide(ctx, store)
    ok = _args(case)
    ref = _ref(case)
    for id in range(100, 162):                                   # 62 more one-landmark entries: 65 possible targets
        live[id] = (np.zeros((1, 32), np.uint8), np.zeros((1, 3)), [7000000 + id])
        ctx.kf_add(id, *live[id])
    many = drops + list(range(100, 162))

    def bad(code, fn, *a, **kw):
        with pytest.raises(pkg.MslamHipError) as e:
            fn(*a, **kw)
        assert e.value.code == code, (a, kw)
        return e.value

    def poses(n):
        return dict(ok, R=np.tile(np.eye(3), (n, 1, 1)), t=np.zeros((n, 3)))

    for fn in (ctx.kf_fuse_search_multi, ctx.kf_fuse_multi):
        bad(pkg.E_INVALID, fn, KEEP, [], **poses(0))                           # n_drop = 0
        bad(pkg.E_INVALID, fn, KEEP, many, **poses(65))                        # n_drop = 65
        bad(pkg.E_INVALID, fn, KEEP, [drops[0], KEEP, drops[2]], **ok)         # keep_id among the targets
        bad(pkg.E_INVALID, fn, KEEP, [drops[0], drops[1], drops[0]], **ok)     # listed twice
        bad(pkg.E_INVALID, fn, KEEP, [drops[0], 40, drops[2]], **ok)           # removed
        bad(pkg.E_INVALID, fn, 999, drops, **ok)
        for k, vals in (("radius", (0.0, -1.0, np.nan)), ("max_distance", (-1, 257)), ("width", (0, 8193)), ("height", (0, 8193)),
                        ("max_world_distance", (0.0, -1.0, np.nan)), ("focal", ((0.0, 1.0), (1.0, np.nan)))):
            for v in vals:
                bad(pkg.E_INVALID, fn, KEEP, drops, **dict(ok, **{k: v}))
        e = bad(pkg.E_CAPACITY, fn, KEEP, drops, capacity=len(ref["keep_pos"]) - 1, **ok)
        assert e.needed == len(ref["keep_pos"])
        _same_store(ctx, live, fn.__name__)                        # kf_fuse_multi: nothing was rewritten
    got = ctx.kf_fuse_search_multi(KEEP, many[:64], **dict(poses(64), R=np.concatenate([case["Rs"], np.tile(np.eye(3), (61, 1, 1))]),
                                                            t=np.concatenate([case["ts"], np.zeros((61, 3))])))
    _same_pairs(got, ref, "64 targets, a clean call after the errors")
    _same_pairs(ctx.kf_fuse_search_multi(KEEP, drops, capacity=len(ref["keep_pos"]), **ok), ref, "capacity exactly")


# ---- the tracker ----------------------------------------------------------------------------------------------------------------

RING = dict(local_map_depth=2, local_ba=True, new_keyframe_min_landmarks=200, loop_closure=True, loop_min_gap=5)


def _run_ring(pkg, seq, **kw):
    c = pkg.Context(width=0, height=0, max_keypoints=4096)
    c.bow_load(synth.make_vocabulary(10, 3))
    t = pkg.HipKeyframeTracker(c, focal=tr.CAM[:2], principal=tr.CAM[2:], **dict(RING, **kw))
    return c, t, [t.processSensorData(f["desc"], f["xy"], f["depth"]) for f in seq["frames"]]


@pytest.fixture(scope="module")
def seq():
    return loop_walk.ring_sequence()


def test_tracker_fuses_into_every_keyframe_as_the_cpu_tracker(pkg, seq):
    cpu_rows, cpu = fm.run_ring(seq)
    c, t, rows = _run_ring(pkg, seq, loop_fusion=True, loop_fusion_keyframes=True)
    want = cpu.loops[0]
    fired = [(f, r["loop"]) for f, r in enumerate(rows) if r["loop"] is not None]
    closed = [a for a in t.loop_results if a["loop"] is not None]
    print("ring walk with fusion into every keyframe: loop events %s, fusion %s, CPU %s" % (
        fired, [a.get("fusion") for a in closed], {k: v for k, v in want["fusion"].items() if k != "pairs"}))
    assert len(cpu.loops) == 1 and fired == [(want["frame"], (want["keyframe"], want["loop"]))] and len(closed) == 1
    fu = closed[0]["fusion"]
    assert (fu["n_pairs"], fu["n_rewritten"], fu["edges"], fu["targets"]) == (
        want["fusion"]["n_pairs"], want["fusion"]["n_rewritten"], want["fusion"]["edges"], want["fusion"]["targets"])
    assert {k: sorted(v) for k, v in t.graph.items()} == {k: sorted(v) for k, v in cpu.graph.items()}
    assert t.ids == cpu.ids and all(r["tracked"] for r in rows)
    for k in t.ids:                                                        # the pairs: every keyframe's ids are the CPU tracker's
        assert c.kf_read_ids(k).tobytes() == cpu.lids[k].tobytes(), k
    for id in (t.LOCAL_MAP_ID, t.FUSE_KEEP_ID, t.FUSE_DROP_ID):
        assert id not in t.ids
    assert c.kf_size() == len(t.ids) + 1                                   # the keyframes and the local map: the union is gone
    cur, loop = want["keyframe"], want["loop"]
    assert len(set(t.backend.obs[cur][0].tolist()) & set(t.backend.obs[loop][0].tolist())) > 0
    assert int(c.kf_covisible(cur, [loop])[0]) > 0
    c.close()


def test_tracker_option_off_is_the_loop_fusion_of_before(pkg, seq):
    """loop_fusion_keyframes named False and omitted: rows, stores and backend poses are byte-identical and the fusion dicts
    are those of tests/test_gpu_fuse.py's run — the CPU tracker's of fuse_ref — without `targets`"""
    c0, t0, a = _run_ring(pkg, seq, loop_fusion=True)
    c1, t1, b = _run_ring(pkg, seq, loop_fusion=True, loop_fusion_keyframes=False)
    want = fr.run_ring(seq, True)[1].loops[0]["fusion"]
    for t in (t0, t1):
        fu = [x["fusion"] for x in t.loop_results if x["loop"] is not None]
        assert len(fu) == 1 and sorted(fu[0]) == ["edges", "n_pairs", "n_rewritten"]
        assert (fu[0]["n_pairs"], fu[0]["n_rewritten"], fu[0]["edges"]) == (want["n_pairs"], want["n_rewritten"], want["edges"])
    assert t0.ids == t1.ids
    for f, (x, y) in enumerate(zip(a, b)):
        assert (x["tracked"], x["n_inliers"], x["keyframe"], x["reference"], x["loop"]) == \
               (y["tracked"], y["n_inliers"], y["keyframe"], y["reference"], y["loop"]), f
        assert x["R"].tobytes() == y["R"].tobytes() and x["tvec"].tobytes() == y["tvec"].tobytes(), f
    for k in t0.ids:
        for u, v in zip(_read(c0, k), _read(c1, k)):
            assert u.tobytes() == v.tobytes(), k
        assert t0.backend.poses[k].tobytes() == t1.backend.poses[k].tobytes()
    c0.close()
    c1.close()
