"""mslam_hip_kf_observers, mslam_hip_kf_cull_search and mslam_hip_kf_cull on the GPU, through Context, against
tests/cull_ref.py: the outputs and the whole store byte for byte, on the smallest shapes where the kernels can go wrong
(entry sizes round a 256-thread block and the greedy workgroup's stride of 1024, listed entries round the 64-entry chunk,
repeats that straddle blocks, probe chains that wrap the table, fresh ids and 2^63 - 1, the greedy order); the slots a cull
frees; a union that is not listed; the errors; and HipKeyframeTracker(kf_cull=True) on cull_ref.triple_walk()."""
import ctypes as C

import numpy as np
import pytest

import cull_ref as cr
import lm_table_ref as lt
import local_map_ref as lm
import reloc_ref as rr
import track_ref as tr

pytestmark = pytest.mark.gpu
K = 2048
CAM = tr.CAM
TOP = (1 << 63) - 1
SIZES = [0, 1, 255, 256, 257, cr.STRIDE + 1]


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(width=0, height=0, max_keypoints=K)
    yield c
    c.close()


def _fill(c, store):
    c.kf_clear()
    for i, (d, w, l) in store.items():
        c.kf_add(i, d, w, lids=l)


def _read(c, i):
    d, w = c.kf_read(i)
    return d, w, c.kf_read_ids(i)


def _snapshot(c, ids):
    return {i: _read(c, i) for i in ids}


def _same(got, ref, what=""):
    assert len(got[0]) == len(got[1]) == len(got[2]) == len(ref[2]), (what, len(got[2]), len(ref[2]))
    assert np.array_equal(got[2], ref[2]), what
    assert np.array_equal(got[0], ref[0]), what
    assert np.array_equal(got[1].view(np.uint64), np.ascontiguousarray(ref[1]).view(np.uint64)), what


def _check(pkg, c, present, ids, cand, remove=False, what="", **kw):
    """one call against the restatement run on the store as read back: the outputs, and every entry afterwards"""
    before = _snapshot(c, present)
    after, ref = cr.cull(before, ids, cand, **kw)
    got = (c.kf_cull if remove else c.kf_cull_search)(ids, cand, **kw)
    assert got["culled"].dtype == bool and got["n_landmarks"].dtype == got["n_redundant"].dtype == np.int32
    assert cr.same_result(got, ref), (what, got, ref)
    left = after if remove else before
    assert c.kf_size() == len(left)
    for i in present:
        if i in left:
            _same(_read(c, i), before[i], (what, i))
        else:
            with pytest.raises(pkg.MslamHipError) as e:
                c.kf_read_ids(i)
            assert e.value.code == pkg.E_INVALID
    return got, sorted(left)


def _observers(c, present, ids, asked):
    ref = cr.observers(_snapshot(c, present), ids, asked)
    got = c.kf_observers(ids, asked)
    assert got.dtype == np.int32 and np.array_equal(got, ref)
    return got


def test_entry_sizes_the_whole_map_as_candidates_and_observers(pkg, ctx):
    store = cr.random_case(1, SIZES + [300] * 5, pool=1400, repeats=0.15)
    ids = sorted(store)
    _fill(ctx, store)
    pool = np.arange(1400, dtype=np.int64)
    counts = _observers(ctx, ids, ids, np.concatenate([pool, [5_000_000, TOP, 7, 7, 1 << 62]]))      # absent and repeated ids
    assert counts.max() >= 5 and counts[:1400].min() == 0 and counts[-5:].tolist()[:2] == [0, 0] and counts[-3] == counts[-2] == counts[7]
    assert len(_observers(ctx, ids, ids, [])) == 0
    for kw in (dict(min_observers=2, ratio=0.5), dict(min_observers=1, ratio=0.0), dict(), dict(min_observers=2, ratio=0.5, min_landmarks=256)):
        got, _ = _check(pkg, ctx, ids, ids, ids, what=kw, **kw)                              # the candidate list is the whole map
        assert got["n_landmarks"].tolist()[:2] == [0, 1] and not got["culled"][0]
    got, _ = _check(pkg, ctx, ids, ids, ids[::-1], min_observers=2, ratio=0.5)
    assert 0 < got["n_culled"] < len(ids)
    got, _ = _check(pkg, ctx, ids, ids, [], min_observers=2, ratio=0.5)                      # n_cand = 0
    assert got["n_culled"] == 0 and len(got["culled"]) == 0


@pytest.mark.parametrize("n", [1, cr.CHUNK - 1, cr.CHUNK, cr.CHUNK + 1, 2 * cr.CHUNK + 1])
def test_listed_entries_round_the_chunk(pkg, ctx, n):
    rng = np.random.default_rng(n)
    store = cr.random_case(10 + n, [int(s) for s in rng.integers(20, 60, n)], pool=120, repeats=0.1)
    store[999] = cr.random_case(5, [90], pool=120)[100]                                     # in the store, not listed
    ids = sorted(store)[:-1]
    _fill(ctx, store)
    counts = _observers(ctx, ids + [999], ids, np.arange(121))
    assert counts[120] == 0 and (n < 40 or counts.max() > 0.3 * n)
    cand = ids[-3:] + ids[:min(n - min(n, 3), 9)]                                            # the last chunk's entries first
    got, _ = _check(pkg, ctx, ids + [999], ids, cand, min_observers=max(1, n // 4), ratio=0.6)
    assert n < cr.CHUNK - 1 or got["n_culled"] > 0
    # every entry listed in another order: the counts do not depend on the position in the list
    assert np.array_equal(ctx.kf_observers(ids[::-1], np.arange(121)), counts)


def test_repeats_that_straddle_a_block_and_the_stride(pkg, ctx):
    n = cr.STRIDE + 200
    l = 10_000 + np.arange(n, dtype=np.int64)
    l[[255, 256]] = 1                                     # across two 256-thread blocks of the counting grid
    l[[100, 300, cr.STRIDE + 76]] = 2                     # across blocks and across the greedy workgroup's stride
    l[[cr.STRIDE - 1, cr.STRIDE]] = 3
    l[500:512] = 4
    lids = {1: l, 2: [1, 2, 3, 4, 1, 2], 3: [4, 3, 2, 1], 4: [1, 2, 3, 4, 4], 5: [1, 2, 3, 4] + list(range(10_000, 10_050))}
    _fill(ctx, cr.store_of(lids))
    ids = sorted(lids)
    assert _observers(ctx, ids, ids, [1, 2, 3, 4, 10_000, 10_101, 10_100]).tolist() == [5, 5, 5, 5, 2, 1, 0]
    got, _ = _check(pkg, ctx, ids, ids, [1, 2], min_observers=4, ratio=0.001)
    assert got["n_landmarks"].tolist() == [n - 1 - 2 - 1 - 11, 4] and got["n_redundant"].tolist() == [4, 0] and got["culled"].tolist() == [True, False]


def test_probe_chains_that_wrap_the_end_of_the_table(pkg, ctx):
    chain = lt.colliding(48, seed=3)                      # the last bucket of every table up to 65536 buckets is their home
    rng = np.random.default_rng(4)
    lids = {}
    for e in range(7):
        own = chain[rng.random(48) < 0.75]
        lids[20 + e] = np.concatenate([own, 500 + rng.choice(100, size=30, replace=False)])[rng.permutation(len(own) + 30)]
    assert lt.lm_bucket_count(sum(len(v) for v in lids.values())) <= 65536
    _fill(ctx, cr.store_of(lids))
    ids = sorted(lids)
    counts = _observers(ctx, ids, ids, np.concatenate([chain, lt.colliding(4, seed=9)]))
    assert counts[:48].max() >= 5 and counts[:48].min() >= 1
    got, _ = _check(pkg, ctx, ids, ids, ids, min_observers=3, ratio=0.5)
    assert 0 < got["n_culled"] < 7


def test_fresh_ids_and_the_largest_id(pkg, ctx):
    lids = {1: np.arange(40), 2: np.arange(40), 3: np.arange(40), 4: np.arange(10, 50)}
    store = cr.store_of(lids)
    _fill(ctx, store)
    ctx.kf_add(5, store[1][0], store[1][1])               # fresh ids (bit 62) ...
    assert ctx.kf_union(6, [5]) == 40 and ctx.kf_union(7, [5, 4]) == 80                     # ... shared through unions, listed as entries
    ctx.kf_union(8, [5])
    assert ctx.kf_replace_ids([12], [TOP]) == 5           # 2^63 - 1 arrives by a replacement
    ids = [1, 2, 3, 4, 5, 6, 7, 8]
    fresh = ctx.kf_read_ids(5)
    assert (fresh >> 62 == 1).all()
    counts = _observers(ctx, ids, ids, np.concatenate([fresh[:3], [TOP, 12, 11, int(lm.fresh_ids(99, 1)[0])]]))
    assert counts.tolist() == [4, 4, 4, 5, 0, 5, 0]
    got, _ = _check(pkg, ctx, ids, ids, [5, 6, 1, 7])
    assert got["culled"].tolist() == [True, False, False, False]                            # 5 goes, so 6 has two others left


@pytest.mark.parametrize("name", cr.HAND_CASES + ["chain"])
def test_hand_cases_and_the_chain(pkg, ctx, name):
    if name == "chain":
        lids, ids, cand, kw, expect = cr.chain_case()
    else:
        lids, ids, cand, kw = cr.hand_case(name)
        expect = cr.cull_search(lids, ids, cand, **kw)["culled"].tolist()
    _fill(ctx, cr.store_of(lids))
    got, _ = _check(pkg, ctx, sorted(lids), ids, cand, what=name, **kw)
    assert got["culled"].tolist() == expect
    if name.startswith("mutual_pair"):
        assert got["culled"].tolist() == [True, False] and got["n_redundant"].tolist() == [20, 0]


def test_two_runs_give_equal_bytes(ctx):
    store = cr.random_case(21, [700, 650, 1025, 300, 512] + [400] * 70, pool=1500, repeats=0.1)
    ids = sorted(store)
    _fill(ctx, store)
    cand = ids[::2]
    a, b = (ctx.kf_cull_search(ids, cand, min_observers=16, ratio=0.7) for _ in range(2))
    assert 0 < a["n_culled"] < len(cand) and a["n_culled"] == b["n_culled"]
    assert all(a[k].tobytes() == b[k].tobytes() for k in ("culled", "n_landmarks", "n_redundant"))
    asked = np.arange(1600)
    assert ctx.kf_observers(ids, asked).tobytes() == ctx.kf_observers(ids, asked).tobytes()


def test_cull_frees_the_slots(pkg, ctx):
    lids, ids, cand, kw, expect = cr.chain_case()
    store = cr.store_of(lids)
    _fill(ctx, store)
    ctx.kf_add(300, store[200][0], store[200][1])         # fresh ids: they carry the creation serial ...
    serial = (int(ctx.kf_read_ids(300)[0]) & ((1 << 62) - 1)) >> 16
    present = ids + [300]
    got, left = _check(pkg, ctx, present, ids, cand, remove=True, **kw)
    gone = [k for k, c in zip(cand, got["culled"]) if c]
    assert got["culled"].tolist() == expect and ctx.kf_size() == len(present) - 4 and left == sorted(set(present) - set(gone))
    for k in gone:
        with pytest.raises(pkg.MslamHipError) as e:
            ctx.kf_remove(k)                               # gone already
        assert e.value.code == pkg.E_INVALID
        with pytest.raises(pkg.MslamHipError):
            ctx.kf_cull_search(left + [k], [])
    # ... and a cull leaves it alone: the next entry made takes the next serial, in a freed slot, and nothing else moves
    before = _snapshot(ctx, left)
    ctx.kf_add(gone[0], store[201][0], store[201][1])
    assert np.array_equal(ctx.kf_read_ids(gone[0]), lm.fresh_ids(serial + 1, len(store[201][2])))
    assert ctx.kf_size() == len(left) + 1
    for i in left:
        _same(_read(ctx, i), before[i], i)
    # the same candidates again: the even ones are not in the store any more
    with pytest.raises(pkg.MslamHipError) as e:
        ctx.kf_cull(ids, cand, **kw)
    assert e.value.code == pkg.E_INVALID and ctx.kf_size() == len(left) + 1
    # what stayed can still be judged, and a search removes nothing
    got, _ = _check(pkg, ctx, left + [gone[0]], left, [k for k in cand if k in left], **kw)
    assert not got["culled"].any()


def test_a_union_that_is_not_listed_does_not_count(pkg, ctx):
    r = list(range(30))
    lids = {1: r, 2: r, 3: r, 4: list(range(100, 110))}
    _fill(ctx, cr.store_of(lids))
    U = pkg.HipKeyframeTracker.LOCAL_MAP_ID
    assert ctx.kf_union(U, [1, 2, 3, 4]) == 40
    present = [1, 2, 3, 4, U]
    assert _observers(ctx, present, [1, 2, 3, 4], [0, 100]).tolist() == [3, 1]
    assert _observers(ctx, present, present, [0, 100]).tolist() == [4, 2]
    got, _ = _check(pkg, ctx, present, [1, 2, 3, 4], [1, 4])
    assert got["culled"].tolist() == [False, False] and got["n_redundant"].tolist() == [0, 0]       # two others, not three
    got, _ = _check(pkg, ctx, present, present, [1, 4])
    assert got["culled"].tolist() == [True, False]                                                   # listed, it would count
    got, left = _check(pkg, ctx, present, [1, 2, 3, 4], [1, 2], remove=True, min_observers=2)
    assert got["culled"].tolist() == [True, False] and left == [2, 3, 4, U]


def test_errors_leave_the_store_and_zero_the_outputs(pkg, ctx):
    store = cr.random_case(8, [300, 40, 257, 0], pool=400)
    ids = sorted(store)
    _fill(ctx, store)
    L, h = pkg.lib(), ctx._h
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(entry, ids_, cand_, mo=3, ratio=0.9, ml=1, n_ids=None, n_cand=None):
        i, c = np.array(ids_, np.int32), np.array(cand_, np.int32)
        m = max(len(c), 1)
        culled, nl, nr, n = np.full(m, 7, np.uint8), np.full(m, 7, np.int32), np.full(m, 7, np.int32), C.c_int(7)
        rc = entry(h, p(i), len(i) if n_ids is None else n_ids, p(c), len(c) if n_cand is None else n_cand, mo, C.c_double(ratio), ml,
                   p(culled), p(nl), p(nr), C.byref(n))
        return rc, culled[:len(c)], nl[:len(c)], nr[:len(c)], n.value

    a, b = ids[0], ids[1]
    bad = [dict(ids_=[a, 9], cand_=[a]), dict(ids_=[a, a], cand_=[a]), dict(ids_=[a, b], cand_=[a, a]), dict(ids_=[a], cand_=[b]),
           dict(ids_=[a, b], cand_=[a], mo=0), dict(ids_=[a, b], cand_=[a], mo=65536), dict(ids_=[a, b], cand_=[a], ratio=float("nan")),
           dict(ids_=[a, b], cand_=[a], ratio=1.0000001), dict(ids_=[a, b], cand_=[a], ratio=-0.1), dict(ids_=[a, b], cand_=[a], ml=0),
           dict(ids_=[], cand_=[]), dict(ids_=[a, b], cand_=[a], n_ids=0), dict(ids_=[a], cand_=[a, a], n_cand=2)]
    for entry in (L.mslam_hip_kf_cull_search, L.mslam_hip_kf_cull):
        for kw in bad:
            rc, culled, nl, nr, n = call(entry, **kw)
            assert rc == pkg.E_INVALID and n == 0, kw
            if kw.get("n_cand", 1) <= len(kw["ids_"]):
                assert not culled.any() and not nl.any() and not nr.any(), kw
            assert ctx.kf_size() == len(ids)
    for i in ids:
        _same(_read(ctx, i), store[i], "after the errors")
    assert L.mslam_hip_kf_cull_search(h, None, 1, None, 0, 3, C.c_double(0.9), 1, None, None, None, None) == pkg.E_INVALID
    i = np.array(ids, np.int32)
    assert L.mslam_hip_kf_cull_search(h, p(i), len(i), p(i), 2, 3, C.c_double(0.9), 1, None, None, None, None) == pkg.E_INVALID
    assert L.mslam_hip_kf_cull_search(h, p(i), len(i), None, 0, 3, C.c_double(0.9), 1, None, None, None, None) == 0      # n_cand = 0
    # kf_observers
    asked, counts = np.array([1, -1, 2], np.int64), np.full(3, 7, np.int32)
    assert L.mslam_hip_kf_observers(h, p(i), len(i), p(asked), 3, p(counts)) == pkg.E_INVALID and not counts.any()
    counts[:] = 7
    j = np.array([ids[0], 9], np.int32)
    assert L.mslam_hip_kf_observers(h, p(j), 2, p(asked[:1]), 1, p(counts)) == pkg.E_INVALID and counts.tolist() == [0, 7, 7]
    assert L.mslam_hip_kf_observers(h, p(i), len(i), None, 2, None) == pkg.E_INVALID
    assert L.mslam_hip_kf_observers(h, p(i), len(i), None, 0, None) == 0
    with pytest.raises(pkg.MslamHipError) as e:
        ctx.kf_cull(ids, [9])
    assert e.value.code == pkg.E_INVALID and "9" in str(e.value)
    # NULL count outputs: the call still judges; and a clean call follows the errors
    culled = np.zeros(2, np.uint8)
    c2 = np.array(ids[:2], np.int32)
    assert L.mslam_hip_kf_cull_search(h, p(i), len(i), p(c2), 2, 1, C.c_double(0.1), 1, p(culled), None, None, None) == 0
    ref = cr.cull_search(store, ids, ids[:2], min_observers=1, ratio=0.1)
    assert culled.astype(bool).tolist() == ref["culled"].tolist()
    _check(pkg, ctx, ids, ids, ids, min_observers=1, ratio=0.1)
    _observers(ctx, ids, ids, np.arange(410))


# ---- the tracker --------------------------------------------------------------------------------------------------------
def _tracker(pkg, **kw):
    c = pkg.Context(width=0, height=0, max_keypoints=4096)
    t = pkg.HipKeyframeTracker(c, focal=CAM[:2], principal=CAM[2:], local_map_depth=cr.WALK_DEPTH, local_ba=True, **dict(cr.WALK_PARAMS, **kw))
    return c, t


def _walk(t, frames):
    return [t.processSensorData(fr["desc"], fr["xy"], fr["depth"]) for fr in frames]


def _errors(rows, frames):
    return (max(rr.rot_err(o["R"], fr["R"]) for o, fr in zip(rows, frames)),
            max(float(np.linalg.norm(o["tvec"] - fr["t"])) for o, fr in zip(rows, frames)))


@pytest.fixture(scope="module")
def walk():
    return cr.triple_walk()


def test_tracker_culls_on_the_triple_walk(pkg, walk):
    """the CPU condition (tests/test_cull.py): the CPU tracker with culling removes 16 of this walk's 25 keyframes"""
    import synth
    frames = walk["frames"]
    c0, t0 = _tracker(pkg)
    plain = _walk(t0, frames)
    c = pkg.Context(width=0, height=0, max_keypoints=4096)
    c.bow_load(synth.make_vocabulary(10, 3))
    # loop_min_score out of reach: the database is fed and never closes a loop, so its entries can be counted
    t = pkg.HipKeyframeTracker(c, focal=CAM[:2], principal=CAM[2:], local_map_depth=cr.WALK_DEPTH, local_ba=True, kf_cull=True,
                               loop_closure=True, loop_min_score=2.0, **cr.WALK_PARAMS)
    calls, real = [], c.kf_cull

    def spy(ids, cand, *a):
        before = {i: c.kf_read_ids(i) for i in ids}
        res = real(ids, cand, *a)
        calls.append((before, list(ids), list(cand), a, res))
        return res
    c.kf_cull = spy
    rows = _walk(t, frames)
    assert len(calls) == len(t.cull_results) > 0
    gone = []
    for (before, ids, cand, a, res), rec in zip(calls, t.cull_results):
        assert a == (3, 0.9) and pkg.HipKeyframeTracker.LOCAL_MAP_ID not in ids
        ref = cr.cull_search(before, ids, cand)
        assert cr.same_result(res, ref), rec["keyframe"]
        assert rec["listed"] == ids and rec["candidates"] == cand and rec["culled"] == [k for k, f in zip(cand, ref["culled"]) if f]
        assert rec["n_landmarks"] == ref["n_landmarks"].tolist() and rec["n_redundant"] == ref["n_redundant"].tolist()
        assert 0 not in cand and rec["keyframe"] not in cand and cand == sorted(cand)
        gone += rec["culled"]
    print("GPU tracker: %d keyframes inserted, culled %s, left %s" % (len(t0.ids), gone, t.ids))
    assert len(gone) >= 2 and len(set(gone)) == len(gone) and sorted(t.ids + gone) == t0.ids
    assert c.kf_size() == len(t.ids) + 1                   # the keyframes and the local map
    assert c.bow_db_size() == len(t0.ids) and sorted(t._bow_entry.values()) == t.ids      # every keyframe was fed ...
    hits, _ = c.bow_db_query(frames[5]["desc"], max_results=64)
    assert len(hits) > 0 and all(int(e) in t._bow_entry for e in hits)                    # ... and a culled one is never a hit again
    for k in gone:
        assert k not in t.graph and k not in t.backend.poses and k not in t.backend.obs and k not in t._bow_entry.values()
        assert all(k not in v for v in t.graph.values())
        with pytest.raises(pkg.MslamHipError):
            c.kf_read_ids(k)
    assert sorted(t.graph) == sorted(t.backend.poses) == t.ids and cr.is_connected(t.graph)
    assert all(t.backend.anchor[l] in t.backend.poses for l in t.backend.landmarks)
    assert all(o["tracked"] for o in rows) and all(o["tracked"] for o in plain)
    e0, e1 = _errors(plain, frames), _errors(rows, frames)
    print("max pose error without culling %.4f deg %.5f m, with culling %.4f deg %.5f m" % (e0 + e1))
    assert e0[0] <= 0.1 and e0[1] <= 0.02                  # the bound of tests/test_gpu_fuse.py's walk ...
    assert e1[0] <= 0.1 and e1[1] <= 0.02                  # ... which the culled map meets as well
    c.close(), c0.close()


def test_tracker_without_kf_cull_is_todays_tracker(pkg, walk):
    frames = walk["frames"][:12]
    c0, t0 = _tracker(pkg)
    c1, t1 = _tracker(pkg, kf_cull=False)
    a, b = _walk(t0, frames), _walk(t1, frames)
    assert t0.ids == t1.ids and t0.graph == t1.graph and t1.cull_results == [] and len(t0.ids) > 5
    for x, y in zip(a, b):
        assert (x["tracked"], x["keyframe"], x["reference"], x["n_inliers"]) == (y["tracked"], y["keyframe"], y["reference"], y["n_inliers"])
        assert np.array_equal(x["R"], y["R"]) and np.array_equal(x["tvec"], y["tvec"]) and sorted(x) == sorted(y)
    assert c0.kf_size() == c1.kf_size()
    for i in t0.ids + [pkg.HipKeyframeTracker.LOCAL_MAP_ID]:
        _same(_read(c1, i), _read(c0, i), i)
    assert sorted(t0.backend.landmarks) == sorted(t1.backend.landmarks) and t0.backend.anchor == t1.backend.anchor
    for k in t0.backend.poses:
        assert t0.backend.poses[k].tobytes() == t1.backend.poses[k].tobytes()
        assert t0.backend.obs[k][0].tobytes() == t1.backend.obs[k][0].tobytes() and t0.backend.obs[k][1].tobytes() == t1.backend.obs[k][1].tobytes()
    assert all(t0.backend.landmarks[l].tobytes() == t1.backend.landmarks[l].tobytes() for l in t0.backend.landmarks)
    c0.close(), c1.close()


@pytest.mark.parametrize("window", [1, 4])
def test_process_window_culls_as_the_frame_loop_does(pkg, walk, window):
    """every frame of this walk is a keyframe, so every window ends at its first frame: the same events in the same order"""
    frames = walk["frames"][:14]
    c0, t0 = _tracker(pkg, kf_cull=True)
    a = _walk(t0, frames)
    c1, t1 = _tracker(pkg, kf_cull=True)
    b = t1.process_window([f["desc"] for f in frames], [f["xy"] for f in frames], [f["depth"] for f in frames], window=window)
    key = lambda t: [(r["keyframe"], r["listed"], r["candidates"], r["culled"], r["n_landmarks"], r["n_redundant"], r["bridges"])
                     for r in t.cull_results]
    assert sum(len(r["culled"]) for r in t0.cull_results) >= 2
    assert t1.ids == t0.ids and t1.graph == t0.graph and key(t1) == key(t0)
    assert [o["keyframe"] for o in b] == [o["keyframe"] for o in a] and all(o["tracked"] for o in b)
    assert c1.kf_size() == c0.kf_size() == len(t0.ids) + 1
    c0.close(), c1.close()
