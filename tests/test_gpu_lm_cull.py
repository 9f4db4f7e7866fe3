"""mslam_hip_kf_remove_landmarks, mslam_hip_kf_cull_landmarks_search and mslam_hip_kf_cull_landmarks on the GPU, through
Context and the C entry points, against tests/lm_cull_ref.py: every output and every entry byte for byte, on the smallest
shapes where the kernels can go wrong (max_keypoints = 600, so an entry spans the compaction's 256-position chunk twice and
ends mid-chunk; entry sizes round the chunk; listed entries round the 64-entry mark chunk; repeats; caller and fresh ids;
an entry lifted on the device); entries that are not listed; the capacity and the NULL list; the errors; determinism; the
fused call against its two halves; and HipKeyframeTracker(lm_cull=True) on lm_cull_ref.sequence()."""
import ctypes as C

import numpy as np
import pytest

import cull_ref as cr
import lm_cull_ref as lc
import local_map_ref as lm
import track_ref as tr

pytestmark = pytest.mark.gpu
K = 600
CAM = tr.CAM
SIZES = [0, 1, 255, 256, 257, 600]


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


def _same_store(c, present, ref, what=""):
    assert c.kf_size() == len(present)
    for i in present:
        _same(_read(c, i), ref[i], (what, i))


def _check_cull(c, present, ids, cand, min_observers=2, fused=True, what=""):
    """one call against the restatement run on the store as read back: the outputs, and every entry afterwards"""
    before = _snapshot(c, present)
    after, ref = lc.cull_landmarks(before, ids, cand, min_observers)
    if fused:
        got = c.kf_cull_landmarks(ids, cand, min_observers)
        assert got["entry_removed"].dtype == np.int32 and np.array_equal(got["entry_removed"], ref["entry_removed"]), what
        assert got["n_removed"] == ref["n_removed"], what
    else:
        got = c.kf_cull_landmarks_search(ids, cand, min_observers)
    assert lc.same_search(got, ref), (what, got, ref)
    _same_store(c, present, after if fused else before, what)
    return got


def _check_remove(c, present, ids, landmark_ids, what=""):
    before = _snapshot(c, present)
    after, ref = lc.remove_landmarks(before, ids, landmark_ids)
    got = c.kf_remove_landmarks(ids, landmark_ids)
    assert got["removed"].dtype == got["entry_removed"].dtype == np.int32
    assert np.array_equal(got["removed"], ref["removed"]) and np.array_equal(got["entry_removed"], ref["entry_removed"]), what
    assert got["n_removed"] == ref["n_removed"], what
    _same_store(c, present, after, what)
    return got


# ---- entry sizes and removed positions ----------------------------------------------------------------------------------
def _sized_store(seed=1):
    """entry 100 + e has SIZES[e] landmarks with ids of its own, 1000 e + position"""
    rng = np.random.default_rng(seed)
    return {100 + e: cr.entry(rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.normal(size=(n, 3)), 1000 * e + np.arange(n, dtype=np.int64))
            for e, n in enumerate(SIZES)}


def _positions(pattern, n):
    pos = {"edges": [0, 255, 256, n - 1], "chunk": range(256, 512) if n > 512 else range(0, min(n, 256)),
           "everything": range(n), "nothing": [], "every_other": range(0, n, 2)}[pattern]
    return sorted({p for p in pos if 0 <= p < n})


PATTERNS = ["edges", "chunk", "everything", "nothing", "every_other"]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_remove_landmarks_entry_sizes_and_positions(ctx, pattern):
    store = _sized_store()
    ids = sorted(store)
    _fill(ctx, store)
    asked = np.concatenate([store[k][2][_positions(pattern, len(store[k][2]))] for k in ids] + [np.array([77_000, (1 << 62) + 5], np.int64)])
    asked = np.concatenate([asked, asked[:3]])                                                            # absent ids, rows twice
    asked = asked[np.random.default_rng(2).permutation(len(asked))]
    got = _check_remove(ctx, ids, ids, asked, pattern)
    assert got["n_removed"] == sum(len(_positions(pattern, n)) for n in SIZES)
    if pattern == "everything":
        assert all(len(ctx.kf_read_ids(k)) == 0 for k in ids) and ctx.kf_size() == len(ids)          # emptied entries stay entries
    # the entries are still usable: a second removal on what is left
    _check_remove(ctx, ids, ids[::-1], [1000 * 5 + 599, 1000 * 5 + 1, 2001], pattern + " again")


@pytest.mark.parametrize("pattern", PATTERNS)
def test_cull_landmarks_entry_sizes_and_positions(ctx, pattern):
    """the same positions leave through the rule: every entry has a mirror that holds the ids that are to stay, so exactly
    the chosen positions have one observer; the mirrors are listed and not candidates and stay byte-identical"""
    store = _sized_store()
    rng = np.random.default_rng(3)
    for e, n in enumerate(SIZES):
        keep = np.setdiff1d(np.arange(n), _positions(pattern, n))
        l = (1000 * e + keep[rng.permutation(len(keep))]).astype(np.int64)
        store[200 + e] = cr.entry(rng.integers(0, 256, (len(l), 32), dtype=np.uint8), rng.normal(size=(len(l), 3)), l)
    present = sorted(store)
    cand = present[:len(SIZES)]
    _fill(ctx, store)
    _check_cull(ctx, present, present, cand, fused=False, what=pattern)
    got = _check_cull(ctx, present, present, cand, what=pattern)
    assert len(got["landmark_ids"]) == got["n_removed"] == sum(len(_positions(pattern, n)) for n in SIZES)
    assert (got["observers"] == 1).all() and not got["entry_removed"][len(SIZES):].any()
    for k in present[len(SIZES):]:
        _same(_read(ctx, k), store[k], ("mirror", k))
    assert len(_check_cull(ctx, present, present, cand, what=pattern + " again")["landmark_ids"]) == 0


# ---- listed entries round the mark chunk ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, lc.MARK_CHUNK, lc.MARK_CHUNK + 1])
def test_listed_entries_round_the_chunk_and_the_candidate_counts(ctx, n):
    rng = np.random.default_rng(n)
    sizes = [int(s) for s in rng.integers(20, 60, n)]
    for which in ("none", "one", "all"):
        store = cr.random_case(10 + n, sizes, pool=max(40 * n // 3, 80), repeats=0.1)
        ids = sorted(store)
        _fill(ctx, store)
        cand = {"none": [], "one": [ids[-1]], "all": ids[::-1]}[which]
        mo = 2 if n < lc.MARK_CHUNK else 3
        _check_cull(ctx, ids, ids, cand, mo, fused=False, what=(n, which))
        got = _check_cull(ctx, ids, ids, cand, mo, what=(n, which))
        assert (which == "none") == (len(got["landmark_ids"]) == 0), (n, which)
        if which == "all" and n > 1:
            assert got["observers"].max() == mo - 1 and got["n_removed"] > len(got["landmark_ids"])   # repeats: more positions than ids


# ---- what is not listed -------------------------------------------------------------------------------------------------
def test_an_unlisted_entry_and_a_union_are_neither_observers_nor_changed(pkg, ctx):
    lids = {1: list(range(0, 40)), 2: list(range(20, 60)), 3: list(range(0, 10)) + list(range(300, 330)), 4: list(range(40, 60))}
    _fill(ctx, cr.store_of(lids))
    U = pkg.HipKeyframeTracker.LOCAL_MAP_ID
    assert ctx.kf_union(U, [1, 2, 3]) == 90
    present = [1, 2, 3, 4, U]
    union, four = _read(ctx, U), _read(ctx, 4)
    # listed 1, 2, 3: ids 40..59 have entry 2 alone (entry 4 and the union hold them too, but are not listed)
    got = _check_cull(ctx, present, [1, 2, 3], [2], fused=False)
    assert got["landmark_ids"].tolist() == list(range(40, 60))
    assert len(ctx.kf_cull_landmarks_search([1, 2, 3, 4], [2])["landmark_ids"]) == 0                  # listed, entry 4 counts
    assert len(ctx.kf_cull_landmarks_search([1, 2, 3, U], [2])["landmark_ids"]) == 0                  # ... and so would the union
    got = _check_cull(ctx, present, [1, 2, 3], [2, 3])
    assert got["landmark_ids"].tolist() == list(range(40, 60)) + list(range(300, 330)) and got["entry_removed"].tolist() == [0, 20, 30]
    _same(_read(ctx, U), union, "the union keeps its copy")
    _same(_read(ctx, 4), four, "the unlisted entry")
    got = _check_remove(ctx, present, [3, 4], [45, 5, 25])                                            # 25: entries 1 and 2 hold it, unlisted
    assert got["removed"].tolist() == [1, 1, 0] and got["entry_removed"].tolist() == [1, 1]
    assert 25 in ctx.kf_read_ids(1) and 5 in ctx.kf_read_ids(1)
    _same(_read(ctx, U), union, "the union keeps its copy")


@pytest.mark.parametrize("name", lc.HAND_CASES)
def test_hand_cases(ctx, name):
    lids, ids, cand, mo = lc.hand_case(name)
    expect = lc.cull_landmarks_search(lids, ids, cand, mo)["landmark_ids"].tolist()
    _fill(ctx, cr.store_of(lids))
    assert _check_cull(ctx, sorted(lids), ids, cand, mo, fused=False, what=name)["landmark_ids"].tolist() == expect
    assert _check_cull(ctx, sorted(lids), ids, cand, mo, what=name)["landmark_ids"].tolist() == expect


def test_repeats_across_chunks_and_inside_one(ctx):
    n = 600
    l = 10_000 + np.arange(n, dtype=np.int64)
    l[[255, 256]] = 1                                     # across the two sides of a chunk edge
    l[[0, 300, 599]] = 2                                  # one position in each chunk
    l[500:520] = 3
    l[[100, 101]] = 4                                     # held by entry 2 as well: stays
    lids = {1: l, 2: np.concatenate([[4, 4], 10_000 + np.arange(3, 598)]), 3: [1, 1, 2]}
    _fill(ctx, cr.store_of(lids))
    got = _check_cull(ctx, [1, 2, 3], [1, 2], [1])        # entry 3 is not listed: 1 and 2 have one observer
    assert got["landmark_ids"].tolist()[:3] == [1, 2, 3] and got["entry_removed"][0] == 2 + 3 + 20 + len(got["landmark_ids"]) - 3
    assert 4 not in got["landmark_ids"]


def test_caller_ids_and_fresh_ids_mixed(ctx):
    lids = {1: np.arange(40), 2: np.arange(20, 60)}
    store = cr.store_of(lids)
    _fill(ctx, store)
    ctx.kf_add(5, store[1][0], store[1][1])               # fresh ids (bit 62) ...
    ctx.kf_add(6, store[2][0][:7], store[2][1][:7])
    assert ctx.kf_union(7, [5, 2]) == 80                  # ... and an entry that mixes them with caller ids
    assert ctx.kf_replace_ids([30], [(1 << 63) - 1]) == 3  # 2^63 - 1 arrives by a replacement
    fresh = ctx.kf_read_ids(5)
    assert (fresh >> 62 == 1).all()
    present = [1, 2, 5, 6, 7]
    got = _check_cull(ctx, present, present, [6, 7, 1], fused=False)
    assert set(ctx.kf_read_ids(6).tolist()) <= set(got["landmark_ids"].tolist())                      # entry 6's fresh ids: one observer
    assert not set(fresh.tolist()) & set(got["landmark_ids"].tolist())                                # entries 5 and 7 hold those
    assert got["landmark_ids"].tolist()[:20] == list(range(20)) and (got["landmark_ids"][-7:] >> 62 == 1).all()
    got = _check_remove(ctx, present, [7, 5], np.concatenate([fresh[::3], np.array([(1 << 63) - 1, 21], np.int64)]))
    assert got["removed"].tolist() == [2] * len(fresh[::3]) + [1, 1]                                  # entries 1 and 2 are not listed
    _check_cull(ctx, present, present, [6, 7, 1], 3)


def test_an_entry_lifted_on_the_device(ctx):
    """a union built without a synchronisation: the host knows only min(sum of sizes, max_keypoints) = 600 of it, the
    device count is 250.  The grids cover the 600, the kernels read the device count, and afterwards the size is exact"""
    rng = np.random.default_rng(6)
    base = np.arange(250, dtype=np.int64)
    lids = {1: base, 2: base[rng.permutation(250)], 3: base[rng.permutation(250)], 4: np.arange(100, 180)}
    store = cr.store_of(lids, seed=6)
    for fused in (False, True, None):
        _fill(ctx, store)
        ctx.kf_union(9, [1, 2, 3], sync=False)
        ctx.sync()
        d, w, l = lm.union({k: v[:2] for k, v in store.items()}, {k: v[2] for k, v in store.items()}, [1, 2, 3])
        before = dict(store)
        before[9] = cr.entry(d, w, l)
        assert len(l) == 250
        if fused is None:
            after, ref = lc.remove_landmarks(before, [9, 4], [5, 249, 150, 999])
            got = ctx.kf_remove_landmarks([9, 4], [5, 249, 150, 999])
            assert got["removed"].tolist() == ref["removed"].tolist() == [1, 1, 2, 0] and got["entry_removed"].tolist() == [3, 1]
        else:
            after, ref = lc.cull_landmarks(before, [9, 4], [9], 2)
            got = (ctx.kf_cull_landmarks if fused else ctx.kf_cull_landmarks_search)([9, 4], [9], 2)
            assert lc.same_search(got, ref) and len(ref["landmark_ids"]) == 250 - 80
            if fused:
                assert got["entry_removed"].tolist() == ref["entry_removed"].tolist() == [170, 0]
            else:
                after = before
        _same_store(ctx, [1, 2, 3, 4, 9], after, fused)


# ---- the capacity, the NULL list, the errors ----------------------------------------------------------------------------
def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _raw(pkg, c, fused, ids, cand, mo=2, cap=4096, with_list=True, n_ids=None, n_cand=None, with_found=True):
    """the C entry point with prefilled outputs -> (rc, ids, observers, n_found, entry_removed, n_removed)"""
    L, h = pkg.lib(), c._h
    i, k = np.array(ids, np.int32), np.array(cand, np.int32)
    l, o = np.full(max(cap, 1), 7, np.int64), np.full(max(cap, 1), 7, np.int32)
    n, lost, nr = C.c_int(7), np.full(max(len(i), 1), 7, np.int32), C.c_int(7)
    args = [h, _p(i), len(i) if n_ids is None else n_ids, _p(k), len(k) if n_cand is None else n_cand, mo,
            _p(l) if with_list else None, _p(o) if with_list else None, cap, C.byref(n) if with_found else None]
    rc = L.mslam_hip_kf_cull_landmarks(*args, _p(lost), C.byref(nr)) if fused else L.mslam_hip_kf_cull_landmarks_search(*args)
    return rc, l, o, n.value, lost[:len(i)], nr.value


def _capacity_store():
    return cr.random_case(8, [300, 40, 257, 0, 600, 120], pool=900, repeats=0.1)


@pytest.mark.parametrize("fused", [False, True])
def test_a_capacity_one_short_changes_nothing_and_reports_the_count(pkg, ctx, fused):
    store = _capacity_store()
    ids = sorted(store)
    _fill(ctx, store)
    cand = ids[:3] + ids[4:5]
    ref = lc.cull_landmarks_search(store, ids, cand, 2)
    need = len(ref["landmark_ids"])
    assert need > 100
    rc, l, o, n, lost, nr = _raw(pkg, ctx, fused, ids, cand, cap=need - 1)
    assert rc == pkg.E_CAPACITY and n == need and not l.any() and not o.any()                        # nothing is copied
    assert not fused or (nr == 0 and not lost.any())
    _same_store(ctx, ids, store, "after E_CAPACITY")
    rc, l, o, n, lost, nr = _raw(pkg, ctx, fused, ids, cand, cap=0)
    assert rc == pkg.E_CAPACITY and n == need
    _same_store(ctx, ids, store, "after E_CAPACITY at capacity 0")
    # exactly enough
    rc, l, o, n, lost, nr = _raw(pkg, ctx, fused, ids, cand, cap=need)
    assert rc == 0 and n == need and np.array_equal(l[:need], ref["landmark_ids"]) and np.array_equal(o[:need], ref["observers"])
    after, full = lc.cull_landmarks(store, ids, cand, 2)
    if fused:
        assert np.array_equal(lost, full["entry_removed"]) and nr == full["n_removed"]
    _same_store(ctx, ids, after if fused else store, "exactly enough")


def test_the_wrapper_grows_its_capacity_and_retries_once(pkg):
    c = pkg.Context(width=0, height=0, max_keypoints=K)
    store = {100 + e: cr.entry(np.zeros((K, 32), np.uint8), np.zeros((K, 3)), 1000 * e + np.arange(K, dtype=np.int64)) for e in range(3)}
    _fill(c, store)
    ids = sorted(store)
    assert c._lm_cull_capacity < 3 * K
    got = c.kf_cull_landmarks(ids, ids)                     # 1800 landmarks with one observer: more than the first capacity
    assert len(got["landmark_ids"]) == got["n_removed"] == 3 * K and c._lm_cull_capacity == 3 * K
    assert all(len(c.kf_read_ids(k)) == 0 for k in ids)
    c.close()


@pytest.mark.parametrize("fused", [False, True])
def test_with_a_null_list_only_the_counts_come_back(pkg, ctx, fused):
    store = _capacity_store()
    ids = sorted(store)
    _fill(ctx, store)
    after, ref = lc.cull_landmarks(store, ids, ids[:2], 2)
    rc, l, o, n, lost, nr = _raw(pkg, ctx, fused, ids, ids[:2], cap=-5, with_list=False)            # the capacity is not consulted
    assert rc == 0 and n == len(ref["landmark_ids"]) > 0
    if fused:
        assert np.array_equal(lost, ref["entry_removed"]) and nr == ref["n_removed"]
    _same_store(ctx, ids, after if fused else store)
    # a list without the observer counts
    _fill(ctx, store)
    L, i = pkg.lib(), np.array(ids, np.int32)
    l, nf = np.zeros(4096, np.int64), C.c_int(0)
    assert L.mslam_hip_kf_cull_landmarks_search(ctx._h, _p(i), len(i), _p(i), 2, 2, _p(l), None, 4096, C.byref(nf)) == 0
    assert np.array_equal(l[:nf.value], ref["landmark_ids"])


def test_errors_leave_the_store_and_zero_the_outputs(pkg, ctx):
    store = _capacity_store()
    ids = sorted(store)
    _fill(ctx, store)
    a, b = ids[0], ids[1]
    bad = [dict(ids=[a, 9], cand=[a]), dict(ids=[a, a], cand=[a]), dict(ids=[a, b], cand=[a, a]), dict(ids=[a], cand=[b]),
           dict(ids=[a, b], cand=[a], mo=0), dict(ids=[a, b], cand=[a], mo=65536), dict(ids=[a, b], cand=[a], mo=-1),
           dict(ids=[], cand=[]), dict(ids=[a, b], cand=[a], n_ids=0), dict(ids=[a], cand=[a, a], n_cand=2),
           dict(ids=[a, b], cand=[a], n_cand=-1), dict(ids=[a, b], cand=[a], cap=-1), dict(ids=[a, b], cand=[a], with_found=False)]
    for fused in (False, True):
        for kw in bad:
            rc, l, o, n, lost, nr = _raw(pkg, ctx, fused, **kw)
            assert rc == pkg.E_INVALID, kw
            assert (n == 0 or not kw.get("with_found", True)) and (kw.get("cap", 1) < 0 or (not l.any() and not o.any())), kw
            if fused:
                assert nr == 0 and (not lost.any() or kw.get("n_ids") == 0 or not kw["ids"]), kw
            assert ctx.kf_size() == len(ids)
    L, h = pkg.lib(), ctx._h
    i = np.array(ids, np.int32)
    n = C.c_int(7)
    assert L.mslam_hip_kf_cull_landmarks_search(h, None, 1, None, 0, 2, None, None, 0, C.byref(n)) == pkg.E_INVALID and n.value == 0
    assert L.mslam_hip_kf_cull_landmarks_search(h, _p(i), len(i), None, 2, 2, None, None, 0, C.byref(n)) == pkg.E_INVALID
    assert L.mslam_hip_kf_cull_landmarks_search(h, _p(i), len(i), None, 0, 2, None, None, 0, C.byref(n)) == 0 and n.value == 0   # n_cand = 0
    # kf_remove_landmarks
    asked = np.array([1, -1, 2], np.int64)
    for kw in (dict(i=i, l=asked, n=3), dict(i=np.array([a, 9], np.int32), l=asked[:1], n=1), dict(i=np.array([a, a], np.int32), l=asked[:1], n=1),
               dict(i=i, l=None, n=2), dict(i=i, l=asked, n=-1), dict(i=i, l=asked, n=(1 << 24) + 1), dict(i=None, l=asked[:1], n=1)):
        removed, lost, nr = np.full(3, 7, np.int32), np.full(len(ids), 7, np.int32), C.c_int(7)
        rc = L.mslam_hip_kf_remove_landmarks(h, None if kw["i"] is None else _p(kw["i"]), 0 if kw["i"] is None else len(kw["i"]),
                                             None if kw["l"] is None else _p(kw["l"]), kw["n"], _p(removed), _p(lost), C.byref(nr))
        assert rc == pkg.E_INVALID and nr.value == 0, kw
        assert kw["n"] > (1 << 24) or not removed[:max(0, min(kw["n"], 3))].any(), kw           # (a count out of range names no array)
        assert kw["i"] is None or not lost[:len(kw["i"])].any(), kw
    with pytest.raises(pkg.MslamHipError) as e:
        ctx.kf_cull_landmarks(ids, [9])
    assert e.value.code == pkg.E_INVALID and "9" in str(e.value)
    _same_store(ctx, ids, store, "after the errors")
    # NULL outputs of the removal, n = 0, and a clean call after the errors
    assert L.mslam_hip_kf_remove_landmarks(h, _p(i), len(i), None, 0, None, None, None) == 0
    one = np.array([int(store[a][2][0])], np.int64)
    assert L.mslam_hip_kf_remove_landmarks(h, _p(i), len(i), _p(one), 1, None, None, None) == 0
    after, _ = lc.remove_landmarks(store, ids, one)
    _same_store(ctx, ids, after, "NULL outputs")
    _check_cull(ctx, ids, ids, ids[:3])


def test_two_runs_on_equal_stores_give_equal_bytes(ctx):
    store = cr.random_case(21, [600, 512, 300, 257] + [150] * 70, pool=4000, repeats=0.1)
    ids = sorted(store)
    cand = ids[::2]
    runs = []
    for _ in range(2):
        _fill(ctx, store)
        s = ctx.kf_cull_landmarks_search(ids, cand, 3)
        f = ctx.kf_cull_landmarks(ids, cand, 3)
        runs.append((s, f, _snapshot(ctx, ids)))
    (s0, f0, e0), (s1, f1, e1) = runs
    assert len(s0["landmark_ids"]) > 500 and set(s0["observers"].tolist()) == {1, 2}
    assert all(s0[k].tobytes() == s1[k].tobytes() == f0[k].tobytes() for k in ("landmark_ids", "observers"))
    assert all(f0[k].tobytes() == f1[k].tobytes() for k in ("landmark_ids", "observers", "entry_removed")) and f0["n_removed"] == f1["n_removed"]
    for k in ids:
        assert all(x.tobytes() == y.tobytes() for x, y in zip(e0[k], e1[k])), k


def test_the_fused_call_equals_the_search_followed_by_the_removal(ctx):
    store = cr.random_case(31, [600, 0, 1, 255, 256, 257, 90, 90, 90], pool=1500, repeats=0.15)
    ids = sorted(store)
    cand = ids[:6]
    _fill(ctx, store)
    fused = ctx.kf_cull_landmarks(ids, cand, 2)
    a = _snapshot(ctx, ids)
    _fill(ctx, store)
    found = ctx.kf_cull_landmarks_search(ids, cand, 2)
    rem = ctx.kf_remove_landmarks(ids, found["landmark_ids"])
    assert lc.same_search(fused, found) and len(found["landmark_ids"]) > 100
    assert np.array_equal(fused["entry_removed"], rem["entry_removed"]) and fused["n_removed"] == rem["n_removed"] == int(rem["removed"].sum())
    _same_store(ctx, ids, a, "search + removal")


# ---- the tracker --------------------------------------------------------------------------------------------------------
KT = 2048      # the unculled union of the sequence needs 1998 on the CPU tracker (tests/test_lm_cull.py)


def _tracker(pkg, **kw):
    c = pkg.Context(width=0, height=0, max_keypoints=KT)
    t = pkg.HipKeyframeTracker(c, focal=CAM[:2], principal=CAM[2:], local_map_depth=lc.DEPTH, **dict(lc.PARAMS, **kw))
    return c, t


def _walk(t, frames):
    return [t.processSensorData(fr["desc"], fr["xy"], fr["depth"]) for fr in frames]


def _spy(c, calls):
    real = c.kf_cull_landmarks

    def spy(ids, cand, *a):
        U = 0x7fffffff
        before = _snapshot(c, list(ids) + [U])
        res = real(ids, cand, *a)
        calls.append((before, list(ids), list(cand), a, res, _snapshot(c, list(ids) + [U])))
        return res
    c.kf_cull_landmarks = spy


def _hold_calls_to_the_restatement(pkg, t, calls):
    U = pkg.HipKeyframeTracker.LOCAL_MAP_ID
    assert len(calls) == len(t.lm_cull_results) > 0
    for (before, ids, cand, a, res, after), rec in zip(calls, t.lm_cull_results):
        assert a == (2,) and U not in ids
        new, ref = lc.cull_landmarks({k: before[k] for k in ids}, ids, cand, 2)
        assert lc.same_search(res, ref) and np.array_equal(res["entry_removed"], ref["entry_removed"]) and res["n_removed"] == ref["n_removed"]
        assert rec["listed"] == ids and rec["candidates"] == cand and np.array_equal(rec["landmark_ids"], ref["landmark_ids"])
        assert rec["n_removed"] == ref["n_removed"]
        for k in ids:
            _same(after[k], new[k], (rec["keyframe"], k))
        _same(after[U], before[U], "the local map keeps its copy until it is rebuilt")


def test_tracker_with_lm_cull_equals_the_cpu_tracker(pkg, orc):
    """without a backend nothing but the culling step differs from tests/test_gpu_local_map.py's tracker, which equals the
    CPU loop bit for bit in its identities: so do the keyframes, every call's culled ids and every keyframe's store ids"""
    seq = lc.sequence()
    rows, trk = lc.run(True)
    c, t = _tracker(pkg, lm_cull=True)
    calls = []
    _spy(c, calls)
    got = _walk(t, seq["frames"])
    _hold_calls_to_the_restatement(pkg, t, calls)
    assert all(o["tracked"] for o in got) and [o["keyframe"] for o in got] == [r["keyframe"] for r in rows]
    assert t.ids == trk.ids and t.graph == trk.graph and len(t.lm_cull_results) == len(trk.lm_cull_results)
    for rec, ref in zip(t.lm_cull_results, trk.lm_cull_results):
        assert (rec["keyframe"], rec["listed"], rec["candidates"], rec["n_removed"], rec["n_backend"]) == \
               (ref["keyframe"], ref["listed"], ref["candidates"], ref["n_removed"], 0)
        assert np.array_equal(rec["landmark_ids"], ref["landmark_ids"])
    for k in trk.ids:
        assert np.array_equal(c.kf_read_ids(k), trk.lids[k]), k
        assert np.array_equal(c.kf_read(k)[0], trk.store[k][0]), k
    print("GPU tracker: %d calls removed %s" % (len(calls), [r["n_removed"] for r in t.lm_cull_results]))
    c.close()


def test_tracker_with_local_ba_and_lm_cull(pkg, orc):
    """HipKeyframeTracker(local_map_depth=2, local_ba=True, lm_cull=True) on the sequence, held call by call to the
    restatement on the store as it was read before the call (the way tests/test_gpu_cull.py holds the culling tracker) and
    to the CPU tracker: the keyframes, every call's listed ids, candidates and culled ids, every keyframe's store ids, every
    frame tracked, a smaller union.  (The CPU tracker has no bundle adjustment; on this sequence the refined points leave
    every consensus set, and with it what a keyframe inherits, as it was: 14 of 14 calls cull the CPU tracker's ids.)"""
    seq = lc.sequence()
    rows, trk = lc.run(True)
    plain, trk0 = lc.run(False)
    c, t = _tracker(pkg, local_ba=True, lm_cull=True)
    calls = []
    _spy(c, calls)
    got = _walk(t, seq["frames"])
    _hold_calls_to_the_restatement(pkg, t, calls)
    assert all(o["tracked"] for o in got) and [o["keyframe"] for o in got] == [r["keyframe"] for r in rows]
    assert t.ids == trk.ids and len(calls) == len(trk.lm_cull_results)
    assert [(r["keyframe"], r["listed"], r["candidates"]) for r in t.lm_cull_results] == \
           [(r["keyframe"], r["listed"], r["candidates"]) for r in trk.lm_cull_results]
    same = [np.array_equal(a["landmark_ids"], b["landmark_ids"]) for a, b in zip(t.lm_cull_results, trk.lm_cull_results)]
    union = len(c.kf_read_ids(t.LOCAL_MAP_ID))
    print("GPU tracker with local BA: %d calls removed %s (backend %s); calls whose ids equal the CPU tracker's: %d of %d; last union %d "
          "(CPU: %d with, %d without)" % (len(calls), [r["n_removed"] for r in t.lm_cull_results], [r["n_backend"] for r in t.lm_cull_results],
                                          sum(same), len(same), union, trk.unions[-1], trk0.unions[-1]))
    assert any(r["n_removed"] > 0 for r in t.lm_cull_results) and union < trk0.unions[-1]
    assert all(same) and [r["n_removed"] for r in t.lm_cull_results] == [r["n_removed"] for r in trk.lm_cull_results]
    for k in trk.ids:
        assert np.array_equal(c.kf_read_ids(k), trk.lids[k]), k
    # the backend's observations name the store's landmarks, keyframe by keyframe, and it forgot what was culled
    gone = set(np.concatenate([r["landmark_ids"] for r in t.lm_cull_results]).tolist())
    for k in t.ids:
        assert np.array_equal(t.backend.obs[k][0], c.kf_read_ids(k)), k
    assert not gone & set(t.backend.landmarks) and not gone & set(t.backend.anchor)
    assert all(r["n_backend"] == r["n_removed"] for r in t.lm_cull_results)
    # after the run no landmark of a judged keyframe has fewer than two observers
    ids_of = {k: c.kf_read_ids(k) for k in t.ids}
    obs = cr.obs_counts(ids_of, t.ids)
    judged = sorted({k for r in t.lm_cull_results for k in r["candidates"]})
    assert all(obs[l] >= 2 for k in judged for l in ids_of[k].tolist())
    c.close()


def test_tracker_without_lm_cull_is_todays_tracker(pkg):
    frames = lc.sequence()["frames"][:8]
    c0 = pkg.Context(width=0, height=0, max_keypoints=KT)
    t0 = pkg.HipKeyframeTracker(c0, focal=CAM[:2], principal=CAM[2:], local_map_depth=lc.DEPTH, local_ba=True, **lc.PARAMS)   # as before
    c1, t1 = _tracker(pkg, local_ba=True, lm_cull=False)
    a, b = _walk(t0, frames), _walk(t1, frames)
    assert t0.ids == t1.ids and t0.graph == t1.graph and t1.lm_cull_results == [] and t1._lm_pending == [] and len(t0.ids) > 5
    for x, y in zip(a, b):
        assert (x["tracked"], x["keyframe"], x["reference"], x["n_inliers"]) == (y["tracked"], y["keyframe"], y["reference"], y["n_inliers"])
        assert np.array_equal(x["R"], y["R"]) and np.array_equal(x["tvec"], y["tvec"]) and sorted(x) == sorted(y)
    assert c0.kf_size() == c1.kf_size()
    for i in t0.ids + [pkg.HipKeyframeTracker.LOCAL_MAP_ID]:
        _same(_read(c1, i), _read(c0, i), i)
    for k in t0.backend.poses:
        assert t0.backend.poses[k].tobytes() == t1.backend.poses[k].tobytes() and t0.backend.obs[k][0].tobytes() == t1.backend.obs[k][0].tobytes()
    # against the CPU loop without the step: the same keyframes and identities as before this option existed
    rows, trk0 = lc.run(False)
    assert [o["keyframe"] for o in b] == [r["keyframe"] for r in rows[:8]]
    c0.close(), c1.close()


@pytest.mark.parametrize("window", [1, 4])
def test_process_window_culls_landmarks_as_the_frame_loop_does(pkg, window):
    frames = lc.sequence()["frames"][:9]
    c0, t0 = _tracker(pkg, lm_cull=True)
    a = _walk(t0, frames)
    c1, t1 = _tracker(pkg, lm_cull=True)
    b = t1.process_window([f["desc"] for f in frames], [f["xy"] for f in frames], [f["depth"] for f in frames], window=window)
    key = lambda t: [(r["keyframe"], r["listed"], r["candidates"], r["landmark_ids"].tolist(), r["n_removed"]) for r in t.lm_cull_results]
    assert sum(r["n_removed"] for r in t0.lm_cull_results) > 0 and key(t1) == key(t0) and t1.ids == t0.ids
    assert [o["keyframe"] for o in b] == [o["keyframe"] for o in a] and all(o["tracked"] for o in b)
    for k in t0.ids:
        assert np.array_equal(c1.kf_read_ids(k), c0.kf_read_ids(k))
    c0.close(), c1.close()
