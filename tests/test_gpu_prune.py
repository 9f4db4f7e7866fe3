"""mslam_hip_kf_remove_observations on the GPU, through Context.kf_remove_observations: the store read back byte for byte
against tests/prune_ref.py over entry sizes round the kernel's chunk, removal patterns, row-list variants and a grid of more
than 64 workgroups; kf_covisible, kf_union and track on a compacted entry against the references run on the restatement's
arrays; the errors; HipBackend.local_ba / global_ba(prune=True) on the three planted scenes against the pruned reference;
and HipKeyframeTracker(ba_prune=True) on a walk with planted depth errors."""
import ctypes as C

import numpy as np
import pytest

import ba_ref
import local_map_ref as lm
import prune_ref as pr
import track_ref as tr
from test_gpu_track import _compare_step, _rvec
from test_prune import check_pruned, _graph

pytestmark = pytest.mark.gpu
K = 2048
T = pr.T
SIZES = (0, 1, T - 1, T, T + 1, 4 * T + 3, K)
CAM = tr.CAM


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


def _same(got, ref, what=""):
    """descriptors, world points (as bytes), ids and count"""
    assert len(got[0]) == len(got[1]) == len(got[2]) == len(ref[2]), (what, len(got[2]), len(ref[2]))
    assert np.array_equal(got[2], ref[2]), what
    assert np.array_equal(got[0], ref[0]), what
    assert np.array_equal(got[1].view(np.uint64), np.ascontiguousarray(ref[1]).view(np.uint64)), what


def _check(c, store, kf, lid, what=""):
    """one call against the restatement: outputs and every entry of the store"""
    new, removed, n = pr.remove_observations(store, kf, lid)
    got = c.kf_remove_observations(kf, lid)
    assert got["removed"].dtype == np.int32 and np.array_equal(got["removed"], removed), what
    assert got["n_removed"] == n, (what, got["n_removed"], n)
    assert c.kf_size() == len(store)
    for i in store:
        _same(_read(c, i), new[i], (what, i))
    return new


@pytest.fixture(scope="module")
def sized():
    rng = np.random.default_rng(1)
    return {10 + k: pr.random_entry(rng, n, 500) for k, n in enumerate(SIZES)}


@pytest.mark.parametrize("pattern", pr.PATTERNS)
def test_entry_sizes_and_removal_patterns(ctx, sized, pattern):
    """every size under one pattern in one call; entry 9 (not named) and the entries the pattern leaves whole stay as they are"""
    store = dict(sized)
    store[9] = pr.random_entry(np.random.default_rng(2), 700, 500)      # the same ids as the others: it must not lose them
    _fill(ctx, store)
    kf, lid = [], []
    for i, (_, _, l) in sized.items():
        pos = pr.pattern_positions(pattern, len(l))
        kf += [i] * len(pos)
        lid += l[pos].tolist()
    if pattern == "nothing":
        kf, lid = list(sized), [499] * len(sized)                       # rows that name every entry and hit nothing
    new = _check(ctx, store, kf, lid, pattern)
    if pattern == "everything":
        assert all(len(new[i][2]) == 0 for i in sized)
        new = _check(ctx, new, [10, 13], [500, 501], "rows for emptied entries")
        d, w, l = pr.random_entry(np.random.default_rng(3), 5, 40)
        ctx.kf_add(10, d, w, lids=l)                                    # an emptied entry is an ordinary entry
        _same(_read(ctx, 10), (d, w, l))


def test_row_list_variants(ctx):
    rng = np.random.default_rng(4)
    n = 3 * T + 17
    d, w, l = pr.random_entry(rng, n, 1)
    top = np.iinfo(np.int64).max
    l[5], l[2 * T + 9] = 77_000, 77_000            # one id at positions in two different chunks
    l[0] = 0
    store = {1: (d, w, l), 2: pr.random_entry(rng, 0, 1), 3: pr.random_entry(rng, 40, 1)}
    _fill(ctx, store)
    # ids an entry cannot be created with: 2^63 - 1 arrives by a replacement, fresh ids by an entry made without ids
    assert ctx.kf_replace_ids([int(l[T])], [top]) == 1
    l[T] = top
    ctx.kf_add(3, store[3][0], store[3][1])
    fresh = ctx.kf_read_ids(3)
    assert len(fresh) == 40 and (fresh >> 62 == 1).all()
    store[3] = (store[3][0], store[3][1], fresh)
    kf = [1, 1, 1, 3, 1, 1, 1, 2, 2, 3, 1, 1]
    lid = [77_000, 0, top, int(fresh[7]), 999_999, 77_000, 0, 5, top, int(lm.fresh_ids(9, 1)[0]), int(l[T + 1]), int(l[T - 1])]
    new, removed, nr = pr.remove_observations(store, kf, lid)
    assert removed.tolist() == [2, 1, 1, 1, 0, 2, 1, 0, 0, 0, 1, 1] and nr == 7 and len(new[3][2]) == 39
    new = _check(ctx, store, kf, lid, "variants")
    # the same rows again: everything is absent now
    got = ctx.kf_remove_observations(kf, lid)
    assert not got["removed"].any() and got["n_removed"] == 0
    # a long list in shuffled order, duplicates included
    store, kf, lid = pr.random_case(11, [900, 3, 0, 2 * T, T + 1, 1500])
    assert not np.array_equal(kf, np.sort(kf))
    _fill(ctx, store)
    _check(ctx, store, kf, lid, "shuffled")


@pytest.mark.parametrize("named", [1, 2, 65])
def test_grid_of_one_two_and_65_entries(ctx, named):
    rng = np.random.default_rng(20 + named)
    sizes = [int(s) for s in rng.integers(0, 700, 70)]
    sizes[:6] = [K, 0, 1, T, T + 1, 3 * T - 1]
    store, kf, lid = pr.random_case(30 + named, sizes, fraction=0.4)
    ids = sorted(store)
    chosen = set(ids[:named])
    sel = np.array([k in chosen for k in kf.tolist()])
    _fill(ctx, store)
    new = _check(ctx, store, kf[sel], lid[sel], named)
    assert sum(new[i] is store[i] for i in ids) == 70 - named          # (and _check compared their bytes)
    assert sum(len(new[i][2]) < len(store[i][2]) for i in ids) == sum(round(0.4 * n) > 0 for n in sizes[:named]) >= named - 8


def test_covisible_union_and_track_on_compacted_entries(pkg, orc):
    """the count and the three arrays of a compacted entry agree: what the store's other calls compute on it is what the
    references compute on the restatement's arrays"""
    seq = lm.make_scene()
    f0, f1 = seq["frames"][0], seq["frames"][1]
    trk = tr.KeyframeTracker(cam=CAM)
    trk.process(f0["desc"], f0["xy"], f0["depth"])
    d0, w0 = trk.store[0]
    n = len(d0)
    assert n > T                                                        # (261: the entry spans two chunks)
    rng = np.random.default_rng(6)
    l0 = np.arange(n, dtype=np.int64)
    m = 2 * T + 40
    other = (rng.integers(0, 256, (m, 32), dtype=np.uint8), rng.normal(size=(m, 3)), n - 30 + np.arange(m, dtype=np.int64) // 2)
    store = {0: (d0, w0, l0), 5: other}                                 # entry 5 holds every id twice and shares 30 with entry 0
    c = pkg.Context(width=0, height=0, max_keypoints=K)
    _fill(c, store)
    kf = [0] * len(range(0, n, 3)) + [5] * 20
    lid = l0[::3].tolist() + list(range(n - 40, n - 20))                # of entry 5's rows ten are absent, ten hit two positions
    new = _check(c, store, kf, lid, "before the consumers")
    assert len(new[0][2]) == n - len(range(0, n, 3)) and len(new[5][2]) < m
    lids = {i: new[i][2] for i in new}
    plain = {i: (new[i][0], new[i][1]) for i in new}
    assert np.array_equal(c.kf_covisible(0, [5, 0]), lm.covisible(lids, 0, [5, 0]))
    assert np.array_equal(c.kf_covisible(5, [0, 5]), lm.covisible(lids, 5, [0, 5]))
    for order in ([0, 5], [5, 0]):
        ref = lm.union(plain, lids, order)
        assert c.kf_union(900, order) == len(ref[2])
        _same(_read(c, 900), ref, order)
    guess = (np.eye(3), np.zeros(3))
    ref = tr.track(f1["desc"], f1["xy"], f1["depth"], plain, 0, [0, 5], seed=1, guess=guess)
    got = c.track(f1["desc"], f1["xy"], f1["depth"], 0, [0, 5], -1, seed=1, rvec=_rvec(guess[0]), tvec=guess[1], with_pairs=True)
    _compare_step(got, ref, "track on the compacted entry")
    assert got["tracked"] and got["n_inliers"] > 50
    c.close()


def test_errors_leave_the_store_and_zero_the_outputs(pkg, ctx):
    rng = np.random.default_rng(8)
    store = {1: pr.random_entry(rng, 300, 10), 2: pr.random_entry(rng, T + 5, 10)}
    _fill(ctx, store)
    L, h = pkg.lib(), ctx._h

    def call(kf, lid, n, with_removed=True, with_n=True):
        kf, lid = np.array(kf, np.int32), np.array(lid, np.int64)
        removed, nr = np.full(max(len(kf), 1), 7, np.int32), C.c_int(7)
        rc = L.mslam_hip_kf_remove_observations(h, kf.ctypes.data_as(C.c_void_p), lid.ctypes.data_as(C.c_void_p), n,
                                                removed.ctypes.data_as(C.c_void_p) if with_removed else None,
                                                C.byref(nr) if with_n else None)
        return rc, removed[:len(kf)], nr.value

    for kf, lid, n in (([1, 9], [10, 10], 2), ([1, 2], [10, -1], 2), ([1], [10], -1)):
        rc, removed, nr = call(kf, lid, n)
        assert rc == pkg.E_INVALID and nr == 0, (kf, lid, n)
        assert n < 0 or not removed.any()
        for i in store:
            _same(_read(ctx, i), store[i], "after an error")
    with pytest.raises(pkg.MslamHipError) as e:
        ctx.kf_remove_observations([1, 9], [10, 10])
    assert e.value.code == pkg.E_INVALID and "9" in str(e.value)
    with pytest.raises(pkg.MslamHipError):
        ctx.kf_remove_observations([1], [10, 11])
    assert L.mslam_hip_kf_remove_observations(h, None, None, 1, None, None) == pkg.E_INVALID
    rc, removed, nr = call([], [], 0)
    assert rc == 0 and nr == 0
    assert L.mslam_hip_kf_remove_observations(h, None, None, 0, None, None) == 0
    got = ctx.kf_remove_observations([], [])
    assert len(got["removed"]) == 0 and got["n_removed"] == 0
    for i in store:
        _same(_read(ctx, i), store[i], "after n = 0")
    # NULL outputs: the removal still happens
    rc, _, nr = call([1, 2], [10, 11], 2, with_removed=False)
    assert rc == 0 and nr == 2
    rc, removed, _ = call([1, 2], [12, 13], 2, with_n=False)
    assert rc == 0 and removed.tolist() == [1, 1]
    new, _, _ = pr.remove_observations(store, [1, 2, 1, 2], [10, 11, 12, 13])
    for i in store:
        _same(_read(ctx, i), new[i], "after the NULL outputs")


# ---- the pruned bundle adjustment ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["bundle_adjust", "bundle_adjust_global"])
@pytest.mark.parametrize("which", range(len(pr.BA_SCENES)))
def test_pruned_ba_on_the_device(pkg, which, entry):
    ref, sch = pr.pruned_reference(which, "qr"), pr.pruned_reference(which, "schur")
    sc = ref["scene"]
    Kf = len(sc["poses"])
    c = pkg.Context(width=0, height=0)
    b = pr.backend_of(pkg, c, sc, global_solver=entry == "bundle_adjust_global")
    res = b.global_ba(prune=True) if entry == "bundle_adjust_global" else b.local_ba(0, _graph(Kf), prune=True)
    c.close()
    assert res["keyframes"] == list(range(Kf)) and res["termination"] != 2
    assert res["pruned"]["pairs"] == sorted(set(zip(sc["obs_kf"][ref["mask"]].tolist(), sc["obs_lm"][ref["mask"]].tolist())))
    check_pruned(res, ref, sc)
    # tests/test_gpu_ba.py's bound against ba_ref: 1000 x the distance of the reference's two linear solvers, at least 1e-9
    dist = float(np.max(np.abs(ref["second"]["poses"] - sch["second"]["poses"])))
    bound = max(1e-9, 1000.0 * dist)
    dx = float(np.max(np.abs(res["poses"] - ref["second"]["poses"])))
    print("pruned BA %d %s: dx %.3e bound %.3e" % (which, entry, dx, bound))
    assert dx <= bound


# ---- the tracker --------------------------------------------------------------------------------------------------------
N_PLANTED, OFFSET = 6, 0.4


def _tracker(pkg, **kw):
    c = pkg.Context(width=0, height=0, max_keypoints=4096)
    return c, pkg.HipKeyframeTracker(c, focal=CAM[:2], principal=CAM[2:], local_map_depth=2, **dict(tr.SEQ_PARAMS, **kw))


def _walk(t, frames):
    return [t.processSensorData(fr["desc"], fr["xy"], fr["depth"]) for fr in frames]


@pytest.fixture(scope="module")
def planted_walk(pkg, orc):
    """lm.make_scene()'s walk; in the frame that makes keyframe 1 the depth at the pixels of N_PLANTED keypoints that become
    inherited landmarks of the keyframe is raised by OFFSET m -> (frames, the frame, the planted keypoints)"""
    seq = lm.make_scene()
    c, t = _tracker(pkg, local_ba=True)
    got = _walk(t, seq["frames"])
    c.close()
    f = next(i for i, o in enumerate(got) if o["keyframe"] == 1)
    step = got[f]["step"]
    fr = dict(seq["frames"][f])
    depth = fr["depth"].copy()
    xy = fr["xy"]
    kps = [int(k) for k in step["entry_kp"][:step["n_inherited"]]
           if 0 < depth[int(xy[k, 1]), int(xy[k, 0])] < 12500][:N_PLANTED]       # below 2.5 m: still below z_max when raised
    assert len(kps) == N_PLANTED
    for k in kps:
        depth[int(xy[k, 1]), int(xy[k, 0])] += np.uint16(round(OFFSET * 5000))
    fr["depth"] = depth
    frames = list(seq["frames"])
    frames[f] = fr
    return frames, f, kps, seq["frames"]


def test_tracker_prunes_the_planted_observations(pkg, planted_walk):
    frames, f, kps, _ = planted_walk
    # the restatement first: the reference's solve of the keyframe's problem flags the planted observations
    c, t = _tracker(pkg, local_ba=True)
    calls, solve = [], c.bundle_adjust
    c.bundle_adjust = lambda *a: calls.append([np.array(x) for x in a[:6]]) or solve(*a)
    got = _walk(t, frames[:f + 1])
    assert got[f]["keyframe"] == 1 and len(calls) == 1
    entry_kp = got[f]["step"]["entry_kp"].tolist()
    ids1 = c.kf_read_ids(1)
    planted = [(1, int(ids1[entry_kp.index(k)])) for k in kps]
    poses, lms, okf, olm, ocam, fixed = calls[0]
    ref = ba_ref.bundle_adjust(poses, lms, okf, olm, ocam, fixed, linear_solver="schur")
    r = ba_ref.residuals(ref["poses"], ref["landmarks"], okf, olm, ocam)
    r2 = np.sum(r * r, 1)
    kf_ids, lm_ids = t.ba_results[0]["keyframes"], t.ba_results[0]["landmark_ids"]
    flagged = {(kf_ids[k], int(lm_ids[l])) for k, l in zip(okf[r2 > 0.15 ** 2], olm[r2 > 0.15 ** 2])}
    print("reference: %d flagged, planted residuals %s" % (len(flagged), np.sqrt([r2[(okf == 1) & (lm_ids[olm] == l)][0] for _, l in planted])))
    assert set(planted) <= flagged
    assert set(planted) <= set(t.ba_results[0]["outlier_observations"])
    unpruned_ids = c.kf_read_ids(1)
    c.close()
    # the pruned tracker
    c, t = _tracker(pkg, local_ba=True, ba_prune=True)
    got = _walk(t, frames)
    assert [o["keyframe"] for o in got][f] == 1 and len(t.ba_results) == len(t.ids) - 1
    ba = t.ba_results[0]
    pairs = ba["pruned"]["pairs"]
    assert set(planted) <= set(pairs) and ba["pruned"]["n_removed"] == len(pairs) > 0
    left = set(c.kf_read_ids(1).tolist())
    assert all(l not in left for k, l in pairs if k == 1)
    assert len(left) == len(unpruned_ids) - sum(k == 1 for k, _ in pairs)
    for k, l in pairs:
        assert l not in set(t.backend.obs[k][0].tolist())
        assert l not in set(c.kf_read_ids(k).tolist())
    assert all(o["tracked"] for o in got[f + 1:]) and len(got) > f + 2
    assert ba["termination"] != 2 and ba["pruned"]["first"]["n_outliers"] >= len(pairs)
    c.close()


def test_tracker_without_ba_prune_is_todays_tracker(pkg, planted_walk):
    frames = planted_walk[0]
    c0, t0 = _tracker(pkg, local_ba=True)
    c1, t1 = _tracker(pkg, local_ba=True, ba_prune=False)
    a, b = _walk(t0, frames), _walk(t1, frames)
    assert t0.ids == t1.ids and t0.graph == t1.graph
    for x, y in zip(a, b):
        assert (x["tracked"], x["keyframe"], x["reference"], x["n_inliers"]) == (y["tracked"], y["keyframe"], y["reference"], y["n_inliers"])
        assert np.array_equal(x["R"], y["R"]) and np.array_equal(x["tvec"], y["tvec"])
    assert [r["termination"] for r in t0.ba_results] == [r["termination"] for r in t1.ba_results]
    assert all("pruned" not in r for r in t1.ba_results)
    for i in t0.ids:
        _same(_read(c1, i), _read(c0, i), i)
    c0.close(), c1.close()
