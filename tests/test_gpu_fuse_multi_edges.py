"""Landmark fusion into many target entries on the MI355X at the edges of k_fuse_multi.hip: the single-target library of
tests/fuse_ref.py (hand cases, entry sizes, frame extents and radii, a real pose) lifted onto one target of many, one drop
entry dealt out to several targets with both cross-target conflicts in every pass of the compaction, 64 targets with more
than 4096 keep landmarks, large slices followed by tiny ones, crowded windows, claim keys decided at a margin of one, long
probe chains in both claim tables, union entries whose capacity exceeds their count, results that fill the pair arrays,
scratch reuse and NULL pair arrays — pairs compared as bytes per key, n_rewritten as an integer, stores read back and
compared as bytes, against tests/fuse_multi_ref.py.  tests/test_fuse_multi_edges.py proves on the CPU that every case of
tests/fuse_multi_edge_cases.py reaches the path it is named for."""
import ctypes as C

import numpy as np
import pytest

import fuse_multi_edge_cases as ec
import fuse_multi_ref as fm
import fuse_ref as fr
import test_gpu_fuse as single
from test_gpu_fuse_multi import KEEP, SEARCH_STAGES, _args, _fill, _same_pairs, _same_store, _stages, _store

pytestmark = pytest.mark.gpu

K_SMALL, K_BIG = 1280, 4608


@pytest.fixture(scope="module")
def small(pkg):
    c = pkg.Context(width=0, height=0, max_keypoints=K_SMALL)
    yield c
    c.close()


@pytest.fixture(scope="module")
def big(pkg):
    c = pkg.Context(width=0, height=0, max_keypoints=K_BIG)
    yield c
    c.close()


def _largest(case):
    return max([len(case["keep"][0])] + [len(d[0]) for d in case["drops"]])


def _load(c, store):
    """_fill; the id 2^63 - 1, which no add takes, is added under a placeholder and put in place by a replacement"""
    held = {k: fr.entry(*e) for k, e in store.items()}
    n_top = sum(int((e[2] == ec.TOP).sum()) for e in held.values())
    _fill(c, {k: (e[0], e[1], np.where(e[2] == ec.TOP, ec.PLACEHOLDER, e[2])) for k, e in held.items()} if n_top else store)
    if n_top:
        assert c.kf_replace_ids([ec.PLACEHOLDER], [ec.TOP]) == n_top


def _others(case, seed=0):
    """two further entries that hold drop ids (some twice), keep ids and strangers"""
    rng = np.random.default_rng(seed)
    dl, kl = np.concatenate([d[2] for d in case["drops"]]), case["keep"][2]

    def other(ids):
        return (rng.integers(0, 256, (len(ids), 32), dtype=np.uint8), rng.normal(size=(len(ids), 3)), ids)

    return {30: other(np.concatenate([dl[::3], kl[:40], dl[:130], 9000000 + np.arange(30)])[:K_SMALL]), 40: other(dl[1::2][:K_SMALL])}


def _check(c, case, what, fuse=True, others=None, expect=None):
    """the search, then (fuse) the fused call, against the restatement -> (pairs, stages)"""
    store, drops = _store(case, others)
    _load(c, store)
    st = {}
    ref = ec.reference(case, st)
    sizes = [len(d[0]) for d in case["drops"]]
    print("%s: %d targets of %s%s, keep %d: %d rows, A drops %d, B drops %d -> %d pairs" % (
        what, len(sizes), sizes[:6], " ..." if len(sizes) > 6 else "", len(case["keep"][0]), len(st["rows"]), len(st["dropped_a"]),
        len(st["dropped_b"]), len(ref["dist"])))
    got = c.kf_fuse_search_multi(KEEP, drops, **_args(case))
    if expect is not None:
        assert fm.rows_of(got) == expect, what
    _same_pairs(got, ref, what)
    if fuse:
        _same_store(c, store, "the search changes nothing")
        pairs, new, n = fm.fuse_multi(store, KEEP, drops, case["Rs"], case["ts"], case["radius"], **case["kw"])
        fused = c.kf_fuse_multi(KEEP, drops, **_args(case))
        _same_pairs(fused, ref, (what, "fuse"))
        assert fused["n_rewritten"] == n, what
        _same_store(c, new, (what, "fuse"))
    return ref, st


# ---- 1. the single-target library, lifted ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", fr.HAND_CASES)
def test_lifted_hand_cases(small, name):
    one = fr.hand_case(name)
    for m, n_drop in ec.LIFTS:
        expect = None if name == "repeated_id" else [(m, j, i, d) for j, i, d in one["expect"]]
        _check(small, ec.lifted(one, m, n_drop), "%s as target %d of %d" % (name, m, n_drop), fuse=m == 1, expect=expect)


@pytest.mark.parametrize("nk,nd", fr.SIZES)
def test_lifted_sizes(small, big, nk, nd):
    case = ec.lifted(fr.sized_case(nk, nd), 2, 4)
    ref, _ = _check(small if max(nk, nd) <= K_SMALL else big, case, "sizes %d / %d as target 2 of 4" % (nk, nd))
    assert min(nk, nd) == 0 or len(ref["dist"]) > 0


@pytest.mark.parametrize("width,height", ec.FRAMES)
def test_lifted_frames_and_radii(small, width, height):
    for nk, nd in fr.FRAME_SIZES:
        case = ec.lifted(fr.frame_case(nk, nd, width, height), 1, 3)
        radii = fr.frame_radii(width, height)
        total = 0
        for radius in radii:
            at = dict(case, radius=radius)
            ref, _ = _check(small, at, "%d x %d, %d / %d, radius %g" % (width, height, nk, nd, radius), fuse=radius == radii[-1])
            total += len(ref["dist"])
        assert total > 0


@pytest.mark.parametrize("nk,nd", fr.POSED_SIZES)
def test_lifted_real_pose(small, nk, nd):
    case = ec.lifted(fr.posed_case(40 + nk, nk, nd, shared=5), 1, 3)
    open_ = dict(case, kw=dict(case["kw"], max_world_distance=np.inf))
    a, _ = _check(small, open_, "posed %d / %d, no gate" % (nk, nd), fuse=False)
    b, _ = _check(small, case, "posed %d / %d" % (nk, nd), others=_others(case))
    assert len(b["dist"]) >= 30 and len(a["dist"]) != len(b["dist"])


# ---- 2. one drop entry dealt out to several targets -----------------------------------------------------------------------

@pytest.mark.parametrize("kind,nk,nd,M", ec.DEALT)
def test_dealt_cases(small, big, kind, nk, nd, M):
    case = ec.dealt(ec.dealt_source(kind, nk, nd), M)
    ref, st = _check(small if nk <= K_SMALL else big, case, "%s %d / %d dealt to %d" % (kind, nk, nd, M), others=_others(case, nk))
    assert len(st["dropped_a"]) >= 3 and len(st["dropped_b"]) >= 3


# ---- 3. shapes only the multi kernels have --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wide():
    case = ec.wide_64()
    store, drops = _store(case)
    st = {}
    ec.reference(case, st)
    pairs, new, n = fm.fuse_multi(store, KEEP, drops, case["Rs"], case["ts"], case["radius"], **case["kw"])
    return dict(case=case, store=store, drops=drops, pairs=pairs, new=new, n=n, st=st)


def _run_wide(c, w):
    _fill(c, w["store"])
    got = c.kf_fuse_search_multi(KEEP, w["drops"], **_args(w["case"]))
    _same_pairs(got, w["pairs"], "wide_64, search")
    fused = c.kf_fuse_multi(KEEP, w["drops"], **_args(w["case"]))
    _same_pairs(fused, w["pairs"], "wide_64, fuse")
    assert fused["n_rewritten"] == w["n"]
    return [got[k].tobytes() for k in fm.KEYS] + [fused[k].tobytes() for k in fm.KEYS]


def test_wide_64(big, wide):
    """64 targets x 4127 keep landmarks: the 256-thread search, a partial last workgroup and count block, and the second
    trip of the compaction's prefix loop; the launches are the nine of any other call"""
    p, st = wide["pairs"], wide["st"]
    print("wide_64: 64 targets, keep %d: %d rows, A drops %d, B drops %d -> %d pairs, %d in targets 61 .. 63, %d at keep positions >= 4096" % (
        ec.WIDE_NK, len(st["rows"]), len(st["dropped_a"]), len(st["dropped_b"]), len(p["dist"]), (p["target"] >= 61).sum(),
        (p["keep_pos"] >= 4096).sum()))
    _fill(big, wide["store"])
    assert _stages(big, big.kf_fuse_search_multi, KEEP, wide["drops"], **_args(wide["case"])) == SEARCH_STAGES
    _same_store(big, wide["store"], "the search changes nothing")
    _run_wide(big, wide)
    _same_store(big, wide["new"], "wide_64, fuse")


@pytest.mark.parametrize("nk", [4096, 4097])
def test_search_form_boundaries(big, nk):
    _check(big, fm.random_case(3, nk), "3 targets, keep %d" % nk)


def test_big_targets(big):
    ref, _ = _check(big, ec.big_targets(), "big_targets")
    assert (ref["target"] == 4).sum() == 1 and (ref["drop_pos"][ref["target"] == 2] >= 2048).any()


def test_crowded(big):
    case = ec.crowded()
    a, _ = _check(big, case, "crowded, ratio 0.7")
    b, _ = _check(big, dict(case, kw=dict(case["kw"], ratio=1.01)), "crowded, ratio 1.01")
    c, _ = _check(big, dict(case, kw=dict(case["kw"], ratio=0.5)), "crowded, ratio 0.5, d1 = 8", fuse=False)
    nine = ec.crowded(d1=9)
    d, _ = _check(big, dict(nine, kw=dict(nine["kw"], ratio=0.5)), "crowded, ratio 0.5, d1 = 9", fuse=False)
    assert [a["keep_pos"].tolist(), b["keep_pos"].tolist(), c["keep_pos"].tolist(), d["keep_pos"].tolist()] == [[0, 2], [0, 1, 2], [0], [2, 0]]
    assert c["target"].tolist() == [2] and d["dist"].tolist() == [4, 5]


@pytest.mark.parametrize("name", ec.KEY_EXTREMES)
def test_key_extremes(small, name):
    case = ec.key_extremes(name)
    _check(small, case, "key_extremes " + name, expect=case["expect"])


@pytest.mark.parametrize("which", ["boundary", "dealt"])
def test_chained_ids(small, big, which):
    base = fm.random_case(3, 4097) if which == "boundary" else ec.dealt(ec.dealt_source(*ec.DEALT[1][:3]), ec.DEALT[1][3])
    case = ec.relabelled(base, 300 + len(which))
    ref, _ = _check(big if which == "boundary" else small, case, "chained ids, " + which, others=_others(case, 9))
    assert len(ref["dist"]) > 50


@pytest.mark.parametrize("big_union", [False, True])
def test_union_sides(small, big_union):
    """keep and target 0 are unions enqueued just before: the host knows their capacity (the sum of their sources, at most
    max_keypoints), not their count, and nothing reads them before the fuse.  Both union ids held full entries before, so
    their slots hold landmarks that would pair from the count up to the capacity"""
    u = ec.union_sides(big_union)
    store, case = ec.union_reference(u)
    st = {}
    ref = ec.reference(case, st)
    _fill(small, {**u["store"], **ec.union_stale(u, case, K_SMALL)[0]})
    small.kf_union(ec.UNION_KEEP, u["keep_sources"], sync=False)
    small.kf_union(ec.UNION_TARGET, u["target_sources"], sync=False)
    print("union sides: keep %d of capacity %d, targets %s: %d rows, A drops %d, B drops %d -> %d pairs" % (
        len(case["keep"][0]), min(sum(len(u["store"][s][2]) for s in u["keep_sources"]), K_SMALL), [len(d[0]) for d in case["drops"]],
        len(st["rows"]), len(st["dropped_a"]), len(st["dropped_b"]), len(ref["dist"])))
    _same_pairs(small.kf_fuse_search_multi(ec.UNION_KEEP, u["drop_ids"], **_args(case)), ref, "search")
    pairs, new, n = fm.fuse_multi(store, ec.UNION_KEEP, u["drop_ids"], case["Rs"], case["ts"], case["radius"], **case["kw"])
    fused = small.kf_fuse_multi(ec.UNION_KEEP, u["drop_ids"], **_args(case))
    _same_pairs(fused, ref, "fuse")
    assert fused["n_rewritten"] == n
    _same_store(small, new, "fuse")


@pytest.mark.parametrize("nk,sizes", ec.TIGHT)
def test_tight(pkg, small, nk, sizes):
    case = ec.tight(nk, sizes)
    store, drops = _store(case)
    st = {}
    ref = ec.reference(case, st)
    P = min(nk, sum(sizes))
    print("tight: keep %d, targets %s: %d rows, A drops %d, B drops %d -> %d pairs" % (
        nk, sizes, len(st["rows"]), len(st["dropped_a"]), len(st["dropped_b"]), len(ref["dist"])))
    assert len(ref["dist"]) == P
    _fill(small, store)
    for fn in (small.kf_fuse_search_multi, small.kf_fuse_multi):
        with pytest.raises(pkg.MslamHipError) as e:
            fn(KEEP, drops, capacity=P - 1, **_args(case))
        assert e.value.code == pkg.E_CAPACITY and e.value.needed == P
        _same_store(small, store, fn.__name__)
    _same_pairs(small.kf_fuse_search_multi(KEEP, drops, capacity=P, **_args(case)), ref, "capacity exactly")
    pairs, new, n = fm.fuse_multi(store, KEEP, drops, case["Rs"], case["ts"], case["radius"], **case["kw"])
    fused = small.kf_fuse_multi(KEEP, drops, capacity=P, **_args(case))
    _same_pairs(fused, ref, "fuse")
    assert fused["n_rewritten"] == n == P
    _same_store(small, new, "fuse")


def test_scratch_reuse(pkg, big, wide):
    """a large call, a tiny one, a single-target search (it shares the table and the arena), an error, the large call again"""
    first = _run_wide(big, wide)
    rng = np.random.default_rng(2)
    d = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    tiny = dict(keep=fr.entry(d, [(100, 100, 1)], [1]), drops=[fr.entry(d, [(100, 100, 1)], [11])], Rs=np.eye(3)[None], ts=np.zeros((1, 3)),
                radius=4.0, kw=dict(cam=fm.gm.IDENTITY_CAM, width=640, height=480, max_distance=50, ratio=0.7, max_world_distance=np.inf))
    _check(big, tiny, "one target, one landmark", expect=[(0, 0, 0, 0)])
    one = fr.sized_case(257, 255)
    _fill(big, {1: one["keep"], 2: one["drop"]})
    single._same_pairs(big.kf_fuse_search(1, 2, **single._args(one)), fr.search(one["keep"], one["drop"], radius=one["radius"], **one["kw"]), "single")
    with pytest.raises(pkg.MslamHipError) as e:
        big.kf_fuse_search_multi(1, [], R=np.zeros((0, 3, 3)), t=np.zeros((0, 3)), radius=4.0, width=640, height=480)
    assert e.value.code == pkg.E_INVALID
    assert _run_wide(big, wide) == first and len(first[0]) > 0
    _same_store(big, wide["new"], "wide_64 again")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_null_pair_arrays(pkg, small):
    """mslam_hip_kf_fuse_multi with the six pair arrays NULL: the counts and the store as the restatement gives them"""
    case = fm.random_case(3, 1024)
    store, drops = _store(case, _others(case, 3))
    _fill(small, store)
    pairs, new, n = fm.fuse_multi(store, KEEP, drops, case["Rs"], case["ts"], case["radius"], **case["kw"])
    a = _args(case)
    ids = np.array(drops, np.int32)
    R, t = np.ascontiguousarray(a["R"], np.float64).reshape(-1), np.ascontiguousarray(a["t"], np.float64).reshape(-1)
    n_pairs, n_rewritten = C.c_int(-7), C.c_int(-7)
    rc = pkg.lib().mslam_hip_kf_fuse_multi(small._h, KEEP, _p(ids), len(ids), _p(R), _p(t), C.c_double(a["focal"][0]), C.c_double(a["focal"][1]),
                                           C.c_double(a["principal"][0]), C.c_double(a["principal"][1]), int(a["width"]), int(a["height"]),
                                           C.c_double(a["radius"]), int(a["max_distance"]), C.c_double(a["ratio"]),
                                           C.c_double(a["max_world_distance"]), None, None, None, None, None, None, K_SMALL,
                                           C.byref(n_pairs), C.byref(n_rewritten))
    print("NULL pair arrays: %d pairs, %d rewritten" % (n_pairs.value, n_rewritten.value))
    assert rc == 0 and n_pairs.value == len(pairs["dist"]) > 50 and n_rewritten.value == n
    _same_store(small, new, "fuse")
