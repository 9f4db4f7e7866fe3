"""What the calls on the keyframe store share, pinned where no other test pins it: the whole message of every "is not in the
keyframe store" failure and of the list checks next to it (with two-fault lists, so each caller's order of checks is pinned
too), the ordered stage names of one call of every entry that works on the landmark-id table (tools/ and profiles/ key on
them), and the list rewrite behind kf_update_world / kf_replace_ids on lists of 0, 1 and 257 ids over live slots that are not
contiguous, exactly against tests/fuse_ref.py and the update_world restatement of tests/test_gpu_ba.py."""
import numpy as np
import pytest

import fuse_ref as fr
from test_gpu_ba import _update_ref
from test_gpu_fuse import _same_store

pytestmark = pytest.mark.gpu
K = 320
MISSING = 7
GONE = " is not in the keyframe store"
OUTSIDE = ": a landmark id lies outside [0, 2^63)"


def _store():
    """entries 3, 4 and 9 of 257, 256 and 1 landmarks (either side of a 256-thread block): 3 and 4 share ids 250..256, and
    9's one id, 255, is in both"""
    rng = np.random.default_rng(12)
    lids = {3: np.arange(0, 257), 4: np.arange(250, 506), 9: np.array([255])}
    return {k: fr.entry(rng.integers(0, 256, (len(l), 32), dtype=np.uint8), rng.normal(size=(len(l), 3)), l) for k, l in lids.items()}


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(width=0, height=0, max_keypoints=K)
    yield c
    c.close()


def _fill(c, store):
    c.kf_clear()
    for i, (d, w, l) in store.items():
        c.kf_add(i, d, w, l)


POSE = dict(R=np.eye(3), t=np.zeros(3), radius=4.0, width=640, height=480)


# ---- error strings -------------------------------------------------------------------------------------------------------------

def test_lookup_and_list_check_messages(pkg, ctx):
    store = _store()
    _fill(ctx, store)
    c, m = ctx, MISSING
    none, depth = np.zeros((0, 32), np.uint8), np.zeros((4, 4), np.uint16)
    xy = np.zeros((0, 2), np.float32)

    def bad(msg, fn, *a, **kw):
        with pytest.raises(pkg.MslamHipError) as e:
            fn(*a, **kw)
        assert e.value.code == pkg.E_INVALID and str(e.value) == "mslam_hip error %d: %s" % (pkg.E_INVALID, msg), (msg, str(e.value))

    # the ten lookup sites, one missing id each
    bad("kf_union: id 7" + GONE, c.kf_union, 900, [3, m])
    bad("kf_union_dev: id 7" + GONE, c.kf_union, 900, [3, m], sync=False)
    bad("kf_covisible: id 7" + GONE, c.kf_covisible, m, [3])
    bad("kf_covisible: id 7" + GONE, c.kf_covisible, 3, [4, m])
    bad("kf_observers: id 7" + GONE, c.kf_observers, [3, m], [1])
    bad("kf_cull_search: id 7" + GONE, c.kf_cull_search, [3, m], [3])
    bad("kf_cull: id 7" + GONE, c.kf_cull, [3, m], [3])
    bad("kf_fuse_search: id 7" + GONE, c.kf_fuse_search, m, 3, **POSE)
    bad("kf_fuse_search: id 7" + GONE, c.kf_fuse_search, 3, m, **POSE)
    bad("kf_fuse: id 7" + GONE, c.kf_fuse, 3, m, **POSE)
    bad("kf_remove_observations: id 7" + GONE, c.kf_remove_observations, [3, m], [1, 1])
    bad("kf_visible: id 7" + GONE, c.kf_visible, [3, m], np.eye(3), np.zeros(3))
    bad("track: reference id 7" + GONE, c.track, none, xy, depth, m)
    bad("track: vote id 7" + GONE, c.track, none, xy, depth, 3, vote_ids=[4, m])
    bad("relocalize: candidate id 7" + GONE, c.relocalize, none, xy, [3, m])
    # each caller's policy for repeats and dst_id
    bad("kf_union: id 3 is listed twice", c.kf_union, 900, [3, 4, 3])
    bad("kf_union: dst_id is one of the listed ids", c.kf_union, 3, [4, 3])
    bad("kf_cull_search: id 3 is listed twice", c.kf_cull_search, [3, 3], [3])
    bad("kf_cull_search: candidate 3 is listed twice", c.kf_cull_search, [3, 4], [3, 3])
    bad("kf_observers: id 3 is listed twice", c.kf_observers, [3, 3], [1])
    # the list checks
    bad("kf_observers" + OUTSIDE, c.kf_observers, [3], [1, -1])
    bad("kf_remove_observations" + OUTSIDE, c.kf_remove_observations, [3, 3], [1, -1])
    bad("kf_replace_ids" + OUTSIDE, c.kf_replace_ids, [1, -1], [5, 5])
    bad("kf_replace_ids" + OUTSIDE, c.kf_replace_ids, [1, 2], [5, -(2 ** 63)])
    # two faults in one call: the order of each caller's checks
    bad("kf_union: id 3 is listed twice", c.kf_union, 900, [3, m, 3])                     # union: a position's repeats before the next lookup
    bad("kf_union: dst_id is one of the listed ids", c.kf_union, 3, [3, m])
    bad("kf_union: id 7" + GONE, c.kf_union, 3, [m, 3])
    bad("kf_cull_search: id 7" + GONE, c.kf_cull_search, [3, m, 3], [3])                  # cull: every lookup before a later repeat
    bad("kf_cull_search: id 7" + GONE, c.kf_cull_search, [3, m], [3], min_observers=0)    # ... and before the thresholds
    bad("kf_cull_search: candidate 9 is not one of the listed ids", c.kf_cull_search, [3, 4], [9, 9])
    bad("kf_observers: id 7" + GONE, c.kf_observers, [3, m], [-1])                        # the entries before the asked ids
    bad("kf_covisible: id 7" + GONE, c.kf_covisible, m, [8])                              # the own id first
    bad("kf_fuse_search: keep_id and drop_id name one entry", c.kf_fuse_search, m, m, **POSE)
    bad("kf_fuse_search: id 7" + GONE, c.kf_fuse_search, m, 8, **POSE)                    # the keep id is named
    bad("kf_fuse_search: id 7" + GONE, c.kf_fuse_search, m, 3, **dict(POSE, radius=0.0))  # the lookup before the radius
    bad("kf_remove_observations: id 7" + GONE, c.kf_remove_observations, [m, 3], [1, -1])  # prune: row by row, id then entry
    bad("kf_remove_observations" + OUTSIDE, c.kf_remove_observations, [3, m], [-1, 1])
    bad("kf_remove_observations" + OUTSIDE, c.kf_remove_observations, [m], [-1])
    bad("track: reference id 7" + GONE, c.track, none, xy, depth, m, vote_ids=[8])
    bad("track: vote id 7" + GONE, c.track, none, xy, depth, 3, vote_ids=[4, m], new_id=4)  # the lookups before new_id's collision
    # kf_remove / kf_read keep their own words
    bad("kf_remove: no such keyframe id", c.kf_remove, m)
    bad("kf_read: no such keyframe id", c.kf_read, m)
    _same_store(ctx, store, "after the errors")


# ---- stage sequences -----------------------------------------------------------------------------------------------------------

def _stages(c, fn, *a, **kw):
    c.set_profiling(1)                                                 # (starts a new list)
    try:
        fn(*a, **kw)
        return [name for name, _ in c.stage_times()]
    finally:
        c.set_profiling(0)


FUSE_SEARCH = ["fuse_clear", "fuse_ids", "fuse_project", "fuse_bin", "fuse_search", "fuse_resolve"]


def test_stage_names_of_one_call_of_each_entry(ctx):
    _fill(ctx, _store())
    c, all3 = ctx, [3, 4, 9]
    union = ["union_clear", "union_insert", "union_select", "union_scan", "union_scatter"]
    assert _stages(c, c.kf_union, 900, [3, 9]) == union                # (257 distinct ids: the three together exceed K)
    assert _stages(c, c.kf_union, 900, [3, 9], sync=False) == union
    c.sync()
    c.kf_remove(900)
    assert _stages(c, c.kf_covisible, 3, all3) == ["covisible_clear", "covisible_insert", "covisible_count"]
    assert _stages(c, c.kf_update_world, [255, 300], np.zeros((2, 3))) == ["update_world_insert", "update_world_write"]
    assert _stages(c, c.kf_replace_ids, [255], [255]) == ["fuse_table", "fuse_replace"]
    assert _stages(c, c.kf_replace_ids, [255], [255], np.zeros((1, 3))) == ["fuse_table", "fuse_replace"]
    assert _stages(c, c.kf_fuse_search, 3, 4, **POSE) == FUSE_SEARCH
    assert _stages(c, c.kf_fuse, 3, 4, **POSE) == FUSE_SEARCH + ["fuse_table", "fuse_replace"]
    assert _stages(c, c.kf_observers, all3, [255, 1000]) == ["cull_upload", "cull_clear", "cull_count", "cull_lookup"]
    assert _stages(c, c.kf_cull_search, all3, [3, 9]) == ["cull_upload", "cull_clear", "cull_count", "cull_greedy"]
    assert _stages(c, c.kf_remove_observations, [3, 4], [255, 255]) == ["prune_upload", "prune_compact"]
    # calls that have nothing to do enqueue nothing
    assert _stages(c, c.kf_update_world, [], np.zeros((0, 3))) == []
    assert _stages(c, c.kf_replace_ids, [], []) == []
    assert _stages(c, c.kf_observers, all3, []) == []
    assert _stages(c, c.kf_cull_search, all3, []) == []
    assert _stages(c, c.kf_remove_observations, [], []) == []


# ---- the list rewrite ----------------------------------------------------------------------------------------------------------

def _list(n):
    """n ids from 200 up: 57 of entry 3, one of them entry 9's, the rest strangers once entry 4 is gone; the last names the
    id at place 10 again (the later place wins)"""
    ids = np.arange(200, 200 + n, dtype=np.int64)
    if n > 10:
        ids[-1] = ids[10]
    return ids


@pytest.mark.parametrize("n", [0, 1, 257])
def test_list_rewrite_over_live_slots_with_a_gap(ctx, n):
    rng = np.random.default_rng(n)
    ids, to, xyz = _list(n), 100000 + np.arange(n, dtype=np.int64), rng.normal(size=(n, 3))
    if n == 1:
        ids[0] = 255                                                   # held by entries 3 and 9
    hits = {0: 0, 1: 2, 257: 57 + 1}[n]

    def fresh():
        store = _store()
        _fill(ctx, store)
        ctx.kf_remove(4)                                               # the live slots are 0 and 2
        del store[4]
        return store

    store = fresh()
    ref, count = _update_ref({k: (e[2], e[1]) for k, e in store.items()}, ids, xyz)
    assert ctx.kf_update_world(ids, xyz) == count == hits
    _same_store(ctx, {k: (store[k][0], ref[k][1], store[k][2]) for k in store}, "update_world")      # every id is as it was
    if n > 10:
        at = int(np.flatnonzero(store[3][2] == ids[10])[0])
        assert ref[3][1][at].tobytes() == xyz[n - 1].tobytes() != xyz[10].tobytes()

    store = fresh()
    ref, count = fr.replace_ids(store, ids, to)
    assert ctx.kf_replace_ids(ids, to) == count == hits
    _same_store(ctx, ref, "replace_ids, ids alone")
    assert all(ref[k][1].tobytes() == store[k][1].tobytes() for k in store)                          # every point is as it was

    store = fresh()
    ref, count = fr.replace_ids(store, ids, to, xyz)
    assert ctx.kf_replace_ids(ids, to, xyz) == count == hits
    _same_store(ctx, ref, "replace_ids with points")
    if n > 10:
        assert ref[3][2][at] == to[n - 1]
