"""Local-map tracking without a GPU: the new C ABI symbols, and the numpy restatement of tests/local_map_ref.py on hand
cases — the neighbourhood walk, the union's most-recent-wins rule and order, covisibility — and on sequences: with no
local map it is track_ref's loop row for row, with one it gets more correspondences out of a frame that sees landmarks of
two keyframes and inserts no more keyframes."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import local_map_ref as lm
import track_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mslam_hip_kf_add_ids", "mslam_hip_kf_read_ids", "mslam_hip_kf_covisible", "mslam_hip_kf_union", "mslam_hip_kf_union_dev"]


def test_library_exports_the_local_map_calls_and_keeps_its_abi_version(pkg):
    assert set(NEW) <= set(pkg.ABI_SYMBOLS)
    text = open(os.path.join(ROOT, "include", "mslam_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, text), name
    assert re.search(r"#define MSLAM_HIP_ABI_VERSION 5\b", text)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH]).decode()
    for name in NEW:
        assert re.search(r"\bT %s\b" % name, exported), name
    try:
        L = ctypes.CDLL(pkg.LIB_PATH)
    except OSError:                           # no HIP runtime to resolve against on this host: the symbol table has told
        return
    assert L.mslam_hip_abi_version() == 5
    for name in ("kf_read_ids", "kf_covisible", "kf_union"):
        assert callable(getattr(pkg.Context, name))
    assert pkg.HipKeyframeTracker.LOCAL_MAP_ID == lm.LOCAL_MAP_ID == 0x7fffffff


def test_fresh_ids_follow_the_rule():
    ids = lm.fresh_ids(3, 4)
    assert ids.dtype == np.int64 and ids.tolist() == [(1 << 62) | (3 << 16) | p for p in range(4)]
    assert lm.fresh_ids(3, 2, first=7).tolist() == [(1 << 62) | (3 << 16) | 7, (1 << 62) | (3 << 16) | 8]
    assert len(lm.fresh_ids(1, 0)) == 0
    both = np.concatenate([lm.fresh_ids(1, 65535), lm.fresh_ids(2, 65535)])          # full entries of two serials never meet
    assert len(np.unique(both)) == len(both) and both.min() >= 1 << 62


def test_neighbours_on_hand_graphs():
    chain = {0: {1}, 1: {0, 2}, 2: {1, 3}, 3: {2, 4}, 4: {3}}
    assert lm.neighbours(chain, 0, 2) == {0, 1, 2, 3}          # level <= depth expands level 2 too: depth + 1 hops
    assert lm.neighbours(chain, 0, 0) == {0, 1}
    assert lm.neighbours(chain, 0, 1) == {0, 1, 2}
    assert lm.neighbours(chain, 2, 2) == {0, 1, 2, 3, 4}
    assert lm.neighbours(chain, 4, 3) == {0, 1, 2, 3, 4}
    cycle = {i: {(i - 1) % 8, (i + 1) % 8} for i in range(8)}
    assert lm.neighbours(cycle, 0, 2) == {5, 6, 7, 0, 1, 2, 3}
    assert lm.neighbours(cycle, 0, 3) == set(range(8))
    assert lm.neighbours({0: set(), 1: {2}, 2: {1}}, 0, 2) == {0}        # an isolated node
    assert lm.neighbours({}, 7, 2) == {7}                                # a node the graph has never heard of


def _entry(rng, lids):
    n = len(lids)
    return (rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.normal(size=(n, 3))), np.array(lids, np.int64)


def test_union_hand_cases():
    rng = np.random.default_rng(0)
    store, lids = {}, {}
    store[3], lids[3] = _entry(rng, [10, 11, 12])
    store[5], lids[5] = _entry(rng, [12, 13, 10])
    store[4], lids[4] = _entry(rng, [11, 14])
    # most recent wins: 10 and 12 from keyframe 5, 11 from keyframe 4 (it beats 3), 13 and 14 where they are
    d, w, l = lm.union(store, lids, [3, 5, 4])
    assert l.tolist() == [12, 13, 10, 11, 14]                    # by position of the winning entry in the list, then inside it
    assert np.array_equal(d, np.concatenate([store[5][0], store[4][0]])) and np.array_equal(w, np.concatenate([store[5][1], store[4][1]]))
    d, w, l = lm.union(store, lids, [4, 3, 5])
    assert l.tolist() == [11, 14, 12, 13, 10]
    d, w, l = lm.union(store, lids, [3, 4])
    assert l.tolist() == [10, 12, 11, 14]
    assert np.array_equal(w, np.stack([store[3][1][0], store[3][1][2], store[4][1][0], store[4][1][1]]))
    # a single entry is itself; entries without landmarks add nothing
    d, w, l = lm.union(store, lids, [3])
    assert l.tolist() == [10, 11, 12] and np.array_equal(d, store[3][0])
    store[9], lids[9] = _entry(rng, [])
    assert lm.union(store, lids, [9, 3])[2].tolist() == [10, 11, 12] and len(lm.union(store, lids, [9])[2]) == 0
    # a repeat inside one entry: the higher position wins, and is placed where it stands
    store[6], lids[6] = _entry(rng, [20, 21, 20])
    d, w, l = lm.union(store, lids, [6])
    assert l.tolist() == [21, 20] and np.array_equal(d, store[6][0][1:])
    # covisibility counts distinct shared ids, self included
    assert lm.covisible(lids, 3, [3, 5, 4, 9, 6]).tolist() == [3, 2, 1, 0, 0]
    assert lm.covisible(lids, 6, [6, 3]).tolist() == [2, 0]


@pytest.fixture(scope="module")
def scene(orc):
    seq = lm.make_scene()
    return seq, lm.run(seq, None), lm.run(seq, 2)


def test_no_local_map_is_the_single_reference_loop(orc):
    seq = tr.make_sequence(seed=0)
    rows, trk = tr.run_reference(seq)
    got, g = lm.run(seq, None)
    assert len(got) == len(rows) and g.ids == trk.ids
    for f, (a, b) in enumerate(zip(got, rows)):
        assert (a["tracked"], a["n_inliers"], a["keyframe"], a["relocalized"], a["reference"]) == \
               (b["tracked"], b["n_inliers"], b["keyframe"], b["relocalized"], b["reference"]), f
        assert np.array_equal(a["R"], b["R"]) and np.array_equal(a["t"], b["t"]), f
    for i in trk.ids:
        assert np.array_equal(g.store[i][0], trk.store[i][0]) and np.array_equal(g.store[i][1], trk.store[i][1])
        assert len(g.lids[i]) == len(g.store[i][0]) == len(np.unique(g.lids[i]))


def test_local_map_sees_more_than_the_reference_keyframe_alone(scene):
    seq, (single, ts), (local, tl) = scene
    assert all(r["tracked"] for r in single) and all(r["tracked"] for r in local)
    k1 = next(f for f, r in enumerate(single) if r["keyframe"] == 1)
    assert local[k1]["keyframe"] == 1 and [r["n_correspondences"] for r in local[:k1 + 1]] == [r["n_correspondences"] for r in single[:k1 + 1]]
    # keyframe 1 inherits only part of keyframe 0's landmarks
    inherited = set(tl.lids[1].tolist()) & set(tl.lids[0].tolist())
    assert 0 < len(inherited) < len(tl.lids[0]) and lm.covisible(tl.lids, 1, [0, 1]).tolist() == [len(inherited), len(tl.lids[1])]
    # the frame after it sees landmarks of both: the local map gives strictly more correspondences
    f = k1 + 1
    assert single[f]["reference"] == local[f]["reference"] == 1 and single[f]["keyframe"] < 0
    print("frame", f, "single", single[f]["n_correspondences"], "local map", local[f]["n_correspondences"])
    assert local[f]["n_correspondences"] > single[f]["n_correspondences"]
    assert all(b["n_correspondences"] >= a["n_correspondences"] for a, b in zip(single, local))
    # and over the sequence no more keyframes
    assert len(tl.ids) <= len(ts.ids) and len(tl.ids) >= 3
    # the graph is symmetric, without self-loops, and what covisibility says
    for a, nb in tl.graph.items():
        assert a not in nb and all(a in tl.graph[b] for b in nb)
        for b in tl.ids:
            if b != a:
                assert (b in nb) == (len(set(tl.lids[a].tolist()) & set(tl.lids[b].tolist())) > 0), (a, b)
    assert 0 in tl.graph[1]
