"""Landmark fusion without a GPU: the three entry points are exported, declared and listed; tests/fuse_ref.py's restatement
proves every rule of include/mslam_hip.h's statement on planted scenes (the GPU tests then hold the library to the
restatement); HipBackend.fuse against its restatement; the constructor's guard; and the CPU tracker on the ring walk closes
the same single loop with and without fusion, fuses landmarks, gains the edge across the loop, and afterwards inserts
keyframes that inherit ids of the old side and fires no second loop."""
import os
import re

import numpy as np
import pytest

import fuse_ref as fr
import guided_match_ref as gm
import local_map_ref as lm
import loop_walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mslam_hip_kf_fuse_search", "mslam_hip_kf_replace_ids", "mslam_hip_kf_fuse"]


@pytest.fixture(autouse=True)
def _entry_points(pkg):
    """every test here states or uses what the three entry points compute: none of it holds for a library without them"""
    assert all(name in pkg.ABI_SYMBOLS for name in NAMES)


def test_symbols_are_exported_declared_and_listed(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mslam_hip.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in pkg.ABI_SYMBOLS and hasattr(pkg.lib(), name), name
    assert pkg.lib().mslam_hip_abi_version() == 5
    for m in ("kf_fuse_search", "kf_replace_ids", "kf_fuse"):
        assert callable(getattr(pkg.Context, m))
    assert callable(pkg.HipBackend.fuse)


def _rows(p):
    return list(zip(p["keep_pos"].tolist(), p["drop_pos"].tolist(), p["dist"].tolist()))


@pytest.mark.parametrize("name", fr.HAND_CASES)
def test_hand_cases(name):
    c = fr.hand_case(name)
    got = fr.search(c["keep"], c["drop"], radius=c["radius"], **c["kw"])
    assert _rows(got) == c["expect"]
    assert got["keep_lid"].tolist() == c["keep"][2][got["keep_pos"]].tolist()
    assert got["drop_lid"].tolist() == c["drop"][2][got["drop_pos"]].tolist()


def test_search_is_guided_matching_plus_gate_and_resolution():
    """without shared ids and with the gate off, what a keep landmark accepts is what guided matching's `match` gives with
    the drop landmarks' projections as keypoints; the pairs are one to one and ordered"""
    c = fr.random_case(3, 60, 90)
    kw = dict(c["kw"], max_world_distance=np.inf)
    acc = fr.accepted(c["keep"], c["drop"], radius=c["radius"], **kw)
    xy, _ = fr.drop_keypoints(c["drop"][1], kw["R"], kw["t"], kw["cam"], kw["width"], kw["height"])
    fi, ti = gm.match(c["drop"][0], xy, c["keep"][0], c["keep"][1], kw["R"], kw["t"], c["radius"], kw["max_distance"], kw["ratio"],
                      kw["cam"], kw["width"], kw["height"])
    assert [(j, a[0]) for j, a in enumerate(acc) if a is not None] == list(zip(ti.tolist(), fi.tolist())) and len(fi) > 10
    got = fr.search(c["keep"], c["drop"], radius=c["radius"], **kw)
    assert len(set(got["drop_pos"].tolist())) == len(got["drop_pos"]) < len(fi)      # some drop landmark was claimed twice
    assert got["keep_pos"].tolist() == sorted(got["keep_pos"].tolist())
    gated = fr.search(c["keep"], c["drop"], radius=c["radius"], **c["kw"])
    assert 0 < len(gated["keep_pos"]) and _rows(gated) != _rows(got)                  # the gate changes the outcome here


def test_replacement_rules():
    D = np.zeros((3, 32), np.uint8)
    W = np.arange(9.0).reshape(3, 3)
    store = {0: (D, W, [5, 6, 7]), 1: (D[:2], W[:2] + 100, [6, 5]), 2: (D[:0], W[:0], [])}
    # simultaneous: 5 -> 6 and 6 -> 5 swap, nothing is applied twice
    new, n = fr.replace_ids(store, [5, 6], [6, 5])
    assert n == 4 and new[0][2].tolist() == [6, 5, 7] and new[1][2].tolist() == [5, 6]
    assert new[0][1].tobytes() == W.tobytes()                                            # world_xyz = None: the ids alone
    # a `from` listed twice: the later wins; from == to: the point alone changes; unknown ids are ignored
    new, n = fr.replace_ids(store, [5, 5, 7, 99], [8, 9, 7, 1], [[1, 1, 1], [2, 2, 2], [3, 3, 3], [4, 4, 4]])
    assert n == 3 and new[0][2].tolist() == [9, 6, 7] and new[1][2].tolist() == [6, 9]
    assert new[0][1].tolist() == [[2, 2, 2], [3, 4, 5], [3, 3, 3]] and new[1][1].tolist() == [[100, 101, 102], [2, 2, 2]]
    # fuse: the pairs' drop ids take the keep ids and the keep points, in every entry
    c = fr.hand_case("repeated_id")
    st = {10: c["keep"], 20: c["drop"], 30: (c["drop"][0][:1], c["drop"][1][:1] + 5, [11])}
    pairs, new, n = fr.fuse(st, 10, 20, radius=c["radius"], **c["kw"])
    assert n == 3 and new[20][2].tolist() == [2, 2] and new[30][2].tolist() == [2]       # 11 listed twice: the later pair wins
    assert new[30][1].tobytes() == c["keep"][1][1:2].tobytes()
    assert len(set(lm.covisible({k: v[2] for k, v in new.items()}, 10, [20, 30]).tolist()) - {1}) == 0


def test_backend_fuse_matches_its_restatement(pkg):
    be = pkg.HipBackend(None)
    rng = np.random.default_rng(0)
    be.add_keyframe(0, (0, 0, 0, 1, 0, 0, 0), [1, 2, 3], rng.normal(size=(3, 3)))
    be.add_keyframe(1, (0, 0, 0, 1, 1, 0, 0), [3, 11, 12], rng.normal(size=(3, 3)))
    be.add_keyframe(2, (0, 0, 0, 1, 2, 0, 0), [12, 13], rng.normal(size=(2, 3)))
    obs, lms, anc = fr.backend_fuse(be.obs, be.landmarks, be.anchor, [1, 2], [11, 12])
    kept = {l: be.landmarks[l].copy() for l in (1, 2)}
    assert be.fuse([1, 2], [11, 12]) == 3
    assert {k: v[0].tolist() for k, v in be.obs.items()} == {k: v[0].tolist() for k, v in obs.items()} == {0: [1, 2, 3], 1: [3, 1, 2], 2: [2, 13]}
    assert sorted(be.landmarks) == sorted(lms) == [1, 2, 3, 13] and be.anchor == anc == {1: 0, 2: 0, 3: 0, 13: 2}
    assert all(be.landmarks[l].tobytes() == kept[l].tobytes() for l in kept)
    assert be.fuse([], []) == 0
    with pytest.raises(pkg.MslamHipError) as e:
        be.fuse([1], [])
    assert e.value.code == pkg.E_INVALID


def test_tracker_needs_loop_closure_for_fusion(pkg):
    with pytest.raises(pkg.MslamHipError) as e:
        pkg.HipKeyframeTracker(None, local_map_depth=2, local_ba=True, loop_fusion=True)
    assert e.value.code == pkg.E_INVALID
    assert (pkg.HipKeyframeTracker.FUSE_KEEP_ID, pkg.HipKeyframeTracker.FUSE_DROP_ID) == (0x7ffffffe, 0x7ffffffd)


@pytest.fixture(scope="module")
def ring():
    seq = loop_walk.ring_sequence()
    return seq, fr.run_ring(seq, False), fr.run_ring(seq, True)


def test_cpu_tracker_fuses_across_the_ring_walk_loop(ring):
    seq, (rows0, t0), (rows1, t1) = ring
    # the same single loop with and without fusion, and no second one
    assert len(t0.loops) == len(t1.loops) == 1
    a, b = t0.loops[0], t1.loops[0]
    assert (a["keyframe"], a["loop"], a["frame"]) == (b["keyframe"], b["loop"], b["frame"]) and b["loop"] == 0
    assert [r["loop"] for r in rows1].count(None) == len(rows1) - 1
    cur, loop, fu = b["keyframe"], b["loop"], b["fusion"]
    print("ring walk: loop (%d, %d) at frame %d, fusion %d pairs, %d rewritten, edges %s; keyframes %d / %d" % (
        cur, loop, b["frame"], fu["n_pairs"], fu["n_rewritten"], fu["edges"], len(t0.ids), len(t1.ids)))
    assert fu["n_pairs"] > 0 and fu["n_rewritten"] >= fu["n_pairs"]
    assert (cur, loop) in fu["edges"] and loop in t1.graph[cur] and cur in t1.graph[loop]
    assert loop not in t0.graph[cur]
    # up to the closure the two runs are one
    for x, y in zip(rows0[:b["frame"] + 1], rows1[:b["frame"] + 1]):
        assert x["keyframe"] == y["keyframe"] and x["R"].tobytes() == y["R"].tobytes()
    # The walk ends 8 frames behind the closure and inserts no keyframe on that stretch, with or without fusion: the vote
    # makes keyframe 0 the reference and its map covers the view.  So the last frame is processed once more with the
    # keyframe threshold out of reach, which forces a keyframe.  With fusion it was tracked on a local map that spans the
    # loop: it inherits ids of the old side and is a neighbour of both sides; without, the new side is out of its reach.
    assert [k for k in t1.ids if k > cur] == [k for k in t0.ids if k > cur] == []
    old_ids = set(t0.lids[loop].tolist())
    last = seq["frames"][-1]
    forced = []
    for t in (t0, t1):
        t.new_keyframe_min_landmarks = 10 ** 6
        r = t.process(last["desc"], last["xy"], last["depth"])
        assert r["tracked"] and r["keyframe"] == cur + 1 and r["loop"] is None      # and no second loop fires
        forced.append(r["keyframe"])
    k = forced[1]
    assert old_ids & set(t1.lids[k].tolist())
    assert loop in t1.graph[k] and cur in t1.graph[k]
    assert cur not in t0.graph[k] and cur not in t0.local and cur in t1.local
    assert len(t0.loops) == len(t1.loops) == 1
    assert all(r["tracked"] for r in rows1)
