"""Landmark fusion into many target entries without a GPU: the two entry points are exported, declared and listed and the
Python surface exists; tests/fuse_multi_ref.py's restatement proves every rule of include/mslam_hip.h's statement on hand
cases, row by row (the GPU tests then hold the library to the restatement); a planted two-pose scene shows what a search
under one pose misses; and the CPU tracker on the ring walk closes the same single loop with every keyframe of the new
side as a target."""
import inspect
import os
import re

import numpy as np
import pytest

import fuse_multi_ref as fm
import fuse_ref as fr
import guided_match_ref as gm
import loop_walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mslam_hip_kf_fuse_search_multi", "mslam_hip_kf_fuse_multi"]


def test_symbols_are_exported_declared_and_listed(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mslam_hip.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in pkg.ABI_SYMBOLS and hasattr(pkg.lib(), name), name
    assert pkg.lib().mslam_hip_abi_version() == 5
    for m in ("kf_fuse_search_multi", "kf_fuse_multi"):
        assert callable(getattr(pkg.Context, m))
    assert inspect.signature(pkg.HipKeyframeTracker.__init__).parameters["loop_fusion_keyframes"].default is False
    with pytest.raises(pkg.MslamHipError) as e:                  # the option needs loop_fusion
        pkg.HipKeyframeTracker(None, local_map_depth=2, local_ba=True, loop_fusion_keyframes=True)
    assert e.value.code == pkg.E_INVALID
    doc = pkg.HipKeyframeTracker.__doc__
    assert "loop_fusion_keyframes" in doc and "STILL OUT: old-side landmarks that no new-side keyframe sees" in doc


@pytest.mark.parametrize("name", fm.HAND_CASES)
def test_hand_cases(name):
    c = fm.hand_case(name)
    got = fm.search_multi(c["keep"], c["drops"], c["Rs"], c["ts"], c["radius"], **c["kw"])
    assert fm.rows_of(got) == c["expect"]
    assert got["keep_lid"].tolist() == c["keep"][2][got["keep_pos"]].tolist()
    assert got["drop_lid"].tolist() == [int(c["drops"][m][2][i]) for m, i in zip(got["target"].tolist(), got["drop_pos"].tolist())]
    assert len(set(got["keep_lid"].tolist())) == len(set(got["drop_lid"].tolist())) == len(got["dist"])     # one to one on ids


def test_one_target_is_fuse_ref_search():
    """(a) with one target, and no id repeated inside an entry, the result is fuse_ref.search's plus a zero target column:
    on fuse_ref's hand cases and on random cases with shared ids and twins, under the identity and under a real pose"""
    cases = [fr.hand_case(n) for n in fr.HAND_CASES if n != "repeated_id"]
    cases += [fr.random_case(4, 60, 90, shared=3), fr.random_case(5, 130, 70, shared=2), fr.posed_case(6, 80, 90, shared=3)]
    n_rows = 0
    for c in cases:
        kw = {k: v for k, v in c["kw"].items() if k not in ("R", "t")}
        ref = fr.search(c["keep"], c["drop"], radius=c["radius"], **c["kw"])
        got = fm.search_multi(c["keep"], [c["drop"]], [c["kw"]["R"]], [c["kw"]["t"]], c["radius"], **kw)
        for k in fr_keys():
            assert got[k].tobytes() == ref[k].tobytes(), k
        assert got["target"].tolist() == [0] * len(ref["dist"])
        n_rows += len(ref["dist"])
    assert n_rows > 100


def fr_keys():
    return ("keep_pos", "drop_pos", "keep_lid", "drop_lid", "dist")


def test_per_target_acceptance_is_fuse_ref_accepted():
    """the all-pairs window and gate of fuse_multi_ref.accepted give what fuse_ref.accepted gives keep landmark by keep
    landmark, when the eligibility passed in is fuse_ref's"""
    for c in (fr.random_case(7, 90, 120, shared=4), fr.posed_case(8, 100, 110, shared=3)):
        kw = c["kw"]
        k_ok, d_ok = fr.eligible(c["keep"][2], c["drop"][2])
        got = fm.accepted(c["keep"], c["drop"], k_ok, d_ok, kw["R"], kw["t"], c["radius"], kw["max_distance"], kw["ratio"],
                          kw["max_world_distance"], kw["cam"], kw["width"], kw["height"])
        assert got == fr.accepted(c["keep"], c["drop"], radius=c["radius"], **kw) and sum(a is not None for a in got) > 20


def test_two_pose_scene_finds_what_one_pose_misses():
    """duplicates that project outside the frame under pose 0 and inside it under pose 1: today's call, the union of the
    targets searched under pose 0 alone, misses them; search_multi finds them as rows of target 1"""
    s = fm.two_pose_scene()
    kw = s["kw"]
    union = tuple(np.concatenate([d[k] for d in s["drops"]]) for k in range(3))
    one = fr.search(s["keep"], union, R=s["Rs"][0], t=s["ts"][0], radius=s["radius"], **kw)
    multi = fm.search_multi(s["keep"], s["drops"], s["Rs"], s["ts"], s["radius"], **kw)
    _, in0 = fr.drop_keypoints(s["drops"][1][1], s["Rs"][0], s["ts"][0], kw["cam"], kw["width"], kw["height"])
    _, in1 = fr.drop_keypoints(s["drops"][1][1], s["Rs"][1], s["ts"][1], kw["cam"], kw["width"], kw["height"])
    outside = [(int(l), int(i)) for m, i, l in zip(multi["target"], multi["drop_pos"], multi["drop_lid"]) if m == 1 and not in0[i]]
    print("two poses: %d pairs under pose 0 alone, %d with both, %d of them outside pose 0's frame" % (
        len(one["dist"]), len(multi["dist"]), len(outside)))
    assert len(outside) > 0 and all(in1[i] for _, i in outside)
    assert not set(l for l, _ in outside) & set(one["drop_lid"].tolist())
    assert set(one["drop_lid"].tolist()) <= set(multi["drop_lid"].tolist())


def test_random_cases_plant_both_conflicts():
    """every random case of the GPU test drops a row in step A and one in step B, and its result is one to one on ids"""
    for n_drop, nk in fm.RANDOM_CASES[:4]:
        c = fm.random_case(n_drop, nk)
        st = {}
        got = fm.search_multi(c["keep"], c["drops"], c["Rs"], c["ts"], c["radius"], stages=st, **c["kw"])
        print("n_drop %d, keep %d, targets %s: %d rows, A drops %d, B drops %d -> %d pairs" % (
            n_drop, nk, [len(d[0]) for d in c["drops"]], len(st["rows"]), len(st["dropped_a"]), len(st["dropped_b"]), len(got["dist"])))
        assert len(st["dropped_a"]) > 0 and len(st["dropped_b"]) > 0 and len(got["dist"]) > 0
        assert len(set(got["keep_lid"].tolist())) == len(set(got["drop_lid"].tolist())) == len(got["dist"])
        assert fm.rows_of(got) == sorted(fm.rows_of(got), key=lambda r: r[:2])
        assert not set(got["keep_lid"].tolist()) & set(np.concatenate([d[2] for d in c["drops"]]).tolist())


def test_fuse_multi_rewrites_every_entry():
    c = fm.hand_case("a_before_b")
    store = {1: c["keep"], 10: c["drops"][0], 11: c["drops"][1], 30: (c["drops"][1][0][:1], c["drops"][1][1][:1] + 5, [12])}
    pairs, new, n = fm.fuse_multi(store, 1, [10, 11], c["Rs"], c["ts"], c["radius"], **c["kw"])
    assert pairs["drop_lid"].tolist() == [12, 11] and pairs["keep_lid"].tolist() == [1, 2]
    assert n == 4 and new[10][2].tolist() == [2] and new[11][2].tolist() == [2, 1] and new[30][2].tolist() == [1]
    assert new[30][1].tobytes() == c["keep"][1][:1].tobytes() and new[10][1].tobytes() == c["keep"][1][1:2].tobytes()


@pytest.fixture(scope="module")
def ring():
    seq = loop_walk.ring_sequence()
    return seq, fr.run_ring(seq, True), fm.run_ring(seq)


def test_cpu_tracker_fuses_into_every_keyframe_of_the_new_side(ring):
    """The ring walk with every keyframe of the new side as a target: the same single loop, at least as many fused ids as
    with the one corrected keyframe as the camera, no second loop.  Whether the ring yields a pair outside the new
    keyframe's view is printed, not asserted: the walk's new side looks at the wall from poses close to the new keyframe's,
    so it may yield none, and test_two_pose_scene_finds_what_one_pose_misses holds that property."""
    seq, (rows1, t1), (rowsm, tm) = ring
    assert len(t1.loops) == len(tm.loops) == 1
    a, b = t1.loops[0], tm.loops[0]
    assert (a["keyframe"], a["loop"], a["frame"]) == (b["keyframe"], b["loop"], b["frame"])
    assert [r["loop"] for r in rowsm].count(None) == len(rowsm) - 1
    fa, fb = a["fusion"], b["fusion"]
    only = set(fb["pairs"]["drop_lid"].tolist()) - set(fa["pairs"]["drop_lid"].tolist())
    print("ring walk: loop (%d, %d); one camera %d pairs / %d rewritten, targets %s: %d pairs / %d rewritten, %d drop ids new; edges %s" % (
        b["keyframe"], b["loop"], fa["n_pairs"], fa["n_rewritten"], fb["targets"], fb["n_pairs"], fb["n_rewritten"], len(only), fb["edges"]))
    assert fb["n_pairs"] >= fa["n_pairs"] > 0 and fb["n_rewritten"] >= fb["n_pairs"]
    assert fb["targets"] == sorted(fb["targets"]) and b["keyframe"] in fb["targets"]
    assert (b["keyframe"], b["loop"]) in fb["edges"] and b["loop"] in tm.graph[b["keyframe"]]
    assert all(r["tracked"] for r in rowsm)
    # one more frame, forced to be a keyframe: no second loop fires
    last = seq["frames"][-1]
    tm.new_keyframe_min_landmarks = 10 ** 6
    r = tm.process(last["desc"], last["xy"], last["depth"])
    assert r["tracked"] and r["keyframe"] == b["keyframe"] + 1 and r["loop"] is None and len(tm.loops) == 1
