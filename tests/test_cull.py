"""Keyframe culling without a GPU: the entry points are exported, declared and listed; tests/cull_ref.py's restatement holds
the rules of include/mslam_hip.h's statement on hand cases (the GPU tests then hold the library to the restatement);
HipBackend.remove_keyframe against its restatement; the bridging rule; HipKeyframeTracker's bookkeeping on a stub context;
the constructor's defaults and guard; and the condition the GPU tracker test rests on."""
import inspect
import os
import re

import numpy as np
import pytest

import cull_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mslam_hip_kf_observers", "mslam_hip_kf_cull_search", "mslam_hip_kf_cull"]


def test_symbols_are_exported_declared_and_listed(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mslam_hip.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr)
        assert name in pkg.ABI_SYMBOLS and hasattr(pkg.lib(), name)
    assert pkg.lib().mslam_hip_abi_version() == 5
    assert int(re.search(r"MSLAM_HIP_CULL_MAX_ENTRIES (\d+)", hdr).group(1)) == pkg.CULL_MAX_ENTRIES == cr.MAX_ENTRIES == 4096
    for f in (pkg.Context.kf_observers, pkg.Context.kf_cull_search, pkg.Context.kf_cull, pkg.HipBackend.remove_keyframe):
        assert callable(f)
    for f in (pkg.Context.kf_cull_search, pkg.Context.kf_cull):
        p = inspect.signature(f).parameters
        assert (p["min_observers"].default, p["ratio"].default, p["min_landmarks"].default) == (3, 0.9, 1)


def test_constructor_defaults_and_guard(pkg):
    p = inspect.signature(pkg.HipKeyframeTracker.__init__).parameters
    assert p["kf_cull"].default is False and p["cull_min_observers"].default == 3 and p["cull_ratio"].default == 0.9
    for kw in (dict(local_map_depth=2), dict()):
        with pytest.raises(pkg.MslamHipError) as e:
            pkg.HipKeyframeTracker(None, kf_cull=True, **kw)
        assert e.value.code == pkg.E_INVALID
    t = pkg.HipKeyframeTracker(None, local_map_depth=2, local_ba=True, kf_cull=True, cull_min_observers=4, cull_ratio=0.8)
    assert (t.kf_cull, t.cull_min_observers, t.cull_ratio, t.cull_results) == (True, 4, 0.8, [])
    assert pkg.HipKeyframeTracker(None).kf_cull is False


# ---- the restatement on hand cases ------------------------------------------------------------------------------------
def _run(name):
    lids, ids, cand, kw = cr.hand_case(name)
    return lids, ids, cand, kw, cr.cull_search(lids, ids, cand, **kw)


def test_a_repeat_inside_an_entry_counts_once():
    lids, ids, cand, kw, res = _run("repeat_inside")
    assert cr.observers(lids, ids, [7, 8, 9, 10, 7]).tolist() == [2, 2, 1, 0, 2]        # 7: entries 1 and 2, not four
    assert res["n_landmarks"].tolist() == [2] and res["n_redundant"].tolist() == [2] and res["culled"].tolist() == [True]
    assert cr.observers(lids, [2, 3], [7, 8]).tolist() == [1, 1]                        # an unlisted entry does not count


def test_min_observers_at_the_boundary():
    lids, ids, cand, kw, res = _run("min_observers_at")
    assert cr.observers(lids, ids, [5, 6]).tolist() == [4, 3]
    assert res["n_landmarks"].tolist() == [2] and res["n_redundant"].tolist() == [1]    # 5: three others; 6: one fewer
    assert cr.cull_search(lids, ids, cand, min_observers=2, ratio=0.4)["n_redundant"].tolist() == [2]
    assert cr.cull_search(lids, ids, cand, min_observers=4, ratio=0.4)["n_redundant"].tolist() == [0]


def test_the_ratio_boundary_is_strict():
    assert _run("ratio_9_of_10")[4]["culled"].tolist() == [False]                       # 9 > 0.9 * 10 is false
    res = _run("ratio_9_of_10")[4]
    assert (res["n_landmarks"].tolist(), res["n_redundant"].tolist()) == ([10], [9])
    res = _run("ratio_91_of_100")[4]
    assert (res["n_landmarks"].tolist(), res["n_redundant"].tolist(), res["culled"].tolist()) == ([100], [91], [True])
    lids, ids, cand, _ = cr.hand_case("ratio_91_of_100")
    assert cr.cull_search(lids, ids, cand, ratio=0.91)["culled"].tolist() == [False]    # 91 > 0.91 * 100 is false
    assert cr.cull_search(lids, ids, cand, ratio=1.0)["culled"].tolist() == [False]
    lids, ids, cand, _ = cr.hand_case("mutual_pair")
    assert cr.cull_search(lids, ids, [1], ratio=1.0)["culled"].tolist() == [False]      # nothing exceeds the whole
    assert cr.cull_search({1: [3], 2: [4]}, [1, 2], [1], ratio=0.0)["culled"].tolist() == [False]   # 0 > 0 is false


@pytest.mark.parametrize("name, first", [("mutual_pair", 1), ("mutual_pair_reversed", 2)])
def test_of_a_mutually_redundant_pair_the_first_goes(name, first):
    lids, ids, cand, kw, res = _run(name)
    assert cand[0] == first and res["culled"].tolist() == [True, False] and res["n_culled"] == 1
    assert res["n_redundant"].tolist() == [20, 0]                                        # what the second saw at its turn
    new, _ = cr.cull(cr.store_of(lids), ids, cand, **kw)
    assert sorted(new) == sorted(set(ids) - {first})
    for k in cand:                                                                       # each alone would go
        assert cr.cull_search(lids, ids, [k])["culled"].tolist() == [True]


def test_an_empty_candidate_and_min_landmarks():
    res = _run("empty_candidate")[4]
    assert res["culled"].tolist() == [False, True] and res["n_landmarks"].tolist() == [0, 5]
    res = _run("min_landmarks")[4]
    assert res["culled"].tolist() == [False, True] and res["n_redundant"].tolist() == [4, 5]
    lids, ids, cand, _ = cr.hand_case("min_landmarks")
    assert cr.cull_search(lids, ids, cand, min_landmarks=4)["culled"].tolist() == [True, True]


def test_the_chain_alternates_and_needs_the_greedy_update():
    lids, ids, cand, kw, expect = cr.chain_case()
    res = cr.cull_search(lids, ids, cand, **kw)
    assert res["culled"].tolist() == expect and res["n_culled"] == 4
    assert all(cr.cull_search(lids, ids, [k], **kw)["culled"][0] for k in cand)


def test_errors_of_the_restatement():
    lids = {1: [1, 2], 2: [2, 3]}
    for bad in (lambda: cr.cull_search(lids, [1, 9], []), lambda: cr.observers(lids, [9], [1])):
        with pytest.raises(KeyError):
            bad()
    for bad in (lambda: cr.cull_search(lids, [1, 1], []), lambda: cr.cull_search(lids, [], []), lambda: cr.cull_search(lids, [1], [2]),
                lambda: cr.cull_search(lids, [1, 2], [1, 1]), lambda: cr.cull_search(lids, [1, 2], [1], min_observers=0),
                lambda: cr.cull_search(lids, [1, 2], [1], min_observers=65536), lambda: cr.cull_search(lids, [1, 2], [1], ratio=np.nan),
                lambda: cr.cull_search(lids, [1, 2], [1], ratio=1.5), lambda: cr.cull_search(lids, [1, 2], [1], min_landmarks=0),
                lambda: cr.observers(lids, [1], [-1])):
        with pytest.raises(ValueError):
            bad()
    assert cr.cull_search(lids, [1, 2], [])["n_culled"] == 0 and len(cr.observers(lids, [1], [])) == 0


def test_random_case_spreads_the_counts():
    store = cr.random_case(3, [0, 1, 40, 300, 300, 300, 300, 300], pool=400)
    ids = sorted(store)
    lids = cr.ids_of(store)
    obs = cr.obs_counts(lids, ids)
    assert min(obs.values()) == 1 and max(obs.values()) >= 5
    assert any(len(set(v.tolist())) < len(v) for v in lids.values())                     # repeats inside entries
    res = cr.cull_search(store, ids, ids, min_observers=2, ratio=0.8)
    assert 0 < res["n_culled"] < len(ids)


# ---- the backend --------------------------------------------------------------------------------------------------------
def _backend(pkg):
    b = pkg.HipBackend(None)
    rng = np.random.default_rng(5)
    I = (0, 0, 0, 1, 0, 0, 0)
    b.add_keyframe(3, I, [10, 11, 12, 11], rng.normal(size=(4, 3)))     # the first keyframe; 11 twice
    b.add_keyframe(5, I, [11, 12, 13, 20], rng.normal(size=(4, 3)))     # 13 and 20 are anchored at 5
    b.add_keyframe(4, I, [12, 13, 14], rng.normal(size=(3, 3)))
    b.add_keyframe(7, I, [13, 14, 15], rng.normal(size=(3, 3)))
    return b


@pytest.mark.parametrize("id", [5, 4, 7])
def test_backend_remove_keyframe_against_the_restatement(pkg, id):
    b = _backend(pkg)
    poses, obs, lms, anchor, ref = cr.backend_remove_keyframe(b.poses, b.obs, b.landmarks, b.anchor, b.first, id)
    got = b.remove_keyframe(id)
    assert got == ref
    assert sorted(b.poses) == sorted(poses) == sorted(b.obs) == sorted(obs) and id not in b.poses
    for k in obs:
        assert b.obs[k][0].tolist() == obs[k][0].tolist() and b.obs[k][1].tobytes() == obs[k][1].tobytes()
    assert b.anchor == anchor and sorted(b.landmarks) == sorted(lms)
    assert all(b.landmarks[l].tobytes() == lms[l].tobytes() for l in lms)


def test_backend_reanchors_drops_orphans_and_refuses_the_gauge(pkg):
    b = _backend(pkg)
    assert b.anchor[13] == 5 and b.anchor[20] == 5 and b.anchor[14] == 4 and b.first == 3
    assert b.remove_keyframe(5) == dict(n_observations=4, orphans=[20])
    assert b.anchor[13] == 4 and 20 not in b.landmarks and 20 not in b.anchor          # 13: keyframes 4 and 7, the smallest
    assert b.anchor[11] == 3 and b.anchor[12] == 3                                     # anchored elsewhere: untouched
    assert b.remove_keyframe(4) == dict(n_observations=3, orphans=[])
    assert b.anchor[13] == 7 and b.anchor[14] == 7
    for bad in (3, 5, 99):
        with pytest.raises(pkg.MslamHipError) as e:
            b.remove_keyframe(bad)
        assert e.value.code == pkg.E_INVALID
    assert sorted(b.poses) == [3, 7]


# ---- the bridging rule --------------------------------------------------------------------------------------------------
GRAPHS = {"path": ({1: {2}, 2: {1, 3}, 3: {2, 4}, 4: {3}}, 2, [(3, 1)]),
          "star": ({1: {5}, 2: {5}, 3: {5}, 4: {5}, 5: {1, 2, 3, 4}}, 5, [(2, 1), (3, 1), (4, 1)]),
          "triangle": ({1: {2, 3}, 2: {1, 3}, 3: {1, 2}}, 3, []),
          "leaf": ({1: {2}, 2: {1}}, 2, []),
          "two_sides": ({1: {2, 9}, 2: {1, 9}, 3: {4, 9}, 4: {3, 9}, 9: {1, 2, 3, 4}}, 9, [(3, 1)])}


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_bridges_keep_the_graph_connected(pkg, name):
    graph, k, bridges = GRAPHS[name]
    ref, ref_bridges = cr.remove_graph_node(graph, k)
    got = {n: set(v) for n, v in graph.items()}
    assert pkg.remove_graph_node(got, k) == ref_bridges == bridges
    assert got == ref and k not in got and all(k not in v for v in got.values())
    assert cr.is_connected(got) and all(n in got[m] for m, v in got.items() for n in v)  # symmetric


# ---- the tracker's bookkeeping --------------------------------------------------------------------------------------------
class StubContext:
    """Context.kf_cull on an id dict, answered by the restatement; bow_db_remove records"""

    def __init__(self, lids):
        self.lids, self.calls, self.bow_removed = {k: np.array(v, np.int64) for k, v in lids.items()}, [], []

    def kf_cull(self, ids, cand, min_observers=3, ratio=0.9, min_landmarks=1):
        self.calls.append((list(ids), list(cand), min_observers, ratio))
        self.lids, res = cr.cull(self.lids, ids, cand, min_observers=min_observers, ratio=ratio, min_landmarks=min_landmarks)
        return res

    def bow_db_remove(self, entry):
        self.bow_removed.append(entry)


def _stub_tracker(pkg, lids, graph, reference, **kw):
    ctx = StubContext(lids)
    t = pkg.HipKeyframeTracker(ctx, local_map_depth=2, local_ba=True, kf_cull=True, **kw)
    for k in sorted(lids):
        t.backend.add_keyframe(k, (0, 0, 0, 1, 0, 0, 0), lids[k], np.zeros((len(lids[k]), 3)))
    t.ids, t.graph, t.reference = sorted(lids), {k: set(v) for k, v in graph.items()}, reference
    t._bow_entry = {100 + k: k for k in lids}
    t._local_map_of = reference
    return ctx, t


def test_tracker_bookkeeping_on_a_stub_context(pkg):
    r = list(range(20))
    lids = {0: list(range(50, 60)), 1: r, 2: r, 3: r, 4: r, 5: r, 6: [90, 91]}
    graph = {0: {1}, 1: {0, 2}, 2: {1, 3, 5}, 3: {2, 4, 5}, 4: {3, 5}, 5: {2, 3, 4}, 6: set()}       # 6: out of reach
    ctx, t = _stub_tracker(pkg, lids, graph, reference=4)
    assert t.cull_candidates(5) == [1, 2, 3]                  # two hops of 5, without 5, the reference 4 and the gauge 0
    t._cull(5)
    assert ctx.calls == [([0, 1, 2, 3, 4, 5, 6], [1, 2, 3], 3, 0.9)]
    rec = t.cull_results[0]
    ref = cr.cull_search(lids, sorted(lids), [1, 2, 3])
    assert ref["culled"].tolist() == [True, True, False]      # five observers: two can go, the third has two others left
    assert rec["culled"] == [1, 2] and rec["candidates"] == [1, 2, 3] and rec["keyframe"] == 5 and rec["listed"] == sorted(lids)
    assert rec["n_landmarks"] == ref["n_landmarks"].tolist() and rec["n_redundant"] == ref["n_redundant"].tolist()
    assert t.ids == [0, 3, 4, 5, 6] and sorted(t.backend.poses) == [0, 3, 4, 5, 6] and sorted(ctx.lids) == [0, 3, 4, 5, 6]
    assert sorted(ctx.bow_removed) == [101, 102] and sorted(t._bow_entry.values()) == [0, 3, 4, 5, 6]
    assert 1 not in t.graph and 2 not in t.graph and all(not {1, 2} & v for v in t.graph.values())
    # 1 went first: its neighbours 0 and 2 lost their path, so 2 was tied to 0; then 2 went: 3 was tied to 0, and 5 reaches
    # 0 through 3
    assert rec["bridges"] == [(2, 0), (3, 0)]
    assert cr.is_connected({k: v for k, v in t.graph.items() if k != 6}) and t._local_map_of is None
    # nothing to judge: no call, no record
    t.reference = 3
    assert t.cull_candidates(5) == [4] and t.cull_candidates(6) == []
    t._cull(6)
    assert len(ctx.calls) == 1 and len(t.cull_results) == 1
    # a call that culls nothing is recorded and leaves the local map alone
    t._local_map_of = 3
    t._cull(5)
    assert len(ctx.calls) == 2 and t.cull_results[1]["culled"] == [] and t.cull_results[1]["bridges"] == [] and t._local_map_of == 3
    assert t.ids == [0, 3, 4, 5, 6]


def test_tracker_never_judges_what_it_does_not_hold_and_refuses_a_map_too_large(pkg):
    r = list(range(10))
    lids = {0: r, 1: r, 2: r, 3: r, 4: r}
    graph = {0: {4}, 1: {4}, 2: {4}, 3: {4}, 4: {0, 1, 2, 3, pkg.HipKeyframeTracker.LOCAL_MAP_ID}}
    ctx, t = _stub_tracker(pkg, lids, graph, reference=4, cull_min_observers=2, cull_ratio=0.5)
    t.backend.remove_keyframe(2)                                # a keyframe the backend does not hold
    assert t.cull_candidates(4) == [1, 3]
    t._cull(4)
    assert ctx.calls[0][2:] == (2, 0.5) and t.cull_results[0]["culled"] == [1, 3]
    t.ids = list(range(pkg.CULL_MAX_ENTRIES + 1))
    with pytest.raises(pkg.MslamHipError) as e:
        t._cull(4)
    assert e.value.code == pkg.E_CAPACITY and len(ctx.calls) == 1


# ---- the walk the GPU tracker test runs -----------------------------------------------------------------------------------
def test_cpu_tracker_culls_on_the_triple_walk(orc):
    seq = cr.triple_walk()
    rows, trk = cr.run_walk(seq, cull=True)
    plain, trk0 = cr.run_walk(seq, cull=False)
    gone = [k for c in trk.cull_results for k in c["culled"]]
    print("triple walk: %d frames, %d keyframes inserted, culled %s, left %s" % (len(rows), len(trk0.ids), gone, trk.ids))
    assert all(r["tracked"] for r in rows) and all(r["tracked"] for r in plain)
    assert len(gone) >= 2 and len(set(gone)) == len(gone)
    assert sorted(trk.ids + gone) == trk0.ids == list(range(len(trk0.ids)))
    assert sorted(trk.graph) == sorted(trk.store) == sorted(trk.lids) == trk.ids and cr.is_connected(trk.graph)
    assert all(0 not in c["candidates"] and c["keyframe"] not in c["candidates"] for c in trk.cull_results)
