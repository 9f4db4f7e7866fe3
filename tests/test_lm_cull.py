"""Landmark culling without a GPU: the entry points are exported, declared and listed; tests/lm_cull_ref.py's restatement
holds the rules of include/mslam_hip.h's statement on hand cases (the GPU tests then hold the library to the restatement);
HipBackend.remove_landmarks against its restatement; HipKeyframeTracker's bookkeeping on a stub context; the constructor's
defaults; and the condition the GPU tracker test rests on."""
import inspect
import os
import re

import numpy as np
import pytest

import cull_ref as cr
import lm_cull_ref as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mslam_hip_kf_remove_landmarks", "mslam_hip_kf_cull_landmarks_search", "mslam_hip_kf_cull_landmarks"]


def test_symbols_are_exported_declared_and_listed(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mslam_hip.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr)
        assert name in pkg.ABI_SYMBOLS and hasattr(pkg.lib(), name)
    assert pkg.lib().mslam_hip_abi_version() == 5
    for f in (pkg.Context.kf_remove_landmarks, pkg.Context.kf_cull_landmarks_search, pkg.Context.kf_cull_landmarks,
              pkg.HipBackend.remove_landmarks):
        assert callable(f)
    for f in (pkg.Context.kf_cull_landmarks_search, pkg.Context.kf_cull_landmarks):
        assert inspect.signature(f).parameters["min_observers"].default == 2


def test_constructor_defaults(pkg):
    p = inspect.signature(pkg.HipKeyframeTracker.__init__).parameters
    assert (p["lm_cull"].default, p["lm_cull_min_observers"].default, p["lm_cull_age"].default) == (False, 2, 2)
    t = pkg.HipKeyframeTracker(None)
    assert (t.lm_cull, t.lm_cull_min_observers, t.lm_cull_age, t.lm_cull_results) == (False, 2, 2, [])
    t = pkg.HipKeyframeTracker(None, lm_cull=True, lm_cull_min_observers=3, lm_cull_age=1)      # it needs no other option
    assert (t.lm_cull, t.lm_cull_min_observers, t.lm_cull_age, t.backend) == (True, 3, 1, None)
    doc = pkg.HipKeyframeTracker.__doc__
    assert "lm_cull = True" in doc and "culling landmarks by age or by observer count" not in doc and "found / visible" in doc


# ---- the restatement on hand cases ------------------------------------------------------------------------------------
def _run(name):
    lids, ids, cand, mo = lc.hand_case(name)
    new, res = lc.cull_landmarks(lids, ids, cand, mo)
    return lids, ids, cand, mo, {k: v[2].tolist() for k, v in new.items()}, res


def test_a_repeat_inside_an_entry_counts_once_and_all_its_positions_go():
    lids, ids, cand, mo, new, res = _run("repeat_inside")
    assert res["landmark_ids"].tolist() == [7] and res["observers"].tolist() == [1]             # one observer, not three
    assert new == {1: [8], 2: [8, 9], 3: [9]} and res["entry_removed"].tolist() == [3, 0, 0] and res["n_removed"] == 3
    _, rem = lc.remove_landmarks(lids, ids, [7, 99, 7, 8])
    assert rem["removed"].tolist() == [3, 0, 3, 2] and rem["entry_removed"].tolist() == [4, 1, 0] and rem["n_removed"] == 5


def test_an_unlisted_holder_does_not_count_and_is_not_changed():
    lids, ids, cand, mo, new, res = _run("unlisted_holder")
    assert res["landmark_ids"].tolist() == [5] and res["observers"].tolist() == [1]
    assert new[1] == [6] and new[3] == [5]                                                       # entry 3 keeps its 5
    assert lc.cull_landmarks_search(lids, [1, 2, 3], cand, mo)["landmark_ids"].tolist() == []    # listed, it would count


def test_an_inherited_id_of_a_candidate_is_judged():
    lids, ids, cand, mo, new, res = _run("inherited")
    assert res["landmark_ids"].tolist() == [4, 11] and res["observers"].tolist() == [2, 1]
    assert new == {1: [10], 2: [], 3: [10, 12]}                                                 # 4 leaves entry 1 as well
    assert res["entry_removed"].tolist() == [1, 2, 0]
    assert lc.cull_landmarks_search(lids, ids, cand, 2)["landmark_ids"].tolist() == [11]


def test_min_observers_1_finds_nothing_and_what_no_candidate_holds_stays():
    lids, ids, cand, mo, new, res = _run("min_observers_1")
    assert len(res["landmark_ids"]) == 0 and res["n_removed"] == 0 and new == {k: list(v) for k, v in lids.items()}
    lids, ids, cand, mo, new, res = _run("not_judged")
    assert res["landmark_ids"].tolist() == [32] and new == {1: [30, 31], 2: [31]}                # 30: one observer, not judged
    assert len(lc.cull_landmarks_search(lids, ids, [], 2)["landmark_ids"]) == 0                  # n_cand = 0


def test_ids_come_out_ascending_and_counts_are_taken_once():
    lids, ids, cand, mo, new, res = _run("ascending")
    assert res["landmark_ids"].tolist() == [5, 70, 90] and new == {1: [20], 2: [20]}
    # removing 7 from entry 1 does not make 8 (two observers) a one-observer landmark within the call
    lids, ids, cand, mo, new, res = _run("repeat_inside")
    assert 8 not in res["landmark_ids"].tolist()


def test_errors_of_the_restatement():
    lids = {1: [1, 2], 2: [2, 3]}
    for bad in (lambda: lc.cull_landmarks_search(lids, [1, 9], []), lambda: lc.remove_landmarks(lids, [9], [1])):
        with pytest.raises(KeyError):
            bad()
    for bad in (lambda: lc.cull_landmarks_search(lids, [1, 1], []), lambda: lc.cull_landmarks_search(lids, [], []),
                lambda: lc.cull_landmarks_search(lids, [1], [2]), lambda: lc.cull_landmarks_search(lids, [1, 2], [1, 1]),
                lambda: lc.cull_landmarks_search(lids, [1, 2], [1], 0), lambda: lc.cull_landmarks_search(lids, [1, 2], [1], 65536),
                lambda: lc.remove_landmarks(lids, [1], [-1]), lambda: lc.remove_landmarks(lids, [], [1])):
        with pytest.raises(ValueError):
            bad()
    assert lc.remove_landmarks(lids, [1, 2], [])[1]["n_removed"] == 0


def test_the_restatement_agrees_with_the_observer_counts_on_a_random_store():
    store = cr.random_case(3, [0, 1, 40, 300, 300, 300], pool=500)
    ids = sorted(store)
    found = lc.cull_landmarks_search(store, ids, ids[2:4], 2)
    assert 0 < len(found["landmark_ids"]) and np.array_equal(cr.observers(store, ids, found["landmark_ids"]), found["observers"])
    assert (found["observers"] == 1).all() and (np.diff(found["landmark_ids"]) > 0).all()
    new, res = lc.cull_landmarks(store, ids, ids[2:4], 2)
    assert res["n_removed"] >= len(found["landmark_ids"]) and sum(len(v[2]) for v in new.values()) == sum(len(v[2]) for v in store.values()) - res["n_removed"]
    assert len(lc.cull_landmarks_search(new, ids, ids[2:4], 2)["landmark_ids"]) == 0


# ---- the backend --------------------------------------------------------------------------------------------------------
def _backend(pkg):
    b = pkg.HipBackend(None)
    rng = np.random.default_rng(5)
    I = (0, 0, 0, 1, 0, 0, 0)
    b.add_keyframe(3, I, [10, 11, 12, 11], rng.normal(size=(4, 3)))     # 11 twice
    b.add_keyframe(5, I, [11, 12, 13, 20], rng.normal(size=(4, 3)))
    b.add_keyframe(4, I, [12, 13, 14], rng.normal(size=(3, 3)))
    return b


@pytest.mark.parametrize("lids", [[11], [20, 99], [], [11, 12, 13, 14, 10, 20], [14, 14]])
def test_backend_remove_landmarks_against_the_restatement(pkg, lids):
    b = _backend(pkg)
    obs, lms, anchor, ref = lc.backend_remove_landmarks(b.obs, b.landmarks, b.anchor, lids)
    assert b.remove_landmarks(lids) == ref
    assert sorted(b.obs) == sorted(obs) == [3, 4, 5] and sorted(b.poses) == [3, 4, 5]
    for k in obs:
        assert b.obs[k][0].tolist() == obs[k][0].tolist() and b.obs[k][1].tobytes() == obs[k][1].tobytes()
    assert b.anchor == anchor and sorted(b.landmarks) == sorted(lms) and not set(lids) & set(b.landmarks)
    assert all(b.landmarks[l].tobytes() == lms[l].tobytes() for l in lms)


def test_backend_remove_landmarks_counts(pkg):
    b = _backend(pkg)
    assert b.remove_landmarks([11, 99]) == dict(n_observations=3, n_landmarks=1)                 # both positions of keyframe 3
    assert b.obs[3][0].tolist() == [10, 12] and b.obs[5][0].tolist() == [12, 13, 20] and 11 not in b.anchor
    assert b.remove_landmarks([11]) == dict(n_observations=0, n_landmarks=0)


# ---- the tracker's bookkeeping --------------------------------------------------------------------------------------------
class StubContext:
    """Context.kf_cull_landmarks on an id dict, answered by the restatement"""

    def __init__(self, lids):
        self.lids, self.calls = {k: np.array(v, np.int64) for k, v in lids.items()}, []

    def kf_cull_landmarks(self, ids, cand, min_observers=2):
        self.calls.append((list(ids), list(cand), min_observers))
        new, res = lc.cull_landmarks(self.lids, ids, cand, min_observers)
        self.lids = {k: v[2] for k, v in new.items()}
        return res


def _stub_tracker(pkg, lids, backend=True, **kw):
    ctx = StubContext(lids)
    t = pkg.HipKeyframeTracker(ctx, lm_cull=True, **(dict(local_map_depth=2, local_ba=True, **kw) if backend else kw))
    return ctx, t


def test_tracker_pending_list_age_rule_and_records(pkg):
    lids = {0: [1, 2, 100], 1: [2, 3, 101], 2: [3, 102], 3: [3, 103]}
    ctx, t = _stub_tracker(pkg, lids)
    for k in sorted(lids):
        t.backend.add_keyframe(k, (0, 0, 0, 1, 0, 0, 0), lids[k], np.zeros((len(lids[k]), 3)))
    U = pkg.HipKeyframeTracker.LOCAL_MAP_ID
    t._local_map_of = 7
    t.ids = [0]
    t._lm_cull(0)
    t.ids = [0, 1]
    t._lm_cull(1)
    assert ctx.calls == [] and t.lm_cull_results == [] and [k for k, _ in t._lm_pending] == [0, 1]   # nothing is two insertions old
    assert t._local_map_of == 7
    t.ids = [0, 1, 2]
    t._lm_cull(2)
    assert ctx.calls == [([0, 1, 2], [0], 2)] and [k for k, _ in t._lm_pending] == [1, 2]
    rec = t.lm_cull_results[0]
    assert (rec["keyframe"], rec["listed"], rec["candidates"], rec["landmark_ids"].tolist(), rec["n_removed"], rec["n_backend"]) == \
           (2, [0, 1, 2], [0], [1, 100], 2, 2)
    assert t._local_map_of is None and U not in rec["listed"]
    assert t.backend.obs[0][0].tolist() == [2] and 1 not in t.backend.landmarks and 100 not in t.backend.anchor
    assert t.backend.obs[3][0].tolist() == [3, 103]                       # keyframe 3 is not in the map yet: untouched
    t.ids, t._local_map_of = [0, 1, 2, 3], 9
    t._lm_cull(3)
    assert ctx.calls[1] == ([0, 1, 2, 3], [1], 2) and t.lm_cull_results[1]["landmark_ids"].tolist() == [101]
    assert ctx.lids[1].tolist() == [2, 3] and t._local_map_of is None


def test_tracker_skips_a_culled_keyframe_resets_the_map_only_on_removal_and_guards_the_capacity(pkg):
    lids = {0: [1, 2], 1: [1, 2], 2: [1, 2], 3: [1, 2], 4: [1, 2, 50]}
    ctx, t = _stub_tracker(pkg, lids, backend=False, lm_cull_age=1)
    t.ids = [0]
    t._lm_cull(0)
    t.ids, t._local_map_of = [0, 1], 5
    t._lm_cull(1)                                                         # candidate 0: every landmark has two observers
    assert ctx.calls == [([0, 1], [0], 2)] and t.lm_cull_results[0]["n_removed"] == 0 and t.lm_cull_results[0]["n_backend"] == 0
    assert t._local_map_of == 5                                           # nothing was removed: the union stays
    t.ids = [0, 2]                                                        # keyframe 1 was culled away before its turn
    t._lm_cull(2)
    assert len(ctx.calls) == 1 and len(t.lm_cull_results) == 1 and [k for k, _ in t._lm_pending] == [2]      # no call: cand is empty
    t.ids = [0, 2, 3]
    t._lm_cull(3)
    assert ctx.calls[1] == ([0, 2, 3], [2], 2)
    # the capacity guard comes before the context is touched; a call with no candidate does not reach it
    t.ids = list(range(pkg.CULL_MAX_ENTRIES + 1))
    with pytest.raises(pkg.MslamHipError) as e:
        t._lm_cull(4)
    assert e.value.code == pkg.E_CAPACITY and len(ctx.calls) == 2


# ---- the condition the GPU tracker test rests on --------------------------------------------------------------------------
def test_cpu_tracker_culls_landmarks_on_the_sequence(orc):
    rows, trk = lc.run(True)
    plain, trk0 = lc.run(False)
    size = lambda t: sum(len(t.lids[k]) for k in t.ids)
    removed = [c["n_removed"] for c in trk.lm_cull_results]
    print("sequence: %d frames, keyframes %d / %d, store landmarks %d without culling, %d with; last union %d / %d; %d calls removed %s"
          % (len(rows), len(trk0.ids), len(trk.ids), size(trk0), size(trk), trk0.unions[-1], trk.unions[-1], len(removed), removed))
    assert len(rows) == 16 and all(r["tracked"] for r in rows) and all(r["tracked"] for r in plain)
    assert any(n >= 1 for n in removed)
    assert trk.unions[-1] < trk0.unions[-1] and size(trk) < size(trk0)
    # after the run, no landmark held by a judged keyframe has fewer than min_observers observers
    judged = sorted({k for c in trk.lm_cull_results for k in c["candidates"]})
    obs = cr.obs_counts(trk.lids, trk.ids)
    assert judged and all(obs[l] >= trk.min_observers for k in judged for l in trk.lids[k].tolist())
    assert all(c["candidates"] == [c["keyframe"] - trk.age] for c in trk.lm_cull_results)     # every frame is a keyframe here
