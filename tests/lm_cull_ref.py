"""Landmark culling restated in numpy from the statement in include/mslam_hip.h (not from the kernels): the reference the
CPU, GPU and host tests of mslam_hip_kf_remove_landmarks, mslam_hip_kf_cull_landmarks_search, mslam_hip_kf_cull_landmarks,
HipBackend.remove_landmarks and HipKeyframeTracker(lm_cull=True) compare with.  An extension: the reference has no such
step; the model is ORB-SLAM's MapPointCulling, of which this is the observer threshold.  Also the hand cases, the scene
file of `mslam_harness --cull-landmarks`, a CPU tracker with the step and the sequence the tracker tests run.

A store is prune_ref's: entry id -> (descriptors [n, 32] u8, world points [n, 3] f64, landmark ids [n] i64); where only the
ids matter, a dict entry id -> landmark ids (cull_ref.ids_of takes both)."""
import numpy as np

import cull_ref as cr
import local_map_ref as lm
import track_ref as tr

CHUNK = 256                   # positions a workgroup compacts between two barriers (kCompactChunk in csrc/compact.hpp)
MARK_CHUNK = cr.CHUNK         # listed entries per counting launch
MAX_ENTRIES = cr.MAX_ENTRIES

entry = cr.entry


def _check(lids, ids, cand, min_observers):
    ids = cr._check_map(lids, ids)
    cand = [int(k) for k in np.asarray(cand).reshape(-1)]
    if len(set(cand)) != len(cand) or not set(cand) <= set(ids):
        raise ValueError("the candidates are distinct listed ids")
    if not 1 <= min_observers <= 65535:
        raise ValueError("min_observers in 1..65535")
    return ids, cand


def cull_landmarks_search(store, ids, cand, min_observers=2):
    """mslam_hip_kf_cull_landmarks_search -> dict(landmark_ids [n] i64 ascending, observers [n] i32): the ids that at least
    one candidate holds and that fewer than min_observers listed entries hold"""
    lids = cr.ids_of(store)
    ids, cand = _check(lids, ids, cand, min_observers)
    obs = cr.obs_counts(lids, ids)
    judged = set()
    for k in cand:
        judged |= set(lids[k].tolist())
    found = sorted(l for l in judged if obs[l] < min_observers)
    return dict(landmark_ids=np.array(found, np.int64), observers=np.array([obs[l] for l in found], np.int32))


def _as_store(store):
    """an id dict gets empty-valued descriptors and points, so that one removal serves both kinds"""
    return {k: v if isinstance(v, tuple) else entry(np.zeros((len(v), 32), np.uint8), np.zeros((len(v), 3)), v) for k, v in store.items()}


def remove_landmarks(store, ids, landmark_ids):
    """mslam_hip_kf_remove_landmarks -> (new store: every position of a listed entry whose id is listed is gone, survivors
    in order; an entry that is not listed is the same object, dict(removed [n] i32, entry_removed [n_ids] i32, n_removed))"""
    store = _as_store(store)
    lids = cr.ids_of(store)
    ids = cr._check_map(lids, ids)
    asked = [int(l) for l in np.asarray(landmark_ids).reshape(-1)]
    if any(l < 0 for l in asked):
        raise ValueError("landmark ids lie in [0, 2^63)")
    gone = set(asked)
    new, lost, held = dict(store), np.zeros(len(ids), np.int32), {}
    for p, k in enumerate(ids):
        d, w, i = entry(*store[k])
        hit = np.array([x in gone for x in i.tolist()], bool).reshape(-1)
        new[k] = (d[~hit].copy(), w[~hit].copy(), i[~hit].copy())
        lost[p] = int(hit.sum())
        for x in i[hit].tolist():
            held[x] = held.get(x, 0) + 1
    removed = np.array([held.get(l, 0) for l in asked], np.int32)
    return new, dict(removed=removed, entry_removed=lost, n_removed=int(lost.sum()))


def cull_landmarks(store, ids, cand, min_observers=2):
    """mslam_hip_kf_cull_landmarks -> (new store, dict(landmark_ids, observers, entry_removed, n_removed)): the search, then
    the removal of what it found; the counts are taken once, before anything is removed"""
    found = cull_landmarks_search(store, ids, cand, min_observers)
    new, rem = remove_landmarks(store, ids, found["landmark_ids"])
    return new, dict(found, entry_removed=rem["entry_removed"], n_removed=rem["n_removed"])


def same_search(got, ref):
    return (got["landmark_ids"].dtype == np.int64 and got["observers"].dtype == np.int32
            and np.array_equal(got["landmark_ids"], ref["landmark_ids"]) and np.array_equal(got["observers"], ref["observers"]))


# ---- the host bookkeeping ---------------------------------------------------------------------------------------------
def backend_remove_landmarks(obs, landmarks, anchor, lids):
    """HipBackend.remove_landmarks on copies -> (obs, landmarks, anchor, dict(n_observations, n_landmarks))"""
    gone = {int(l) for l in np.asarray(lids).reshape(-1)}
    new_obs, n_obs = {}, 0
    for k, (i, cam) in obs.items():
        i, cam = np.array(i, np.int64), np.array(cam, np.float64)
        hit = np.isin(i, sorted(gone)) if gone else np.zeros(len(i), bool)
        n_obs += int(hit.sum())
        new_obs[k] = (i[~hit], cam[~hit])
    n_lm = len(gone & set(landmarks))
    landmarks = {l: v for l, v in landmarks.items() if l not in gone}
    anchor = {l: v for l, v in anchor.items() if l not in gone}
    return new_obs, landmarks, anchor, dict(n_observations=n_obs, n_landmarks=n_lm)


# ---- cases ------------------------------------------------------------------------------------------------------------
def hand_case(name):
    """small id dicts with one rule each -> (lids, ids, cand, min_observers)"""
    if name == "repeat_inside":       # 7 three times in entry 1 and nowhere else: one observer, and all three positions go
        return {1: [7, 7, 8, 7], 2: [8, 9], 3: [9]}, [1, 2, 3], [1], 2
    if name == "unlisted_holder":     # entry 3 holds 5 as well, but is not listed: 5 has one observer
        return {1: [5, 6], 2: [6], 3: [5]}, [1, 2], [1], 2
    if name == "inherited":           # candidate 2 inherited 4 from entry 1 (not a candidate) and nobody else has it ...
        return {1: [4, 10], 2: [4, 11], 3: [10, 12]}, [1, 2, 3], [2], 3          # ... so at min_observers 3 it goes, from 1 too
    if name == "min_observers_1":
        return {1: [1, 2], 2: [3]}, [1, 2], [1, 2], 1
    if name == "ascending":
        return {1: [90, 5, 70, 20], 2: [20]}, [1, 2], [1], 2
    if name == "not_judged":          # 30 has one observer and no candidate holds it: it stays
        return {1: [30, 31], 2: [31, 32]}, [1, 2], [2], 2
    raise KeyError(name)


HAND_CASES = ["repeat_inside", "unlisted_holder", "inherited", "min_observers_1", "ascending", "not_judged"]


def write_scene(path, store, ids, cand, min_observers=2):
    """the scene file `mslam_harness --cull-landmarks` reads: cull_ref.write_scene's layout under a magic of its own and
    with min_observers as the only parameter: "MSLC", i32 version 1, i32 entries, i32 listed, i32 candidates, i32
    min_observers; per entry i32 id, i32 n (>= 1), n x 32 descriptor bytes, n x 3 f64 world points, n x i64 landmark ids;
    then the listed ids and the candidates as i32"""
    ids, cand = np.asarray(ids, "<i4").reshape(-1), np.asarray(cand, "<i4").reshape(-1)
    with open(path, "wb") as f:
        f.write(b"MSLC" + np.array([1, len(store), len(ids), len(cand), min_observers], "<i4").tobytes())
        for k in store:
            d, w, i = entry(*store[k])
            f.write(np.array([k, len(i)], "<i4").tobytes() + d.tobytes() + w.astype("<f8").tobytes() + i.astype("<i8").tobytes())
        f.write(ids.tobytes() + cand.tobytes())


# ---- the tracker ------------------------------------------------------------------------------------------------------
class LmCullTracker(lm.LocalMapTracker):
    """local_map_ref.LocalMapTracker with HipKeyframeTracker's landmark-culling step: every inserted keyframe (the first
    one too) joins a pending list; the keyframes inserted at least `age` insertions ago leave it, and those still in the
    map are the candidates of cull_landmarks over every keyframe."""

    def __init__(self, lm_cull=True, min_observers=2, age=2, **kw):
        super().__init__(**kw)
        self.lm_cull, self.min_observers, self.age = lm_cull, min_observers, age
        self.pending, self.inserted, self.lm_cull_results, self.unions = [], 0, [], []

    def process(self, desc, xy, depth):
        out = super().process(desc, xy, depth)
        if self.map is not None:
            self.unions.append(len(self.map[2]))          # the size of the union this frame was tracked on
        new_id = out["keyframe"]
        if self.lm_cull and new_id >= 0:
            self.inserted += 1
            self.pending.append((new_id, self.inserted))
            due = [k for k, at in self.pending if self.inserted - at >= self.age]
            self.pending = [(k, at) for k, at in self.pending if self.inserted - at < self.age]
            cands = [k for k in due if k in self.ids]
            if cands:
                listed = list(self.ids)
                full = {k: (self.store[k][0], self.store[k][1], self.lids[k]) for k in listed}
                new, res = cull_landmarks(full, listed, cands, self.min_observers)
                for k in listed:
                    self.store[k], self.lids[k] = (new[k][0], new[k][1]), new[k][2]
                if res["n_removed"] > 0:
                    self._map_of = None
                self.lm_cull_results.append(dict(keyframe=new_id, listed=listed, candidates=cands, landmark_ids=res["landmark_ids"],
                                                 n_removed=res["n_removed"]))
        return out


SEQ_ARGS = dict(seed=5, n_frames=16, n_landmarks=900, n_distractors=200)
DEPTH = cr.WALK_DEPTH
PARAMS = cr.WALK_PARAMS

_SEQ, _RUNS = [], {}


def sequence():
    """track_ref.make_sequence(**SEQ_ARGS): 16 frames in which every frame becomes a keyframe (PARAMS) and every keyframe
    adds some hundred part-B landmarks, most of them distractors nobody sees again; built once"""
    if not _SEQ:
        _SEQ.append(tr.make_sequence(**SEQ_ARGS))
    return _SEQ[0]


def run(lm_cull=True):
    """the CPU tracker over sequence() -> (rows, tracker); computed once per mode and left unchanged"""
    if lm_cull not in _RUNS:
        seq = sequence()
        trk = LmCullTracker(lm_cull=lm_cull, depth=DEPTH, cam=seq["cam"], **PARAMS)
        _RUNS[lm_cull] = ([trk.process(fr["desc"], fr["xy"], fr["depth"]) for fr in seq["frames"]], trk)
    return _RUNS[lm_cull]
