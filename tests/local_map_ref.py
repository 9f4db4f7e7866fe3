"""Reference restatement of local-map tracking (not a test): landmark ids, the union of the most recent observations
(RecentObservationsVisitor, rgbd_feature_frontend.cpp:57-80, as getLandmarksWithKeypoints uses it, :256-277), covisibility
(BasicMap::updateCovisibility, basic_map.cpp:141-164), the neighbourhood (BasicMap::getNeighbourKeyframes, :209-237) and the
loop of tests/track_ref.py::KeyframeTracker run against the local map instead of the reference keyframe's own entry.
Plain numpy and dicts; shares no code with the product.

A store is track_ref's {id: (desc [n, 32] u8, world [n, 3] f64)} plus a second dict {id: landmark ids [n] i64}."""
from collections import deque

import numpy as np

import reloc_ref as rr
import track_ref as tr

FRESH_BIT = 1 << 62
LOCAL_MAP_ID = 0x7fffffff


def fresh_ids(serial, n, first=0):
    """the ids an entry made under creation serial `serial` gives its landmarks at positions first .. first + n - 1"""
    return np.array([FRESH_BIT | (serial << 16) | p for p in range(first, first + n)], np.int64)


def union(store, lids, ids):
    """One landmark per distinct landmark id of the listed entries: the observation of the listed entry with the largest id
    (inside it, the highest position), ordered by the winning entry's position in `ids`, then by landmark position.
    -> (desc, world, landmark ids)"""
    assert len(set(ids)) == len(ids)
    best = {}                                     # landmark id -> (keyframe id, position, list position)
    for k, kf in enumerate(ids):
        for i, l in enumerate(np.asarray(lids[kf]).tolist()):
            if l not in best or (kf, i) > best[l][:2]:
                best[l] = (kf, i, k)
    win = sorted((k, i, kf) for kf, i, k in best.values())
    desc = np.array([store[kf][0][i] for _, i, kf in win], np.uint8).reshape(-1, 32)
    world = np.array([store[kf][1][i] for _, i, kf in win], np.float64).reshape(-1, 3)
    lid = np.array([lids[kf][i] for _, i, kf in win], np.int64).reshape(-1)
    return desc, world, lid


def covisible(lids, id, ids):
    """per listed entry: how many distinct landmark ids of entry `id` it holds as well"""
    own = set(np.asarray(lids[id]).tolist())
    return np.array([len(own & set(np.asarray(lids[k]).tolist())) for k in ids], np.int32)


def neighbours(graph, ref, depth):
    """getNeighbourKeyframes: a queue of (keyframe, level) from (ref, 0); a popped keyframe joins the result, and while
    level <= depth its neighbours that are not in the result yet are pushed with level + 1.  Nodes at level `depth` are
    still expanded, so the result reaches depth + 1 hops: the reference's behaviour, kept."""
    result, queue = set(), deque([(ref, 0)])
    while queue:
        cur, level = queue.popleft()
        result.add(cur)
        if level <= depth and cur in graph:
            for nb in sorted(graph[cur]):
                if nb not in result:
                    queue.append((nb, level + 1))
    return result


class LocalMapTracker(tr.KeyframeTracker):
    """track_ref.KeyframeTracker with landmark ids and, for depth != None, the covisibility graph and the local map: each
    frame is tracked against the union of the reference keyframe's neighbourhood (the 64 largest ids of it), rebuilt when
    the reference changed or a keyframe was added; a new keyframe gets an edge to every member of that local map it shares
    a landmark with.  depth = None is KeyframeTracker itself.  The creation serial advances as the library's does: once per
    entry made, per union built and per track step (which always names a new id)."""

    def __init__(self, depth=None, **kw):
        super().__init__(**kw)
        self.depth, self.lids, self.graph, self.serial = depth, {}, {}, 0
        self.local, self._map_of, self.map = [], None, None

    def process(self, desc, xy, depth):
        desc = np.asarray(desc, np.uint8).reshape(-1, 32)
        if self.reference is None:
            out = super().process(desc, xy, depth)
            self.serial += 1
            self.lids[0], self.graph[0] = fresh_ids(self.serial, len(self.store[0][0])), set()
            out["n_correspondences"] = 0
            return out
        seed = self.seed + self.frame
        self.frame += 1
        ids = self.ids[-64:]
        store, ref_id = self.store, self.reference
        if self.depth is not None:
            if self._map_of != self.reference:
                self.local = sorted(neighbours(self.graph, self.reference, self.depth))[-64:]
                self.serial += 1
                self.map, self._map_of = union(self.store, self.lids, self.local), self.reference
            store = dict(self.store)
            store[LOCAL_MAP_ID] = self.map[:2]
            ref_id = LOCAL_MAP_ID
        ref_lids = self.map[2] if self.depth is not None else self.lids[self.reference]
        s = tr.track(desc, xy, depth, store, ref_id, ids, self.cam, self.factor, self.ratio, self.iterations, self.thr, seed,
                     (self.R, self.t), self.min_matched_points, self.new_keyframe_min_landmarks, self.z_max)
        self.serial += 1
        out = dict(tracked=s["tracked"], n_inliers=s["n_inliers"], n_correspondences=s["n_correspondences"], keyframe=-1,
                   relocalized=False)
        if s["tracked"]:
            self.R, self.t = s["R"], s["t"]
            if s["vote_best"] >= 0:
                self.reference = ids[s["vote_best"]]
            if s["entry"] is not None:
                e, new_id = s["entry"], self.ids[-1] + 1
                na = e["n_inherited"]
                self.store[new_id] = (e["desc"], e["world"])
                self.lids[new_id] = np.concatenate([ref_lids[e["src"][:na]], fresh_ids(self.serial, len(e["kp"]) - na, na)])
                self.ids.append(new_id)
                self.reference = out["keyframe"] = new_id
                if self.depth is not None:
                    self.graph[new_id] = set()
                    for other, n in zip(self.local, covisible(self.lids, new_id, self.local)):
                        if n > 0 and other != new_id:
                            self.graph[new_id].add(other)
                            self.graph[other].add(new_id)
                    self._map_of = None
        else:
            best = rr.relocalize(desc, xy, self.store, ids, self.cam, ratio=self.ratio, iterations=self.iterations, thr=self.thr,
                                 seed=seed, min_inliers=self.reloc_min_inliers)["best"]
            if best >= 0:
                self.reference, out["relocalized"] = ids[best], True
        out.update(R=self.R.copy(), t=self.t.copy(), reference=self.reference)
        return out


def run(seq, depth, **kw):
    """the loop over a sequence -> (rows, tracker), as track_ref.run_reference"""
    params = dict(tr.SEQ_PARAMS)
    params.update(kw)
    trk = LocalMapTracker(depth=depth, cam=seq["cam"], **params)
    rows = [trk.process(fr["desc"], fr["xy"], fr["depth"]) for fr in seq["frames"]]
    return rows, trk


# ---- the behavioural scene -------------------------------------------------------------------------------------------------

def make_scene():
    """track_ref.make_sequence's wall and camera, cut to the way out (the first frames of a longer sequence) and thinned to
    keep the numpy loop quick.  Keyframe 1 is inserted while most of keyframe 0's landmarks are still in view, but it
    inherits only those that were inlier correspondences in its frame: a landmark whose depth was missing there (8 % of
    them, drawn per frame) or that RANSAC left out stays keyframe 0's alone.  The frames after it see landmarks of both."""
    seq = tr.make_sequence(seed=3, n_frames=32, n_landmarks=900, n_distractors=150)
    seq["frames"] = seq["frames"][:12]
    return seq
