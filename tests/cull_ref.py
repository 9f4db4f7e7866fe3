"""Keyframe culling restated in numpy from the statement in include/mslam_hip.h (not from the kernels): the reference the
CPU, GPU and host tests of mslam_hip_kf_observers, mslam_hip_kf_cull_search, mslam_hip_kf_cull, HipBackend.remove_keyframe
and HipKeyframeTracker(kf_cull=True) compare with.  The model is ORB-SLAM's KeyFrameCulling; the reference has the removal
primitives (BasicMap::removeKeyframe, basic_map.cpp:110-115) and no policy.  Also the hand cases, the random stores, the
scene file of `mslam_harness --cull`, a CPU tracker with culling and the walk the tracker tests run.

A store is prune_ref's: entry id -> (descriptors [n, 32] u8, world points [n, 3] f64, landmark ids [n] i64); where only the
ids matter, a dict entry id -> landmark ids."""
import numpy as np

import local_map_ref as lm
import prune_ref as pr
import track_ref as tr

CHUNK = 64        # listed entries per counting launch (kCullChunk in csrc/k_cull.hip)
STRIDE = 1024     # the greedy workgroup's stride over an entry (kCullThreads)
MAX_ENTRIES = 4096

entry = pr.entry


def ids_of(store):
    """a store or an id dict -> entry id -> landmark ids [n] i64"""
    return {k: np.asarray(v[2] if isinstance(v, tuple) else v, np.int64).reshape(-1) for k, v in store.items()}


def _check_map(lids, ids):
    ids = [int(k) for k in np.asarray(ids).reshape(-1)]
    if not 1 <= len(ids) <= MAX_ENTRIES or len(set(ids)) != len(ids):
        raise ValueError("1 to %d distinct listed ids" % MAX_ENTRIES)
    for k in ids:
        if k not in lids:
            raise KeyError(k)
    return ids


def obs_counts(lids, ids):
    """obs(l) for every landmark id some listed entry holds: the number of listed entries that hold it at one position at
    least (a repeat inside an entry counts once)"""
    obs = {}
    for k in ids:
        for l in set(lids[k].tolist()):
            obs[l] = obs.get(l, 0) + 1
    return obs


def observers(store, ids, landmark_ids):
    """mslam_hip_kf_observers -> counts [n] i32"""
    lids = ids_of(store)
    ids = _check_map(lids, ids)
    asked = [int(l) for l in np.asarray(landmark_ids).reshape(-1)]
    if any(l < 0 for l in asked):
        raise ValueError("landmark ids lie in [0, 2^63)")
    obs = obs_counts(lids, ids)
    return np.array([obs.get(l, 0) for l in asked], np.int32)


def cull_search(store, ids, cand, min_observers=3, ratio=0.9, min_landmarks=1):
    """mslam_hip_kf_cull_search -> dict(culled [n_cand] bool, n_landmarks, n_redundant [n_cand] i32, n_culled)"""
    lids = ids_of(store)
    ids = _check_map(lids, ids)
    cand = [int(k) for k in np.asarray(cand).reshape(-1)]
    if len(set(cand)) != len(cand) or not set(cand) <= set(ids):
        raise ValueError("the candidates are distinct listed ids")
    if not 1 <= min_observers <= 65535 or not 0.0 <= ratio <= 1.0 or min_landmarks < 1:      # (a NaN ratio fails the chain)
        raise ValueError("min_observers in 1..65535, ratio in [0, 1], min_landmarks >= 1")
    obs = obs_counts(lids, ids)
    culled, nl, nr = np.zeros(len(cand), bool), np.zeros(len(cand), np.int32), np.zeros(len(cand), np.int32)
    for c, k in enumerate(cand):
        D = set(lids[k].tolist())
        nl[c] = len(D)
        nr[c] = sum(obs[l] - 1 >= min_observers for l in D)
        culled[c] = nl[c] >= min_landmarks and float(nr[c]) > ratio * float(nl[c])
        if culled[c]:
            for l in D:
                obs[l] -= 1
    return dict(culled=culled, n_landmarks=nl, n_redundant=nr, n_culled=int(culled.sum()))


def cull(store, ids, cand, **kw):
    """mslam_hip_kf_cull -> (new store: the culled entries are gone, every other entry is the same object, the result)"""
    res = cull_search(store, ids, cand, **kw)
    gone = {int(k) for k, c in zip(np.asarray(cand).reshape(-1), res["culled"]) if c}
    return {k: v for k, v in store.items() if k not in gone}, res


def same_result(got, ref):
    return (np.array_equal(got["culled"], ref["culled"]) and np.array_equal(got["n_landmarks"], ref["n_landmarks"])
            and np.array_equal(got["n_redundant"], ref["n_redundant"]) and got["n_culled"] == ref["n_culled"])


# ---- the host bookkeeping ---------------------------------------------------------------------------------------------
def backend_remove_keyframe(poses, obs, landmarks, anchor, first, id):
    """HipBackend.remove_keyframe on copies -> (poses, obs, landmarks, anchor, dict(n_observations, orphans)); the first
    keyframe and an unknown id raise ValueError"""
    if id not in poses or id == first:
        raise ValueError(id)
    poses = {k: np.array(v) for k, v in poses.items() if k != id}
    mine = set(np.asarray(obs[id][0]).tolist())
    n = len(obs[id][0])
    obs = {k: (np.array(v[0], np.int64), np.array(v[1], np.float64)) for k, v in obs.items() if k != id}
    landmarks, anchor, orphans = dict(landmarks), dict(anchor), []
    for l in sorted(mine):
        who = sorted(k for k in obs if l in set(obs[k][0].tolist()))
        if not who:
            landmarks.pop(l, None)
            anchor.pop(l, None)
            orphans.append(l)
        elif anchor.get(l) == id:
            anchor[l] = who[0]
    return poses, obs, landmarks, anchor, dict(n_observations=n, orphans=orphans)


def connected(graph, a, b):
    seen, stack = {a}, [a]
    while stack:
        for m in graph[stack.pop()]:
            if m not in seen:
                seen.add(m)
                stack.append(m)
    return b in seen


def is_connected(graph):
    nodes = sorted(graph)
    return all(connected(graph, nodes[0], n) for n in nodes[1:])


def remove_graph_node(graph, k):
    """the bridging rule on a copy: node k and its edges go; every former neighbour, ascending, that has no path left to the
    smallest former neighbour gets an edge to it -> (graph, bridges)"""
    nbrs = sorted(graph[k])
    graph = {n: set(v) - {k} for n, v in graph.items() if n != k}
    bridges = []
    for n in nbrs[1:]:
        if not connected(graph, n, nbrs[0]):
            graph[n].add(nbrs[0])
            graph[nbrs[0]].add(n)
            bridges.append((n, nbrs[0]))
    return graph, bridges


# ---- cases ------------------------------------------------------------------------------------------------------------
def store_of(lids, seed=0):
    """a store with random descriptors and points around an id dict"""
    rng = np.random.default_rng(seed)
    return {k: entry(rng.integers(0, 256, (len(v), 32), dtype=np.uint8), rng.normal(size=(len(v), 3)), v) for k, v in lids.items()}


def hand_case(name):
    """small id dicts with one rule each -> (lids, ids, cand, kw)"""
    r = lambda a, b: list(range(a, b))
    if name == "repeat_inside":         # id 7 three times in entry 1: one observer, and one landmark of entry 1
        return {1: [7, 7, 8, 7], 2: [7, 9], 3: [8]}, [1, 2, 3], [1], dict(min_observers=1, ratio=0.5)
    if name == "min_observers_at":      # id 5 has exactly 3 other observers, id 6 two
        return {1: [5, 6], 2: [5, 6], 3: [5, 6], 4: [5]}, [1, 2, 3, 4], [1], dict(min_observers=3, ratio=0.4)
    if name == "ratio_9_of_10":         # 9 redundant of 10: 9 > 0.9 * 10 is false
        return {1: r(0, 10), 2: r(0, 9), 3: r(0, 9), 4: r(0, 9)}, [1, 2, 3, 4], [1], {}
    if name == "ratio_91_of_100":
        return {1: r(0, 100), 2: r(0, 91), 3: r(0, 91), 4: r(0, 91)}, [1, 2, 3, 4], [1], {}
    if name == "mutual_pair":           # 1 and 2 each need the other as the third observer
        return {1: r(0, 20), 2: r(0, 20), 3: r(0, 20), 4: r(0, 20)}, [1, 2, 3, 4], [1, 2], {}
    if name == "mutual_pair_reversed":
        return {1: r(0, 20), 2: r(0, 20), 3: r(0, 20), 4: r(0, 20)}, [1, 2, 3, 4], [2, 1], {}
    if name == "empty_candidate":
        return {1: [], 2: r(0, 5), 3: r(0, 5)}, [1, 2, 3], [1, 2], dict(min_observers=1, ratio=0.0)
    if name == "min_landmarks":         # entry 1 is wholly redundant and too small to judge; entry 2 has just enough
        return {1: r(0, 4), 2: r(0, 5), 3: r(0, 5), 4: r(0, 5), 5: r(0, 5)}, [1, 2, 3, 4, 5], [1, 2], dict(min_landmarks=5)
    raise KeyError(name)


HAND_CASES = ["repeat_inside", "min_observers_at", "ratio_9_of_10", "ratio_91_of_100", "mutual_pair", "mutual_pair_reversed",
              "empty_candidate", "min_landmarks"]


def chain_case(n=8, width=10):
    """a chain in which every cull changes the next decision: candidate c holds the id blocks A_c and A_(c+1) (`width` ids
    each); two keepers hold every block and a third holds A_0 and A_n.  So block A_c (0 < c < n) has exactly three other
    observers for candidate c while candidate c - 1 is there, and two once it has gone: with the defaults the candidates go
    and stay in turn, and without the greedy update all of them would go -> (lids, ids, cand, kw, the expected flags)"""
    block = lambda c: list(range(c * width, (c + 1) * width))
    lids = {100 + c: block(c) + block(c + 1) for c in range(n)}
    every = [l for c in range(n + 1) for l in block(c)]
    lids.update({200: every, 201: every[::-1], 202: block(0) + block(n)})
    return lids, sorted(lids), [100 + c for c in range(n)], {}, [c % 2 == 0 for c in range(n)]


def random_case(seed, sizes, pool=None, repeats=0.1, first_id=100):
    """a store of len(sizes) entries whose ids are drawn from one pool (so that observer counts spread from 1 to many), with
    a fraction of positions repeating an id of the same entry -> the store"""
    rng = np.random.default_rng(seed)
    pool = int(pool if pool is not None else max(2 * max(sizes + [1]), 64))
    store = {}
    for e, n in enumerate(sizes):
        n_own = min(n, pool)
        l = rng.choice(pool, size=n_own, replace=False).astype(np.int64) if n_own else np.zeros(0, np.int64)
        if n > n_own:
            l = np.concatenate([l, rng.choice(l, size=n - n_own)])
        rep = np.flatnonzero(rng.random(n) < repeats)
        if n > 1 and len(rep):
            l[rep] = l[rng.integers(0, n, len(rep))]
        store[first_id + e] = entry(rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.normal(size=(n, 3)), l)
    return store


def write_scene(path, store, ids, cand, min_observers=3, ratio=0.9, min_landmarks=1):
    """the scene file `mslam_harness --cull` reads: "MSCL", i32 version 1, i32 entries, i32 listed, i32 candidates, i32
    min_observers, i32 min_landmarks, f64 ratio; per entry i32 id, i32 n (>= 1), n x 32 descriptor bytes, n x 3 f64 world
    points, n x i64 landmark ids; then the listed ids and the candidates as i32"""
    ids, cand = np.asarray(ids, "<i4").reshape(-1), np.asarray(cand, "<i4").reshape(-1)
    with open(path, "wb") as f:
        f.write(b"MSCL" + np.array([1, len(store), len(ids), len(cand), min_observers, min_landmarks], "<i4").tobytes())
        f.write(np.array([ratio], "<f8").tobytes())
        for k in store:
            d, w, i = entry(*store[k])
            f.write(np.array([k, len(i)], "<i4").tobytes() + d.tobytes() + w.astype("<f8").tobytes() + i.astype("<i8").tobytes())
        f.write(ids.tobytes() + cand.tobytes())


# ---- the tracker ------------------------------------------------------------------------------------------------------
class CullTracker(lm.LocalMapTracker):
    """local_map_ref.LocalMapTracker with HipKeyframeTracker's culling step: after a keyframe was inserted and its edges
    were added, the neighbours of the new keyframe (HipBackend.neighbours: getNeighbourKeyframes with deepLevel 1, the 64
    largest ids, ascending) without the new keyframe, the reference and keyframe 0 are judged by cull_search over every
    keyframe; a culled one leaves the store, the ids and, with the bridging rule, the graph."""

    def __init__(self, cull=True, min_observers=3, ratio=0.9, **kw):
        super().__init__(**kw)
        self.cull, self.min_observers, self.cull_ratio, self.cull_results = cull, min_observers, ratio, []

    def process(self, desc, xy, depth):
        out = super().process(desc, xy, depth)
        new_id = out["keyframe"]
        if self.cull and new_id > 0:
            keep = {new_id, self.reference, 0}
            cands = [k for k in sorted(lm.neighbours(self.graph, new_id, 1))[-64:] if k not in keep]
            if cands:
                listed = list(self.ids)
                res = cull_search(self.lids, listed, cands, self.min_observers, self.cull_ratio)
                gone, bridges = [k for k, c in zip(cands, res["culled"]) if c], []
                for k in gone:
                    self.ids.remove(k)
                    del self.store[k], self.lids[k]
                    self.graph, b = remove_graph_node(self.graph, k)
                    bridges += b
                if gone:
                    self._map_of = None
                self.cull_results.append(dict(keyframe=new_id, listed=listed, candidates=cands, culled=gone,
                                              n_landmarks=res["n_landmarks"].tolist(), n_redundant=res["n_redundant"].tolist(),
                                              bridges=bridges))
        return out


WALK_PARAMS = dict(new_keyframe_min_landmarks=10000)   # out of reach: every tracked frame becomes a keyframe, as for a camera
WALK_DEPTH = 2                                         # whose tracking stays thin; a landmark is then seen by five or six


def triple_walk():
    """track_ref.make_sequence's wall, thinned, with next to no distractors (a distractor with a depth becomes a landmark
    nobody sees again, and a keyframe full of those is never redundant); the camera goes over the first stretch of the way
    out, back over it and out over it again (25 frames).  With WALK_PARAMS the keyframes in the middle of a run of
    keyframes become redundant on every pass (measured on the CPU tracker: 16 of 25 are culled, every frame is tracked)
    -> dict(frames, cam, width, height)"""
    seq = tr.make_sequence(seed=5, n_frames=32, n_landmarks=900, n_distractors=8)
    out = seq["frames"][:9]
    seq["frames"] = out + out[-2::-1] + out[1:]
    return seq


def run_walk(seq, cull=True, **kw):
    params = dict(WALK_PARAMS)
    params.update(kw)
    trk = CullTracker(cull=cull, depth=WALK_DEPTH, cam=seq["cam"], **params)
    rows = [trk.process(fr["desc"], fr["xy"], fr["depth"]) for fr in seq["frames"]]
    return rows, trk
