"""Inputs of the match-to-PnP sequence's edge tests (not a test): each builder plants one condition the natural scenes of
the relocalize / track / track_window tests never meet — landmark twins and an entry cut at the store's capacity, one to
seven correspondences, rows without slack, keypoint indices in the upper half of the `used` bitmap, rankings without a
winner — out of tests/reloc_ref.py's scene and tests/track_ref.py's sequence, in numpy alone.  tests/test_seq_edge_cases.py
proves on the CPU references that every builder meets the condition it is named for; tests/test_gpu_seq_edges.py runs the
same inputs on the device.  A reference result is computed once per input (`ref`) and shared."""
import numpy as np

import reloc_ref as rr
import track_ref as tr
import track_window_ref as twr

CAM = tr.CAM
BIG = 10 ** 6                      # a new_keyframe_min_landmarks no inlier count reaches: every tracked frame requires a keyframe
IDENTITY = (np.eye(3), np.zeros(3))

_CACHE = {}


def ref(key, make):
    """the value of make(), computed once per key"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- A / B: twins and the cut at the store's capacity ----------------------------------------------------------------

def twin_sequence():
    return ref("twin sequence", lambda: tr.make_sequence(n_frames=8, n_landmarks=600, n_distractors=100))


def first_entry(fr, z_max=3.0):
    """initFirstKeyframe at the identity pose: (desc, world, landmark number per row) of the frame's lift"""
    xyz, valid = tr._oracle().backproject(fr["depth"], fr["xy"], tr.FACTOR, CAM[:2], CAM[2:])
    d, w = rr.lift(fr["desc"], xyz, valid, np.eye(3), np.zeros(3), z_max)
    keep = (valid != 0) & (xyz[:, 2] <= z_max)
    return d, w, fr["landmark"][keep]


def twin_case(copies):
    """Frame 1 of the sequence against `copies` copies of keyframe 0's landmarks in one entry, under distinct landmark ids
    (what a loop closure without fusion leaves in a local map): every keypoint that matches is named by `copies` landmarks,
    part A lists it that often, and parts A and B together exceed the keypoint count nq.  The context's max_keypoints K is
    nq, so three copies are cut at K.  The store rejects an entry above K, so the copies are of the landmarks frame 1 sees
    (the others match nothing and change no pair).
    -> dict(frames, store = {0: entry}, lids, K, frame, next = the first K keypoints of frame 2, seed, guess)"""
    seq = twin_sequence()
    f0, f1, f2 = seq["frames"][:3]
    d, w, lm = first_entry(f0)
    seen = np.isin(lm, f1["landmark"][f1["landmark"] >= 0])
    d, w = np.concatenate([d[seen]] * copies), np.concatenate([w[seen]] * copies)
    K = len(f1["desc"])
    nxt = dict(desc=f2["desc"][:K].copy(), xy=f2["xy"][:K].copy(), depth=f2["depth"])      # frame 2 has more keypoints than K
    return dict(frames=seq["frames"], store={0: (d, w)}, lids=1000 + np.arange(len(d), dtype=np.int64), K=K, frame=f1, next=nxt,
                seed=1, guess=IDENTITY)


def twin_track(copies, capacity="K"):
    """the reference step of twin_case(copies); capacity "K": the entry cut at the case's K, None: uncut"""
    def make():
        tc = twin_case(copies)
        fr = tc["frame"]
        return tr.track(fr["desc"], fr["xy"], fr["depth"], tc["store"], 0, [0], seed=tc["seed"], guess=tc["guess"],
                        new_keyframe_min_landmarks=BIG, capacity=tc["K"] if capacity == "K" else None)
    return ref(("twin track", copies, capacity), make)


def twin_window():
    """Three frames against the three-copy entry of twin_case whose event is frame 1: frame 0 of the sequence sees every
    copied landmark and stays above new_keyframe_min_landmarks, frame 1 (twin_case's frame, with the seed it has there)
    falls below and requires the keyframe, so the entry is built from row 1 of every per-frame array; frame 6 follows.
    Every frame has at most K keypoints.  -> dict(frames, kf_min, seed, guess, steps, first, entry (uncut))"""
    def make():
        tc = twin_case(3)
        fr = [tc["frames"][0], tc["frames"][1], tc["frames"][6]]
        kf_min = twin_track(3)["n_inliers"] + 1
        steps, first, entry = twr.track_window([x["desc"] for x in fr], [x["xy"] for x in fr], [x["depth"] for x in fr], tc["store"],
                                               0, [0], 0, seed=tc["seed"] - 1, guess=tc["guess"], new_keyframe_min_landmarks=kf_min)
        return dict(frames=fr, kf_min=kf_min, seed=tc["seed"] - 1, guess=tc["guess"], steps=steps, first=first, entry=entry)
    return ref("twin window", make)


# ---- C: k correspondences -----------------------------------------------------------------------------------------------

def few_scene():
    return ref("few scene", lambda: rr.make_scene(seed=4))


def few_full():
    """the ordinary call that precedes the small ones: it leaves a mask row of ones in the scratch"""
    sc = few_scene()
    return ref("few full", lambda: rr.relocalize(sc["desc"], sc["xy"], sc["store"], [sc["target_id"]], seed=1))


def few_valid(k):
    """a keypoint mask with ones at the keypoints of the first k matches of the target alone"""
    sc = few_scene()
    v = np.zeros(len(sc["desc"]), bool)
    v[few_full()["candidates"][0]["pairs"][0][:k]] = True
    return v


def few_ref(k):
    sc = few_scene()
    return ref(("few", k), lambda: rr.relocalize(sc["desc"], sc["xy"], sc["store"], [sc["target_id"]], valid=few_valid(k), seed=1))


def few_depth(k):
    """Frame 1 of the twin sequence with a depth image that is valid at k of its keypoints only: those of the first k
    matches against keyframe 0's plain entry (landmark keypoints: one per pixel).
    -> dict(store, frame (with that depth), ref = the reference step with the vote list [0])"""
    def make():
        seq = twin_sequence()
        d, w, _ = first_entry(seq["frames"][0])
        store, f1 = {0: (d, w)}, seq["frames"][1]
        fi, _ = rr.match(f1["desc"], d)
        xyz, valid = tr._oracle().backproject(f1["depth"], f1["xy"], tr.FACTOR, CAM[:2], CAM[2:])
        pick = [i for i in fi if valid[i]][:k]
        depth = np.zeros_like(f1["depth"])
        for i in pick:
            x, y = int(f1["xy"][i, 0]), int(f1["xy"][i, 1])
            depth[y, x] = f1["depth"][y, x]
        fr = dict(f1, depth=depth)
        step = tr.track(fr["desc"], fr["xy"], depth, store, 0, [0], seed=1, guess=IDENTITY, new_keyframe_min_landmarks=BIG)
        return dict(store=store, frame=fr, ref=step)
    return ref(("few depth", k), make)


# ---- D: full and adjacent rows ------------------------------------------------------------------------------------------

FULL_SIZES = (255, 256, 257, 512)
# which matches of candidate 0 lose their keypoint: whole waves, whole 256-chunks, every other one, all, all but the last
VALID_PATTERNS = ("wave0", "chunk_64_319", "alternate", "none", "last_only")


def full_rows(n, n_cand):
    """n_cand entries that are slices of the query's own descriptors, q[j : j + n] (offsets 0 and 100 for two candidates,
    0 .. 63 for 64) with random world points: every landmark finds its keypoint at distance 0, so each candidate has
    exactly n matches — n = 256 and 512 fill a row of the 256-block stride, and the next candidate's row lies directly
    behind it.  -> dict(desc, xy, store, ids)"""
    sc = few_scene()
    rng = np.random.default_rng(1000 + n)
    offs = (0, 100) if n_cand == 2 else tuple(range(n_cand))
    store = {j: (sc["desc"][o:o + n].copy(), np.stack([rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.uniform(2, 6, n)], 1))
             for j, o in enumerate(offs)}
    return dict(desc=sc["desc"], xy=sc["xy"], store=store, ids=list(range(n_cand)), offsets=offs)


def full_ref(n, n_cand, pattern=None, seed=3):
    case = full_rows(n, n_cand)
    v = None if pattern is None else pattern_valid(n, pattern)
    return ref(("full", n, n_cand, pattern), lambda: rr.relocalize(case["desc"], case["xy"], case["store"], case["ids"], valid=v, seed=seed))


def pattern_valid(n, pattern):
    """the keypoint mask that switches off the matches of candidate 0 (of full_rows(n, 2)) the pattern names"""
    fi = full_ref(n, 2)["candidates"][0]["pairs"][0]
    m = len(fi)
    off = {"wave0": np.arange(m) < 64, "chunk_64_319": (np.arange(m) >= 64) & (np.arange(m) < 320), "alternate": np.arange(m) % 2 == 1,
           "none": np.ones(m, bool), "last_only": np.arange(m) < m - 1}[pattern]
    v = np.ones(len(few_scene()["desc"]), bool)
    if pattern in ("none", "last_only"):
        v[:] = False
        v[fi[~off]] = True
    else:
        v[fi[off]] = False
    return v


# ---- F: z == z_max in part B of a track entry ---------------------------------------------------------------------------

def zmax_case():
    """Frame 1 of the twin sequence against keyframe 0's plain entry, a keyframe required; i = a keypoint of part B (z_max =
    3 m) and z = its depth: with z_max = z it is lifted, with the next double below z it is not.
    -> dict(store, frame, ref = the reference step at 3 m, i, z)"""
    def make():
        seq = twin_sequence()
        d, w, _ = first_entry(seq["frames"][0])
        store, f1 = {0: (d, w)}, seq["frames"][1]
        step = tr.track(f1["desc"], f1["xy"], f1["depth"], store, 0, [0], seed=1, guess=IDENTITY, new_keyframe_min_landmarks=BIG)
        e = step["entry"]
        i = int(e["kp"][e["n_inherited"] + (len(e["kp"]) - e["n_inherited"]) // 2])
        return dict(store=store, frame=f1, ref=step, i=i, z=float(step["xyz"][i, 2]))
    return ref("zmax", make)


def zmax_entry(z_max, R=None, t=None, pairs=None, mask=None):
    """the entry of zmax_case at another z_max, from the reference step or from a device's own pairs, mask and pose"""
    zc = zmax_case()
    st, fr = zc["ref"], zc["frame"]
    return tr.build_entry(fr["desc"], st["xyz"], st["valid"], st["pairs"] if pairs is None else pairs, st["mask"] if mask is None else mask,
                          zc["store"][0][1], st["R"] if R is None else R, st["t"] if t is None else t, z_max)


# ---- G: the upper half of the `used` bitmap ---------------------------------------------------------------------------

def upper_used():
    """A query of 33000 keypoints — random distractors first, then the keypoints of a view of a 200-landmark entry, so
    every matched keypoint has an index >= 32768 — with a depth image that is valid everywhere (1 .. 4 m across the
    columns: z_max = 3 m cuts part B) and a keyframe required.  K = 33024.
    -> dict(desc, xy, depth, store, K, ref = the reference step)"""
    def make():
        sc = rr.make_scene(seed=9, n_kf=1, n_landmarks=200, target=0, n_distractors=20)
        rng = np.random.default_rng(10)
        lead = 33000 - len(sc["desc"])
        desc = np.concatenate([rng.integers(0, 256, (lead, 32), dtype=np.uint8), sc["desc"]])
        xy = np.concatenate([rng.uniform(0, [640, 480], (lead, 2)).astype(np.float32), sc["xy"]])
        depth = np.tile((np.linspace(1.0, 4.0, 640) * 5000).astype(np.uint16), (480, 1))
        store = {0: sc["store"][sc["target_id"]]}
        step = tr.track(desc, xy, depth, store, 0, [0], seed=2, new_keyframe_min_landmarks=BIG, capacity=33024)
        return dict(desc=desc, xy=xy, depth=depth, store=store, K=33024, lead=lead, ref=step)
    return ref("upper used", make)


# ---- H: ranking -------------------------------------------------------------------------------------------------------------

def ranking_store():
    """the scene's keyframes plus 64 small unrelated ones (ids 200 ..): candidates without a model"""
    def make():
        sc = few_scene()
        rng = np.random.default_rng(12)
        store = dict(sc["store"])
        for i in range(64):
            n = 20 + i
            store[200 + i] = (rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.normal(size=(n, 3)) + [0, 0, 4])
        return store
    return ref("ranking store", make)


def ranking_ref(name):
    """-> (candidate ids, min_inliers, reference result).  "no_model": 64 candidates, none with a model; "last": the only
    model at position 63; "at_min" / "below_min": that list with min_inliers at / one above the winner's inlier count"""
    sc, store = few_scene(), ranking_store()
    cand = [200 + i for i in range(64)]
    if name != "no_model":
        cand[63] = sc["target_id"]
    base = ref(("ranking", "last"), lambda: rr.relocalize(sc["desc"], sc["xy"], store, cand[:63] + [sc["target_id"]], seed=5))
    n_in = base["candidates"][63]["n_inliers"]
    min_inliers = {"no_model": 60, "last": 60, "at_min": n_in, "below_min": n_in + 1}[name]
    if name == "last":
        return cand, min_inliers, base
    return cand, min_inliers, ref(("ranking", name), lambda: rr.relocalize(sc["desc"], sc["xy"], store, cand, seed=5, min_inliers=min_inliers))


# ---- E: a query with a known pose for an entry the test has read back ----------------------------------------------

def query_of_entry(desc, world, seed=0, n_distractors=200, flip=6, width=640, height=480, cam=CAM):
    """a view of the landmarks (desc, world) from a small known pose: their projections that fall into the frame, with
    `flip` flipped descriptor bits, plus random keypoints, shuffled -> (desc, xy)"""
    rng = np.random.default_rng(seed)
    R, t = rr.po.rodrigues([0.02, -0.03, 0.01]), np.array([0.05, -0.02, 0.04])
    img, front = rr.po.project(R, t, np.asarray(world, np.float32).astype(np.float64), cam)
    inside = front & (img[:, 0] >= 0) & (img[:, 0] < width) & (img[:, 1] >= 0) & (img[:, 1] < height)
    qd = np.concatenate([rr._flip_bits(rng, np.asarray(desc)[inside], flip), rng.integers(0, 256, (n_distractors, 32), dtype=np.uint8)])
    qxy = np.concatenate([img[inside], rng.uniform(0, [width, height], (n_distractors, 2))]).astype(np.float32)
    perm = rng.permutation(len(qd))
    return qd[perm].copy(), qxy[perm].copy()
