"""Inputs the window-tracking tests share (not a test): windows cut from track_ref.make_sequence(seed=0) at states of the
reference loop, each planted to produce one event kind at one position, and the small 64 x 48 scene of the scan-width tests.
tests/test_track_window.py proves on the CPU reference that every case produces what it claims; tests/test_gpu_track_window.py
runs the same inputs on the device."""
import numpy as np

import reloc_ref as rr
import track_ref as tr
import track_window_ref as twr
from reloc_ref import po

KF_MIN = tr.SEQ_PARAMS["new_keyframe_min_landmarks"]

# the failure sequence of the existing tracker tests: out to keyframe 2, then a jump home, which keyframe 2 does not see
FAILURE_ORDER = list(range(13)) + [1, 2]


def state(rows, trk, f):
    """the reference loop's state in front of frame f: the keyframes inserted so far, the reference, the last pose"""
    last = max(r["keyframe"] for r in rows[:f])
    ids = [i for i in trk.ids if i <= last]
    return dict(store={i: trk.store[i] for i in ids}, ids=ids, ref=rows[f - 1]["reference"], guess=(rows[f - 1]["R"], rows[f - 1]["t"]))


# name -> (state in front of this frame, the window's frames, the vote: "ref" = every keyframe of the state with
# ref_vote_pos at the reference, "off" = the same list with ref_vote_pos = -1, "empty" = no vote list, an int = that
# ref_vote_pos, expected first_event, kinds of the events in the window by position)
CASES = {
    "none": (1, [1, 2, 3, 4], "ref", 4, {}),
    "at_0": (6, [6, 7], "ref", 0, {0: "keyframe", 1: "keyframe"}),
    "at_last": (3, [3, 4, 5, 6], "ref", 3, {3: "keyframe"}),
    "vote": (23, [23, 24, 25], "ref", 2, {2: "vote"}),
    "vote_nonwinner": (23, [23, 24], 0, 0, {0: "vote", 1: "vote"}),
    "failure": (12, [12, 1, 2], "ref", 1, {1: "failure", 2: "failure"}),
    "two_events": (5, [5, 6, 7], "ref", 1, {1: "keyframe", 2: "keyframe"}),
    "mixed_events": (11, [11, 1, 12], "ref", 0, {0: "keyframe", 1: "vote", 2: "keyframe"}),
    "vote_then_keyframe": (11, [1, 11], "ref", 0, {0: "vote", 1: "keyframe"}),
    "vote_off": (23, [23, 24, 25], "off", 3, {}),
    "vote_empty": (23, [23, 24, 25], "empty", 3, {}),
}


def case_inputs(seq, rows, trk, name):
    """-> dict(frames, store, ref, ids (vote list), pos (ref_vote_pos), guess, seed, first, kinds)"""
    f, order, vote, first, kinds = CASES[name]
    st = state(rows, trk, f)
    ids = [] if vote == "empty" else list(st["ids"])
    pos = {"ref": st["ids"].index(st["ref"]), "off": -1, "empty": -1}.get(vote, vote)
    return dict(frames=[seq["frames"][k] for k in order], store=st["store"], ref=st["ref"], ids=ids, pos=pos, guess=st["guess"],
                seed=f, first=first, kinds=kinds)


def kind(step, n_vote, pos):
    if not step["tracked"]:
        return "failure"
    if step["keyframe_required"]:
        return "keyframe"
    if n_vote > 0 and pos >= 0 and step["vote_best"] != pos:
        return "vote"
    return None


def run_case_ref(inp, **kw):
    fr = inp["frames"]
    return twr.track_window([x["desc"] for x in fr], [x["xy"] for x in fr], [x["depth"] for x in fr], inp["store"], inp["ref"],
                            inp["ids"], inp["pos"], seed=inp["seed"], guess=inp["guess"], new_keyframe_min_landmarks=KF_MIN, **kw)


# ---- the scan-width scene: 200 landmarks in front of a 64 x 48 camera ------------------------------------------------

SMALL_CAM = (60.0, 60.0, 31.5, 23.5)
SMALL_W, SMALL_H = 64, 48


def small_scene(S, event_at, seed=5, n_landmarks=200):
    """S frames of one 64 x 48 view of 200 landmarks (their descriptors with 4 flipped bits per frame, depth = each
    landmark's z at its pixel over a 2 m background) plus 15 random keypoints, the camera creeping sideways; frame event_at keeps 20 landmarks only,
    so it is tracked with fewer than 30 inliers: the window's one event, a required keyframe.
    -> dict(store = {0: (desc, world)}, frames = [dict(desc, xy, depth)], cam, guess)"""
    rng = np.random.default_rng(seed)
    L = np.stack([rng.uniform(-0.9, 0.9, n_landmarks), rng.uniform(-0.65, 0.65, n_landmarks), rng.uniform(1.8, 2.6, n_landmarks)], 1)
    ldesc = rng.integers(0, 256, (n_landmarks, 32), dtype=np.uint8)
    frames = []
    for s in range(S):
        R = po.rodrigues([0.0, 0.002 * np.sin(0.3 * s), 0.0])
        t = np.array([0.01 * np.sin(0.2 * s), 0.0, 0.0])
        img, front = po.project(R, t, L, SMALL_CAM)
        img = img.astype(np.float32)
        z = (L @ R.T + t)[:, 2]
        depth = np.full((SMALL_H, SMALL_W), 10000, np.uint16)
        seen, taken = [], set()
        for i in range(n_landmarks):
            x, y = int(img[i, 0]), int(img[i, 1])
            if not front[i] or not (1 <= img[i, 0] < SMALL_W - 1 and 1 <= img[i, 1] < SMALL_H - 1) or (x, y) in taken:
                continue
            taken.add((x, y))
            depth[y, x] = np.uint16(round(z[i] * 5000))
            seen.append(i)
        seen = np.array(seen)
        if s == event_at:
            seen = seen[:20]
        dxy = rng.uniform([1, 1], [SMALL_W - 1, SMALL_H - 1], (15, 2)).astype(np.float32)    # keypoints no landmark explains
        qd = np.concatenate([rr._flip_bits(rng, ldesc[seen], 4), rng.integers(0, 256, (15, 32), dtype=np.uint8)])
        qxy = np.concatenate([img[seen], dxy]).astype(np.float32)
        perm = rng.permutation(len(qd))
        frames.append(dict(desc=qd[perm].copy(), xy=qxy[perm].copy(), depth=depth))
    return dict(store={0: (ldesc, L)}, frames=frames, cam=SMALL_CAM, guess=(np.eye(3), np.zeros(3)))
