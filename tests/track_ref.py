"""Reference composition of the keyframe tracking step (not a test): RgbdFeatureFrontend::track
(rgbd_feature_frontend.cpp:279-400) put together in numpy from the oracle's back-projection (oracle/mslam_oracle.py),
tests/reloc_ref.py::relocalize with one candidate, the depth mask and the guess, findBetterReferenceKeyframe's count
(:544-575, projection.cpp:42-62) and the construction of the new keyframe's entry (:373-397 with addNewLandmarks, :402-431),
plus the loop of processSensorData (:185-222) over a frame sequence.  Shares no code with the product.

Every f64 expression is written out elementwise in the order include/mslam_hip.h states, so numpy rounds each operation on
its own exactly as the library (built with -ffp-contract=off) does, and results can be compared bit for bit.

Also here: the synthetic sequence tests/test_track.py, tests/test_gpu_track.py and tests/test_host_track.py run on, and the
scene file `harness --track` reads."""
import struct

import numpy as np

import reloc_ref as rr
from reloc_ref import po

CAM = rr.CAM
FACTOR = 1.0 / 5000.0


def _oracle():
    return rr._oracle()


# ---- the vote ------------------------------------------------------------------------------------------------------------

def visible(world, R, t, cam=CAM, width=640, height=480):
    """isVisibleInFrame per world point: c = R p + t, u = (c0 / c2) fx + cx, v = (c1 / c2) fy + cy,
    u >= 0 && u < (double)(float)width && v >= 0 && v < (double)(float)height && c2 > 0"""
    w = np.asarray(world, np.float64).reshape(-1, 3)
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64).reshape(3)
    X, Y, Z = w[:, 0], w[:, 1], w[:, 2]
    c = [((R[r, 0] * X + R[r, 1] * Y) + R[r, 2] * Z) + t[r] for r in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = (c[0] / c[2]) * np.float64(cam[0]) + np.float64(cam[2])
        v = (c[1] / c[2]) * np.float64(cam[1]) + np.float64(cam[3])
        wl, hl = np.float64(np.float32(width)), np.float64(np.float32(height))
        return (u >= 0) & (u < wl) & (v >= 0) & (v < hl) & (c[2] > 0)


def vote(store, ids, R, t, cam=CAM, width=640, height=480):
    """-> (counts per id, position of the first maximum in list order or -1 for an empty list)"""
    counts = np.array([int(visible(store[i][1], R, t, cam, width, height).sum()) for i in ids], np.int32)
    best, top = -1, -1
    for k, n in enumerate(counts):
        if n > top:
            best, top = k, int(n)
    return counts, best


# ---- the new keyframe's entry -----------------------------------------------------------------------------------------

def build_entry(desc, xyz, valid, pairs, mask, ref_world, R, t, z_max=3.0, capacity=None):
    """Part A: the inlier correspondences in correspondence order (descriptor of the query keypoint, the reference entry's
    world point as it is).  Part B: the keypoints no correspondence used, with a valid depth and z <= z_max, in keypoint
    order, world = R^T (p - t) as ((R[0][r] (x - t0) + R[1][r] (y - t1)) + R[2][r] (z - t2)).
    -> dict(desc, world, src, kp, n_inherited)"""
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    valid = np.asarray(valid).reshape(-1) != 0
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64).reshape(3)
    ref_world = np.asarray(ref_world, np.float64).reshape(-1, 3)
    fi, ti = np.asarray(pairs[0], np.int64), np.asarray(pairs[1], np.int64)
    corr = valid[fi]                              # matches with a valid depth = the correspondences, in match order
    cf, ct = fi[corr], ti[corr]
    mask = np.asarray(mask, bool).reshape(-1)
    assert len(mask) == len(cf)
    a_kp, a_src = cf[mask], ct[mask]
    used = np.zeros(len(desc), bool)
    used[cf] = True                               # used = matched with a valid depth, inlier or not
    b_kp = np.flatnonzero(~used & valid & (xyz[:, 2] <= np.float64(z_max)))
    p = xyz[b_kp]
    dx, dy, dz = p[:, 0] - t[0], p[:, 1] - t[1], p[:, 2] - t[2]
    lifted = np.stack([(R[0, r] * dx + R[1, r] * dy) + R[2, r] * dz for r in range(3)], 1).reshape(-1, 3)
    out = dict(desc=np.concatenate([desc[a_kp], desc[b_kp]]), world=np.concatenate([ref_world[a_src], lifted]),
               src=np.concatenate([a_src, np.full(len(b_kp), -1)]).astype(np.int32),
               kp=np.concatenate([a_kp, b_kp]).astype(np.int32), n_inherited=len(a_kp))
    if capacity is not None and len(out["kp"]) > capacity:     # (an entry never exceeds the store's capacity)
        for k in ("desc", "world", "src", "kp"):
            out[k] = out[k][:capacity]
        out["n_inherited"] = min(out["n_inherited"], capacity)
    return out


# ---- one step -------------------------------------------------------------------------------------------------------------

def track(desc, xy, depth, store, ref_id, vote_ids=(), cam=CAM, factor=FACTOR, ratio=0.7, iterations=100, thr=5.0, seed=0,
          guess=None, min_matched_points=10, new_keyframe_min_landmarks=30, z_max=3.0, want_keyframe=True, capacity=None):
    """-> dict(pairs, mask, n_matches, n_correspondences, n_inliers, status, R, t, tracked, keyframe_required, vote_counts,
    vote_best, vote_best_count, entry (or None), xyz, valid); capacity: the store's entry capacity, handed to build_entry"""
    h, w = np.asarray(depth).shape
    xyz, valid = _oracle().backproject(depth, xy, factor, cam[:2], cam[2:])
    c = rr.relocalize(desc, xy, store, [ref_id], cam, valid=valid, ratio=ratio, iterations=iterations, thr=thr, seed=seed,
                      guess=guess, min_inliers=0)["candidates"][0]
    tracked = bool(c["status"]) and c["n_correspondences"] >= min_matched_points
    required = tracked and c["n_inliers"] < new_keyframe_min_landmarks
    out = dict(pairs=c["pairs"], mask=c["mask"], n_matches=c["n_matches"], n_correspondences=c["n_correspondences"],
               n_inliers=c["n_inliers"], status=c["status"], R=c["R"], t=c["t"], tracked=tracked, keyframe_required=required,
               vote_counts=np.zeros(len(vote_ids), np.int32), vote_best=-1, vote_best_count=0, entry=None, xyz=xyz, valid=valid)
    if tracked and len(vote_ids):
        out["vote_counts"], out["vote_best"] = vote(store, vote_ids, c["R"], c["t"], cam, w, h)
        out["vote_best_count"] = int(out["vote_counts"][out["vote_best"]])
    if required and want_keyframe:
        out["entry"] = build_entry(desc, xyz, valid, c["pairs"], c["mask"], store[ref_id][1], c["R"], c["t"], z_max, capacity)
    return out


# ---- the loop ---------------------------------------------------------------------------------------------------------------

class KeyframeTracker:
    """processSensorData's loop, as modular-slam_amd's HipKeyframeTracker states it: the first frame becomes keyframe 0 at
    the identity pose; then track against the reference with the previous pose as the guess and seed + frame number; the
    vote's winner becomes the reference; a required keyframe is inserted under the next id and becomes the reference; when
    tracking fails, relocalize over the (most recent 64) stored keyframes names the new reference."""

    def __init__(self, cam=CAM, factor=FACTOR, ratio=0.7, iterations=100, thr=5.0, seed=0, min_matched_points=10,
                 new_keyframe_min_landmarks=30, z_max=3.0, reloc_min_inliers=60):
        self.cam, self.factor, self.ratio, self.iterations, self.thr, self.seed = cam, factor, ratio, iterations, thr, seed
        self.min_matched_points, self.new_keyframe_min_landmarks = min_matched_points, new_keyframe_min_landmarks
        self.z_max, self.reloc_min_inliers = z_max, reloc_min_inliers
        self.store, self.ids, self.reference = {}, [], None
        self.R, self.t = np.eye(3), np.zeros(3)
        self.frame = 0

    def process(self, desc, xy, depth):
        seed = self.seed + self.frame
        self.frame += 1
        desc = np.asarray(desc, np.uint8).reshape(-1, 32)
        if self.reference is None:
            xyz, valid = _oracle().backproject(depth, xy, self.factor, self.cam[:2], self.cam[2:])
            keep = valid & (xyz[:, 2] <= self.z_max)
            self.store[0] = (desc[keep].copy(), xyz[keep].copy())
            self.ids, self.reference = [0], 0
            return dict(tracked=True, n_inliers=0, R=self.R.copy(), t=self.t.copy(), reference=0, keyframe=0, relocalized=False)
        ids = self.ids[-64:]
        s = track(desc, xy, depth, self.store, self.reference, ids, self.cam, self.factor, self.ratio, self.iterations,
                  self.thr, seed, (self.R, self.t), self.min_matched_points, self.new_keyframe_min_landmarks, self.z_max)
        out = dict(tracked=s["tracked"], n_inliers=s["n_inliers"], keyframe=-1, relocalized=False)
        if s["tracked"]:
            self.R, self.t = s["R"], s["t"]
            if s["vote_best"] >= 0:
                self.reference = ids[s["vote_best"]]
            if s["entry"] is not None:
                new_id = self.ids[-1] + 1
                self.store[new_id] = (s["entry"]["desc"], s["entry"]["world"])
                self.ids.append(new_id)
                self.reference = out["keyframe"] = new_id
        else:
            best = rr.relocalize(desc, xy, self.store, ids, self.cam, ratio=self.ratio, iterations=self.iterations, thr=self.thr,
                                 seed=seed, min_inliers=self.reloc_min_inliers)["best"]
            if best >= 0:
                self.reference, out["relocalized"] = ids[best], True
        out.update(R=self.R.copy(), t=self.t.copy(), reference=self.reference)
        return out


# ---- the synthetic sequence -----------------------------------------------------------------------------------------------

SEQ_PARAMS = dict(new_keyframe_min_landmarks=100)      # what the sequence tests run the loop with


def make_sequence(seed=0, n_frames=32, n_landmarks=1500, n_distractors=400, flip=6, width=640, height=480):
    """A wall of landmarks (random 256-bit descriptors) 1.6 .. 2.9 m in front of a camera that slides 5.6 m to the right
    along it and back, yawing a little: landmarks leave the view and new ones enter, so the loop has to insert keyframes
    on the way out and finds older keyframes better on the way back.  Per frame: the visible landmarks' projections (f32)
    with `flip` flipped descriptor bits, plus n_distractors random keypoints, shuffled; a depth image that holds each
    landmark's z at its pixel (1/5000 m units: the only noise is that quantisation; 8 % of them have no depth) over a
    background sloping from 2 to 4 m with a band of invalid depth, so distractors have valid depths on both sides of
    z_max = 3 m and some have none.  The first camera is the world frame.
    -> dict(frames = [dict(desc, xy, depth, R, t, landmark)], cam, width, height)"""
    rng = np.random.default_rng(seed)
    L = np.stack([rng.uniform(-2.0, 8.0, n_landmarks), rng.uniform(-1.2, 1.2, n_landmarks), rng.uniform(1.6, 2.9, n_landmarks)], 1)
    ldesc = rng.integers(0, 256, (n_landmarks, 32), dtype=np.uint8)
    background = np.tile(((2.0 + 2.0 * np.arange(width) / width) * 5000).astype(np.uint16), (height, 1))
    frames = []
    for f in range(n_frames):
        s = f / (n_frames - 1)
        tri = 1.0 - abs(2.0 * s - 1.0)                                   # 0 -> 1 -> 0
        C = np.array([5.6 * tri, 0.05 * np.sin(6.0 * s), 0.1 * np.sin(3.0 * s)])
        R = po.rodrigues([0.02 * np.sin(5.0 * s), 0.08 * np.sin(7.0 * s), 0.03 * s])
        t = -R @ C
        img, front = po.project(R, t, L, CAM)
        img = img.astype(np.float32)
        z = (L @ R.T + t)[:, 2]
        ix, iy = img[:, 0].astype(np.float64).astype(np.int64), img[:, 1].astype(np.float64).astype(np.int64)
        inside = front & (img[:, 0] >= 1) & (img[:, 0] < width - 1) & (img[:, 1] >= 1) & (img[:, 1] < height - 1)
        depth = background.copy()
        depth[:, 300:330] = 0                                             # a band without depth
        hole = rng.random(n_landmarks) < 0.08                             # and landmarks the sensor has no depth for
        seen, taken = [], set()
        for i in np.flatnonzero(inside):
            if (ix[i], iy[i]) in taken:
                continue                                                  # one landmark per pixel: the depth image has one z there
            taken.add((ix[i], iy[i]))
            depth[iy[i], ix[i]] = 0 if hole[i] else np.uint16(round(z[i] * 5000))
            seen.append(i)
        seen = np.array(seen)
        dxy = rng.uniform([1, 1], [width - 1, height - 1], (n_distractors, 2)).astype(np.float32)
        free = np.array([(int(x), int(y)) not in taken for x, y in dxy])  # a distractor on a landmark's pixel would share its depth: harmless, but keep the scene simple
        dxy = dxy[free]
        qd = np.concatenate([rr._flip_bits(rng, ldesc[seen], flip), rng.integers(0, 256, (len(dxy), 32), dtype=np.uint8)])
        qxy = np.concatenate([img[seen], dxy]).astype(np.float32)
        src = np.concatenate([seen, np.full(len(dxy), -1)])
        perm = rng.permutation(len(qd))
        frames.append(dict(desc=qd[perm].copy(), xy=qxy[perm].copy(), depth=depth, R=R, t=t, landmark=src[perm]))
    # poses relative to the first camera (the loop's world frame): X_f = R_f R_0^T X_0 + (t_f - R_f R_0^T t_0)
    R0, t0 = frames[0]["R"], frames[0]["t"]
    for fr in frames:
        Rr = fr["R"] @ R0.T
        fr["R"], fr["t"] = Rr, fr["t"] - Rr @ t0
    return dict(frames=frames, cam=CAM, width=width, height=height)


def run_reference(seq, **kw):
    """the reference loop over a sequence -> list of per-frame dicts (with ground-truth errors err_deg, err_m)"""
    params = dict(SEQ_PARAMS)
    params.update(kw)
    trk = KeyframeTracker(cam=seq["cam"], **params)
    rows = []
    for fr in seq["frames"]:
        o = trk.process(fr["desc"], fr["xy"], fr["depth"])
        o["err_deg"], o["err_m"] = rr.rot_err(o["R"], fr["R"]), float(np.linalg.norm(o["t"] - fr["t"]))
        rows.append(o)
    return rows, trk


def summarize(rows):
    """-> (tracked flags, frames at which a keyframe was inserted, frames at which the reference changed without one)"""
    tracked = [bool(r["tracked"]) for r in rows]
    inserted = [f for f, r in enumerate(rows) if r["keyframe"] >= 0]
    switched = [f for f in range(1, len(rows)) if rows[f]["reference"] != rows[f - 1]["reference"] and rows[f]["keyframe"] < 0]
    return tracked, inserted, switched


# ---- scene file of `harness --track` --------------------------------------------------------------------------------------

def write_scene(path, seq, seed=0, **kw):
    """little-endian: magic 'MSTK', i32 version = 1, n_frames, width, height; f64 fx, fy, cx, cy; f32 factor; i32 seed,
    min_matched_points, new_keyframe_min_landmarks; f64 z_max; then per frame: i32 n, desc n x 32, xy n x 2 f32, depth
    height x width u16"""
    params = dict(min_matched_points=10, new_keyframe_min_landmarks=30, z_max=3.0)
    params.update(SEQ_PARAMS)
    params.update(kw)
    with open(path, "wb") as f:
        f.write(b"MSTK" + struct.pack("<4i", 1, len(seq["frames"]), seq["width"], seq["height"]))
        f.write(struct.pack("<4d", *seq["cam"]) + struct.pack("<f", FACTOR))
        f.write(struct.pack("<3i", seed, params["min_matched_points"], params["new_keyframe_min_landmarks"]))
        f.write(struct.pack("<d", params["z_max"]))
        for fr in seq["frames"]:
            f.write(struct.pack("<i", len(fr["desc"])))
            f.write(np.ascontiguousarray(fr["desc"], np.uint8).tobytes())
            f.write(np.ascontiguousarray(fr["xy"], "<f4").tobytes())
            f.write(np.ascontiguousarray(fr["depth"], "<u2").tobytes())
