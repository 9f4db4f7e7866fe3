"""tests/track_ref.py's tracking step and loop with the pose stage replaced by RANSAC rigid alignment (tests/align_ref.py):
what mslam_hip_track computes under mslam_hip_set_track_pose(ALIGN).  Not a test; shares no code with the product.

The correspondences are track_ref's (matches whose keypoint has a valid depth, in match order); src = (float) the reference
entry's world point, dst = (float) the keypoint's camera-frame point; the estimator runs `iterations` hypotheses with the
step's seed and max_distance.  The guess takes no part.  Everything behind the pose (tracked, the vote, the new entry, the
loop, the relocalisation after a failure — which has no depth and stays PnP) is track_ref's code."""
import numpy as np

import align_ref as ar
import reloc_ref as rr
import track_ref as tr

CAM, FACTOR = tr.CAM, tr.FACTOR


def track(desc, xy, depth, store, ref_id, vote_ids=(), cam=CAM, factor=FACTOR, ratio=0.7, iterations=100, max_distance=0.05,
          seed=0, min_matched_points=10, new_keyframe_min_landmarks=30, z_max=3.0, want_keyframe=True, capacity=None,
          confidence=0.99):
    """-> track_ref.track's dict, plus best (the winning hypothesis) and margin (align_ref's)"""
    h, w = np.asarray(depth).shape
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    xyz, valid = tr._oracle().backproject(depth, xy, factor, cam[:2], cam[2:])
    kd, kw = store[ref_id]
    fi, ti = rr.match(desc, kd, ratio)
    keep = np.asarray(valid).reshape(-1)[fi] != 0
    src = np.asarray(kw, np.float64).reshape(-1, 3)[ti[keep]].astype(np.float32)
    dst = np.asarray(xyz, np.float64).reshape(-1, 3)[fi[keep]].astype(np.float32)
    res = ar.align_ransac(src, dst, max_distance, iterations, seed, confidence) if len(src) >= 3 else dict(best=-1, margin=np.inf)
    ok = res["best"] >= 0
    n_corr = len(src)
    mask = res["mask"] if ok else np.zeros(n_corr, bool)
    n_inl = int(mask.sum())
    tracked = ok and n_corr >= min_matched_points
    required = tracked and n_inl < new_keyframe_min_landmarks
    out = dict(pairs=(fi, ti), mask=mask, n_matches=len(fi), n_correspondences=n_corr, n_inliers=n_inl, status=int(ok),
               R=res["R"] if ok else None, t=res["t"] if ok else None, tracked=tracked, keyframe_required=required,
               vote_counts=np.zeros(len(vote_ids), np.int32), vote_best=-1, vote_best_count=0, entry=None, xyz=xyz, valid=valid,
               best=res["best"], margin=res["margin"])
    if tracked and len(vote_ids):
        out["vote_counts"], out["vote_best"] = tr.vote(store, vote_ids, out["R"], out["t"], cam, w, h)
        out["vote_best_count"] = int(out["vote_counts"][out["vote_best"]])
    if required and want_keyframe:
        out["entry"] = tr.build_entry(desc, xyz, valid, out["pairs"], mask, store[ref_id][1], out["R"], out["t"], z_max, capacity)
    return out


class KeyframeTracker(tr.KeyframeTracker):
    """track_ref's loop with the step above"""

    def __init__(self, max_distance=0.05, **kw):
        super().__init__(**kw)
        self.max_distance = max_distance
        self.margin = np.inf

    def process(self, desc, xy, depth):
        if self.reference is None:
            return super().process(desc, xy, depth)
        seed = self.seed + self.frame
        self.frame += 1
        desc = np.asarray(desc, np.uint8).reshape(-1, 32)
        ids = self.ids[-64:]
        s = track(desc, xy, depth, self.store, self.reference, ids, self.cam, self.factor, self.ratio, self.iterations,
                  self.max_distance, seed, self.min_matched_points, self.new_keyframe_min_landmarks, self.z_max)
        self.margin = min(self.margin, s["margin"])
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


def run_reference(seq, max_distance=0.05, **kw):
    """the reference loop over a sequence -> (per-frame dicts with err_deg / err_m against ground truth, the tracker)"""
    params = dict(tr.SEQ_PARAMS)
    params.update(kw)
    trk = KeyframeTracker(max_distance=max_distance, cam=seq["cam"], **params)
    rows = []
    for fr in seq["frames"]:
        o = trk.process(fr["desc"], fr["xy"], fr["depth"])
        o["err_deg"], o["err_m"] = rr.rot_err(o["R"], fr["R"]), float(np.linalg.norm(o["t"] - fr["t"]))
        rows.append(o)
    return rows, trk
