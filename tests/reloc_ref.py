"""Reference composition of the verified relocalisation (not a test): what RgbdFeatureFrontend::relocalize's commented body
does (rgbd_feature_frontend.cpp:495-534), put together from the oracle's matcher + ratio test (oracle/mslam_oracle.py) and
the PnP oracle (oracle/mslam_pnp_oracle.py::pnp_ransac) with seed + position, plus the landmark lift of addNewLandmarks
(:402-431) and the ranking rule (max_element: most inliers, first maximum).  Shares no code with the product.

Also here: the synthetic scene tests/test_reloc.py and tests/test_gpu_reloc.py run on."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import mslam_pnp_oracle as po  # noqa: E402

CAM = (525.0, 525.0, 319.5, 239.5)      # TUM intrinsics, rgbd_file_provider.cpp:136-145


def _oracle():
    import mslam_oracle
    mslam_oracle.lib()
    return mslam_oracle


def lift(desc, xyz, valid, R, t, z_max=3.0):
    """addNewLandmarks: keypoints with a valid depth and z <= z_max, in keypoint order; world = R p + t, every f64 operation
    rounded on its own in the order ((R0 x + R1 y) + R2 z) + t (numpy elementwise: no fused multiply-add, no reordering)"""
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64).reshape(3)
    keep = (np.asarray(valid).reshape(-1) != 0) & (xyz[:, 2] <= np.float64(z_max))
    p = xyz[keep]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    world = np.stack([((R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z) + t[r] for r in range(3)], 1)
    return desc[keep].copy(), world


def match(query_desc, kf_desc, ratio=0.7):
    """matchLandmarks -> match(from = query keypoints, to = keyframe landmarks); fewer than 2 `from` rows: no matches"""
    q = np.asarray(query_desc, np.uint8).reshape(-1, 32)
    k = np.asarray(kf_desc, np.uint8).reshape(-1, 32)
    if len(q) < 2 or len(k) == 0:
        return np.empty(0, np.int32), np.empty(0, np.int32)
    return _oracle().match(q, k, ratio)


def rank(statuses, inliers, min_inliers):
    """position of the candidate with the most inliers among those with a model, the first one on ties; -1 when there is
    none or the winner has fewer than min_inliers"""
    best, top = -1, -1
    for k, (s, n) in enumerate(zip(statuses, inliers)):
        if s and n > top:
            best, top = k, n
    return best if best >= 0 and top >= min_inliers else -1


def relocalize(desc, xy, store, cand_ids, cam=CAM, valid=None, ratio=0.7, iterations=100, thr=5.0, seed=0, guess=None,
               min_inliers=60, confidence=0.99):
    """store: {id: (desc [n, 32], world_xyz [n, 3] f64)}; guess = (R0, t0) or None.
    -> dict(best, candidates = [dict(pairs = (from, to), n_matches, n_correspondences, n_inliers, status, R, t, mask)])"""
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    cands = []
    for pos, cid in enumerate(cand_ids):
        kd, kw = store[cid]
        fi, ti = match(desc, kd, ratio)
        keep = np.ones(len(fi), bool) if valid is None else np.asarray(valid).reshape(-1)[fi] != 0
        obj = np.asarray(kw, np.float64).reshape(-1, 3)[ti[keep]].astype(np.float32)
        img = xy[fi[keep]]
        res = po.pnp_ransac(obj, img, cam, iterations, thr, seed + pos, guess, confidence) if len(obj) >= 4 else None
        c = dict(pairs=(fi, ti), n_matches=len(fi), n_correspondences=len(obj), status=0 if res is None else 1,
                 n_inliers=0 if res is None else int(res["mask"].sum()), R=None if res is None else res["R"],
                 t=None if res is None else res["t"], mask=np.zeros(len(obj), bool) if res is None else res["mask"],
                 obj=obj, img=img)
        cands.append(c)
    return dict(best=rank([c["status"] for c in cands], [c["n_inliers"] for c in cands], min_inliers), candidates=cands)


# ---- the synthetic scene -----------------------------------------------------------------------------------------------

def _flip_bits(rng, desc, n_bits):
    out = desc.copy()
    for row in out:
        for b in rng.choice(256, n_bits, replace=False):
            row[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def make_scene(seed=0, n_kf=4, n_landmarks=600, target=2, n_distractors=1300, flip=6, noise=0.0, drop=0.1):
    """n_kf keyframes of n_landmarks landmarks with random 256-bit descriptors (ids 10, 11, ...), one DECOY (id 99: the
    target's descriptors with its world points permuted), and a query: the target keyframe seen from a known pose (R, t:
    world -> camera) — image points with `noise` px of Gaussian noise, descriptors with `flip` flipped bits, a share `drop`
    of the landmarks unseen — plus n_distractors keypoints with random descriptors, all shuffled.
    -> dict(store, ids, decoy, target_id, desc, xy, R, t, from_landmark)"""
    rng = np.random.default_rng(seed)
    R = po.rodrigues(rng.normal(size=3) * 0.3)
    t = rng.normal(size=3) * 0.2 + np.array([0.1, -0.1, 0.3])
    store, ids = {}, []
    for k in range(n_kf):
        d = rng.integers(0, 256, (n_landmarks, 32), dtype=np.uint8)
        cam_pts = np.stack([rng.uniform(-1.6, 1.6, n_landmarks), rng.uniform(-1.2, 1.2, n_landmarks),
                            rng.uniform(2.5, 6.0, n_landmarks)], 1)
        store[10 + k] = (d, (cam_pts - t) @ R)          # world points whose camera coordinates are the box above
        ids.append(10 + k)
    tid = ids[target]
    td, tw = store[tid]
    store[99] = (td.copy(), tw[rng.permutation(n_landmarks)].copy())
    seen = np.flatnonzero(rng.random(n_landmarks) >= drop)
    img, ok = po.project(R, t, tw[seen].astype(np.float32).astype(np.float64), CAM)
    assert ok.all()
    img = img + rng.normal(size=img.shape) * noise
    qd = np.concatenate([_flip_bits(rng, td[seen], flip), rng.integers(0, 256, (n_distractors, 32), dtype=np.uint8)])
    qxy = np.concatenate([img, rng.uniform(0, [640, 480], (n_distractors, 2))]).astype(np.float32)
    src = np.concatenate([seen, np.full(n_distractors, -1)])
    perm = rng.permutation(len(qd))
    return dict(store=store, ids=ids, decoy=99, target_id=tid, desc=qd[perm].copy(), xy=qxy[perm].copy(), R=R, t=t,
                from_landmark=src[perm])


def rot_err(Ra, Rb):
    return np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))
