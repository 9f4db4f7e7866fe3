"""A synthetic walk that returns to its start without tracking through it, for the loop-closure tests: the camera stands in
a ring of landmarks (random 256-bit descriptors, 1.6 .. 2.9 m away) and turns once round and a little further, 5 degrees a
frame, its centre on a small circle.  Built like tests/track_ref.py's wall sequence, with its helpers: per frame the visible
landmarks' projections (f32) with `flip` flipped descriptor bits plus random distractors, shuffled, and a depth image that
holds each landmark's z at its pixel over a background beyond z_max.  The keyframes inserted on the way round chain their
covisibility backwards only, so the keyframe inserted when the first keyframe's landmarks come into view again is no
neighbour of it: the loop detector has to find it.  This is test infrastructure (not a conftest.py, not under oracle/)."""
import numpy as np

import reloc_ref as rr
import track_ref as tr

po = tr.po
STEP_DEG = 5.0


def ring_sequence(seed=0, n_frames=76, n_landmarks=2400, n_distractors=300, flip=6, width=640, height=480):
    """-> dict(frames = [dict(desc, xy, depth, R, t)], cam, width, height); the first camera is the world frame"""
    rng = np.random.default_rng(seed)
    ang, rad = rng.uniform(0.0, 2.0 * np.pi, n_landmarks), rng.uniform(1.6, 2.9, n_landmarks)
    L = np.stack([rad * np.sin(ang), rng.uniform(-1.0, 1.0, n_landmarks), rad * np.cos(ang)], 1)
    ldesc = rng.integers(0, 256, (n_landmarks, 32), dtype=np.uint8)
    background = np.full((height, width), int(3.5 * 5000), np.uint16)
    frames = []
    for f in range(n_frames):
        th = np.deg2rad(STEP_DEG * f)
        C = np.array([0.2 * np.sin(th), 0.02 * np.sin(3.0 * th), 0.2 * (1.0 - np.cos(th))])
        R = po.rodrigues([0.0, -th, 0.0])                                  # world -> camera: the camera has turned by th
        t = -R @ C
        img, front = po.project(R, t, L, tr.CAM)
        img = img.astype(np.float32)
        z = (L @ R.T + t)[:, 2]
        ix, iy = img[:, 0].astype(np.float64).astype(np.int64), img[:, 1].astype(np.float64).astype(np.int64)
        inside = front & (img[:, 0] >= 1) & (img[:, 0] < width - 1) & (img[:, 1] >= 1) & (img[:, 1] < height - 1)
        depth = background.copy()
        seen, taken = [], set()
        for i in np.flatnonzero(inside):
            if (ix[i], iy[i]) in taken:
                continue                                                  # one landmark per pixel: the depth image has one z there
            taken.add((ix[i], iy[i]))
            depth[iy[i], ix[i]] = np.uint16(round(z[i] * 5000))
            seen.append(i)
        seen = np.array(seen)
        dxy = rng.uniform([1, 1], [width - 1, height - 1], (n_distractors, 2)).astype(np.float32)
        dxy = dxy[np.array([(int(x), int(y)) not in taken for x, y in dxy])]
        qd = np.concatenate([rr._flip_bits(rng, ldesc[seen], flip), rng.integers(0, 256, (len(dxy), 32), dtype=np.uint8)])
        qxy = np.concatenate([img[seen], dxy]).astype(np.float32)
        perm = rng.permutation(len(qd))
        frames.append(dict(desc=qd[perm].copy(), xy=qxy[perm].copy(), depth=depth, R=R, t=t))
    return dict(frames=frames, cam=tr.CAM, width=width, height=height)
