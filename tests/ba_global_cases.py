"""The trajectory scenes the tests of mslam_hip_bundle_adjust_global share, and their reference solutions (tests/ba_ref.py),
solved once per process.  A trajectory is a ring of K keyframes: group g of `per` landmarks is seen from the keyframes
g .. g + span - 1 (mod K; the wrap is the loop), so only neighbouring keyframes share landmarks and almost every pair of
keyframes is not covisible: blocks of the reduced system that no pair writes must read 0 in every iteration.
This is test infrastructure like ba_cases.py (not a conftest.py, not under oracle/)."""
import functools

import numpy as np

import ba_cases
import ba_ref


def trajectory(K, per, span, seed, noise=0.005, start=0.03, fix_first=True):
    sc = ba_ref.make_scene(K, 1, seed, noise=noise, views=2, start_angle=start, start_shift=start, fix_first=fix_first)
    rng = np.random.default_rng(seed + 1)
    L = per * K
    own = np.stack([rng.uniform(-1.5, 1.5, L), rng.uniform(-1.0, 1.0, L), rng.uniform(1.5, 4.0, L)], 1)
    sc["truth_landmarks"] = np.concatenate([sc["truth_landmarks"], own])
    sc["landmarks"] = np.concatenate([sc["landmarks"], own + start * rng.normal(size=own.shape)])
    l = np.repeat(np.arange(L), span)
    kf, lm = (l // per + np.tile(np.arange(span), L)) % K, 1 + l
    cam = ba_ref.residuals(sc["truth_poses"], sc["truth_landmarks"], kf, lm, np.zeros((len(kf), 3))) + noise * rng.normal(size=(len(kf), 3))
    sc["obs_kf"] = np.concatenate([sc["obs_kf"], kf.astype(np.int32)])
    sc["obs_lm"] = np.concatenate([sc["obs_lm"], lm.astype(np.int32)])
    sc["obs_cam"] = np.concatenate([sc["obs_cam"], cam])
    return sc


def hard(K, seed, angle):
    """the trajectory with every free pose's orientation `angle` rad off the truth: the first steps are rejected"""
    sc = trajectory(K, 3, 3, K)
    rng = np.random.default_rng(seed)
    for k in range(1, K):
        d = rng.normal(size=3)
        q = ba_ref.quaternion_plus(sc["truth_poses"][k, :4], angle * d / np.linalg.norm(d))
        sc["poses"][k, :4] = q / np.linalg.norm(q)
    return sc


def scene(name):
    kind, _, rest = name.partition(":")
    if kind == "traj":             # traj:K -> trajectory(K, 3, 3, K)
        K = int(rest)
        return trajectory(K, 3, 3, K)
    if kind == "traj193":
        return trajectory(193, 2, 3, 193)
    if kind == "free65":           # no constant keyframe: the gauge is free
        return trajectory(65, 3, 3, 65, fix_first=False)
    if kind == "hard66":
        return hard(66, 4, 1.0)
    if kind == "gross80":
        sc = trajectory(80, 3, 3, 80)
        sc["obs_cam"][[5, 300, 700]] += ba_cases.GROSS
        return sc
    if kind == "traj300":          # noise-free, several panels; too large for the QR reference
        return trajectory(300, 2, 3, 300, noise=0.0)
    raise KeyError(name)


# name -> free keyframes; every one has the QR reference
TABLE = {"traj:%d" % K: K - 1 for K in (8, 9, 10, 16, 17, 18, 32, 33, 34, 65, 66, 97, 130)}
TABLE.update({"traj193": 192, "free65": 65, "hard66": 65, "gross80": 79})
WITH_QR = list(TABLE)


def pairs(sc):
    """-> (pairs k1 <= k2 of keyframes that are free and observed and share a landmark, diagonal included; all such pairs)"""
    free = [k for k in range(len(sc["poses"])) if not sc["fixed"][k] and np.any(sc["obs_kf"] == k)]
    isfree = np.zeros(len(sc["poses"]), bool)
    isfree[free] = True
    seen = set((k, k) for k in free)
    order = np.argsort(sc["obs_lm"], kind="stable")
    lm, kf = sc["obs_lm"][order], sc["obs_kf"][order]
    for s, e in zip(np.flatnonzero(np.r_[True, lm[1:] != lm[:-1]]), np.flatnonzero(np.r_[lm[1:] != lm[:-1], True]) + 1):
        ks = sorted(set(int(k) for k in kf[s:e] if isfree[k]))
        seen.update((a, b) for i, a in enumerate(ks) for b in ks[i:])
    return seen, len(free) * (len(free) + 1) // 2


@functools.lru_cache(maxsize=None)
def reference(name):
    """as ba_cases.reference: (scene, qr solution, schur solution, |x_schur - x_qr|_inf, outlier mask at the qr solution,
    distance of the closest residual norm to the 0.15 threshold)"""
    sc = scene(name)
    qr = ba_ref.solve_scene(sc, linear_solver="qr")
    sch = ba_ref.solve_scene(sc, linear_solver="schur")
    dist = max(float(np.max(np.abs(qr["poses"] - sch["poses"]))), float(np.max(np.abs(qr["landmarks"] - sch["landmarks"]))))
    r = ba_ref.residuals(qr["poses"], qr["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"])
    norms = np.sqrt(np.sum(r * r, 1))
    return sc, qr, sch, dist, norms > 0.15, float(np.min(np.abs(norms - 0.15)))


@functools.lru_cache(maxsize=None)
def schur_reference(name):
    """the CPU Schur solve alone (traj300)"""
    sc = scene(name)
    return sc, ba_ref.solve_scene(sc, linear_solver="schur")
