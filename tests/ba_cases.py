"""The bundle-adjustment cases the CPU and the GPU tests share, and their reference solutions (tests/ba_ref.py), solved once
per process.  Scenes are small on purpose: the dense QR of the reference is cubic in the number of parameters.
This is test infrastructure (not a conftest.py, not under oracle/)."""
import functools

import numpy as np

import ba_ref

SIZES = [(2, 20), (3, 65), (5, 150), (8, 200)]
NOISES = [0.0, 0.005, 0.010]
START = {0.0: 0.02, 0.005: 0.1, 0.010: 0.3}   # tangent length of the start error per noise level, rad


def _append(sc, kf, lm, cam):
    sc["obs_kf"] = np.concatenate([sc["obs_kf"], np.asarray(kf, np.int32)])
    sc["obs_lm"] = np.concatenate([sc["obs_lm"], np.asarray(lm, np.int32)])
    sc["obs_cam"] = np.concatenate([sc["obs_cam"], np.asarray(cam, np.float64).reshape(-1, 3)])
    return sc


def _exact(sc, kf, lm):
    return ba_ref.residuals(sc["truth_poses"], sc["truth_landmarks"], np.asarray(kf), np.asarray(lm), np.zeros((len(kf), 3)))


def _k64():
    """64 keyframes, 8 landmarks each seen from that keyframe alone, one landmark seen by all: 63 free poses, the 378-wide
    reduced system"""
    sc = ba_ref.make_scene(64, 1, 64, noise=0.002, start_angle=0.02, start_shift=0.02)
    rng = np.random.default_rng(640)
    own = np.stack([rng.uniform(-1.5, 1.5, 512), rng.uniform(-1.0, 1.0, 512), rng.uniform(1.5, 4.0, 512)], 1)
    sc["truth_landmarks"] = np.concatenate([sc["truth_landmarks"], own])
    sc["landmarks"] = np.concatenate([sc["landmarks"], own + 0.02 * rng.normal(size=own.shape)])
    kf, lm = np.repeat(np.arange(64), 8), 1 + np.arange(512)
    return _append(sc, kf, lm, _exact(sc, kf, lm) + 0.002 * rng.normal(size=(512, 3)))


GROSS = [[0.4, 0, 0], [0, -0.5, 0.1], [0.2, 0.2, 0.3]]      # the three offsets of gross_outliers


def _blocks(M):
    """M observations of a 4-keyframe, 48-landmark scene in which every landmark is seen from every keyframe: the 192
    (keyframe, landmark) pairs tiled, every repeat with noise of its own.  k_ba_eval's blocks are 256 observations: M = 16384
    is 64 of them, one trip of the 64-lane folds of k_ba_check and k_ba_control, M = 16385 starts the second trip.  Rows of
    M / 4 per keyframe, about M / 192 observations of every landmark in every keyframe.  Gross offsets on the first
    observation, the last of block 64 and the last of all."""
    sc = ba_ref.make_scene(4, 48, 7, noise=0.005, start_angle=0.1)
    n = len(sc["obs_kf"])
    reps = -(-M // n) - 1
    kf, lm = np.tile(sc["obs_kf"], reps), np.tile(sc["obs_lm"], reps)
    _append(sc, kf, lm, _exact(sc, kf, lm) + 0.005 * np.random.default_rng(8).normal(size=(len(kf), 3)))
    for k in ("obs_kf", "obs_lm", "obs_cam"):
        sc[k] = sc[k][:M]
    for m, off in zip((0, 16383, M - 1), GROSS):
        sc["obs_cam"][m] += off
    return sc


def _fixed_middle(two):
    """6 keyframes, none constant at first: keyframe 1 loses its observations and keyframe 3 is constant at its truth, so the
    free keyframes 0, 2, 4, 5 are blocks 0, 1, 2, 3 of the reduced system (ci[k] != k - 1); two: keyframe 0 constant too"""
    sc = ba_ref.make_scene(6, 80, 21, noise=0.005, views=3, start_angle=0.1, fix_first=False)
    keep = sc["obs_kf"] != 1
    for k in ("obs_kf", "obs_lm", "obs_cam"):
        sc[k] = sc[k][keep]
    for k in (0, 3) if two else (3,):
        sc["fixed"][k] = 1
        sc["poses"][k] = sc["truth_poses"][k]
    return sc


def _capped(sc, cap):
    sc["max_iterations"] = cap
    return sc


def scene(name):
    """-> the scene dict of ba_ref.make_scene (plus max_iterations where the case caps it)"""
    kind, _, rest = name.partition(":")
    if kind in ("fixed", "free"):
        K, L, mm = (int(v) for v in rest.split(","))
        noise = mm / 1000.0
        return ba_ref.make_scene(K, L, 1000 * K + L + mm, noise=noise, views=min(K, 4), start_angle=START[noise],
                                 fix_first=kind == "fixed")
    if kind in ("rejected", "cap3"):
        sc = ba_ref.make_scene(4, 100, 2, start_angle=1.0)
        if kind == "cap3":
            sc["max_iterations"] = 3
        return sc
    if kind == "all_fixed":
        sc = ba_ref.make_scene(3, 65, 5, noise=0.005, start_angle=0.1)
        sc["poses"] = sc["truth_poses"].copy()      # every pose constant, at the truth: the landmarks alone move
        sc["fixed"][:] = 1
        return sc
    if kind == "k1_fixed":
        return ba_ref.make_scene(1, 30, 6, noise=0.005)
    if kind == "single_view":      # K = 2, one observation per landmark; rest = L, so M = L
        return ba_ref.make_scene(2, int(rest), 70 + int(rest), noise=0.005, views=1, start_angle=0.1)
    if kind == "two_views":        # K = 2, every landmark in both keyframes: rows of L, M = 2 L
        return ba_ref.make_scene(2, int(rest), 90 + int(rest), noise=0.005, start_angle=0.1)
    if kind == "twice_in_keyframe":
        sc = ba_ref.make_scene(3, 40, 8, noise=0.005, start_angle=0.1)
        rng = np.random.default_rng(80)
        kf, lm = np.array([1, 1, 2, 0, 1]), np.array([3, 17, 17, 30, 3])   # landmark 3 ends up three times in keyframe 1
        return _append(sc, kf, lm, _exact(sc, kf, lm) + 0.005 * rng.normal(size=(5, 3)))
    if kind == "fixed_only_landmarks":
        sc = ba_ref.make_scene(3, 40, 9, noise=0.005, start_angle=0.1)
        keep = ~((sc["obs_lm"] >= 30) & (sc["obs_kf"] != 0))              # landmarks 30..39: seen from the constant keyframe only
        for k in ("obs_kf", "obs_lm", "obs_cam"):
            sc[k] = sc[k][keep]
        return sc
    if kind == "keyframe_one_observation":
        sc = ba_ref.make_scene(4, 40, 10, noise=0.005, start_angle=0.1)
        keep = (sc["obs_kf"] != 3) | (sc["obs_lm"] == 7)
        for k in ("obs_kf", "obs_lm", "obs_cam"):
            sc[k] = sc[k][keep]
        return sc
    if kind == "gross_outliers":
        sc = ba_ref.make_scene(3, 65, 11, noise=0.005, start_angle=0.1)
        sc["obs_cam"][[4, 77, 150]] += GROSS
        return sc
    if kind == "empty":
        sc = ba_ref.make_scene(2, 5, 12)
        for k in ("obs_kf", "obs_lm", "obs_cam"):
            sc[k] = sc[k][:0]
        return sc
    if kind == "k64":
        return _k64()
    if kind == "blocks":
        return _blocks(int(rest))
    if kind == "k64_dense":        # every landmark in 16 of 64 keyframes: every off-diagonal block of S sums over shared landmarks
        return ba_ref.make_scene(64, 120, 64, noise=0.005, views=16, start_angle=0.05)
    if kind in ("fixed_middle", "fixed_two"):
        return _fixed_middle(kind == "fixed_two")
    if kind in ("cap0", "cap1"):
        return _capped(scene("rejected"), int(kind[3:]))
    if kind == "cap4_converges":   # converges in its 4th iteration, the last kernel of the host's first batch
        return _capped(scene("fixed:3,65,5"), 4)
    if kind == "cap4_stops":       # would need a 5th
        return _capped(scene("free:5,150,10"), 4)
    if kind == "at_minimum":       # the start is the minimum: the gradient test ends the solve before the first iteration
        sc = ba_ref.make_scene(3, 65, 5, noise=0.0)
        sc["poses"], sc["landmarks"] = sc["truth_poses"].copy(), sc["truth_landmarks"].copy()
        return sc
    raise KeyError(name)


FAMILIES = {
    "fixed": ["fixed:%d,%d,%d" % (K, L, int(n * 1000)) for K, L in SIZES for n in NOISES],
    "free": ["free:%d,%d,%d" % (K, L, int(n * 1000)) for K, L in SIZES for n in NOISES],
    "rejected": ["rejected"],
    "all_fixed": ["all_fixed"],
}
EDGES = (["k1_fixed", "twice_in_keyframe", "fixed_only_landmarks", "keyframe_one_observation", "gross_outliers", "empty", "cap3",
          "k64"] + ["single_view:%d" % L for L in (63, 64, 65, 257)] + ["two_views:%d" % L for L in (63, 64, 65, 257)] +
         ["blocks:16384", "blocks:16385", "k64_dense", "fixed_middle", "fixed_two", "cap0", "cap1", "cap4_converges", "cap4_stops",
          "at_minimum"])
ALL = [c for f in FAMILIES.values() for c in f] + EDGES


def family(name):
    for f, cases in FAMILIES.items():
        if name in cases:
            return f
    return "edges"


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (scene, qr solution, schur solution, |x_schur - x_qr|_inf, outlier mask at the qr solution, distance of the
    closest residual norm to the 0.15 threshold)"""
    sc = scene(name)
    kw = dict(max_iterations=sc.get("max_iterations", 100))
    qr = ba_ref.solve_scene(sc, linear_solver="qr", **kw)
    sch = ba_ref.solve_scene(sc, linear_solver="schur", **kw)
    dist = max(float(np.max(np.abs(qr["poses"] - sch["poses"]), initial=0.0)),
               float(np.max(np.abs(qr["landmarks"] - sch["landmarks"]), initial=0.0)))
    r = ba_ref.residuals(qr["poses"], qr["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"])
    norms = np.sqrt(np.sum(r * r, 1))
    return sc, qr, sch, dist, norms > 0.15, float(np.min(np.abs(norms - 0.15), initial=np.inf))


def write_scene(path, sc):
    """the scene file `mslam_harness --ba` reads: "MSBA", i32 version 1, K, L, M, max_iterations; K x i32 keyframe id (the
    adapter holds keyframe id 1 constant, as the reference does: the constant pose, if any, must be the first); K x 7 f64;
    L x 3 f64; M x i32 keyframe index; M x i32 landmark index; M x 3 f64 camera-frame point"""
    K, L, M = len(sc["poses"]), len(sc["landmarks"]), len(sc["obs_kf"])
    assert not sc["fixed"][1:].any()
    ids = np.arange(K, dtype="<i4") + (1 if sc["fixed"][0] else 2)
    with open(path, "wb") as f:
        f.write(b"MSBA" + np.array([1, K, L, M, sc.get("max_iterations", 100)], "<i4").tobytes())
        f.write(ids.tobytes())
        for a, dt in ((sc["poses"], "<f8"), (sc["landmarks"], "<f8"), (sc["obs_kf"], "<i4"), (sc["obs_lm"], "<i4"), (sc["obs_cam"], "<f8")):
            f.write(np.ascontiguousarray(a, dt).tobytes())
    return ids
