"""The scenes the tests of mslam_hip_bundle_adjust_global's SPARSE solver share, built on ba_global_cases.trajectory, and
their reference solutions (the two sparse CPU solvers of tests/ba_global_sparse_ref.py), solved once per process or, for the
scenes above the dense cap, recorded under tests/golden/ba_global_sparse/ (tests/golden/ba_global_sparse/README.md says how).

  shuffled:K          traj:K (K >= 1000: ring:K) with the keyframe indices permuted: NATURAL is wide, RCM is chosen, and
                      blocks are written transposed
  ring:K              trajectory(K, 2, 3, K): the ring above the dense cap; ring0:K / shuffled0:K its noise-free twins
  thin:16384          trajectory(16384, 1, 2, 16384, noise = 0): the cap, 32770 observations, under an iteration cap of 3
  open:K              traj:K without the observations that wrap: a chain
  isolated            open:12 and one more free keyframe whose 8 landmarks nobody else sees: a node of degree 0
  fixed_only_partner  open:12 and one more free keyframe that shares its 8 landmarks with the constant keyframe only: degree 0 too
  two_rings           two rings of 10 and 9 free keyframes that share no landmark; both share some with the constant keyframe
  complete12          12 keyframes that all see all 40 landmarks: the whole triangle
  loop_row            open:40 and one late keyframe that sees landmarks of keyframe 1 and of keyframe 39: a long row with
                      fill-in inside it
This is test infrastructure like ba_global_cases.py (not a conftest.py, not under oracle/)."""
import functools
import hashlib
import os

import numpy as np

import ba_global_cases as bg
import ba_global_sparse_ref as bs
import ba_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ba_global_sparse")
NEW = ["shuffled:66", "open:33", "isolated", "fixed_only_partner", "two_rings", "complete12", "loop_row"]
RECORDED = ["ring:1100", "ring0:1100", "shuffled:1100", "shuffled0:1100", "thin:16384"]


def _base(K, noise=0.005):
    return bg.trajectory(K, 2, 3, K, noise=noise) if K >= 1000 else bg.trajectory(K, 3, 3, K, noise=noise)


def shuffled(sc, seed):
    """the scene with keyframe k renamed to p[k], p a permutation drawn from `seed`"""
    K = len(sc["poses"])
    p = np.random.default_rng(seed).permutation(K)
    out = dict(sc, obs_kf=p[sc["obs_kf"]].astype(np.int32))
    for key in ("poses", "truth_poses", "fixed"):
        out[key] = np.empty_like(sc[key])
        out[key][p] = sc[key]
    return out


def opened(K, noise=0.005):
    """traj:K without the wrap: group g is seen from the keyframes g .. min(g + 2, K - 1)"""
    sc = bg.trajectory(K, 3, 3, K, noise=noise)
    i = np.arange(len(sc["obs_kf"]) - 2)                    # the ring's observations follow the two of make_scene's landmark
    keep = np.r_[True, True, (i // 3) // 3 + i % 3 < K]
    return dict(sc, obs_kf=sc["obs_kf"][keep], obs_lm=sc["obs_lm"][keep], obs_cam=sc["obs_cam"][keep])


def with_keyframe(sc, seed, partners, own=8, noise=0.005, start=0.03):
    """one more free keyframe (index K) that sees `own` new landmarks, which every constant keyframe of `partners` sees
    too, and the first 3 landmarks of every free keyframe in `partners`"""
    rng = np.random.default_rng(seed)
    K, L = len(sc["poses"]), len(sc["landmarks"])
    tp = np.concatenate([ba_ref.random_rotation_quaternion(rng, 0.2), rng.uniform(-0.4, 0.4, 3)])
    sp = tp.copy()
    axis = rng.normal(size=3)
    q = ba_ref.quaternion_plus(tp[:4], start * axis / np.linalg.norm(axis))
    sp[:4], sp[4:] = q / np.linalg.norm(q), tp[4:] + start * rng.normal(size=3) / np.sqrt(3.0)
    tl = np.stack([rng.uniform(-1.5, 1.5, own), rng.uniform(-1.0, 1.0, own), rng.uniform(1.5, 4.0, own)], 1)
    constant = [k for k in partners if sc["fixed"][k]]
    kf = [K] * own + [k for k in constant for _ in range(own)]
    lm = list(range(L, L + own)) * (1 + len(constant))
    for k in partners:
        if not sc["fixed"][k]:
            mine = sc["obs_lm"][sc["obs_kf"] == k][:3]
            kf += [K] * len(mine)
            lm += mine.tolist()
    out = dict(sc, truth_poses=np.vstack([sc["truth_poses"], tp]), poses=np.vstack([sc["poses"], sp]),
               truth_landmarks=np.vstack([sc["truth_landmarks"], tl]),
               landmarks=np.vstack([sc["landmarks"], tl + start * rng.normal(size=tl.shape)]), fixed=np.r_[sc["fixed"], 0].astype(np.uint8))
    kf, lm = np.array(kf, np.int32), np.array(lm, np.int32)
    cam = ba_ref.residuals(out["truth_poses"], out["truth_landmarks"], kf, lm, np.zeros((len(kf), 3))) + noise * rng.normal(size=(len(kf), 3))
    out.update(obs_kf=np.r_[sc["obs_kf"], kf].astype(np.int32), obs_lm=np.r_[sc["obs_lm"], lm].astype(np.int32),
               obs_cam=np.vstack([sc["obs_cam"], cam]))
    return out


def two_rings():
    """keyframe 0 constant; rings of the keyframes 1 .. 10 and 11 .. 19 (groups of 3 landmarks seen from 3 keyframes in a row,
    wrapping inside the ring); keyframes 1 and 11 share 6 landmarks each with keyframe 0"""
    sc = ba_ref.make_scene(20, 1, 20, noise=0.005, views=2, start_angle=0.03, start_shift=0.03)
    rng = np.random.default_rng(21)
    kf, lm, n = [0, 0], [0, 0], 1
    for lo, size in ((1, 10), (11, 9)):
        for g in range(size):
            for _ in range(3):
                kf += [lo + (g + j) % size for j in range(3)]
                lm += [n] * 3
                n += 1
        for _ in range(6):
            kf += [0, lo]
            lm += [n] * 2
            n += 1
    kf, lm = np.array(kf[2:], np.int32), np.array(lm[2:], np.int32)
    tl = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(1.5, 4.0, n)], 1)
    cam = ba_ref.residuals(sc["truth_poses"], tl, kf, lm, np.zeros((len(kf), 3))) + 0.005 * rng.normal(size=(len(kf), 3))
    return dict(sc, truth_landmarks=tl, landmarks=tl + 0.03 * rng.normal(size=tl.shape), obs_kf=kf, obs_lm=lm, obs_cam=cam)


@functools.lru_cache(maxsize=None)
def scene(name):
    kind, _, rest = name.partition(":")
    if kind in ("ring", "ring0"):
        return _base(int(rest), 0.005 if kind == "ring" else 0.0)
    if kind in ("shuffled", "shuffled0"):
        return shuffled(_base(int(rest), 0.005 if kind == "shuffled" else 0.0), int(rest) + 7)
    if kind == "thin":
        return dict(bg.trajectory(int(rest), 1, 2, int(rest), noise=0.0), max_iterations=3)
    if kind == "open":
        return opened(int(rest))
    if kind == "isolated":
        return with_keyframe(opened(12), 5, [])
    if kind == "fixed_only_partner":
        return with_keyframe(opened(12), 6, [0])
    if kind == "two_rings":
        return two_rings()
    if kind == "complete12":
        return ba_ref.make_scene(12, 40, 12, noise=0.005, start_angle=0.03, start_shift=0.03)
    if kind == "loop_row":
        return with_keyframe(opened(40), 8, [1, 39], own=2)
    if kind == "wide":             # one landmark that 1500 keyframes see: both envelopes are the whole triangle, above the bound
        K = int(rest)
        kf = np.arange(K, dtype=np.int32)
        return dict(poses=np.tile([0, 0, 0, 1.0, 0, 0, 0], (K, 1)), landmarks=np.array([[0.0, 0.0, 2.0]]), fixed=np.zeros(K, np.uint8),
                    obs_kf=kf, obs_lm=np.zeros(K, np.int32), obs_cam=np.tile([0.0, 0.0, 2.0], (K, 1)))
    return bg.scene(name)


def digest(sc):
    h = hashlib.sha256()
    for key in ("poses", "landmarks", "fixed", "obs_kf", "obs_lm", "obs_cam"):
        h.update(np.ascontiguousarray(sc[key]).tobytes())
    return h.hexdigest()


def _path(name):
    return os.path.join(GOLDEN, name.replace(":", "_") + ".npz")


def record(name):
    """solve `name` with both CPU solvers and write the fixture (run by hand: tests/golden/ba_global_sparse/README.md): the
    "normal" solution, both summaries, the distance of the two and of "normal" to the truth.  Poses above 512 KiB go into a
    second file, so that none exceeds 1 MiB"""
    sc = scene(name)
    a, b, dist = bs.solve_pair(sc)
    seen = np.zeros(len(sc["landmarks"]), bool)
    seen[sc["obs_lm"]] = True
    truth = max(float(np.max(np.abs(a["poses"] - sc["truth_poses"]))), float(np.max(np.abs(a["landmarks"][seen] - sc["truth_landmarks"][seen]))))
    os.makedirs(GOLDEN, exist_ok=True)
    arrays = dict(landmarks=a["landmarks"], poses=a["poses"])
    if a["poses"].nbytes > 512 * 1024:
        np.savez_compressed(_path(name + "_poses"), poses=arrays.pop("poses"))
    np.savez_compressed(_path(name), digest=digest(sc), dist=dist, truth=truth,
                        summary=np.array([[r["termination"], r["iterations"], r["trace"]["rejected"]] for r in (a, b)], np.int64),
                        costs=np.array([[r["initial_cost"], r["final_cost"]] for r in (a, b)], np.float64), **arrays)
    return a, b, dist, truth


@functools.lru_cache(maxsize=None)
def recorded(name):
    """-> (scene, the "normal" solution, the "augmented" solve's summary, their distance, the "normal" solution's distance to
    the truth) of a recorded scene; the fixture must carry the digest of the scene this tree builds"""
    sc = scene(name)
    z = np.load(_path(name))
    assert str(z["digest"]) == digest(sc), "the fixture of %s was recorded for another scene" % name
    out = []
    for row, cost in zip(z["summary"].tolist(), z["costs"].tolist()):
        out.append(dict(termination=row[0], iterations=row[1], trace=dict(rejected=row[2]), initial_cost=cost[0], final_cost=cost[1]))
    out[0]["landmarks"] = z["landmarks"]
    out[0]["poses"] = z["poses"] if "poses" in z.files else np.load(_path(name + "_poses"))["poses"]
    return sc, out[0], out[1], float(z["dist"]), float(z["truth"])


@functools.lru_cache(maxsize=None)
def reference(name, loss=None):
    """-> (scene, normal solution, augmented solution, their distance, outlier mask at the normal solution); computed once
    and shared: do not write into what this returns"""
    sc = scene(name)
    a, b, dist = bs.solve_pair(sc, loss=loss)
    return sc, a, b, dist, ba_ref.outliers(a["poses"], a["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"])
