"""The scenes the tests of mslam_hip_set_ba_global_pcg add to those of ba_global_cases.py and ba_global_sparse_cases.py, and
their reference solutions, solved once per process.

  revisit:K    the ring trajectory(K, 2, 3, K) plus K landmarks, each seen from three keyframes drawn at random (seeds
               from K): a map that revisits its ground.  The covisibility graph has few edges (about 6 K pairs) and no
               order with a thin envelope: at K = 1900 the envelope is above the SPARSE solver's bound and K above DENSE's
  revisit0:K   its noise-free twin: the minimum is the truth
  complete:K   K keyframes that all see all 40 landmarks (ba_global_sparse_cases' complete12 at any K): every row of the
               reduced system has K - 1 blocks
Everything else goes to ba_global_sparse_cases.scene.  This is test infrastructure (not a conftest.py, not under oracle/)."""
import functools

import numpy as np

import ba_cases
import ba_global_cases as bg
import ba_global_pcg_ref as pr
import ba_global_sparse_cases as bc
import ba_global_sparse_ref as bs
import ba_ref


def revisit(K, noise=0.005):
    sc = bg.trajectory(K, 2, 3, K, noise=noise)
    rng = np.random.default_rng(7 * K + 3)
    L0 = len(sc["landmarks"])
    tl = np.stack([rng.uniform(-1.5, 1.5, K), rng.uniform(-1.0, 1.0, K), rng.uniform(1.5, 4.0, K)], 1)
    kf = np.concatenate([np.sort(rng.choice(K, size=3, replace=False)) for _ in range(K)]).astype(np.int32)
    lm = np.repeat(L0 + np.arange(K), 3).astype(np.int32)
    truth = np.concatenate([sc["truth_landmarks"], tl])
    cam = ba_ref.residuals(sc["truth_poses"], truth, kf, lm, np.zeros((len(kf), 3))) + noise * rng.normal(size=(len(kf), 3))
    return dict(sc, truth_landmarks=truth, landmarks=np.concatenate([sc["landmarks"], tl + 0.03 * rng.normal(size=tl.shape)]),
                obs_kf=np.concatenate([sc["obs_kf"], kf]), obs_lm=np.concatenate([sc["obs_lm"], lm]), obs_cam=np.concatenate([sc["obs_cam"], cam]))


@functools.lru_cache(maxsize=None)
def scene(name):
    kind, _, rest = name.partition(":")
    if kind == "revisit":
        return revisit(int(rest))
    if kind == "revisit0":
        return revisit(int(rest), noise=0.0)
    if kind == "complete":
        return ba_ref.make_scene(int(rest), 40, int(rest), noise=0.005, start_angle=0.03, start_shift=0.03)
    try:
        return bc.scene(name)
    except KeyError:
        return ba_cases.scene(name)


def truth_error(x, sc):
    """|x - truth|_inf over the poses and the observed landmarks"""
    seen = np.zeros(len(sc["landmarks"]), bool)
    seen[sc["obs_lm"]] = True
    return max(float(np.max(np.abs(x["poses"] - sc["truth_poses"]))), float(np.max(np.abs(x["landmarks"][seen] - sc["truth_landmarks"][seen]))))


@functools.lru_cache(maxsize=None)
def pcg_reference(name, cg_max_iterations=pr.MAX_ITERATIONS, cg_tolerance=pr.TOLERANCE, loss=None):
    """-> (scene, the CPU PCG reference's solution); computed once and shared: do not write into what this returns"""
    sc = scene(name)
    return sc, pr.solve(sc, cg_max_iterations=cg_max_iterations, cg_tolerance=cg_tolerance, loss=loss)


@functools.lru_cache(maxsize=None)
def direct_reference(name, loss=None):
    """-> (scene, a direct solution, the distance of two direct solvers, the outlier mask at that solution): "qr" and "schur"
    of ba_ref on the scenes of ba_global_cases.WITH_QR and ba_cases, "normal" and "augmented" of ba_global_sparse_ref
    elsewhere"""
    if loss is None and name in bg.WITH_QR:
        sc, qr, sch, dist, mask, margin = bg.reference(name)
        return sc, qr, dist, mask
    sc = scene(name)
    a, b, dist = bs.solve_pair(sc, loss=loss)
    return sc, a, dist, ba_ref.outliers(a["poses"], a["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"])
