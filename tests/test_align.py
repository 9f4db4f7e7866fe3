"""RANSAC rigid alignment of 3-D points (mslam_hip_align_ransac; no reference counterpart) on the CPU: the numpy reference
(tests/align_ref.py) recovers ground truth, a second closed form that shares nothing with it (Horn's unit quaternion by
cyclic Jacobi sweeps, the method the kernel uses) agrees with its SVD, every scene of the GPU tests keeps its nearest point
well away from the inlier bound, and the library exports the new entry points."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_ref as ar  # noqa: E402


def rot_err(Ra, Rb):
    return np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))


def horn(S, D, sweeps=8):
    """the rigid transform of the pairs by Horn's quaternion: the eigenvector of the largest eigenvalue of the 4 x 4 matrix of
    the cross-covariance, by cyclic Jacobi sweeps (scalar arithmetic, no numpy.linalg)"""
    sbar, dbar = S.mean(0), D.mean(0)
    M = (S - sbar).T @ (D - dbar)
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = M
    A = [[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
         [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
         [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
         [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]]
    A = [[float(v) for v in row] for row in A]
    V = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for _ in range(sweeps):
        for p in range(3):
            for q in range(p + 1, 4):
                apq = A[p][q]
                if not abs(apq) > 1e-300:
                    continue
                theta = (A[q][q] - A[p][p]) / (2.0 * apq)
                if abs(theta) > 1e150:
                    t = 0.5 / theta
                else:
                    t = 1.0 / (abs(theta) + (theta * theta + 1.0) ** 0.5)
                    if theta < 0:
                        t = -t
                c = 1.0 / (t * t + 1.0) ** 0.5
                s = t * c
                for k in range(4):
                    akp, akq = A[k][p], A[k][q]
                    A[k][p], A[k][q] = c * akp - s * akq, s * akp + c * akq
                for k in range(4):
                    apk, aqk = A[p][k], A[q][k]
                    A[p][k], A[q][k] = c * apk - s * aqk, s * apk + c * aqk
                for k in range(4):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p], V[k][q] = c * vkp - s * vkq, s * vkp + c * vkq
    k = max(range(4), key=lambda i: (A[i][i], -i))
    w, x, y, z = (V[i][k] for i in range(4))
    nrm = (w * w + x * x + y * y + z * z) ** 0.5
    w, x, y, z = w / nrm, x / nrm, y / nrm, z / nrm
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return R, dbar - R @ sbar


def test_reference_recovers_ground_truth():
    for seed in range(4):
        src, dst, R, t, good = ar.scene(seed)
        res = ar.align_ransac(src, dst, ar.MAX_DISTANCE, seed=seed)
        assert res["best"] >= 0 and rot_err(res["R"], R) < 0.05 and np.linalg.norm(res["t"] - t) < 0.005
        assert (res["mask"] & ~good).sum() <= 2 and res["mask"].sum() > 0.95 * good.sum()
        assert abs(np.linalg.det(res["R"]) - 1) < 1e-12
    # pure garbage: no consensus, no model
    rng = np.random.default_rng(5)
    res = ar.align_ransac(rng.normal(size=(50, 3)) + [0, 0, 5], rng.normal(size=(50, 3)) + [0, 0, 5], 0.005, seed=1)
    assert res["best"] == -1 and res["R"] is None
    # confidence 0.99 ends a clean scene early; 1.0 looks at every hypothesis and finds the same best one or a later, larger
    src, dst, R, t, good = ar.scene(9, outliers=0.0, noise=0.0)
    early, full = ar.align_ransac(src, dst, 0.05, seed=2), ar.align_ransac(src, dst, 0.05, seed=2, confidence=1.0)
    assert early["looked_at"] < 10 and full["looked_at"] == 100 and early["best"] == full["best"] == 0


def test_second_closed_form_agrees_with_the_svd():
    """Horn's quaternion against the SVD with the determinant fix, on the consensus sets of the scenes and on every minimal
    sample the loops look at in two of them"""
    worst = 0.0
    for name, kw, it, conf in ar.shape_cases():
        src, dst = ar.scene(**kw)[:2]
        res = ar.align_ransac(src, dst, ar.MAX_DISTANCE, it, kw["seed"], conf)
        if res["best"] < 0:
            continue
        S, D = src.astype(np.float64)[res["mask"]], dst.astype(np.float64)[res["mask"]]
        R2, t2 = horn(S, D)
        worst = max(worst, np.abs(R2 - res["R"]).max(), np.abs(t2 - res["t"]).max())
        assert abs(np.linalg.det(R2) - 1) < 1e-12
    for name, (src, dst, dist, expect) in ar.edge_scenes().items():
        res = ar.align_ransac(src, dst, dist, seed=5)
        if res["best"] < 0:
            continue
        S, D = src.astype(np.float64)[res["mask"]], dst.astype(np.float64)[res["mask"]]
        R2, t2 = horn(S, D)
        worst = max(worst, np.abs(R2 - res["R"]).max(), np.abs(t2 - res["t"]).max())
    for seed in (300, 305):
        src, dst = ar.scene(seed, 400, 0.3, 0.005)[:2]
        S, D = src.astype(np.float64), dst.astype(np.float64)
        for h in range(40):
            idx = ar.sample_indices(seed, h, len(S))
            if ar.triple_ok(S[idx]) and ar.triple_ok(D[idx]):
                Ra, ta = ar.rigid(S[idx], D[idx])
                Rb, tb = horn(S[idx], D[idx])
                worst = max(worst, np.abs(Ra - Rb).max(), np.abs(ta - tb).max())
    print("worst difference between the two closed forms: %.3g" % worst)
    # two closed forms of one optimum in f64 on well-conditioned sets: rounding only (coordinates up to 7 m, a minimal
    # sample's conditioning up to ~1e3)
    assert worst < 1e-11


def test_every_gpu_scene_keeps_its_margin():
    """a condition of the GPU comparison: no point of any hypothesis the loop looks at lies within 1e-6 (relative, squared)
    of the inlier bound, so a rounding difference between two correct implementations cannot move a point across it"""
    worst = np.inf
    for name, kw, it, conf in ar.shape_cases():
        src, dst = ar.scene(**kw)[:2]
        res = ar.align_ransac(src, dst, ar.MAX_DISTANCE, it, kw["seed"], conf)
        assert res["margin"] >= 1e-6, (name, res["margin"])
        worst = min(worst, res["margin"])
    for name, (src, dst, dist, expect) in ar.edge_scenes().items():
        for conf in (0.99, 1.0):
            res = ar.align_ransac(src, dst, dist, seed=5, confidence=conf)
            assert res["margin"] >= 1e-6, (name, res["margin"])
            worst = min(worst, res["margin"])
            if expect == "no_model":
                assert res["best"] == -1, name
            elif expect != "reference":
                assert res["best"] >= 0 and np.abs(res["R"] - expect[1]).max() < 1e-5 and np.abs(res["t"] - expect[2]).max() < 1e-4, name
                assert abs(np.linalg.det(res["R"]) - 1) < 1e-12
    print("smallest margin: %.3g" % worst)


def test_edge_scenes_of_the_reference():
    e = ar.edge_scenes()
    res = ar.align_ransac(*e["mirrored"][:3], seed=5, confidence=1.0)
    # a mirrored set has no rigid explanation: whatever consensus there is stays small, and is never a reflection
    assert res["best"] == -1 or (res["mask"].sum() < 0.25 * len(res["mask"]) and abs(np.linalg.det(res["R"]) - 1) < 1e-12)
    src, dst = e["nan_point"][:2]
    res = ar.align_ransac(src, dst, ar.MAX_DISTANCE, seed=5)
    assert not res["mask"][7] and not res["mask"][31] and res["mask"].sum() == len(src) - 2
    assert all(c == -1 for c in ar.align_ransac(*e["collinear"][:3], seed=5)["counts"])


def test_library_exports_the_alignment_entry_points(pkg):
    lib = pkg.lib()
    for name in ("mslam_hip_align_ransac", "mslam_hip_align_batch_dev", "mslam_hip_get_align_view", "mslam_hip_set_track_pose",
                 "mslam_hip_get_track_pose"):
        assert hasattr(lib, name), name
        assert name in pkg.ABI_SYMBOLS
    assert lib.mslam_hip_abi_version() == 5
    assert (pkg.TRACK_POSE_PNP, pkg.TRACK_POSE_ALIGN) == (0, 1)
