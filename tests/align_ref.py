"""numpy reference of RANSAC rigid alignment (mslam_hip_align_ransac): dst_i ~ R src_i + t.  Not a test.  It shares no code
with the product: the closed form here is the SVD of the cross-covariance with a determinant fix (Kabsch / Umeyama), where the
kernel computes Horn's quaternion by Jacobi sweeps.  The sampler and the iteration rule are the PnP oracle's (_splitmix,
update_num_iters), as the kernel's are k_pnp.hip's."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import mslam_pnp_oracle as po  # noqa: E402

M64 = (1 << 64) - 1
MODEL_POINTS = 3


def sample_indices(seed, h, n):
    """three distinct indices of hypothesis h, or None (n < 3, or more than 64 redraws of one draw)"""
    if n < 3:
        return None
    x = (seed + 0x9E3779B97F4A7C15 * (h + 1)) & M64
    idx = []
    for _ in range(3):
        tries = 0
        while True:
            x, r = po._splitmix(x)
            i = int(r % n)
            if i not in idx:
                break
            tries += 1
            if tries > 64:
                return None
        idx.append(i)
    return idx


def triple_ok(P):
    a, b = P[1] - P[0], P[2] - P[0]
    c = np.cross(a, b)
    with np.errstate(invalid="ignore", over="ignore"):
        return bool(c @ c > 1e-6 * ((a @ a) * (b @ b)))


def rigid(S, D):
    """the least-squares rigid transform of the pairs (S_i, D_i), f64 [m, 3] each: R = argmax over SO(3) of
    sum (D_i - Dbar) . R (S_i - Sbar), t = Dbar - R Sbar"""
    sbar, dbar = S.mean(0), D.mean(0)
    H = (S - sbar).T @ (D - dbar)
    U, _, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d if d != 0 else 1.0]) @ U.T
    return R, dbar - R @ sbar


def residual2(R, t, src, dst):
    r = src @ R.T + t - dst
    return np.sum(r * r, axis=1)


def align_ransac(src, dst, max_distance, iterations=100, seed=0, confidence=0.99):
    """-> dict(R, t, mask, best, counts, looked_at, margin); R, t, mask are None and best = -1 when no hypothesis reached
    4 inliers.  counts[h]: inliers of hypothesis h (-1: no hypothesis; 0 beyond looked_at).  margin: the smallest
    | |r|^2 - max_distance^2 | / max_distance^2 over every point of every hypothesis looked at, the hypothesis's own sample
    points left out (non-finite residuals too: they are on no side) — how far the nearest point is from changing sides."""
    src32, dst32 = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(dst, np.float32).reshape(-1, 3)
    S, D = src32.astype(np.float64), dst32.astype(np.float64)
    n, thr2 = len(S), float(max_distance) ** 2
    counts = np.zeros(iterations, np.int64)
    hyps = [None] * iterations
    best, bc, niters, h, margin = -1, -1, iterations, 0, np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        while h < niters:
            idx = sample_indices(seed, h, n)
            ok = idx is not None and triple_ok(S[idx]) and triple_ok(D[idx])
            if not ok:
                counts[h] = -1
            else:
                R, t = rigid(S[idx], D[idx])
                hyps[h] = (R, t)
                r2 = residual2(R, t, S, D)
                inl = r2 <= thr2
                counts[h] = int(inl.sum())
                others = np.ones(n, bool)
                others[idx] = False
                m = np.abs(r2[others] - thr2) / thr2
                m = m[np.isfinite(m)]
                if len(m):
                    margin = min(margin, float(m.min()))
                if counts[h] > max(bc, MODEL_POINTS):
                    bc, best = int(counts[h]), h
                    niters = po.update_num_iters(confidence, (n - bc) / n, MODEL_POINTS, niters)
            h += 1
    out = dict(R=None, t=None, mask=None, best=best, counts=counts, looked_at=h, margin=margin)
    if best < 0:
        return out
    R, t = hyps[best]
    with np.errstate(invalid="ignore", over="ignore"):
        mask = residual2(R, t, S, D) <= thr2
    out["mask"] = mask
    out["R"], out["t"] = rigid(S[mask], D[mask])
    return out


def rodrigues(r):
    return po.rodrigues(r)


def scene(seed, n=400, outliers=0.3, noise=0.005):
    """n pairs (src world point, dst camera point) under a random pose, modelled on tests/test_pnp.py's scene: the camera
    points fill the box x +-2, y +-1.5, z 2..7 m; `noise` metres of gaussian noise on every dst coordinate; a share
    `outliers` of the dst points is replaced by random points of the box -> (src f32, dst f32, R, t, good mask)"""
    rng = np.random.default_rng(seed)
    R = po.rodrigues(rng.normal(size=3) * 0.4)
    t = rng.normal(size=3) * 0.3 + np.array([0.1, -0.2, 0.5])
    cam = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(2, 7, n)], 1)
    src = ((cam - t) @ R).astype(np.float32)
    dst = src.astype(np.float64) @ R.T + t + rng.normal(size=(n, 3)) * noise
    bad = rng.random(n) < outliers
    k = int(bad.sum())
    dst[bad] = np.stack([rng.uniform(-2, 2, k), rng.uniform(-1.5, 1.5, k), rng.uniform(2, 7, k)], 1)
    return src, dst.astype(np.float32), R, t, ~bad


def write_scene(path, src, dst, max_distance, iterations=100, seed=0):
    """the text scene `mslam_harness --align` reads: a line `n iterations max_distance seed`, then n lines of six floats
    (src xyz, dst xyz), every float written so that it reads back to the same f32"""
    src, dst = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(dst, np.float32).reshape(-1, 3)
    with open(path, "w") as f:
        f.write("%d %d %.17g %d\n" % (len(src), iterations, max_distance, seed))
        for s, d in zip(src, dst):
            f.write(" ".join("%.9g" % v for v in (*s, *d)) + "\n")


# ---- the scenes the GPU tests run (tests/test_align.py checks each one's margin on the CPU) ---------------------------------
MAX_DISTANCE = 0.05
LDS_POINTS, LDS_HYPOTHESES = 1024, 128     # k_align.hip's kAlignLdsPts, kAlignLdsHyp: the kernel takes another path beyond


def shape_cases():
    """(name, scene arguments, iterations, confidence) of the comparison with this reference"""
    cases = []
    for n in (4, 5, 63, 64, 65, 255, 256, 257, LDS_POINTS, LDS_POINTS + 1):
        cases.append(("n%d" % n, dict(seed=100 + n, n=n, outliers=0.3 if n >= 63 else 0.0, noise=0.005), 100, 0.99))
    for it in (1, 4, 5, LDS_HYPOTHESES, LDS_HYPOTHESES + 1):
        cases.append(("it%d" % it, dict(seed=200 + it, n=300, outliers=0.3, noise=0.005), it, 1.0))
    k = 0
    for noise in (0.0, 0.005, 0.01):
        for outl in (0.0, 0.3, 0.6):
            for conf in (0.99, 1.0):
                cases.append(("noise%g_out%g_conf%g" % (noise, outl, conf), dict(seed=300 + k, n=400, outliers=outl, noise=noise),
                              100, conf))
            k += 1
    return cases


def _pose(rvec, t):
    return po.rodrigues(np.asarray(rvec, np.float64)), np.asarray(t, np.float64)


def _apply(src, R, t):
    return (src.astype(np.float64) @ R.T + t).astype(np.float32)


def edge_scenes():
    """name -> (src, dst, max_distance, expectation): expectation is "model" (with the true R, t), "no_model" or "reference"
    (whatever this reference finds)"""
    rng = np.random.default_rng(77)
    out = {}
    box = lambda m: np.stack([rng.uniform(-2, 2, m), rng.uniform(-1.5, 1.5, m), rng.uniform(2, 7, m)], 1).astype(np.float32)
    s3 = box(3)
    R, t = _pose([0.1, -0.2, 0.3], [0.2, 0.1, -0.3])
    out["n3"] = (s3, _apply(s3, R, t), MAX_DISTANCE, "no_model")
    plane = box(200)
    plane[:, 2] = 3.0
    out["coplanar"] = (plane, _apply(plane, R, t), MAX_DISTANCE, ("model", R, t))
    ax = np.array([0.3, -0.5, 0.81])
    Rg, tg = _pose(np.pi * ax / np.linalg.norm(ax), [0.1, 0.2, 0.3])
    s = box(150)
    out["rot180_generic"] = (s, _apply(s, Rg, tg), MAX_DISTANCE, ("model", Rg, tg))
    Rz, tz = _pose([0, 0, np.pi], [0.0, 0.0, 0.0])
    out["rot180_z"] = (s, _apply(s, Rz, tz), MAX_DISTANCE, ("model", Rz, tz))
    out["identity"] = (s, s.copy(), MAX_DISTANCE, ("model", np.eye(3), np.zeros(3)))
    m = box(120)
    out["mirrored"] = (m, (m * np.array([1, 1, -1], np.float32)).astype(np.float32), 0.01, "reference")
    line = (np.array([[0.1, 0.2, 3.0]]) + np.linspace(-1, 1, 80)[:, None] * np.array([[0.5, -0.3, 0.8]])).astype(np.float32)
    out["collinear"] = (line, _apply(line, R, t), MAX_DISTANCE, "no_model")
    same = np.tile(np.array([[0.4, -0.2, 3.5]], np.float32), (40, 1))
    out["coincident"] = (same, _apply(same, R, t), MAX_DISTANCE, "no_model")
    sn = box(100)
    dn = _apply(sn, R, t)
    sn[7, 1] = np.nan
    dn[31, 0] = np.nan
    out["nan_point"] = (sn, dn, MAX_DISTANCE, ("model", R, t))
    return out
