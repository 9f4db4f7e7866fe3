"""numpy restatement of the TSDF ray-cast (include/mslam_hip.h, "ray-cast of the dense TSDF map"): the field value F of every
sample of every pixel, vectorised, with + - * / sqrt floor and casts only, every operation an IEEE f64 operation of its own,
and the march's state machine per ray on top of it — what k_tsdf_raycast computes, bit for bit.  Also: the defaults of
Context.tsdf_raycast, and the views file of `mslam_harness <plugin> --dense <scene> --raycast <views>`."""
import math
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_ref as tr  # noqa: E402

Q = tr.Q


def camera_of(p):
    """the volume's own camera as a render camera"""
    return dict(width=p["width"], height=p["height"], focal=p["focal"], principal=p["principal"])


def n_last_of(z_near, z_far, step):
    """the last n with z_near + (double)n * step <= z_far"""
    n = int(math.floor((z_far - z_near) / step))
    while z_near + float(n + 1) * step <= z_far:
        n += 1
    while n > 0 and z_near + float(n) * step > z_far:
        n -= 1
    return n


def defaults(p, R, t, z_near=0.1, z_far=None, step=None, coarse=None):
    """z_far, step, coarse as Context.tsdf_raycast chooses them"""
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    if z_far is None:
        z_far = p["max_depth"]
        if not np.isfinite(z_far):
            ext = np.asarray(p["dims"], np.float64) * p["voxel"]
            mid = np.asarray(p["origin"], np.float64) + 0.5 * ext
            z_far = float(np.linalg.norm(ext) + np.linalg.norm(-R.T @ t - mid))
    if step is None:
        step = p["voxel"] / 2
    if coarse is None:
        coarse = max(1, int(math.floor(p["trunc"] / (2 * step))))
    return float(z_far), float(step), int(coarse)


def field(S, W, p, P, min_weight=1):
    """P: three arrays of one shape (world x, y, z) -> (F f64, valid bool); F is 0 where the sample is not valid"""
    nz, ny, nx = S.shape
    n = (nx, ny, nz)
    with np.errstate(all="ignore"):
        g = [(P[a] - p["origin"][a]) / p["voxel"] - 0.5 for a in range(3)]
        b = [np.floor(g[a]) for a in range(3)]
        w = [g[a] - b[a] for a in range(3)]
        inside = np.ones(g[0].shape, bool)
        for a in range(3):
            inside &= (b[a] >= 0) & (b[a] + 1 <= n[a] - 1)    # false for NaN
    i, j, k = (np.where(inside, b[a], 0).astype(np.int64) for a in range(3))
    valid = inside.copy()
    v = {}
    for dk in (0, 1):
        for dj in (0, 1):
            for di in (0, 1):
                kk, jj, ii = np.where(inside, k + dk, 0), np.where(inside, j + dj, 0), np.where(inside, i + di, 0)
                s, wt = S[kk, jj, ii], W[kk, jj, ii]
                valid &= wt >= min_weight
                with np.errstate(all="ignore"):
                    v[di, dj, dk] = s.astype(np.float64) / wt.astype(np.float64)

    def lerp(a, c, wgt):
        return a + wgt * (c - a)
    with np.errstate(all="ignore"):
        x = {(dj, dk): lerp(v[0, dj, dk], v[1, dj, dk], w[0]) for dj in (0, 1) for dk in (0, 1)}
        y = {dk: lerp(x[0, dk], x[1, dk], w[1]) for dk in (0, 1)}
        F = lerp(y[0], y[1], w[2])
    return np.where(valid, F, 0.0), valid


def raycast(S, W, p, R, t, camera=None, z_near=0.1, z_far=None, step=None, coarse=None, min_weight=1, with_stats=False):
    """-> depth f32 [h][w], xyz f32 [h][w][3], normal f32 [h][w][3] (with_stats: and a dict with `evaluations`, the number of
    field evaluations the march made, and `n_last`)"""
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    cam = camera_of(p) if camera is None else camera
    width, height = int(cam["width"]), int(cam["height"])
    fx, fy = (float(v) for v in cam["focal"])
    cx, cy = (float(v) for v in cam["principal"])
    z_far, step, K = defaults(p, R, t, z_near, z_far, step, coarse)
    z_near = float(z_near)
    n_last = n_last_of(z_near, z_far, step)
    voxel = p["voxel"]
    C = [-((R[0, a] * t[0] + R[1, a] * t[1]) + R[2, a] * t[2]) for a in range(3)]
    px, py = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    dx, dy = (px - cx) / fx, (py - cy) / fy
    D = [(R[0, a] * dx + R[1, a] * dy) + R[2, a] for a in range(3)]
    z = z_near + np.arange(n_last + 1, dtype=np.float64) * step    # [n]
    with np.errstate(all="ignore"):
        P = [C[a] + z[None, None, :] * D[a][:, :, None] for a in range(3)]
    F, valid = field(S, W, p, P, min_weight)
    near = valid & (F < Q)
    below = valid & (F <= 0)

    depth = np.zeros((height, width), np.float32)
    zs = np.zeros((height, width), np.float64)
    hit = np.zeros((height, width), bool)
    evaluations = 0
    for y in range(height):
        for x in range(width):
            nr, bl, vl, f = near[y, x], below[y, x], valid[y, x], F[y, x]
            seen = {0}
            if bl[0]:
                evaluations += 1
                continue
            n, found = 0, None
            while found is None:
                if n + K <= n_last:
                    seen.add(n + K)
                    if not nr[n] and not nr[n + K]:
                        n += K
                        continue
                for m in range(n + 1, n + K + 1):
                    if m > n_last:
                        found = -1
                        break
                    seen.add(m)
                    if bl[m]:
                        found = m if vl[m - 1] else -1
                        break
                n += K
            evaluations += len(seen)
            if found > 0:
                m = found
                hit[y, x] = True
                zs[y, x] = z[m - 1] + (f[m - 1] / (f[m - 1] - f[m])) * step
    with np.errstate(all="ignore"):
        Ph = [C[a] + zs * D[a] for a in range(3)]
    xyz = np.stack([np.where(hit, Ph[a], 0.0) for a in range(3)], axis=-1).astype(np.float32)
    depth = np.where(hit, zs, 0.0).astype(np.float32)
    h, ok = [], hit.copy()
    for a in range(3):
        hi = [Ph[e] + voxel if e == a else Ph[e] for e in range(3)]
        lo = [Ph[e] - voxel if e == a else Ph[e] for e in range(3)]
        Fh, vh = field(S, W, p, hi, min_weight)
        Fl, vl = field(S, W, p, lo, min_weight)
        ok &= vh & vl
        h.append(Fh - Fl)
    with np.errstate(all="ignore"):
        length = np.sqrt((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2])
        ok &= length > 0
        normal = np.stack([np.where(ok, h[a] / length, 0.0) for a in range(3)], axis=-1).astype(np.float32)
    if with_stats:
        return depth, xyz, normal, dict(evaluations=evaluations, n_last=n_last, hits=int(hit.sum()))
    return depth, xyz, normal


# ---- the views file of `mslam_harness <plugin> --dense <scene> --raycast <views>` --------------------------------------------
VIEWS_MAGIC = b"MSTSDFV1"
DUMP_MAGIC = b"MSTSDFR1"


def write_views(path, views):
    """views: [dict(width, height, focal, principal, z_near, z_far, step, coarse, min_weight, R, t)], every value explicit.
    Little endian: magic[8]; int32 V, 0; V x {mslam_hip_tsdf_raycast_params (72 bytes: int32 width, height; f64 fx, fy, cx, cy,
    z_near, z_far, step; int32 coarse, min_weight); f64 R[9], t[3]}"""
    with open(path, "wb") as f:
        f.write(VIEWS_MAGIC)
        f.write(struct.pack("<2i", len(views), 0))
        for v in views:
            f.write(struct.pack("<2i7d2i", int(v["width"]), int(v["height"]), *(float(x) for x in v["focal"]),
                                *(float(x) for x in v["principal"]), float(v["z_near"]), float(v["z_far"]), float(v["step"]),
                                int(v["coarse"]), int(v["min_weight"])))
            f.write(np.concatenate([np.asarray(v["R"], np.float64).reshape(9), np.asarray(v["t"], np.float64).reshape(3)]).astype("<f8").tobytes())


def read_dump(path):
    """the harness's --dump of a --raycast run: magic[8]; int32 V, 0; V x {int32 width, height, n_hits, 0; f32 depth[h][w],
    xyz[h][w][3], normal[h][w][3]} -> [(depth, xyz, normal, n_hits)]"""
    raw = open(path, "rb").read()
    assert raw[:8] == DUMP_MAGIC
    n, _ = struct.unpack_from("<2i", raw, 8)
    off, out = 16, []
    for _ in range(n):
        w, h, hits, _ = struct.unpack_from("<4i", raw, off)
        off += 16
        px = w * h
        depth = np.frombuffer(raw, "<f4", px, off).reshape(h, w)
        xyz = np.frombuffer(raw, "<f4", 3 * px, off + 4 * px).reshape(h, w, 3)
        normal = np.frombuffer(raw, "<f4", 3 * px, off + 16 * px).reshape(h, w, 3)
        off += 28 * px
        out.append((depth, xyz, normal, hits))
    assert off == len(raw)
    return out
