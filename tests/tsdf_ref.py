"""numpy restatement of the dense TSDF map (include/mslam_hip.h, "dense TSDF map"): the per-voxel integration rule and the
surface extraction, vectorised over the volume, with + - * / sqrt floor rint and casts only, every operation an IEEE f64 (or,
for the depth product, f32) operation of its own — what k_tsdf.hip computes, bit for bit.  Also: analytic depth renders of a
sphere and of a plane, the shapes the GPU tests run, and the scene file tests and the C++ harness share."""
import struct

import numpy as np

Q = 32767.0
FACTOR = np.float32(1.0 / 5000.0)
FLT_EPSILON = np.float32(1.1920928955078125e-07)
CHUNK = 64    # MSLAM_HIP_TSDF_CHUNK


def params(dims, voxel, origin, trunc=None, max_depth=3.0, max_frames=1024, width=40, height=30, factor=FACTOR, focal=(40.0, 40.0),
           principal=(19.5, 14.5)):
    return dict(dims=tuple(int(v) for v in dims), voxel=float(voxel), origin=tuple(float(v) for v in origin),
                trunc=4.0 * float(voxel) if trunc is None else float(trunc), max_depth=float(max_depth), max_frames=int(max_frames),
                width=int(width), height=int(height), factor=np.float32(factor), focal=(float(focal[0]), float(focal[1])),
                principal=(float(principal[0]), float(principal[1])))


def create_kwargs(p):
    """the keyword arguments of Context.tsdf_create for these parameters"""
    return dict(dims=p["dims"], voxel=p["voxel"], origin=p["origin"], trunc=p["trunc"], max_depth=p["max_depth"],
                max_frames=p["max_frames"], width=p["width"], height=p["height"], factor=float(p["factor"]), focal=p["focal"],
                principal=p["principal"])


def zeros(p):
    nx, ny, nz = p["dims"]
    return np.zeros((nz, ny, nx), np.int32), np.zeros((nz, ny, nx), np.int32)


def centres(p):
    """X [nx], Y [ny], Z [nz]: X = ox + ((double)i + 0.5) * voxel"""
    return tuple(p["origin"][a] + (np.arange(p["dims"][a], dtype=np.float64) + 0.5) * p["voxel"] for a in range(3))


def integrate(S, W, p, depth, R, t, sign=1):
    """applies one frame in place: depth u16 [height][width], (R, t) world -> camera, sign +1 or -1"""
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    depth = np.asarray(depth, np.uint16)
    assert depth.shape == (p["height"], p["width"])
    X, Y, Z = centres(p)
    X, Y, Z = X[None, None, :], Y[None, :, None], Z[:, None, None]
    fx, fy = p["focal"]
    cx, cy = p["principal"]
    with np.errstate(all="ignore"):
        c = [((R[r, 0] * X + R[r, 1] * Y) + R[r, 2] * Z) + t[r] for r in range(3)]
        ok = c[2] > 0
        u = (c[0] / c[2]) * fx + cx
        v = (c[1] / c[2]) * fy + cy
        uh, vh = u + 0.5, v + 0.5
        ok = ok & (uh >= 0) & (uh < float(p["width"])) & (vh >= 0) & (vh < float(p["height"]))
        px = np.floor(np.where(ok, uh, 0.0)).astype(np.int64)
        py = np.floor(np.where(ok, vh, 0.0)).astype(np.int64)
        d = depth.astype(np.float32)[py, px] * np.float32(p["factor"])
        assert d.dtype == np.float32
        ok = ok & (d > FLT_EPSILON) & (d.astype(np.float64) <= p["max_depth"])
        sdf = d.astype(np.float64) - c[2]
        ok = ok & ~(sdf < -p["trunc"])
        x = sdf / p["trunc"]
        x = np.where(x > 1.0, 1.0, x)
        q = np.rint(np.where(ok, x, 0.0) * Q).astype(np.int32)
    S += np.where(ok, np.int32(sign) * q, 0).astype(np.int32)
    W += np.where(ok, np.int32(sign), 0).astype(np.int32)
    return S, W


def fresh(p, frames):
    """frames: iterable of (depth, R, t) -> the integration into a zeroed volume"""
    S, W = zeros(p)
    for depth, R, t in frames:
        integrate(S, W, p, depth, R, t, +1)
    return S, W


def extract(S, W, p, min_weight=1, with_index=False):
    """-> xyz f32 [n][3], normal f32 [n][3] in the order (k ny + j) nx + i, then axis (with_index: and each row's voxel index)"""
    nz, ny, nx = S.shape
    obs = W >= min_weight
    with np.errstate(all="ignore"):
        f = S.astype(np.float64) / W.astype(np.float64)
    neg = S < 0

    def fwd(a, axis, fill):
        """a shifted so that position p holds a[p + e]; `fill` where p + e leaves the volume"""
        out = np.full(a.shape, fill, a.dtype)
        src = [slice(None)] * 3
        dst = [slice(None)] * 3
        src[axis], dst[axis] = slice(1, None), slice(0, -1)
        out[tuple(dst)] = a[tuple(src)]
        return out

    axes = (2, 1, 0)    # x, y, z in [nz][ny][nx]
    ok_b = [fwd(obs, ax, False) for ax in axes]
    f_b = [fwd(f, ax, 0.0) for ax in axes]
    neg_b = [fwd(neg, ax, False) for ax in axes]
    cross = np.stack([obs & ok_b[e] & (neg != neg_b[e]) for e in range(3)], axis=-1)    # [nz][ny][nx][3]
    with np.errstate(all="ignore"):
        g = [f_b[e] - f for e in range(3)]
        length = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
        has_n = ok_b[0] & ok_b[1] & ok_b[2] & (length > 0)
        nrm = np.stack([np.where(has_n, g[e] / length, 0.0) for e in range(3)], axis=-1).astype(np.float32)
        off = [(f / (f - f_b[e])) * p["voxel"] for e in range(3)]
    X, Y, Z = centres(p)
    where = np.argwhere(cross)    # rows (k, j, i, e), lexicographic: the output order
    k, j, i, e = where.T
    pts = np.stack([X[i], Y[j], Z[k]], axis=-1)
    for axis in range(3):
        sel = e == axis
        pts[sel, axis] = pts[sel, axis] + off[axis][k[sel], j[sel], i[sel]]
    if with_index:
        return pts.astype(np.float32), nrm[k, j, i], (k * ny + j) * nx + i
    return pts.astype(np.float32), nrm[k, j, i]


# ---- scenes ------------------------------------------------------------------------------------------------------------------
def rot(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    a, b = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[a, a], R[a, b], R[b, a], R[b, b] = c, -s, s, c
    return R


def _rays(p, R, t):
    """camera centre and per-pixel world directions (camera z component 1) of a world -> camera pose"""
    fx, fy = p["focal"]
    cx, cy = p["principal"]
    u, v = np.meshgrid(np.arange(p["width"], dtype=np.float64), np.arange(p["height"], dtype=np.float64))
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], axis=-1)
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    return -R.T @ t, d @ R    # row vector d times R = R^T d


def _quantise(z, p):
    raw = np.rint(np.where(np.isfinite(z) & (z > 0), z, 0.0) / float(p["factor"]))
    return np.clip(raw, 0, 65535).astype(np.uint16)


def render_sphere(p, R, t, centre=(0.0, 0.0, 1.0), radius=0.3):
    """the depth image (u16, z along the optical axis) of a sphere seen from the pose; 0 where the ray misses"""
    C, d = _rays(p, R, t)
    oc = C - np.asarray(centre, np.float64)
    a = np.einsum("hwc,hwc->hw", d, d)
    b = 2.0 * (d @ oc)
    cc = oc @ oc - radius * radius
    disc = b * b - 4.0 * a * cc
    with np.errstate(all="ignore"):
        s = (-b - np.sqrt(disc)) / (2.0 * a)
    return _quantise(np.where(disc >= 0, s, np.nan), p)


def render_plane(p, R, t, normal=(0.0, 0.0, 1.0), offset=1.0):
    """the depth image of the plane normal . x = offset"""
    C, d = _rays(p, R, t)
    n = np.asarray(normal, np.float64)
    with np.errstate(all="ignore"):
        s = (offset - n @ C) / (d @ n)
    return _quantise(s, p)


SPHERE_POSES = [(np.eye(3), np.zeros(3)), (rot(1, 0.2), np.array([0.2, 0.0, 0.05])), (rot(0, -0.15), np.array([0.0, -0.15, 0.0]))]


def sphere_scene(dims=(24, 20, 16), voxel=0.05, origin=(-0.6, -0.5, 0.6), trunc=0.2, poses=None, **kw):
    """the issue's sphere scene -> (params, [(depth, R, t), ...])"""
    p = params(dims, voxel, origin, trunc, **kw)
    poses = SPHERE_POSES if poses is None else poses
    return p, [(render_sphere(p, R, t), R, t) for R, t in poses]


def plane_scene(dims=(24, 20, 16), voxel=0.05, origin=(-0.6, -0.5, 0.6), trunc=0.2, offset=1.0, poses=None, normal=(0.0, 0.0, 1.0), **kw):
    """the plane normal . x = offset (by default fronto-parallel, z = offset) seen from the identity (and, with poses, from
    elsewhere)"""
    p = params(dims, voxel, origin, trunc, **kw)
    poses = [(np.eye(3), np.zeros(3))] if poses is None else poses
    return p, [(render_plane(p, R, t, normal, offset), R, t) for R, t in poses]


def shape_cases():
    """name -> (params, frames): the smallest volumes at which k_tsdf.hip's tiling (a wave: 16 x 4 x 1 voxels, a workgroup: 4
    of them along z; extraction: 256 consecutive voxels per workgroup) can go wrong"""
    return {
        "ny_not_block": sphere_scene((24, 20, 16)),                                  # ny = 20: 5 tiles of 4; nx = 24: a cut tile
        "below_one_wave": sphere_scene((9, 7, 5), voxel=0.1, origin=(-0.45, -0.35, 0.75), trunc=0.3),
        "nx_crosses_wave": sphere_scene((70, 9, 9), voxel=0.02, origin=(-0.7, -0.09, 0.64), trunc=0.08),
        "plane_many_groups": plane_scene((70, 40, 33), voxel=0.03, origin=(-1.05, -0.6, 0.5), trunc=0.12, normal=(0.4, 0.0, 1.0),
                                         poses=[(np.eye(3), np.zeros(3)), (rot(1, 0.1), np.array([0.05, 0.0, 0.0]))]),
    }


# ---- the scene file of `mslam_harness <plugin> --dense <scene>` --------------------------------------------------------------
SCENE_MAGIC = b"MSTSDF1\0"


def write_scene(path, p, frames, updates=(), removals=(), min_weight=1):
    """frames: [(id, depth, R, t)]; updates: [(id, R, t)] (one update_poses call); removals: [id].  Little endian:
    magic[8]; mslam_hip_tsdf_params (112 bytes); int32 F, U, M, min_weight; F x {int32 id, 0; f64 R[9], t[3]; u16
    depth[height][width]}; U x {int32 id, 0; f64 R[9], t[3]}; M x int32 id"""
    with open(path, "wb") as f:
        f.write(SCENE_MAGIC)
        f.write(struct.pack("<4i6d2ifi4d", *p["dims"], p["max_frames"], p["voxel"], *p["origin"], p["trunc"], p["max_depth"],
                            p["width"], p["height"], float(p["factor"]), 0, *p["focal"], *p["principal"]))
        f.write(struct.pack("<4i", len(frames), len(updates), len(removals), int(min_weight)))
        for fid, depth, R, t in frames:
            f.write(struct.pack("<2i", int(fid), 0))
            f.write(np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)]).astype("<f8").tobytes())
            f.write(np.ascontiguousarray(depth, "<u2").tobytes())
        for fid, R, t in updates:
            f.write(struct.pack("<2i", int(fid), 0))
            f.write(np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)]).astype("<f8").tobytes())
        f.write(np.asarray(list(removals), "<i4").tobytes())
