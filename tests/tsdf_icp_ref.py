"""numpy restatement of frame-to-model point-to-plane ICP (include/mslam_hip.h, "frame-to-model alignment"): the frame's
vertices and normals, the pairs of one linearisation vectorised over the level's pixels, the sum tree (butterfly per run of
64, four runs per chunk of 256, chunks in ascending order), the LDL^T of the 6 x 6, the Cayley update and the level loop, with
+ - * / sqrt floor and casts only, every operation an IEEE f64 (for the depth product, f32) operation of its own — what
k_icp.hip computes, bit for bit.  Also: the room-corner scenes of the tests, and the frames file and the dump of
`mslam_harness <plugin> --dense <scene> --icp <frames>`."""
import math
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_ref as tr  # noqa: E402
import tsdf_raycast_ref as rr  # noqa: E402

CONVERGED, ITERATIONS, DEGENERATE = 0, 1, 2
LEVELS = ((4, 4), (2, 5), (1, 10))
DIST_MAX, COS_MIN, MIN_PAIRS = 0.1, math.cos(0.6), 64
CHUNK = 256
N_SUMS = 28    # 21 of A (upper triangle, row-major), 6 of g, r r
REASONS = ("no_normal", "behind", "outside", "no_model", "far", "angle")


def frame_camera(p):
    """the volume's camera as a frame camera"""
    return dict(width=p["width"], height=p["height"], focal=p["focal"], principal=p["principal"], factor=p["factor"],
                max_depth=p["max_depth"])


def frame(depth, cam):
    """-> V f64 [h][w][3], n f64 [h][w][3], has_normal bool [h][w]"""
    depth = np.asarray(depth, np.uint16)
    h, w = int(cam["height"]), int(cam["width"])
    assert depth.shape == (h, w)
    fx, fy = (float(v) for v in cam["focal"])
    cx, cy = (float(v) for v in cam["principal"])
    d = depth.astype(np.float32) * np.float32(cam["factor"])
    assert d.dtype == np.float32
    valid = (d > tr.FLT_EPSILON) & (d.astype(np.float64) <= float(cam["max_depth"]))
    z = d.astype(np.float64)
    px, py = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    with np.errstate(all="ignore"):
        V = np.stack([(px - cx) / fx * z, (py - cy) / fy * z, z], axis=-1)
    n = np.zeros((h, w, 3), np.float64)
    has = np.zeros((h, w), bool)
    if w < 3 or h < 3:
        return V, n, has
    ok = valid[1:-1, 1:-1] & valid[1:-1, 2:] & valid[1:-1, :-2] & valid[2:, 1:-1] & valid[:-2, 1:-1]
    with np.errstate(all="ignore"):
        a = V[1:-1, 2:] - V[1:-1, :-2]
        b = V[2:, 1:-1] - V[:-2, 1:-1]
        c = [b[..., 1] * a[..., 2] - b[..., 2] * a[..., 1], b[..., 2] * a[..., 0] - b[..., 0] * a[..., 2],
             b[..., 0] * a[..., 1] - b[..., 1] * a[..., 0]]
        length = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
        ok = ok & (length > 0)
        for e in range(3):
            n[1:-1, 1:-1, e] = np.where(ok, c[e] / length, 0.0)
    has[1:-1, 1:-1] = ok
    return V, n, has


def start_state(R0, t0):
    """(Q, s): the camera -> world transform of the world -> camera guess"""
    R0, t0 = np.asarray(R0, np.float64).reshape(3, 3), np.asarray(t0, np.float64).reshape(3)
    Q = [[float(R0[c, r]) for c in range(3)] for r in range(3)]
    s = [-((float(R0[0, a]) * float(t0[0]) + float(R0[1, a]) * float(t0[1])) + float(R0[2, a]) * float(t0[2])) for a in range(3)]
    return Q, s


def tree_sum(x):
    """x f64 [M][K] -> [K]: per chunk of 256 the butterfly of each run of 64 as seen from position 0, the four runs as
    ((g0 + g1) + g2) + g3, positions past M +0.0; then the chunks in ascending order, from +0.0"""
    M, K = x.shape
    C = max(1, -(-M // CHUNK))
    v = np.zeros((C * CHUNK, K), np.float64)
    v[:M] = x
    v = v.reshape(C, 4, 64, K)
    with np.errstate(all="ignore"):
        for m in (32, 16, 8, 4, 2, 1):
            v = v[:, :, :m] + v[:, :, m:2 * m]
        g = v[:, :, 0]
        chunk = ((g[:, 0] + g[:, 1]) + g[:, 2]) + g[:, 3]
        acc = np.zeros(K, np.float64)
        for c in range(C):
            acc = acc + chunk[c]
    return acc


def pairs(fr, Q, s, model, mcam, Rm, tm, stride, dist_max=DIST_MAX, cos_min=COS_MIN):
    """the level's pixels in row-major order -> (terms f64 [M][28], paired bool [M], reason int [M]: index into REASONS of
    the test that skipped the pixel, -1 for a pair)"""
    V, n, has = fr
    xyz, normal = model
    Rm, tm = np.asarray(Rm, np.float64).reshape(3, 3), np.asarray(tm, np.float64).reshape(3)
    mw, mh = int(mcam["width"]), int(mcam["height"])
    assert xyz.shape == (mh, mw, 3) and normal.shape == (mh, mw, 3) and xyz.dtype == np.float32 and normal.dtype == np.float32
    mfx, mfy = (float(v) for v in mcam["focal"])
    mcx, mcy = (float(v) for v in mcam["principal"])
    V, n, has = V[::stride, ::stride].reshape(-1, 3), n[::stride, ::stride].reshape(-1, 3), has[::stride, ::stride].reshape(-1)
    reason = np.full(len(V), -1, np.int64)

    def gate(ok, passed, k):
        reason[ok & ~passed & (reason < 0)] = k
        return ok & passed
    with np.errstate(all="ignore"):
        ok = gate(np.ones(len(V), bool), has, 0)
        X = [((Q[r][0] * V[:, 0] + Q[r][1] * V[:, 1]) + Q[r][2] * V[:, 2]) + s[r] for r in range(3)]
        N = [(Q[r][0] * n[:, 0] + Q[r][1] * n[:, 1]) + Q[r][2] * n[:, 2] for r in range(3)]
        c = [((Rm[r, 0] * X[0] + Rm[r, 1] * X[1]) + Rm[r, 2] * X[2]) + tm[r] for r in range(3)]
        ok = gate(ok, c[2] > 0, 1)
        u = (c[0] / c[2]) * mfx + mcx
        v = (c[1] / c[2]) * mfy + mcy
        uh, vh = u + 0.5, v + 0.5
        ok = gate(ok, (uh >= 0) & (uh < float(mw)) & (vh >= 0) & (vh < float(mh)), 2)
        ix = np.floor(np.where(ok, uh, 0.0)).astype(np.int64)
        iy = np.floor(np.where(ok, vh, 0.0)).astype(np.int64)
        q = xyz[iy, ix].astype(np.float64)
        m = normal[iy, ix].astype(np.float64)
        ok = gate(ok, ~((m[:, 0] == 0) & (m[:, 1] == 0) & (m[:, 2] == 0)), 3)
        e = [X[a] - q[:, a] for a in range(3)]
        ok = gate(ok, (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] <= dist_max * dist_max, 4)
        ok = gate(ok, (N[0] * m[:, 0] + N[1] * m[:, 1]) + N[2] * m[:, 2] >= cos_min, 5)
        r = (m[:, 0] * e[0] + m[:, 1] * e[1]) + m[:, 2] * e[2]
        J = [X[1] * m[:, 2] - X[2] * m[:, 1], X[2] * m[:, 0] - X[0] * m[:, 2], X[0] * m[:, 1] - X[1] * m[:, 0],
             m[:, 0], m[:, 1], m[:, 2]]
        terms = [J[i] * J[j] for i in range(6) for j in range(i, 6)] + [J[i] * r for i in range(6)] + [r * r]
        terms = np.stack([np.where(ok, t, 0.0) for t in terms], axis=-1)
    return terms, ok, reason


def linearize(fr, Q, s, model, mcam, Rm, tm, stride, dist_max=DIST_MAX, cos_min=COS_MIN):
    """-> (A21 f64 [21], g f64 [6], count, cost = sum r r)"""
    terms, ok, _ = pairs(fr, Q, s, model, mcam, Rm, tm, stride, dist_max, cos_min)
    sums = tree_sum(terms)
    return sums[:21].copy(), sums[21:27].copy(), int(ok.sum()), float(sums[27])


def tri6(r, c):
    return r * 6 - r * (r - 1) // 2 + (c - r)


def ldl_solve(A21, g):
    """A x = -g by an LDL^T without pivoting -> (x or None, pivots[6]); the pivots after a failing one stay 0.0"""
    A = [[float(A21[tri6(min(i, j), max(i, j))]) for j in range(6)] for i in range(6)]
    L = [[0.0] * 6 for _ in range(6)]
    D = [0.0] * 6
    for j in range(6):
        v = [L[j][k] * D[k] for k in range(j)]
        d = A[j][j]
        for k in range(j):
            d = d - L[j][k] * v[k]
        D[j] = d
        if not d > 0:
            return None, D
        for i in range(j + 1, 6):
            e = A[i][j]
            for k in range(j):
                e = e - L[i][k] * v[k]
            L[i][j] = e / d
    y = [0.0] * 6
    for i in range(6):
        b = -float(g[i])
        for k in range(i):
            b = b - L[i][k] * y[k]
        y[i] = b
    x = [0.0] * 6
    for i in range(5, -1, -1):
        b = y[i] / D[i]
        for k in range(i + 1, 6):
            b = b - L[k][i] * x[k]
        x[i] = b
    return x, D


def cayley_update(Q, s, x):
    a = [x[0] * 0.5, x[1] * 0.5, x[2] * 0.5]
    aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    den, one = 1.0 + aa, 1.0 - aa
    dR = [[(one + 2.0 * (a[0] * a[0])) / den, (2.0 * (a[0] * a[1]) - 2.0 * a[2]) / den, (2.0 * (a[0] * a[2]) + 2.0 * a[1]) / den],
          [(2.0 * (a[0] * a[1]) + 2.0 * a[2]) / den, (one + 2.0 * (a[1] * a[1])) / den, (2.0 * (a[1] * a[2]) - 2.0 * a[0]) / den],
          [(2.0 * (a[0] * a[2]) - 2.0 * a[1]) / den, (2.0 * (a[1] * a[2]) + 2.0 * a[0]) / den, (one + 2.0 * (a[2] * a[2])) / den]]
    Qn = [[(dR[i][0] * Q[0][j] + dR[i][1] * Q[1][j]) + dR[i][2] * Q[2][j] for j in range(3)] for i in range(3)]
    sn = [((dR[i][0] * s[0] + dR[i][1] * s[1]) + dR[i][2] * s[2]) + x[3 + i] for i in range(3)]
    return Qn, sn


def pose_of(Q, s):
    """(R, t) world -> camera of the state"""
    R = np.array([[Q[c][r] for c in range(3)] for r in range(3)], np.float64)
    t = np.array([-((Q[0][r] * s[0] + Q[1][r] * s[1]) + Q[2][r] * s[2]) for r in range(3)], np.float64)
    return R, t


RECORD = np.dtype([("level", "<i4"), ("count", "<i4"), ("cost", "<f8"), ("rot2", "<f8"), ("trans2", "<f8")])


def solve(depth, cam, model, mcam, Rm, tm, R0, t0, levels=LEVELS, dist_max=DIST_MAX, cos_min=COS_MIN, min_pairs=MIN_PAIRS,
          rot_tol=0.0, trans_tol=0.0):
    """-> dict(R, t, status, iterations, count, level, cost, pivots f64 [6], record RECORD [iterations], Q, s)"""
    R0, t0 = np.array(R0, np.float64).reshape(3, 3), np.array(t0, np.float64).reshape(3)
    fr = frame(depth, cam)
    Q, s = start_state(R0, t0)
    rows, status, count, cost, D, level = [], ITERATIONS, 0, 0.0, [0.0] * 6, 0
    for level, (stride, iterations) in enumerate(levels):
        status = ITERATIONS
        for _ in range(iterations):
            A21, g, count, cost = linearize(fr, Q, s, model, mcam, Rm, tm, stride, dist_max, cos_min)
            x, D = (None, [0.0] * 6) if count < min_pairs else ldl_solve(A21, g)
            if x is None:
                rows.append((level, count, cost, 0.0, 0.0))
                status = DEGENERATE
                break
            Q, s = cayley_update(Q, s, x)
            rot2 = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]
            trans2 = (x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]
            rows.append((level, count, cost, rot2, trans2))
            if rot2 <= rot_tol * rot_tol and trans2 <= trans_tol * trans_tol:
                status = CONVERGED
                break
        if status == DEGENERATE:
            break
    R, t = (R0, t0) if status == DEGENERATE else pose_of(Q, s)
    return dict(R=R, t=t, status=status, iterations=len(rows), count=count, level=level, cost=cost,
                pivots=np.array(D, np.float64), record=np.array(rows, RECORD), Q=np.array(Q), s=np.array(s))


def result_bytes(out):
    """mslam_hip_icp_result as the library fills it: int32 status, iterations, count, level; f64 cost, pivots[6]"""
    return struct.pack("<4i7d", out["status"], out["iterations"], out["count"], out["level"], out["cost"], *out["pivots"])


# ---- scenes ------------------------------------------------------------------------------------------------------------------
APEX = np.array([0.02, -0.03, 1.3])
TRUE_POSE = (tr.rot(1, 0.03) @ tr.rot(0, -0.02) @ tr.rot(2, 0.025), np.array([0.02, -0.01, 0.015]))


def corner_normals():
    """three mutually orthogonal unit normals, each with a z component of 1 / sqrt 3 (their horizontal parts at 30, 150 and
    270 degrees), turned 0.3 rad about z (columns)"""
    k = np.pi / 6.0 + np.arange(3) * (2.0 * np.pi / 3.0)
    B = np.stack([np.sqrt(2.0 / 3.0) * np.cos(k), np.sqrt(2.0 / 3.0) * np.sin(k), np.full(3, 1.0 / np.sqrt(3.0))])
    return tr.rot(2, 0.3) @ B


def render_corner(p, R, t, apex=APEX):
    """the depth image of the room corner: the smallest positive plane depth of the three"""
    N = corner_normals()
    d = np.stack([tr.render_plane(p, R, t, N[:, k], float(N[:, k] @ np.asarray(apex))) for k in range(3)]).astype(np.int64)
    d = np.where(d > 0, d, 1 << 20).min(axis=0)
    return np.where(d < (1 << 20), d, 0).astype(np.uint16)


def corner_scene(kind="small"):
    """-> (params, [(depth, R, t)]): the corner seen from tsdf_ref.SPHERE_POSES"""
    if kind == "small":
        p = tr.params((24, 20, 16), 0.05, (-0.6, -0.5, 0.6), 0.2)
    else:
        p = tr.params((40, 34, 24), 0.03, (-0.6, -0.51, 0.7), 0.12, width=64, height=48, focal=(64.0, 64.0), principal=(31.5, 23.5))
    return p, [(render_corner(p, R, t), R, t) for R, t in tr.SPHERE_POSES]


def pose_error(R, t, R_true, t_true):
    """(distance of the camera centres in metres, angle of the relative rotation in radians)"""
    R, R_true = np.asarray(R).reshape(3, 3), np.asarray(R_true).reshape(3, 3)
    dc = -R.T @ np.asarray(t).reshape(3) + R_true.T @ np.asarray(t_true).reshape(3)
    c = (np.trace(R @ R_true.T) - 1.0) / 2.0
    return float(np.linalg.norm(dc)), float(np.arccos(np.clip(c, -1.0, 1.0)))


# ---- the cases the GPU tests run and the CPU tests check the conditions of -----------------------------------------------
I3, Z3 = np.eye(3), np.zeros(3)
ODD = dict(width=23, height=17, focal=(22.0, 23.0), principal=(11.0, 8.0))
AWAY = (tr.rot(1, 0.05) @ tr.rot(0, -0.03), np.array([0.03, -0.02, 0.01]))
OFF = (tr.rot(2, -0.02) @ tr.rot(1, 0.01), np.array([-0.01, 0.015, 0.0]))
SIDE = (tr.rot(1, 1.2), np.zeros(3))    # a model pose that puts part of the frame behind the model camera


def world():
    """the scenes, frames and models of the cases, computed once: dict(p, frames, vol, cam, depth, model)"""
    w = dict(p={}, frames={}, vol={}, cam={}, depth={}, model={})
    for kind in ("small", "fine"):
        p, frames = corner_scene(kind)
        w["p"][kind], w["frames"][kind], w["vol"][kind] = p, frames, tr.fresh(p, frames)
        w["cam"][kind] = frame_camera(p)
        w["depth"][kind] = render_corner(p, *TRUE_POSE)
        w["model"][kind] = (rr.camera_of(p), I3, Z3) + tuple(rr.raycast(*w["vol"][kind], p, I3, Z3)[1:])
    p, vol = w["p"]["small"], w["vol"]["small"]
    p23 = dict(p, **ODD)
    w["cam"]["small23"], w["depth"]["small23"] = frame_camera(p23), render_corner(p23, *TRUE_POSE)
    big = dict(p, width=160, height=120, focal=(160.0, 160.0), principal=(79.5, 59.5))    # 75 chunks: more than one tile of partials
    w["cam"]["small160"], w["depth"]["small160"] = frame_camera(big), render_corner(big, *TRUE_POSE)
    for name, shape in (("1x1", (1, 1)), ("65x1", (1, 65))):
        w["cam"][name] = dict(frame_camera(p), width=shape[1], height=shape[0], principal=(shape[1] / 2 - 0.5, 0.0))
        w["depth"][name] = np.full(shape, 6500, np.uint16)
    w["model"]["odd"] = (ODD, I3, Z3) + tuple(rr.raycast(*vol, p, I3, Z3, camera=ODD)[1:])
    w["model"]["away"] = (rr.camera_of(p),) + AWAY + tuple(rr.raycast(*vol, p, *AWAY)[1:])
    cam, Rm, tm, xyz, nrm = w["model"]["small"]
    w["model"]["side"] = (cam,) + SIDE + (xyz, nrm)
    w["model"]["blank"] = (cam, Rm, tm, xyz, np.zeros_like(nrm))
    return w


# name -> (frame, model, guess, keywords of solve, the status it must end in or None, the skip reasons it must meet at the guess
# on the full-resolution frame)
SMALL = dict(min_pairs=16)    # level 0 of a 40 x 30 frame has 80 pixels
SOLVES = {
    "fine_default": ("fine", "fine", (I3, Z3), {}, ITERATIONS, ("no_normal", "no_model")),
    "fine_converged": ("fine", "fine", (I3, Z3), dict(rot_tol=1e-9, trans_tol=1e-9), CONVERGED, ()),
    "fine_level_ends_early": ("fine", "fine", (I3, Z3), dict(rot_tol=2e-3, trans_tol=2e-3), None, ()),
    "small_default_levels": ("small", "small", (I3, Z3), SMALL, ITERATIONS, ("no_normal", "no_model")),
    "small_one_level": ("small", "small", (I3, Z3), dict(levels=((1, 3),)), ITERATIONS, ()),
    "small_four_levels": ("small", "small", (I3, Z3), dict(levels=((3, 2), (2, 2), (3, 1), (1, 2)), min_pairs=16), ITERATIONS, ()),
    "frame_23x17": ("small23", "small", (I3, Z3), dict(levels=((2, 3), (1, 4)), min_pairs=16), ITERATIONS, ()),
    "frame_160x120": ("small160", "small", (I3, Z3), dict(levels=((4, 2), (1, 3))), ITERATIONS, ()),
    "model_23x17": ("small", "odd", (I3, Z3), SMALL, ITERATIONS, ()),
    "model_away": ("small", "away", (I3, Z3), SMALL, ITERATIONS, ("outside",)),
    "guess_off": ("small", "small", OFF, SMALL, ITERATIONS, ()),
    "tight_gates": ("small", "away", OFF, dict(levels=((1, 4),), dist_max=0.03, cos_min=0.995, min_pairs=16), ITERATIONS,
                    ("no_normal", "outside", "no_model", "far", "angle")),
    "behind": ("small", "side", (I3, Z3), dict(levels=((1, 2),), dist_max=1e150, cos_min=-1.0, min_pairs=6), None, ("behind",)),
    "min_pairs_above": ("small", "small", (I3, Z3), dict(min_pairs=2000), DEGENERATE, ()),
    "frame_1x1": ("1x1", "small", (I3, Z3), {}, DEGENERATE, ("no_normal",)),
    "frame_65x1": ("65x1", "small", (I3, Z3), {}, DEGENERATE, ("no_normal",)),
    "blank_model": ("small", "blank", (I3, Z3), SMALL, DEGENERATE, ("no_model",)),
    "dist_max_huge": ("small", "small", (I3, Z3), dict(SMALL, dist_max=1e150), ITERATIONS, ()),
    "dist_max_tiny": ("small", "small", (I3, Z3), dict(SMALL, dist_max=1e-200), DEGENERATE, ("far",)),
    "cos_min_low": ("small", "small", (I3, Z3), dict(SMALL, cos_min=-1.0), ITERATIONS, ()),
    "cos_min_high": ("small", "small", (I3, Z3), dict(SMALL, cos_min=1.0), DEGENERATE, ("angle",)),
}
# name -> (frame, model, pose, stride)
LINEARIZES = {
    "stride_1": ("small", "small", (I3, Z3), 1),
    "stride_2": ("small", "small", (I3, Z3), 2),
    "stride_3": ("small", "small", OFF, 3),
    "stride_4": ("small", "small", (I3, Z3), 4),
    "stride_beyond": ("small", "small", (I3, Z3), 64),
    "frame_23x17": ("small23", "small", (I3, Z3), 1),
    "frame_160x120": ("small160", "small", OFF, 1),
    "model_23x17_away": ("small", "odd", AWAY, 1),
    "fine": ("fine", "fine", OFF, 1),
}


def solve_case(w, name):
    frame_key, model_key, guess, kw, _, _ = SOLVES[name]
    mcam, Rm, tm, xyz, nrm = w["model"][model_key]
    return solve(w["depth"][frame_key], w["cam"][frame_key], (xyz, nrm), mcam, Rm, tm, *guess, **kw)


def linearize_case(w, name):
    frame_key, model_key, pose, stride = LINEARIZES[name]
    mcam, Rm, tm, xyz, nrm = w["model"][model_key]
    Q, s = start_state(*pose)
    return linearize(frame(w["depth"][frame_key], w["cam"][frame_key]), Q, s, (xyz, nrm), mcam, Rm, tm, stride)


# ---- the frames file and the dump of `mslam_harness <plugin> --dense <scene> --icp <frames> [--dump <path>]` -------------
FRAMES_MAGIC = b"MSTSDFI1"
ALIGN_MAGIC = b"MSTSDFA1"


def write_frames(path, frames):
    """frames: [dict(render = a view of tsdf_raycast_ref.write_views without its pose, every value explicit; levels, dist_max,
    cos_min, min_pairs, rot_tol, trans_tol; R0, t0; depth u16 [h][w] of the volume's camera)].  Little endian: magic[8]; int32
    F, 0; F x {the render (72 bytes: int32 width, height; f64 fx, fy, cx, cy, z_near, z_far, step; int32 coarse, min_weight);
    int32 n_levels, min_pairs, stride[4], iterations[4]; f64 dist_max, cos_min, rot_tol, trans_tol; f64 R0[9], t0[3]; the depth}"""
    with open(path, "wb") as f:
        f.write(FRAMES_MAGIC)
        f.write(struct.pack("<2i", len(frames), 0))
        for fr in frames:
            v = fr["render"]
            f.write(struct.pack("<2i7d2i", int(v["width"]), int(v["height"]), *(float(x) for x in v["focal"]),
                                *(float(x) for x in v["principal"]), float(v["z_near"]), float(v["z_far"]), float(v["step"]),
                                int(v["coarse"]), int(v["min_weight"])))
            levels = list(fr["levels"])
            stride = [int(a) for a, _ in levels] + [0] * (4 - len(levels))
            iterations = [int(b) for _, b in levels] + [0] * (4 - len(levels))
            f.write(struct.pack("<10i4d", len(levels), int(fr["min_pairs"]), *stride, *iterations, float(fr["dist_max"]),
                                float(fr["cos_min"]), float(fr["rot_tol"]), float(fr["trans_tol"])))
            f.write(np.concatenate([np.asarray(fr["R0"], np.float64).reshape(9), np.asarray(fr["t0"], np.float64).reshape(3)]).astype("<f8").tobytes())
            f.write(np.ascontiguousarray(fr["depth"], "<u2").tobytes())


def read_dump(path):
    """the harness's --dump of an --icp run: magic[8]; int32 F, 0; F x {f64 R[9], t[3]; int32 status, iterations, count, level;
    f64 cost, pivots[6]; int32 rows, 0; rows x RECORD} -> [dict(R, t, result = the 72 bytes of mslam_hip_icp_result, record)]"""
    raw = open(path, "rb").read()
    assert raw[:8] == ALIGN_MAGIC
    n, _ = struct.unpack_from("<2i", raw, 8)
    off, out = 16, []
    for _ in range(n):
        pose = np.frombuffer(raw, "<f8", 12, off)
        result = raw[off + 96:off + 168]
        rows, _ = struct.unpack_from("<2i", raw, off + 168)
        record = np.frombuffer(raw, RECORD, rows, off + 176)
        off += 176 + 32 * rows
        out.append(dict(R=pose[:9].reshape(3, 3), t=pose[9:], result=result, record=record))
    assert off == len(raw)
    return out
