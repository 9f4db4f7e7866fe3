"""The ray-cast of the dense TSDF map (mslam_hip_tsdf_raycast; no reference counterpart) on the CPU: the numpy reference
(tests/tsdf_raycast_ref.py) finds the surface of two analytic scenes within a voxel, gives the fronto-parallel plane its normal,
reproduces the hit counts its rule was prototyped with (conditions on the inputs: a degenerate scene cannot pass silently), a
scalar restatement of the rule that shares no code with the vectorised one agrees with it, and the library exports the entry
points, each of which refuses its argument errors without a GPU."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_ref as tr  # noqa: E402
import tsdf_raycast_ref as rr  # noqa: E402

I, Z = np.eye(3), np.zeros(3)


@pytest.fixture(scope="module")
def sphere():
    p, frames = tr.sphere_scene()
    return p, frames, tr.fresh(p, frames)


@pytest.fixture(scope="module")
def sphere_render(sphere):
    p, _, (S, W) = sphere
    return rr.raycast(S, W, p, I, Z, with_stats=True)


def hits_of(depth):
    return int((depth > 0).sum())


def test_sphere_depth_within_a_voxel(sphere, sphere_render):
    p, _, _ = sphere
    depth, xyz, nrm, stats = sphere_render
    assert hits_of(depth) == 388 and depth.size == 1200
    analytic = tr.render_sphere(p, I, Z).astype(np.float64) * float(p["factor"])
    both = (depth > 0) & (analytic > 0)
    err = np.abs(depth[both].astype(np.float64) - analytic[both]) / p["voxel"]
    print("sphere: %d hits, %d compared, worst %.3f voxel, median %.4f m" % (hits_of(depth), both.sum(), err.max(),
                                                                             np.median(err) * p["voxel"]))
    assert both.sum() >= 300 and err.max() <= 1.0
    # xyz is the point of the ray at that depth, and the normal points towards free space: away from the centre
    assert np.all(np.abs(xyz[..., 2][depth > 0] - depth[depth > 0]) <= 1e-6)
    have = np.linalg.norm(nrm, axis=-1) > 0
    assert have.sum() >= 200 and np.all(depth[have] > 0)
    assert np.allclose(np.linalg.norm(nrm[have], axis=-1), 1.0, atol=1e-6)
    assert np.all(np.einsum("ij,ij->i", nrm[have].astype(np.float64), xyz[have].astype(np.float64) - np.array([0, 0, 1.0])) > 0)
    # a miss is all zeros
    miss = depth == 0
    assert not xyz[miss].any() and not nrm[miss].any()


def test_tilted_plane_depth_within_a_voxel():
    p, frames = tr.shape_cases()["plane_many_groups"]
    S, W = tr.fresh(p, frames)
    depth, _, _ = rr.raycast(S, W, p, I, Z)
    assert hits_of(depth) == 1106 and depth.size == 1200
    analytic = tr.render_plane(p, I, Z, (0.4, 0.0, 1.0), 1.0).astype(np.float64) * float(p["factor"])
    both = (depth > 0) & (analytic > 0)
    err = np.abs(depth[both].astype(np.float64) - analytic[both]) / p["voxel"]
    print("tilted plane: %d compared, worst %.3f voxel" % (both.sum(), err.max()))
    assert both.sum() >= 1000 and err.max() <= 1.0


def test_fronto_parallel_plane_normals():
    p, frames = tr.plane_scene()
    S, W = tr.fresh(p, frames)
    depth, _, nrm = rr.raycast(S, W, p, I, Z)
    have = np.linalg.norm(nrm, axis=-1) > 0
    assert 0 < hits_of(depth) < depth.size and have.sum() >= 100
    assert np.abs(nrm[have].astype(np.float64) - np.array([0.0, 0.0, -1.0])).max() <= 1e-6
    assert np.abs(depth[depth > 0].astype(np.float64) - 1.0).max() / p["voxel"] <= 0.1


def test_pinned_hit_counts(sphere, sphere_render):
    p, _, (S, W) = sphere
    # the camera centre (0, 0, 0.65) inside the volume: every ray finds the sphere's front or the volume's observed shell
    assert hits_of(rr.raycast(S, W, p, I, np.array([0.0, 0.0, -0.65]), z_near=0.01)[0]) == 1200
    # rays that start in unobserved space behind the surface; a camera that looks away
    assert hits_of(rr.raycast(S, W, p, I, Z, z_near=0.9)[0]) == 0
    assert hits_of(rr.raycast(S, W, p, tr.rot(1, np.pi), np.array([0.0, 0.0, -3.0]))[0]) == 0
    assert hits_of(rr.raycast(S, W, p, I, Z, min_weight=2)[0]) == 336
    assert hits_of(rr.raycast(S, W, p, I, Z, min_weight=3)[0]) == 146
    pl, fl = tr.shape_cases()["nx_crosses_wave"]
    assert hits_of(rr.raycast(*tr.fresh(pl, fl), pl, I, Z)[0]) == 176
    # the 9 x 7 x 5 volume as shipped holds no surface; with its origin moved to z = 0.55 it does
    ps, fs = tr.shape_cases()["below_one_wave"]
    assert hits_of(rr.raycast(*tr.fresh(ps, fs), ps, I, Z)[0]) == 0
    ps, fs = tr.sphere_scene((9, 7, 5), voxel=0.1, origin=(-0.45, -0.35, 0.55), trunc=0.3)
    assert hits_of(rr.raycast(*tr.fresh(ps, fs), ps, I, Z)[0]) == 248


def test_coarse_stride_is_part_of_the_rule(sphere, sphere_render):
    p, _, (S, W) = sphere
    d4, _, _, s4 = sphere_render
    assert rr.defaults(p, I, Z)[1:] == (0.025, 4)
    d1, x1, n1, s1 = rr.raycast(S, W, p, I, Z, coarse=1, with_stats=True)
    assert int((d1 != d4).sum()) == 8
    # a stride beyond the last sample walks every sample: coarse = 1, bit for bit
    dn, xn, nn = rr.raycast(S, W, p, I, Z, coarse=s1["n_last"] + 1)
    assert dn.tobytes() == d1.tobytes() and xn.tobytes() == x1.tobytes() and nn.tobytes() == n1.tobytes()
    ratio = s1["evaluations"] / s4["evaluations"]
    print("field evaluations: coarse 4 %d, coarse 1 %d, ratio %.2f" % (s4["evaluations"], s1["evaluations"], ratio))
    assert 2.0 <= ratio <= 4.5
    # one sample: no hit
    assert hits_of(rr.raycast(S, W, p, I, Z, z_near=0.8, z_far=0.8)[0]) == 0
    assert rr.n_last_of(0.1, 3.0, 0.025) == s4["n_last"] and 0.1 + float(s4["n_last"]) * 0.025 <= 3.0 < 0.1 + float(s4["n_last"] + 1) * 0.025


def scalar_field(S, W, p, P, min_weight):
    """F(P) of include/mslam_hip.h with Python floats -> F or None"""
    n, b, w = p["dims"], [], []
    for a in range(3):
        g = (P[a] - p["origin"][a]) / p["voxel"] - 0.5
        if not g == g:
            return None
        fl = math.floor(g)
        if not (fl >= 0 and fl + 1 <= n[a] - 1):
            return None
        b.append(fl)
        w.append(g - float(fl))
    v = {}
    for dk in (0, 1):
        for dj in (0, 1):
            for di in (0, 1):
                s, wt = int(S[b[2] + dk, b[1] + dj, b[0] + di]), int(W[b[2] + dk, b[1] + dj, b[0] + di])
                if wt < min_weight:
                    return None
                v[di, dj, dk] = float(s) / float(wt)
    x = {(dj, dk): v[0, dj, dk] + w[0] * (v[1, dj, dk] - v[0, dj, dk]) for dj in (0, 1) for dk in (0, 1)}
    y = {dk: x[0, dk] + w[1] * (x[1, dk] - x[0, dk]) for dk in (0, 1)}
    return y[0] + w[2] * (y[1] - y[0])


def scalar_pixel(S, W, p, R, t, cam, px, py, z_near, z_far, step, K, min_weight):
    """the rule for one pixel, written from the text of the header: -> (z*, P) or None"""
    Cc = [-((R[0][a] * t[0] + R[1][a] * t[1]) + R[2][a] * t[2]) for a in range(3)]
    dx, dy = (float(px) - cam["principal"][0]) / cam["focal"][0], (float(py) - cam["principal"][1]) / cam["focal"][1]
    D = [(R[0][a] * dx + R[1][a] * dy) + R[2][a] for a in range(3)]
    n_last = 0
    while z_near + float(n_last + 1) * step <= z_far:
        n_last += 1
    memo = {}

    def F(n):
        if n not in memo:
            z = z_near + float(n) * step
            memo[n] = scalar_field(S, W, p, [Cc[a] + z * D[a] for a in range(3)], min_weight)
        return memo[n]

    def near(n):
        return F(n) is not None and F(n) < 32767.0
    if F(0) is not None and F(0) <= 0:
        return None
    n = 0
    while True:
        if n + K <= n_last and not near(n) and not near(n + K):
            n += K
            continue
        for m in range(n + 1, n + K + 1):
            if m > n_last:
                return None
            if F(m) is not None and F(m) <= 0:
                if F(m - 1) is None:
                    return None
                zs = (z_near + float(m - 1) * step) + (F(m - 1) / (F(m - 1) - F(m))) * step
                return zs, [Cc[a] + zs * D[a] for a in range(3)]
        n += K


@pytest.mark.parametrize("K", [1, 3, 4])
def test_vectorised_rule_equals_the_scalar_rule(sphere, K):
    p, _, (S, W) = sphere
    R, t = tr.rot(1, -0.12) @ tr.rot(0, 0.07), np.array([-0.1, 0.05, 0.02])
    cam = dict(width=23, height=17, focal=(22.0, 23.0), principal=(11.0, 8.0))
    depth, xyz, _ = rr.raycast(S, W, p, R, t, camera=cam, coarse=K, min_weight=2)
    assert 0 < hits_of(depth) < depth.size
    Rl, tl = R.tolist(), t.tolist()
    for py in range(cam["height"]):
        for px in range(cam["width"]):
            got = scalar_pixel(S, W, p, Rl, tl, cam, px, py, 0.1, 3.0, 0.025, K, 2)
            if got is None:
                assert depth[py, px] == 0 and not xyz[py, px].any(), (px, py)
            else:
                assert depth[py, px] == np.float32(got[0]) and np.array_equal(xyz[py, px], np.asarray(got[1]).astype(np.float32)), (px, py)


def test_views_file_layout(tmp_path):
    v = dict(width=23, height=17, focal=(22.0, 23.0), principal=(11.0, 8.0), z_near=0.1, z_far=3.0, step=0.025, coarse=4,
             min_weight=2, R=tr.rot(1, 0.1), t=np.array([0.1, 0.2, 0.3]))
    path = tmp_path / "views.bin"
    rr.write_views(str(path), [v, dict(v, width=40)])
    raw = path.read_bytes()
    assert raw[:8] == rr.VIEWS_MAGIC and len(raw) == 16 + 2 * (72 + 96)
    assert np.frombuffer(raw[8:16], "<i4").tolist() == [2, 0]
    assert np.frombuffer(raw[16:24], "<i4").tolist() == [23, 17] and np.frombuffer(raw[24:80], "<f8").tolist() == [22, 23, 11, 8, 0.1, 3.0, 0.025]
    assert np.frombuffer(raw[80:88], "<i4").tolist() == [4, 2] and np.frombuffer(raw[160:184], "<f8").tolist() == [0.1, 0.2, 0.3]


def test_exports_and_argument_errors(pkg):
    """the entry points exist, the parameter block has the header's layout, and what can be refused without a context is"""
    L = pkg.lib()
    assert L.mslam_hip_abi_version() == 5
    for n in ("mslam_hip_tsdf_raycast", "mslam_hip_tsdf_raycast_dev"):
        assert n in pkg.ABI_SYMBOLS
        getattr(L, n)
    assert C.sizeof(pkg.TsdfRaycastParams) == 72
    assert pkg.TsdfRaycastParams.z_near.offset == 40 and pkg.TsdfRaycastParams.coarse.offset == 64
    q = pkg.TsdfRaycastParams()
    R, t = (C.c_double * 9)(), (C.c_double * 3)()
    depth = (C.c_float * 4)(7.0, 7.0, 7.0, 7.0)
    n = C.c_int(-5)
    for form in (L.mslam_hip_tsdf_raycast, L.mslam_hip_tsdf_raycast_dev):
        assert form(None, C.byref(q), R, t, depth, None, None, C.byref(n)) == pkg.E_INVALID
        assert form(None, None, None, None, None, None, None, None) == pkg.E_INVALID
    assert list(depth) == [7.0] * 4 and n.value == -5
