"""The dense TSDF map (mslam_hip_tsdf_*; no reference counterpart) on the CPU: the numpy reference (tests/tsdf_ref.py) keeps the
invariant "the volume equals a fresh integration of the retained frames at their poses", its surface points sit on the ground
truth of two analytic scenes, a scalar restatement of the rule that shares no code with the vectorised one agrees with it,
and the library exports the new entry points, each of which refuses a NULL context without a GPU."""
import ctypes as C
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_ref as tr  # noqa: E402


def test_reference_keeps_the_invariant():
    """three frames added, one moved, one removed == a fresh integration of what is left at the final poses"""
    p, frames = tr.sphere_scene()
    S, W = tr.zeros(p)
    for d, R, t in frames:
        tr.integrate(S, W, p, d, R, t, +1)
    assert W.max() == 3 and np.any(S < 0) and np.any(S > 0)
    d1, R1, t1 = frames[1]
    R1n, t1n = tr.rot(1, 0.23) @ R1, t1 + np.array([0.01, -0.02, 0.015])
    tr.integrate(S, W, p, d1, R1, t1, -1)
    tr.integrate(S, W, p, d1, R1n, t1n, +1)
    d2, R2, t2 = frames[2]
    tr.integrate(S, W, p, d2, R2, t2, -1)
    Sf, Wf = tr.fresh(p, [frames[0], (d1, R1n, t1n)])
    assert np.array_equal(S, Sf) and np.array_equal(W, Wf)
    # all three out again: zeros
    tr.integrate(S, W, p, frames[0][0], frames[0][1], frames[0][2], -1)
    tr.integrate(S, W, p, d1, R1n, t1n, -1)
    assert not S.any() and not W.any()


def scalar_voxel(p, depth, R, t, i, j, k):
    """the rule of include/mslam_hip.h for one voxel with Python floats -> (q, 1) or None"""
    X = p["origin"][0] + (float(i) + 0.5) * p["voxel"]
    Y = p["origin"][1] + (float(j) + 0.5) * p["voxel"]
    Z = p["origin"][2] + (float(k) + 0.5) * p["voxel"]
    c = [((float(R[r][0]) * X + float(R[r][1]) * Y) + float(R[r][2]) * Z) + float(t[r]) for r in range(3)]
    if not c[2] > 0:
        return None
    uh = ((c[0] / c[2]) * p["focal"][0] + p["principal"][0]) + 0.5
    vh = ((c[1] / c[2]) * p["focal"][1] + p["principal"][1]) + 0.5
    if not (0 <= uh < float(p["width"]) and 0 <= vh < float(p["height"])):
        return None
    d = np.float32(depth[int(math.floor(vh)), int(math.floor(uh))]) * np.float32(p["factor"])
    if not (d > tr.FLT_EPSILON and float(d) <= p["max_depth"]):
        return None
    sdf = float(d) - c[2]
    if sdf < -p["trunc"]:
        return None
    x = min(sdf / p["trunc"], 1.0)
    return int(round(x * 32767.0)), 1    # Python's round is half to even


def test_vectorised_rule_equals_the_scalar_rule():
    p, frames = tr.sphere_scene((9, 7, 5), voxel=0.1, origin=(-0.45, -0.35, 0.75), trunc=0.3)
    for d, R, t in frames:
        S, W = tr.fresh(p, [(d, R, t)])
        for k in range(5):
            for j in range(7):
                for i in range(9):
                    got = scalar_voxel(p, d, R, t, i, j, k)
                    assert (S[k, j, i], W[k, j, i]) == (got if got else (0, 0)), (i, j, k)


def test_sphere_points_sit_on_the_sphere():
    p, frames = tr.sphere_scene()
    S, W = tr.fresh(p, frames)
    xyz, nrm = tr.extract(S, W, p)
    assert len(xyz) >= 100
    rel = xyz.astype(np.float64) - np.array([0.0, 0.0, 1.0])
    err = np.abs(np.linalg.norm(rel, axis=1) - 0.3) / p["voxel"]
    print("sphere: %d points, worst error %.3f voxel" % (len(xyz), err.max()))
    assert err.max() <= 0.5
    # the normal points from behind the surface towards free space: away from the centre
    have = np.linalg.norm(nrm, axis=1) > 0
    assert have.sum() >= 50
    assert np.allclose(np.linalg.norm(nrm[have], axis=1), 1.0, atol=1e-6)
    assert np.all(np.einsum("ij,ij->i", nrm[have], rel[have]) > 0)
    # min_weight = 2 keeps a subset, in the same order
    xyz2, _ = tr.extract(S, W, p, min_weight=2)
    assert 0 < len(xyz2) < len(xyz)
    rows = {r.tobytes() for r in xyz}
    assert all(r.tobytes() in rows for r in xyz2)


def test_plane_points_and_normals():
    p, frames = tr.plane_scene()
    S, W = tr.fresh(p, frames)
    xyz, nrm = tr.extract(S, W, p)
    assert len(xyz) >= 100
    assert np.abs(xyz[:, 2].astype(np.float64) - 1.0).max() / p["voxel"] <= 0.1
    have = np.linalg.norm(nrm, axis=1) > 0
    assert have.sum() >= 50
    assert np.abs(nrm[have].astype(np.float64) - np.array([0.0, 0.0, -1.0])).max() <= 1e-6


def test_extraction_order_and_empty_volume():
    p, frames = tr.sphere_scene()
    S, W = tr.zeros(p)
    xyz, nrm = tr.extract(S, W, p)
    assert xyz.shape == (0, 3) and nrm.shape == (0, 3)
    S, W = tr.fresh(p, frames)
    xyz, _, idx = tr.extract(S, W, p, with_index=True)
    assert np.all(np.diff(idx) >= 0) and len(np.unique(idx)) < len(idx)    # ascending voxel index, several axes per voxel
    # a row lies within one voxel of its voxel's centre, along one axis
    X, Y, Z = tr.centres(p)
    nx, ny, nz = p["dims"]
    ctr = np.stack([X[idx % nx], Y[idx // nx % ny], Z[idx // (nx * ny)]], axis=-1)
    off = np.abs(xyz.astype(np.float64) - ctr) / p["voxel"]
    assert np.all((off > 1e-6).sum(axis=1) <= 1) and off.max() <= 1.0 + 1e-6
    # the plane scene of the GPU tests spreads its rows over many of the extraction's 256-voxel workgroups
    p, frames = tr.shape_cases()["plane_many_groups"]
    groups = np.unique(tr.extract(*tr.fresh(p, frames), p, 1, with_index=True)[2] // 256)
    assert len(groups) >= 64


def test_exports_and_null_context(pkg):
    L = pkg.lib()
    assert L.mslam_hip_abi_version() == 5
    names = ["mslam_hip_tsdf_create", "mslam_hip_tsdf_destroy", "mslam_hip_tsdf_info", "mslam_hip_tsdf_add_frame",
             "mslam_hip_tsdf_add_frame_dev", "mslam_hip_tsdf_get_frame", "mslam_hip_tsdf_update_poses", "mslam_hip_tsdf_remove_frame",
             "mslam_hip_tsdf_read", "mslam_hip_tsdf_extract"]
    for n in names:
        assert n in pkg.ABI_SYMBOLS
        getattr(L, n)
    assert C.sizeof(pkg.TsdfParams) == 112
    assert (pkg.TSDF_CHUNK, pkg.TSDF_MAX_VOXELS, pkg.TSDF_MAX_FRAMES) == (64, 1 << 30, 32768)
    p = pkg.TsdfParams()
    R, t = (C.c_double * 9)(), (C.c_double * 3)()
    depth = (C.c_uint16 * 4)()
    ids = (C.c_int32 * 1)()
    n = C.c_int(0)
    buf = (C.c_int32 * 4)()
    xyz = (C.c_float * 3)()
    E = pkg.E_INVALID
    assert L.mslam_hip_tsdf_create(None, C.byref(p)) == E
    assert L.mslam_hip_tsdf_destroy(None) == E
    assert L.mslam_hip_tsdf_info(None, C.byref(p), C.byref(n)) == E
    assert L.mslam_hip_tsdf_add_frame(None, 0, depth, R, t) == E
    assert L.mslam_hip_tsdf_add_frame_dev(None, 0, depth, R, t) == E
    assert L.mslam_hip_tsdf_get_frame(None, 0, R, t) == E
    assert L.mslam_hip_tsdf_update_poses(None, ids, R, t, 1, C.byref(n)) == E
    assert L.mslam_hip_tsdf_remove_frame(None, 0) == E
    assert L.mslam_hip_tsdf_read(None, buf, buf) == E
    assert L.mslam_hip_tsdf_extract(None, 1, xyz, xyz, 1, C.byref(n)) == E


def test_scene_file_layout(tmp_path):
    p, frames = tr.sphere_scene()
    path = tmp_path / "scene.bin"
    tr.write_scene(str(path), p, [(10 + q, d, R, t) for q, (d, R, t) in enumerate(frames)],
                   updates=[(11, frames[0][1], frames[0][2])], removals=[12], min_weight=2)
    raw = path.read_bytes()
    per_frame = 8 + 96 + 2 * p["width"] * p["height"]
    assert raw[:8] == tr.SCENE_MAGIC
    assert len(raw) == 8 + 112 + 16 + 3 * per_frame + (8 + 96) + 4
    assert np.frombuffer(raw[8:24], "<i4").tolist() == [24, 20, 16, p["max_frames"]]
    assert np.frombuffer(raw[120:136], "<i4").tolist() == [3, 1, 1, 2]
