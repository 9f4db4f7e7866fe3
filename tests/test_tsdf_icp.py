"""Frame-to-model point-to-plane ICP (mslam_hip_icp_*, mslam_hip_tsdf_icp; no reference counterpart) on the CPU: the numpy
reference (tests/tsdf_icp_ref.py) pulls a frame of a room corner onto the ray-cast of the corner's volume, a scalar restatement
of one linearisation that shares no code with the vectorised one agrees with it byte for byte, the state stays a rotation, the
degenerate shapes end DEGENERATE with the guess returned, the cases the GPU tests run meet what they are there for (a
degenerate case cannot pass silently), and the library exports the entry points, each of which refuses what can be refused
without a GPU.

Measured with this reference (start error 26.9 mm / 44.0 mrad, the guess at identity):
  small (24 x 20 x 16 voxels of 5 cm, 40 x 30 frame, min_pairs 16: level 0 has 80 pixels and 45 pairs):
        end error 2.2 mm / 0.8 mrad, 12x / 54x better; it does not settle: nearest-pixel association flips, steps stay near 2e-3
  fine  (40 x 34 x 24 voxels of 3 cm, 64 x 48 frame, the defaults): end error 2.7 mm / 3.1 mrad, 10x / 14x better; with
        rot_tol = trans_tol = 1e-9 CONVERGED after 12 linearisations (4 + 5 + 3), the last step 4.5e-11 / 2.6e-11."""
import ctypes as C
import math
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_ref as tr  # noqa: E402
import tsdf_icp_ref as ir  # noqa: E402

I, Z = ir.I3, ir.Z3


@pytest.fixture(scope="module")
def world():
    return ir.world()


@pytest.fixture(scope="module")
def solves(world):
    return {name: ir.solve_case(world, name) for name in ir.SOLVES}


@pytest.mark.parametrize("kind,case", [("small", "small_default_levels"), ("fine", "fine_default")])
def test_converges_on_the_corner(world, solves, kind, case):
    out = solves[case]
    e0 = ir.pose_error(I, Z, *ir.TRUE_POSE)
    e1 = ir.pose_error(out["R"], out["t"], *ir.TRUE_POSE)
    print("%s: start %.1f mm / %.1f mrad, end %.2f mm / %.2f mrad: %.1fx / %.1fx; %d linearisations, %d pairs, last step %.2g / %.2g"
          % (kind, 1e3 * e0[0], 1e3 * e0[1], 1e3 * e1[0], 1e3 * e1[1], e0[0] / e1[0], e0[1] / e1[1], out["iterations"], out["count"],
             math.sqrt(out["record"]["rot2"][-1]), math.sqrt(out["record"]["trans2"][-1])))
    assert out["status"] == ir.ITERATIONS and out["iterations"] == 19
    assert e0[0] / e1[0] >= 4.0 and e0[1] / e1[1] >= 4.0
    assert e1[0] < 0.5 * world["p"][kind]["voxel"]


def test_fine_reaches_converged(solves):
    out = solves["fine_converged"]
    print("fine, tolerances 1e-9: status %d after %d linearisations, last step %.2g / %.2g"
          % (out["status"], out["iterations"], math.sqrt(out["record"]["rot2"][-1]), math.sqrt(out["record"]["trans2"][-1])))
    assert out["status"] == ir.CONVERGED and out["iterations"] < 19 and out["level"] == 2
    assert out["record"]["rot2"][-1] <= 1e-18 and out["record"]["trans2"][-1] <= 1e-18


def test_state_stays_a_rotation(solves):
    for name in ("small_default_levels", "fine_default", "guess_off"):
        Q = solves[name]["Q"]
        assert np.abs(Q.T @ Q - np.eye(3)).max() < 1e-14, name
        R = solves[name]["R"]
        assert R.tobytes() == np.ascontiguousarray(Q.T).tobytes() and abs(np.linalg.det(R) - 1.0) < 1e-13


# ---- a scalar restatement of one linearisation: loops and Python floats, no code shared with the reference ------------------
def f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def scalar_vertex(depth, cam, px, py):
    d = f32(f32(float(depth[py][px])) * float(np.float32(cam["factor"])))
    if not (d > 1.1920928955078125e-07 and d <= cam["max_depth"]):
        return None
    return ((float(px) - cam["principal"][0]) / cam["focal"][0] * d, (float(py) - cam["principal"][1]) / cam["focal"][1] * d, d)


def scalar_terms(depth, cam, px, py, Q, s, xyz, nrm, mcam, Rm, tm, dist_max, cos_min):
    """the 28 terms of the pixel, or None for a skipped one"""
    w, h = cam["width"], cam["height"]
    if not (1 <= px <= w - 2 and 1 <= py <= h - 2):
        return None
    V = scalar_vertex(depth, cam, px, py)
    nb = [scalar_vertex(depth, cam, px + 1, py), scalar_vertex(depth, cam, px - 1, py), scalar_vertex(depth, cam, px, py + 1),
          scalar_vertex(depth, cam, px, py - 1)]
    if V is None or any(v is None for v in nb):
        return None
    a = [nb[0][k] - nb[1][k] for k in range(3)]
    b = [nb[2][k] - nb[3][k] for k in range(3)]
    c = [b[1] * a[2] - b[2] * a[1], b[2] * a[0] - b[0] * a[2], b[0] * a[1] - b[1] * a[0]]
    length = math.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
    if not length > 0:
        return None
    n = [c[k] / length for k in range(3)]
    X = [((Q[r][0] * V[0] + Q[r][1] * V[1]) + Q[r][2] * V[2]) + s[r] for r in range(3)]
    N = [(Q[r][0] * n[0] + Q[r][1] * n[1]) + Q[r][2] * n[2] for r in range(3)]
    cc = [((Rm[r][0] * X[0] + Rm[r][1] * X[1]) + Rm[r][2] * X[2]) + tm[r] for r in range(3)]
    if not cc[2] > 0:
        return None
    uh = ((cc[0] / cc[2]) * mcam["focal"][0] + mcam["principal"][0]) + 0.5
    vh = ((cc[1] / cc[2]) * mcam["focal"][1] + mcam["principal"][1]) + 0.5
    if not (0 <= uh < float(mcam["width"]) and 0 <= vh < float(mcam["height"])):
        return None
    q, m = xyz[math.floor(vh)][math.floor(uh)], nrm[math.floor(vh)][math.floor(uh)]
    if m[0] == 0 and m[1] == 0 and m[2] == 0:
        return None
    e = [X[k] - q[k] for k in range(3)]
    if not (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] <= dist_max * dist_max:
        return None
    if not (N[0] * m[0] + N[1] * m[1]) + N[2] * m[2] >= cos_min:
        return None
    r = (m[0] * e[0] + m[1] * e[1]) + m[2] * e[2]
    J = [X[1] * m[2] - X[2] * m[1], X[2] * m[0] - X[0] * m[2], X[0] * m[1] - X[1] * m[0], m[0], m[1], m[2]]
    return [J[i] * J[j] for i in range(6) for j in range(i, 6)] + [J[i] * r for i in range(6)] + [r * r]


def scalar_tree(values):
    """one column of terms in pixel order -> its sum by the header's tree"""
    total = 0.0
    for c0 in range(0, max(len(values), 1), 256):
        runs = []
        for r0 in range(c0, c0 + 256, 64):
            v = [values[i] if i < len(values) else 0.0 for i in range(r0, r0 + 64)]
            m = 32
            while m >= 1:
                v = [v[p] + v[p + m] for p in range(m)]
                m //= 2
            runs.append(v[0])
        total = total + (((runs[0] + runs[1]) + runs[2]) + runs[3])
    return total


@pytest.mark.parametrize("name", ["stride_1", "stride_3", "model_23x17_away"])
def test_vectorised_rule_equals_the_scalar_rule(world, name):
    frame_key, model_key, pose, stride = ir.LINEARIZES[name]
    mcam, Rm, tm, xyz, nrm = world["model"][model_key]
    cam, depth = world["cam"][frame_key], world["depth"][frame_key].tolist()
    A, g, count, cost = ir.linearize_case(world, name)
    R0, t0 = np.asarray(pose[0]).tolist(), np.asarray(pose[1]).tolist()
    Q = [[R0[c][r] for c in range(3)] for r in range(3)]
    s = [-((R0[0][a] * t0[0] + R0[1][a] * t0[1]) + R0[2][a] * t0[2]) for a in range(3)]
    xyz_l, nrm_l = xyz.astype(np.float64).tolist(), nrm.astype(np.float64).tolist()
    rows, n = [], 0
    for py in range(0, cam["height"], stride):
        for px in range(0, cam["width"], stride):
            t = scalar_terms(depth, cam, px, py, Q, s, xyz_l, nrm_l, mcam, np.asarray(Rm).tolist(), np.asarray(tm).tolist(), ir.DIST_MAX,
                             ir.COS_MIN)
            n += t is not None
            rows.append([0.0] * 28 if t is None else t)
    sums = np.array([scalar_tree([row[k] for row in rows]) for k in range(28)])
    assert n == count and count > ir.MIN_PAIRS
    assert sums[:21].tobytes() == A.tobytes() and sums[21:27].tobytes() == g.tobytes()
    assert np.float64(sums[27]).tobytes() == np.float64(cost).tobytes()


def test_ldl_solves_the_system(world):
    A21, g, _, _ = ir.linearize_case(world, "stride_1")
    x, D = ir.ldl_solve(A21, g)
    A = np.array([[A21[ir.tri6(min(i, j), max(i, j))] for j in range(6)] for i in range(6)])
    assert np.all(np.array(D) > 0) and np.allclose(A @ np.array(x), -g, rtol=1e-9, atol=1e-9 * np.abs(g).max())
    x0, D0 = ir.ldl_solve(np.zeros(21), np.zeros(6))
    assert x0 is None and D0 == [0.0] * 6
    bad = A21.copy()
    bad[ir.tri6(2, 2)] = np.nan
    xn, Dn = ir.ldl_solve(bad, g)
    assert xn is None and Dn[0] > 0 and Dn[1] > 0 and math.isnan(Dn[2]) and Dn[3:] == [0.0] * 3


def test_degenerate_shapes_return_the_guess(world, solves):
    for name in ("frame_1x1", "frame_65x1", "blank_model", "min_pairs_above", "dist_max_tiny", "cos_min_high"):
        out, guess = solves[name], ir.SOLVES[name][2]
        assert out["status"] == ir.DEGENERATE and out["iterations"] == 1 and len(out["record"]) == 1, name
        assert out["R"].tobytes() == np.ascontiguousarray(guess[0], np.float64).tobytes(), name
        assert out["t"].tobytes() == np.ascontiguousarray(guess[1], np.float64).tobytes(), name
        assert not out["pivots"].any() and out["record"]["rot2"][0] == 0 and out["record"]["trans2"][0] == 0, name
    for name in ("frame_1x1", "frame_65x1", "blank_model"):
        assert solves[name]["count"] == 0 and solves[name]["cost"] == 0.0, name
    assert solves["min_pairs_above"]["count"] == 45


def test_the_gpu_cases_meet_their_conditions(world, solves):
    for name, (frame_key, model_key, guess, kw, status, reasons) in ir.SOLVES.items():
        out = solves[name]
        assert status is None or out["status"] == status, name
        if out["status"] != ir.DEGENERATE:
            assert np.all(out["record"]["count"] > kw.get("min_pairs", ir.MIN_PAIRS)), name
        mcam, Rm, tm, xyz, nrm = world["model"][model_key]
        Q, s = ir.start_state(*guess)
        fr = ir.frame(world["depth"][frame_key], world["cam"][frame_key])
        _, _, reason = ir.pairs(fr, Q, s, (xyz, nrm), mcam, Rm, tm, 1, kw.get("dist_max", ir.DIST_MAX), kw.get("cos_min", ir.COS_MIN))
        for r in reasons:
            assert int((reason == ir.REASONS.index(r)).sum()) >= 1, (name, r)
    met = set(r for case in ir.SOLVES.values() for r in case[5])
    assert met == set(ir.REASONS)
    # chunk edges: 1200 pixels are 4.7 chunks, 23 x 17 = 391 are 1.5, and stride 3 of 40 x 30 is 14 x 10
    assert world["depth"]["small"].size == 1200 and world["depth"]["small23"].size == 391
    assert world["depth"]["small160"].size == 75 * 256    # more than the 64 rows of partials the finish kernel stages at a time
    for name, (frame_key, _, _, stride) in ir.LINEARIZES.items():
        count = ir.linearize_case(world, name)[2]
        assert (count == 0) == (name == "stride_beyond"), name
    # a level that ends early while the solve goes on, so that later launches of the level have nothing to do
    early, levels = solves["fine_level_ends_early"]["record"]["level"], ir.LEVELS
    assert [int((early == l).sum()) for l in range(3)] == [3, 1, 1] and all(int((early == l).sum()) < levels[l][1] for l in range(3))
    assert solves["fine_level_ends_early"]["status"] == ir.CONVERGED
    # the model pose of model_away differs from the guess, the model camera of model_23x17 from the frame's
    assert world["model"]["away"][1].tobytes() != I.tobytes() and world["model"]["odd"][0]["width"] == 23
    # the two orders of the gate extremes change the pairs
    assert solves["cos_min_low"]["record"]["count"][0] > solves["small_default_levels"]["record"]["count"][0]


def test_exports_and_argument_errors(pkg):
    """the entry points exist, the blocks have the header's layout, and what can be refused without a context is"""
    L = pkg.lib()
    assert L.mslam_hip_abi_version() == 5
    names = ("mslam_hip_icp_point_plane", "mslam_hip_icp_point_plane_dev", "mslam_hip_icp_linearize", "mslam_hip_tsdf_icp",
             "mslam_hip_tsdf_icp_dev")
    for n in names:
        assert n in pkg.ABI_SYMBOLS
        getattr(L, n)
    assert C.sizeof(pkg.IcpParams) == 168 and C.sizeof(pkg.IcpResult) == 72 and pkg.ICP_RECORD.itemsize == 32
    assert pkg.IcpParams.max_depth.offset == 48 and pkg.IcpParams.mfx.offset == 64 and pkg.IcpParams.stride.offset == 96
    assert pkg.IcpParams.dist_max.offset == 128 and pkg.IcpParams.rot_tol.offset == 152 and pkg.IcpResult.pivots.offset == 24
    assert (pkg.ICP_LEVELS, pkg.ICP_DIST_MAX, pkg.ICP_COS_MIN, pkg.ICP_MIN_PAIRS) == (ir.LEVELS, ir.DIST_MAX, ir.COS_MIN, ir.MIN_PAIRS)
    assert (pkg.ICP_CONVERGED, pkg.ICP_ITERATIONS, pkg.ICP_DEGENERATE) == (ir.CONVERGED, ir.ITERATIONS, ir.DEGENERATE)
    assert pkg.ICP_RECORD == ir.RECORD
    cam = dict(width=2, height=2, focal=(1.0, 1.0), principal=(0.5, 0.5), factor=0.001, max_depth=3.0)
    q = pkg.Context.icp_params(cam, cam)
    assert q.n_levels == 3 and list(q.stride) == [4, 2, 1, 0] and list(q.iterations) == [4, 5, 10, 0] and q.min_pairs == 64
    ray = pkg.TsdfRaycastParams()
    R, t = (C.c_double * 9)(*([7.0] * 9)), (C.c_double * 3)(*([7.0] * 3))
    depth, img = (C.c_uint16 * 4)(), (C.c_float * 12)()
    res = pkg.IcpResult()
    res.status = -5
    E = pkg.E_INVALID
    for form in (L.mslam_hip_icp_point_plane, L.mslam_hip_icp_point_plane_dev):
        assert form(None, C.byref(q), depth, img, img, R, t, R, t, R, t, C.byref(res), None, 0) == E
        assert form(None, None, None, None, None, None, None, None, None, None, None, None, None, 0) == E
    for form in (L.mslam_hip_tsdf_icp, L.mslam_hip_tsdf_icp_dev):
        assert form(None, C.byref(q), C.byref(ray), depth, R, t, R, t, C.byref(res), None, 0) == E
        assert form(None, None, None, None, None, None, None, None, None, None, 0) == E
    n, cost = C.c_int(-5), C.c_double(7.0)
    assert L.mslam_hip_icp_linearize(None, C.byref(q), depth, img, img, R, t, R, t, 1, R, t, C.byref(n), C.byref(cost)) == E
    assert list(R) == [7.0] * 9 and list(t) == [7.0] * 3 and res.status == -5 and n.value == -5 and cost.value == 7.0
