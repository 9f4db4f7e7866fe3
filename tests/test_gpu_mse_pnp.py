"""Min-MSE PnP on the MI355X (k_pnp_mse.hip): the single call against the numpy restatement of the Ceres solve
(tests/mse_pnp_ref.py) and ground truth, the batched device call against single calls (bit for bit), the failure paths,
and the plugin's hipMinMseTrackerFactory through the loader."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mse_pnp_ref as mr  # noqa: E402
from test_mse_pnp import CAM, HARNESS, HOST, PLUGIN, perturbed, scene64  # noqa: E402

pytestmark = pytest.mark.gpu
FOCAL, PRINCIPAL = CAM[:2], CAM[2:]


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(width=0, height=0)
    yield c
    c.close()


def _single(ctx, obj, img, x0):
    """the raw C call: (rc, rvec, tvec, termination, iterations, cost) with the caller's arrays as they come back"""
    obj = np.ascontiguousarray(obj, np.float64).reshape(-1, 3)
    img = np.ascontiguousarray(img, np.float64).reshape(-1, 2)
    r = np.array(x0[:3], np.float64)
    t = np.array(x0[3:6], np.float64)
    term, iters, cost = C.c_int(-1), C.c_int(-1), C.c_double(-1)
    rc = ctx.L.mslam_hip_pnp_min_mse(ctx._h, obj.ctypes.data_as(C.c_void_p), img.ctypes.data_as(C.c_void_p), len(obj),
                                     *[C.c_double(v) for v in CAM], r.ctypes.data_as(C.c_void_p),
                                     t.ctypes.data_as(C.c_void_p), C.byref(term), C.byref(iters), C.byref(cost))
    return rc, r, t, term.value, iters.value, cost.value


@pytest.mark.parametrize("n", [3, 6, 50, 400, 2000])
@pytest.mark.parametrize("noise,outliers", [(0.0, 0.0), (0.5, 0.0), (0.0, 0.2), (0.5, 0.2)])
def test_single_call_matches_restatement(ctx, n, noise, outliers):
    for seed in range(2):
        obj, img, x = scene64(100 * n + seed, n=n, outliers=outliers, noise=noise)
        x0 = perturbed(x, seed, scale=0.3 if n == 3 else 1.0)
        ref = mr.min_mse_pnp(obj, img, CAM, x0)
        assert ref["termination"] != mr.FAILURE, ref
        r, t, term, iters, cost = ctx.pnp_min_mse(obj, img, FOCAL, PRINCIPAL, x0[:3], x0[3:])
        got = np.concatenate([r, t])
        assert term == ref["termination"], (term, ref)
        assert abs(iters - ref["iterations"]) <= 1, (iters, ref)
        assert np.abs(got - ref["x"]).max() < 1e-6, (got - ref["x"], ref)
        assert abs(cost - ref["final_cost"]) <= 1e-6 * max(ref["final_cost"], 1e-12) + 1e-15, (cost, ref["final_cost"])
        if noise == 0.0 and outliers == 0.0:
            assert term == mr.CONVERGENCE
            # n = 3: six residuals, six parameters, a square Jacobian.  The solve ends on the parameter tolerance, whose
            # untaken last step may be up to 1e-8 (|x| + 1e-8) long, and both sides stop a few 1e-9 from the truth
            # (together within 1e-14).  Every larger n lands within 1e-9.
            tol = 1e-8 * (np.linalg.norm(x) + 1e-8) if n == 3 else 1e-9
            assert np.abs(got - x).max() < tol and np.abs(ref["x"] - x).max() < tol, (got - x, ref["x"] - x)


def test_batch_is_bit_identical_to_single_calls(ctx):
    import torch
    cap, P = 256, 1024
    rng = np.random.default_rng(77)
    ns = rng.integers(4, cap + 1, P)
    ns[:6] = [0, 1, 2, 3, cap, cap]
    obj = np.zeros((P, cap, 3))
    img = np.zeros((P, cap, 2))
    pose = np.zeros((P, 6))
    for p in range(P):
        o, i, x = scene64(5000 + p, n=cap, noise=0.5 * (p % 3 != 0), outliers=0.2 * (p % 5 == 0))
        obj[p], img[p] = o, i
        pose[p] = perturbed(x, p)
    dev = torch.device("cuda")
    d_obj = torch.from_numpy(obj).to(dev)
    d_img = torch.from_numpy(img).to(dev)
    d_n = torch.from_numpy(ns.astype(np.int32)).to(dev)
    runs = []
    for _ in range(2):
        d_pose = torch.from_numpy(pose).to(dev)
        d_info = torch.full((P, 4), -7.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ctx.pnp_min_mse_batch_dev(d_obj.data_ptr(), d_img.data_ptr(), d_n.data_ptr(), P, cap, d_pose.data_ptr(),
                                  d_info.data_ptr(), FOCAL, PRINCIPAL)
        ctx.sync()
        runs.append((d_pose.cpu().numpy(), d_info.cpu().numpy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    bpose, binfo = runs[0]
    for p in range(P):
        n = int(ns[p])
        rc, r, t, term, iters, cost = _single(ctx, obj[p, :n], img[p, :n], pose[p])
        assert rc == 0 and term != mr.FAILURE, (p, n, rc, term)
        assert binfo[p, 0] == term and binfo[p, 1] == iters and binfo[p, 3] == cost, (p, binfo[p], term, iters, cost)
        assert np.array_equal(bpose[p], np.concatenate([r, t])), p
        if n == 0:
            assert np.array_equal(bpose[p], pose[p]) and term == mr.CONVERGENCE and cost == 0.0
        if n in (1, 2):   # underdetermined: a usable, finite result whose cost did not increase
            assert np.all(np.isfinite(bpose[p])) and np.isfinite(cost) and cost <= binfo[p, 2], (p, binfo[p])


def test_failure_paths_leave_the_pose_unchanged(ctx, pkg):
    obj, img, x = scene64(4, n=30)
    obj0 = obj.copy()
    obj0[7] = [0.4, -0.3, 0.0]                              # camera depth 0 under the start pose r = 0, t = 0
    x0 = np.zeros(6)
    rc, r, t, term, iters, _ = _single(ctx, obj0, img, x0)
    assert rc == pkg.E_NO_MODEL and term == mr.FAILURE and np.array_equal(np.concatenate([r, t]), x0)
    assert mr.min_mse_pnp(obj0, img, CAM, x0)["termination"] == mr.FAILURE
    for arr, idx in ((obj, (3, 1)), (img, (5, 0))):
        bad = arr.copy()
        bad[idx] = np.nan
        args = (bad, img) if arr is obj else (obj, bad)
        rc, r, t, term, _, _ = _single(ctx, *args, x)
        assert rc == pkg.E_NO_MODEL and term == mr.FAILURE and np.array_equal(np.concatenate([r, t]), x)
    with pytest.raises(pkg.MslamHipError) as e:
        ctx.pnp_min_mse(obj0, img, FOCAL, PRINCIPAL, x0[:3], x0[3:])
    assert e.value.code == pkg.E_NO_MODEL
    rc, r, t, term, iters, cost = _single(ctx, np.zeros((0, 3)), np.zeros((0, 2)), x)
    assert rc == 0 and term == mr.CONVERGENCE and iters == 0 and cost == 0.0 and np.array_equal(np.concatenate([r, t]), x)
    # the context still works after the failures
    rc, r, t, term, _, _ = _single(ctx, obj, img, perturbed(x, 1))
    assert rc == 0 and term == mr.CONVERGENCE and np.abs(np.concatenate([r, t]) - x).max() < 1e-9


def _quat_of_rvec(r):
    th = np.linalg.norm(r)
    return np.concatenate([[np.cos(th / 2)], np.sin(th / 2) * r / th])


def _rvec_of_quat(q):
    # Eigen::AngleAxisd(q): angle 2 atan2(|v|, |w|), axis v / |v|, negated for w < 0
    nv = np.linalg.norm(q[1:])
    d = -nv if q[0] < 0 else nv
    return q[1:] / d * (2 * np.arctan2(nv, abs(q[0])))


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", HOST])
    return True


def _run_plugin(tmp_path, obj, img, position, quat, name):
    path = tmp_path / name
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(obj)))
        for P, uv in zip(obj, img):
            f.write(struct.pack("<5d", *P, *uv))
        f.write(struct.pack("<7d", *position, *quat))
        f.write(struct.pack("<4d", *CAM))
    r = subprocess.run([HARNESS, PLUGIN, "--pnp-mse", str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return [l for l in r.stdout.splitlines() if l.startswith("pnp ")][0]


@pytest.mark.parametrize("noise,outliers", [(0.0, 0.0), (0.5, 0.2)])
def test_plugin_min_mse_tracker(built, tmp_path, noise, outliers):
    """hipMinMseTrackerFactory: the MinMseTracker drop-in through the loader.  The reference's conversions are written out
    here: the initial orientation is the rotation r as Eigen::AngleAxisd(q) gives it, the initial position is the
    translation t itself (:71-75); the result's angle, axis and position are rounded to float, the axis divided by the float
    angle, and the quaternion built from them (:99-109).  A start quaternion with negative w is the same rotation."""
    obj, img, x = scene64(31, n=300, noise=noise, outliers=outliers)
    x0 = perturbed(x, 3)
    q0 = _quat_of_rvec(x0[:3])
    line = _run_plugin(tmp_path, obj, img, x0[3:], q0, "a.bin")
    assert line == _run_plugin(tmp_path, obj, img, x0[3:], -q0, "b.bin")     # -q: bit-identical result
    f = line.split()
    assert f[0:2] == ["pnp", "position"] and f[5] == "orientation" and f[10:] == ["inliers", "0"], line
    pos = np.array([float(v) for v in f[2:5]])
    q = np.array([float(v) for v in f[6:10]])
    ref = mr.min_mse_pnp(obj, img, CAM, np.concatenate([_rvec_of_quat(q0), x0[3:]]))
    assert ref["termination"] == mr.CONVERGENCE
    rr = ref["x"]
    angle = np.float32(np.sqrt(rr[:3] @ rr[:3]))
    axis = rr[:3].astype(np.float32).astype(np.float64) / np.float64(angle)
    q_ref = np.concatenate([[np.cos(0.5 * np.float64(angle))], np.sin(0.5 * np.float64(angle)) * axis])
    pos_ref = rr[3:].astype(np.float32).astype(np.float64)
    # float rounding: one float ulp of a value near 1 is 1.2e-7
    assert np.abs(pos - pos_ref).max() < 1e-6 and np.abs(q - q_ref).max() < 1e-6, (pos - pos_ref, q - q_ref)
    if noise == 0.0:
        assert np.abs(pos - x[3:]).max() < 1e-6 and np.abs(q - _quat_of_rvec(x[:3])).max() < 1e-6
