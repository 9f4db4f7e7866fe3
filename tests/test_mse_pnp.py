"""Min-MSE PnP (MinMseTracker, reference ceres_reprojection_error_pnp.cpp:18-110) on the CPU: the numpy restatement of
the Ceres solve (tests/mse_pnp_ref.py) against finite differences and ground truth, and the plugin's new factory.
The GPU side is tests/test_gpu_mse_pnp.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mse_pnp_ref as mr  # noqa: E402

HOST = os.path.join(ROOT, "modular-slam_amd", "host")
HARNESS = os.path.join(HOST, "mslam_harness")
PLUGIN = os.path.join(HOST, "libmslam_hip_plugin.so")
CAM = (525.0, 525.0, 319.5, 239.5)      # TUM intrinsics, rgbd_file_provider.cpp:136-145


def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def scene64(seed, n=400, outliers=0.0, noise=0.0):
    """tests/test_pnp.py's scene() construction in double precision (the reference's Vector3 / Vector2 are double): the
    ground truth x = (r, t) is the solver's own parameterisation, and noise-free image points are the functor's
    projection at it, so the true pose is a zero-residual minimum."""
    rng = np.random.default_rng(seed)
    r = rng.normal(size=3) * 0.4
    t = rng.normal(size=3) * 0.3 + np.array([0.1, -0.2, 0.5])
    obj = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(2, 7, n)], 1)
    obj = (obj - t) @ rodrigues(r)                       # world points whose camera coordinates are the box above
    x = np.concatenate([r, t])
    img = mr.project(x, obj, CAM)
    img += rng.normal(size=img.shape) * noise
    bad = rng.random(n) < outliers
    img[bad] = rng.uniform(0, [640, 480], (int(bad.sum()), 2))
    return obj, img, x


def perturbed(x, seed, scale=1.0):
    rng = np.random.default_rng(1000 + seed)
    return x + scale * np.concatenate([rng.uniform(-0.03, 0.03, 3), rng.uniform(-0.05, 0.05, 3)])


# ---- 1. derivatives of AngleAxisRotatePoint, both branches ------------------------------------------------------------
@pytest.mark.parametrize("r", [[0.3, -0.5, 0.8], [2.9, 0.4, -1.1], [1e-9, -2e-9, 3e-9], [0.0, 0.0, 0.0]])
def test_rotate_point_derivatives_match_central_differences(r):
    r = np.array(r)
    small = r @ r <= mr.DBL_EPSILON
    h = 1e-8 if small else 1e-6
    rng = np.random.default_rng(3)
    for p in rng.uniform(-3, 3, (5, 3)):
        val, jac = mr.angle_axis_rotate_point(r, p)
        assert np.allclose(val, mr.rotate_plain(r, p[None])[0], rtol=0, atol=0)
        fd = np.zeros((3, 3))
        for k in range(3):
            e = np.zeros(3)
            e[k] = h
            # both probes stay on the branch of r (theta^2 well below / above DBL_EPSILON)
            assert ((r + e) @ (r + e) <= mr.DBL_EPSILON) == small and ((r - e) @ (r - e) <= mr.DBL_EPSILON) == small
            fd[:, k] = (mr.rotate_plain(r + e, p[None])[0] - mr.rotate_plain(r - e, p[None])[0]) / (2 * h)
        assert np.allclose(jac, fd, rtol=0, atol=1e-7 if small else 1e-8), (jac, fd)
    if small:
        # the first-order branch: R p = p + r x p, whose derivative d/dr = -[p]x
        p = np.array([0.7, -1.3, 2.1])
        val, jac = mr.angle_axis_rotate_point(r, p)
        assert np.array_equal(val, p + np.cross(r, p))
        assert np.array_equal(jac, -np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]]))
    else:
        val, _ = mr.angle_axis_rotate_point(r, [0.7, -1.3, 2.1])
        assert np.allclose(val, rodrigues(r) @ [0.7, -1.3, 2.1], atol=1e-14)


def test_residual_jacobian_matches_central_differences():
    obj, img, x = scene64(5, n=20, noise=0.5)
    res, J = mr.residuals_and_jacobian(x, obj, img, CAM)
    assert np.allclose(res, img - mr.project(x, obj, CAM), rtol=0, atol=1e-12)
    fd = np.zeros_like(J)
    for k in range(6):
        e = np.zeros(6)
        e[k] = 1e-6
        fd[:, :, k] = ((img - mr.project(x + e, obj, CAM)) - (img - mr.project(x - e, obj, CAM))) / 2e-6
    assert np.allclose(J, fd, rtol=1e-6, atol=1e-4)


# ---- 2. behaviour of the restated solve ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [6, 50, 400])
def test_restatement_reaches_ground_truth_on_noise_free_scenes(n):
    for seed in range(3):
        obj, img, x = scene64(seed, n=n)
        out = mr.min_mse_pnp(obj, img, CAM, perturbed(x, seed))
        assert out["termination"] == mr.CONVERGENCE, out
        assert np.abs(out["x"] - x).max() < 1e-9, (out["x"] - x, out)
        assert out["final_cost"] < 1e-12 < out["initial_cost"]


@pytest.mark.parametrize("n,outliers", [(50, 0.0), (400, 0.0), (400, 0.2), (2000, 0.0)])
def test_restatement_stops_at_a_minimum_on_noisy_scenes(n, outliers):
    for seed in range(2):
        obj, img, x = scene64(10 + seed, n=n, outliers=outliers, noise=0.5)
        out = mr.min_mse_pnp(obj, img, CAM, perturbed(x, seed))
        assert out["termination"] == mr.CONVERGENCE, out
        assert out["gradient_max_norm"] <= 1e-8 or out["reason"] in ("parameter tolerance", "function tolerance"), out
        assert out["final_cost"] <= mr.cost(x, obj, img, CAM)
        assert out["final_cost"] <= out["initial_cost"]
        if outliers == 0.0:
            assert np.abs(out["x"] - x).max() < 0.02


def test_restatement_failure_and_empty_problem():
    obj, img, x = scene64(4, n=30)
    # a point at camera depth 0 under the start pose (r = 0: the first-order branch, R p = p exactly): FAILURE, pose kept
    x0 = np.zeros(6)
    obj0 = obj.copy()
    obj0[7] = [0.4, -0.3, 0.0]
    out = mr.min_mse_pnp(obj0, img, CAM, x0)
    assert out["termination"] == mr.FAILURE and out["iterations"] == 0 and np.array_equal(out["x"], x0)
    objn = obj.copy()
    objn[3, 1] = np.nan
    assert mr.min_mse_pnp(objn, img, CAM, x)["termination"] == mr.FAILURE
    # n = 0: no parameter blocks (solver.cc): CONVERGENCE, cost 0, parameters untouched
    out = mr.min_mse_pnp(np.zeros((0, 3)), np.zeros((0, 2)), CAM, x)
    assert out["termination"] == mr.CONVERGENCE and out["final_cost"] == 0.0 and np.array_equal(out["x"], x)


# ---- 3. the plugin's factory ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", HOST])
    return True


def test_plugin_exports_min_mse_tracker_factory(built):
    out = subprocess.check_output(["nm", "-D", PLUGIN]).decode()
    assert any(l.split()[-1] == "hipMinMseTrackerFactory" and l.split()[-2] in "DdBb" for l in out.splitlines())
    r = subprocess.run([HARNESS, PLUGIN], capture_output=True, text=True)
    assert r.returncode == 0 and "loaded ok" in r.stdout
