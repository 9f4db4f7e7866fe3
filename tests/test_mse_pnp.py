"""Min-MSE PnP (MinMseTracker, reference ceres_reprojection_error_pnp.cpp:18-110) on the CPU: the numpy restatement of
the Ceres solve (tests/mse_pnp_ref.py) against finite differences and ground truth, and the plugin's new factory.
The GPU side is tests/test_gpu_mse_pnp.py.  Section 3 builds the edge cases that tests/test_gpu_mse_pnp_edges.py runs on
the device, and proves here, from the reference's own path counters and without a GPU, that each case takes the path it
is named for and that two independently written CPU solvers (QR and normal equations) agree on it."""
import functools
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


# ---- 3. the edge cases of the GPU suite, proved on the CPU -------------------------------------------------------------
CAM2 = (610.5, 455.25, 301.0, 255.5)                     # fx != fy, cx != cy: a swap inside the residual shows
BOUNDARY_AXIS = np.array([0.6, -0.48, 0.64])             # unit; theta^2 = DBL_EPSILON at |r| = 1.49e-8
OVERFLOW = "overflow"

EDGE_FAMILIES = {
    "large": ["large:%d:%d" % (scale, seed) for scale in (10, 30, 100) for seed in (0, 1)],
    "half": ["half:0", "half:9"],
    "full": ["full:0", "full:1"],
    "first": ["first:zeros", "first:t", "first:tiny"],
    "boundary": ["boundary:%g" % m for m in (1.0e-8, 1.4e-8, 1.6e-8, 2.0e-8, 1e-6)],
    "cam2": ["cam2"],
    "ill": ["ill:planar", "ill:line", "ill:x1000", "ill:repeated"] + ["few:%d" % n for n in (1, 2, 3, 4, 5)],
    "stride": ["stride:%d" % n for n in (63, 64, 65, 127, 128, 129, 4097)],
}
EDGE_CASES = [name for names in EDGE_FAMILIES.values() for name in names]
# the cases that run all 50 iterations, and the ones with rejected steps that still converge
MAX_ITERATION_CASES = ["large:30:1", "large:100:0", "half:0", "half:9"]
REJECTING_CONVERGING_CASES = ["large:100:1"]


def _lengthened(x, angle):
    """x with its rotation vector made `angle` longer along its own axis"""
    r = x[:3]
    return np.concatenate([r * (1.0 + angle / np.linalg.norm(r)), x[3:]])


def _world_points(camera_points, x):
    return (camera_points - x[3:]) @ rodrigues(x[:3])


@functools.lru_cache(maxsize=None)
def edge_case(name):
    """(obj, img, cam, x0, x_true) of one named edge case; the arrays are shared between the tests and read-only.
    Every case is scene64 / perturbed / mr.project at n = 65 unless its name says otherwise."""
    family, *arg = name.split(":")
    cam = CAM
    if family == "large":                                 # a start far from the minimum: rejected steps, the iteration cap
        scale, seed = int(arg[0]), int(arg[1])
        obj, img, x = scene64(50 + seed, n=65, noise=0.5)
        x0 = perturbed(x, seed, scale)
    elif family in ("half", "full"):                      # the start rotation half a turn / a whole turn off
        seed = int(arg[0])
        obj, img, x = scene64(50 + seed, n=65, noise=0.5)
        x0 = _lengthened(x, np.pi if family == "half" else 2 * np.pi)
    elif family == "first":                               # the start on the first-order branch p + r x p
        obj, img, x = scene64(50, n=65, noise=0.5)
        x0 = {"zeros": np.zeros(6), "t": np.concatenate([np.zeros(3), x[3:]]),
              "tiny": np.concatenate([[1e-9, -2e-9, 3e-9], x[3:]])}[arg[0]]
    elif family == "boundary":                            # a minimum below theta^2 = DBL_EPSILON, starts on both sides
        obj, _, xs = scene64(50, n=65)
        x = np.concatenate([1.2e-8 * BOUNDARY_AXIS, xs[3:]])
        obj = _world_points(mr.rotate_plain(xs[:3], obj) + xs[3:], x)
        img = mr.project(x, obj, cam)
        x0 = perturbed(x, 0)
        x0[:3] = float(arg[0]) * BOUNDARY_AXIS
    elif family == "cam2":
        cam = CAM2
        obj, _, x = scene64(50, n=65)
        img = mr.project(x, obj, cam)
        x0 = perturbed(x, 0)
    elif family == "ill":                                 # ill-conditioned geometry, noise-free but for `repeated`
        obj, _, x = scene64(50, n=65)
        pc = mr.rotate_plain(x[:3], obj) + x[3:]
        x0 = perturbed(x, 0)
        if arg[0] == "planar":
            pc[:, 2] = 4.0
        elif arg[0] == "line":
            pc = np.array([0.2, -0.1, 4.0]) + np.linspace(-1, 1, 65)[:, None] * np.array([1.5, 0.7, 1.0])
        elif arg[0] == "x1000":                           # the scene and the start error 1000 times as large
            pc = pc * 1000.0
            x0[3:] = (x[3:] + (x0[3:] - x[3:])) * 1000.0
            x = np.concatenate([x[:3], x[3:] * 1000.0])
        elif arg[0] == "repeated":
            pc = np.repeat(pc[:1], 65, 0)
        obj = _world_points(pc, x)
        img = mr.project(x, obj, cam)
        if arg[0] == "repeated":
            img = img + np.random.default_rng(7).normal(size=img.shape) * 0.5
    elif family == "few":
        n = int(arg[0])
        obj, img, x = scene64(50 + n, n=n)
        x0 = perturbed(x, n, 0.3)
    elif family == "stride":                              # n around the multiples of the 64 lanes
        n = int(arg[0])
        obj, img, x = scene64(50 + n, n=n, noise=0.5, outliers=0.1)
        x0 = perturbed(x, n % 7)
    elif family == OVERFLOW:
        # a finite Jacobian entry whose square is not: 10 points at depth 4, one at X = 1, Z = 1e-150 under the start
        # zeros(6), where d(fx X / Z)/dZ = -525e300
        rng = np.random.default_rng(11)
        obj = np.stack([rng.uniform(-2, 2, 10), rng.uniform(-1.5, 1.5, 10), np.full(10, 4.0)], 1)
        x = np.zeros(6)
        img = mr.project(x, obj, cam)
        obj[4] = [1.0, obj[4, 1], 1e-150]
        x0 = np.zeros(6)
    else:
        raise KeyError(name)
    for a in (obj, img, x0, x):
        a.setflags(write=False)
    return obj, img, cam, x0, x


@functools.lru_cache(maxsize=None)
def edge_solves(name):
    """the two CPU solves of a case, computed once: (QR, normal equations)"""
    obj, img, cam, x0, _ = edge_case(name)
    return mr.min_mse_pnp(obj, img, cam, x0), mr.min_mse_pnp(obj, img, cam, x0, linear_solver="normal")


def solver_drift(name):
    """|x_normal - x_qr|_inf: how far two correct solvers end apart on the case"""
    qr, normal = edge_solves(name)
    return float(np.abs(normal["x"] - qr["x"]).max())


@pytest.mark.parametrize("name", EDGE_CASES)
def test_edge_case_takes_its_named_path_and_the_two_solvers_agree(name):
    qr, normal = edge_solves(name)
    obj, img, cam, x0, x = edge_case(name)
    t = qr["trace"]
    family = name.split(":")[0]
    assert qr["termination"] == normal["termination"] and abs(qr["iterations"] - normal["iterations"]) <= 1, (qr, normal)
    assert abs(qr["final_cost"] - normal["final_cost"]) <= 1e-6 * max(qr["final_cost"], 1e-12) + 1e-15
    # DESIGN.md 4.8, "covered by reading only": no case reaches these paths, and none may start to without being noticed
    assert t["invalid"] == 0 and t["dbl_max"] == 0 and qr["reason"] != "min trust region radius"
    assert t["small_angle"] + t["rodrigues"] == len(t["branches"]) == 1 + qr["iterations"]
    drift = solver_drift(name)
    if name in MAX_ITERATION_CASES:
        assert qr["termination"] == mr.NO_CONVERGENCE and qr["reason"] == "max iterations" and qr["iterations"] == 50
        # rejected steps in a row (the decrease factor doubles) and accepted ones after them (it is reset to 2)
        assert t["rejected"] >= 7 and t["accepted_after_rejected"] >= 1, t
        assert qr["final_cost"] < qr["initial_cost"]
        assert normal["trace"]["rejected"] == t["rejected"]
        assert drift <= 3e-9, drift
    else:
        assert qr["termination"] == mr.CONVERGENCE, qr
        assert drift <= 1e-12, drift
        if name in REJECTING_CONVERGING_CASES:
            assert 13 <= qr["iterations"] < 50 and t["rejected"] >= 3 and t["accepted_after_rejected"] >= 1, qr
        else:
            assert qr["iterations"] <= 12 and t["rejected"] == 0, qr
    if family == "full":
        # the same rotation as the truth, so the solve is short and ends a whole turn away, |r| > pi, unwrapped
        assert 3 <= qr["iterations"] <= 4 and np.linalg.norm(qr["x"][:3]) > np.pi
        assert np.abs(qr["x"] - _lengthened(x, 2 * np.pi)).max() < 0.02
    if family == "first":
        assert t["branches"][0] == "s" and t["small_angle"] == 1 and 5 <= qr["iterations"] <= 6, qr
        assert np.abs(qr["x"] - x).max() < 0.02
    if family == "boundary":
        # both branches, more than once each, inside one short solve; the start decides which comes first
        assert qr["iterations"] == 4 and 2 <= t["small_angle"] <= 4 and 2 <= t["rodrigues"] <= 4, t
        assert (t["branches"][0] == "s") == (float(name.split(":")[1]) ** 2 <= mr.DBL_EPSILON)
        assert np.abs(qr["x"] - x).max() < 1e-9
    if family == "cam2":
        assert np.abs(qr["x"] - x).max() < 1e-9 and qr["final_cost"] < 1e-12
    if family == "stride":
        assert len(obj) == int(name.split(":")[1])


def test_normal_equations_solver_is_a_second_solver_and_the_default_is_qr():
    obj, img, x = scene64(12, n=50, noise=0.5)
    x0 = perturbed(x, 2)
    a, b, c = mr.min_mse_pnp(obj, img, CAM, x0), mr.min_mse_pnp(obj, img, CAM, x0, "qr"), mr.min_mse_pnp(obj, img, CAM, x0, "normal")
    assert np.array_equal(a["x"], b["x"]) and a["final_cost"] == b["final_cost"] and a["trace"] == b["trace"]
    assert a["termination"] == c["termination"] == mr.CONVERGENCE and np.abs(a["x"] - c["x"]).max() < 1e-12
    with pytest.raises(KeyError):
        mr.min_mse_pnp(obj, img, CAM, x0, "svd")
    # one step of each from the same Jacobian: the same step to rounding, the same model cost change
    res, J = mr.residuals_and_jacobian(x0, obj, img, CAM)
    Js, f = J.reshape(-1, 6) / (1.0 + np.linalg.norm(J.reshape(-1, 6), axis=0)), res.reshape(-1)
    D = np.sqrt(np.clip(np.sum(Js * Js, axis=0), 1e-6, 1e32) / 1e4)
    (sq, mq), (sn, mn) = mr._lm_step_qr(Js, D, f), mr._lm_step_normal(Js, D, f)
    assert np.allclose(sq, sn, rtol=1e-9, atol=0) and np.isclose(mq, mn, rtol=1e-9) and mq > 0
    # a matrix that is not positive definite (NaN): a non-finite step, which the loop counts as invalid
    sn, mn = mr._lm_step_normal(Js * np.nan, D, f)
    assert not np.all(np.isfinite(sn))


def test_overflow_case_does_not_fail_in_the_reference():
    """include/mslam_hip.h, DEVIATES `evaluation valid`: the kernel sums squares, so a finite derivative above 1.3e154
    is a failed evaluation there.  Ceres, and this restatement, look at the entries themselves and carry on."""
    obj, img, cam, x0, _ = edge_case(OVERFLOW)
    res, J = mr.residuals_and_jacobian(x0, obj, img, cam)
    assert np.all(np.isfinite(res)) and np.all(np.isfinite(J)) and np.abs(J).max() > 1.3e154
    with np.errstate(over="ignore"):
        assert np.isinf(np.sum(J.reshape(-1, 6) ** 2, axis=0)).any() and np.isfinite(mr.cost(x0, obj, img, cam))
    for out in edge_solves(OVERFLOW):
        assert out["termination"] == mr.CONVERGENCE and out["iterations"] == 3, out


# ---- 4. the cost in 50 digits ----------------------------------------------------------------------------------------------
def mp_cost(x, obj, img, cam):
    """cost(x) in 50-digit arithmetic: Rodrigues' formula as it stands, no small-angle branch (at r = 0 exactly the
    rotation is the identity), then the pin-hole.  Returns an mpf."""
    import mpmath as mp
    with mp.workdps(50):
        fx, fy, cx, cy = (mp.mpf(float(v)) for v in cam)
        r = [mp.mpf(float(v)) for v in x[:3]]
        t = [mp.mpf(float(v)) for v in x[3:6]]
        theta = mp.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
        if theta != 0:
            k = [v / theta for v in r]
            c, s = mp.cos(theta), mp.sin(theta)
        total = mp.mpf(0)
        for P, uv in zip(np.asarray(obj, np.float64).reshape(-1, 3), np.asarray(img, np.float64).reshape(-1, 2)):
            p = [mp.mpf(float(v)) for v in P]
            if theta != 0:
                kxp = [k[1] * p[2] - k[2] * p[1], k[2] * p[0] - k[0] * p[2], k[0] * p[1] - k[1] * p[0]]
                kp = k[0] * p[0] + k[1] * p[1] + k[2] * p[2]
                p = [p[i] * c + kxp[i] * s + k[i] * kp * (1 - c) for i in range(3)]
            X, Y, Z = (p[i] + t[i] for i in range(3))
            du = mp.mpf(float(uv[0])) - (fx * X / Z + cx)
            dv = mp.mpf(float(uv[1])) - (fy * Y / Z + cy)
            total += (du * du + dv * dv) / 2
        return +total


def cost_error(value, x, obj, img, cam):
    """|value - cost(x)| with cost(x) in 50 digits, as a float"""
    import mpmath as mp
    with mp.workdps(50):
        return float(abs(mp.mpf(float(value)) - mp_cost(x, obj, img, cam)))


def cost_bound(x, obj, img, cam):
    """how far a correct double-precision cost may be from the exact one at x.  Each projected coordinate carries the
    rounding of the rotation, the division and the scaling: taken as 8 ulps of the largest one, delta.  A term
    (r0^2 + r1^2) / 2 then moves by (|r0| + |r1|) delta, and sum (|r0| + |r1|) <= sqrt(2 n) sqrt(2 cost) (Cauchy-Schwarz);
    squaring and summing n terms adds n 2^-52 cost."""
    c = float(mp_cost(x, obj, img, cam))
    delta = 8 * 2.0 ** -52 * float(np.abs(mr.project(x, obj, cam)).max())
    n = len(obj)
    return delta * np.sqrt(4 * n * c) + n * 2.0 ** -52 * c


COST_CASES = [names[0] for names in EDGE_FAMILIES.values()] + ["large:100:0", "first:tiny", "boundary:2e-08", "ill:x1000"]


@pytest.mark.parametrize("name", COST_CASES)
def test_cost_matches_50_digit_arithmetic(name):
    """mr.cost (plain doubles) and the costs the solve reports (the value part of the jets: 1 / Z times X instead of X / Z)
    against 50 digits, at the start and at the result.  On the first-order branch p + r x p leaves out r x (r x p) / 2,
    |r|^2 |p| / 2 < 1e-15 relative to the point: inside delta."""
    obj, img, cam, x0, x = edge_case(name)
    qr, _ = edge_solves(name)
    for pose, reported in ((x0, qr["initial_cost"]), (qr["x"], qr["final_cost"])):
        bound = cost_bound(pose, obj, img, cam)
        for value in (reported, mr.cost(pose, obj, img, cam)):
            err = cost_error(value, pose, obj, img, cam)
            print("%s: cost %.17g, error %.3g, bound %.3g" % (name, value, err, bound))
            assert err <= bound, (name, value, err, bound)


# ---- 5. the plugin's factory ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", HOST])
    return True


def test_plugin_exports_min_mse_tracker_factory(built):
    out = subprocess.check_output(["nm", "-D", PLUGIN]).decode()
    assert any(l.split()[-1] == "hipMinMseTrackerFactory" and l.split()[-2] in "DdBb" for l in out.splitlines())
    r = subprocess.run([HARNESS, PLUGIN], capture_output=True, text=True)
    assert r.returncode == 0 and "loaded ok" in r.stdout
