"""The loss of min-MSE PnP on the MI355X (mslam_hip_set_pnp_mse_loss: k_pnp_min_mse_loss in k_pnp_mse.hip): the single call
against tests/mse_pnp_loss_ref.py's QR solve on its cases (tests/test_mse_pnp_loss.py shows on the CPU that every case is what
its name says), the batched device call against single calls (bit for bit), the exact checks, the failure path, the
independence of the three loss settings, and hipMinMseTrackerFactory with IRobustPnp::setLoss through the loader.

Bounds: the rule of tests/test_gpu_mse_pnp.py, unchanged: |x - x_ref|_inf < 1e-6, iterations within 1, cost 1e-6 relative.  The
exact checks are derived, not measured: with a Huber scale no point reaches every weight is exactly 1.0 and rho = s, and a
product with 1.0 keeps its bits, so the result is the one without a loss, byte for byte."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mse_pnp_loss_ref as ml  # noqa: E402
import mse_pnp_ref as mr  # noqa: E402
from test_mse_pnp import CAM, HARNESS, HOST, PLUGIN, perturbed, scene64  # noqa: E402

pytestmark = pytest.mark.gpu
FOCAL, PRINCIPAL = CAM[:2], CAM[2:]


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(width=0, height=0)
    yield c
    c.close()


def _single(ctx, obj, img, x0, how=None):
    """the raw C call under the loss `how`: (rc, x, termination, iterations, cost); the setting is put back to NONE"""
    obj = np.ascontiguousarray(obj, np.float64).reshape(-1, 3)
    img = np.ascontiguousarray(img, np.float64).reshape(-1, 2)
    r = np.array(x0[:3], np.float64)
    t = np.array(x0[3:6], np.float64)
    term, iters, cost = C.c_int(-1), C.c_int(-1), C.c_double(-1)
    ctx.set_pnp_mse_loss(*(how or ("none",)))
    try:
        rc = ctx.L.mslam_hip_pnp_min_mse(ctx._h, obj.ctypes.data_as(C.c_void_p), img.ctypes.data_as(C.c_void_p), len(obj),
                                         *[C.c_double(v) for v in CAM], r.ctypes.data_as(C.c_void_p),
                                         t.ctypes.data_as(C.c_void_p), C.byref(term), C.byref(iters), C.byref(cost))
    finally:
        ctx.set_pnp_mse_loss("none")
    return rc, np.concatenate([r, t]), term.value, iters.value, cost.value


@pytest.mark.parametrize("kind", ml.LOSSES)
@pytest.mark.parametrize("name", ml.CASES)
def test_single_call_matches_restatement(ctx, name, kind):
    c, ref, _ = ml.reference(name, kind)
    rc, got, term, iters, cost = _single(ctx, c["obj"], c["img"], c["start"], (kind, ml.SCALE))
    print("MPL %-12s %-6s term %d/%d it %d/%d cost %.9g/%.9g dx %.3e" % (
        name, kind, term, ref["termination"], iters, ref["iterations"], cost, ref["final_cost"], np.abs(got - ref["x"]).max()))
    assert rc == 0 and term == ref["termination"], (rc, term, ref["termination"], ref["reason"])
    assert abs(iters - ref["iterations"]) <= 1, (iters, ref["iterations"])
    assert np.all(np.isfinite(got)) and np.isfinite(cost)
    assert np.abs(got - ref["x"]).max() < 1e-6, got - ref["x"]
    assert abs(cost - ref["final_cost"]) <= 1e-6 * max(ref["final_cost"], 1e-12) + 1e-15, (cost, ref["final_cost"])
    if name == "n0":
        assert got.tobytes() == c["start"].tobytes() and term == mr.CONVERGENCE and iters == 0 and cost == 0.0
    if (name, kind) == ("mixed:6:0", "huber"):                 # the restatement runs to the 50-iteration cap
        assert term == mr.NO_CONVERGENCE and ref["iterations"] == 50


@pytest.mark.parametrize("name", [m for m in ml.MIXED if int(m.split(":")[1]) >= 64] + ["from64", "last"])
def test_what_it_is_for(ctx, name):
    """max |x - x_true| with each loss is below that without"""
    c = ml.case(name)
    rc, none, _, _, _ = _single(ctx, c["obj"], c["img"], c["start"])
    err0 = np.abs(none - c["truth"]).max()
    for kind in ml.LOSSES:
        rc, got, term, _, _ = _single(ctx, c["obj"], c["img"], c["start"], (kind, ml.SCALE))
        err = np.abs(got - c["truth"]).max()
        print("MPL %s %s: max |x - x_true| %.3g (none %.3g)" % (name, kind, err, err0))
        assert rc == 0 and err < err0


@pytest.mark.parametrize("name", ["mixed:6:1", "mixed:65:0", "mixed:400:1", "all_bad", "n1"])
def test_a_huber_loss_no_point_reaches_is_no_loss_byte_for_byte(ctx, name):
    c = ml.case(name)
    none, huge = _single(ctx, c["obj"], c["img"], c["start"]), _single(ctx, c["obj"], c["img"], c["start"], ("huber", 1e6))
    assert none[0] == huge[0] == 0 and none[1].tobytes() == huge[1].tobytes() and none[2:4] == huge[2:4]
    assert np.float64(none[4]).tobytes() == np.float64(huge[4]).tobytes() and none[3] >= 3


def _batch(ctx, obj, img, ns, pose, how):
    import torch
    dev = torch.device("cuda")
    d_obj, d_img = torch.from_numpy(obj).to(dev), torch.from_numpy(img).to(dev)
    d_n = torch.from_numpy(np.asarray(ns, np.int32)).to(dev)
    d_pose = torch.from_numpy(pose).to(dev)
    d_info = torch.full((len(ns), 4), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.set_pnp_mse_loss(*(how or ("none",)))
    try:
        ctx.pnp_min_mse_batch_dev(d_obj.data_ptr(), d_img.data_ptr(), d_n.data_ptr(), len(ns), obj.shape[1], d_pose.data_ptr(),
                                  d_info.data_ptr(), FOCAL, PRINCIPAL)
        ctx.sync()
    finally:
        ctx.set_pnp_mse_loss("none")
    return d_pose.cpu().numpy(), d_info.cpu().numpy()


@pytest.mark.parametrize("kind", ml.LOSSES)
def test_batch_is_bit_identical_to_single_calls_with_a_loss(ctx, kind):
    cap, P = 130, 64
    rng = np.random.default_rng(78)
    ns = rng.integers(0, cap + 1, P)
    ns[:8] = [0, 1, 2, 63, 64, 65, 129, cap]
    obj, img, pose = np.zeros((P, cap, 3)), np.zeros((P, cap, 2)), np.zeros((P, 6))
    for p in range(P):
        o, i, x = scene64(6000 + p, n=cap, noise=0.5, outliers=0.2 * (p % 4 != 0))
        obj[p], img[p], pose[p] = o, i, perturbed(x, p)
    how = (kind, ml.SCALE)
    a, b = _batch(ctx, obj, img, ns, pose, how), _batch(ctx, obj, img, ns, pose, how)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    bpose, binfo = a
    for p in range(P):
        n = int(ns[p])
        rc, x, term, iters, cost = _single(ctx, obj[p, :n], img[p, :n], pose[p], how)
        assert rc == 0 and term != mr.FAILURE, (p, n, rc, term)
        assert binfo[p, 0] == term and binfo[p, 1] == iters and binfo[p, 3] == cost, (p, binfo[p], term, iters, cost)
        assert np.array_equal(bpose[p], x), p
        if n == 0:
            assert np.array_equal(bpose[p], pose[p]) and term == mr.CONVERGENCE and cost == 0.0
    none = _batch(ctx, obj, img, ns, pose, None)
    assert not np.array_equal(none[0], bpose)
    huge = _batch(ctx, obj, img, ns, pose, ("huber", 1e6))
    assert np.array_equal(none[0], huge[0]) and np.array_equal(none[1], huge[1])


def test_hubers_branch_point(ctx):
    """s == b exactly is the inlier branch: the batch call's info[2] == b / 2; at nextafter the other branch is taken and the
    cost is the restatement's"""
    obj, img, x0 = ml.threshold_case()
    a = ml.THRESHOLD_A
    pose, info = _batch(ctx, obj[None], img[None], [1], x0[None].copy(), ("huber", a))
    assert info[0, 2] == a * a / 2.0
    lo = float(np.nextafter(a, 0.0))
    ref = ml.min_mse_pnp(obj, img, CAM, x0, "qr", ("huber", lo))
    pose, info = _batch(ctx, obj[None], img[None], [1], x0[None].copy(), ("huber", lo))
    assert lo * lo < 4.0 and ref["initial_cost"] == 0.5 * (2.0 * lo * 2.0 - lo * lo)
    assert abs(info[0, 2] - ref["initial_cost"]) <= 1e-6 * ref["initial_cost"] and info[0, 0] == ref["termination"]


@pytest.mark.parametrize("kind", ml.LOSSES)
def test_a_nan_image_point_is_failure_with_the_pose_unchanged(ctx, pkg, kind):
    obj, img, x = scene64(4, n=70)
    bad = img.copy()
    bad[66, 0] = np.nan
    rc, got, term, iters, _ = _single(ctx, obj, bad, x, (kind, ml.SCALE))
    assert rc == pkg.E_NO_MODEL and term == mr.FAILURE and iters == 0 and got.tobytes() == x.tobytes()
    with np.errstate(all="ignore"):
        assert ml.min_mse_pnp(obj, bad, CAM, x, "qr", (kind, ml.SCALE))["termination"] == mr.FAILURE
    rc, got, term, _, _ = _single(ctx, obj, img, perturbed(x, 1), (kind, ml.SCALE))      # the context still works
    assert rc == 0 and term == mr.CONVERGENCE and np.abs(got - x).max() < 1e-9


def test_the_setting_defaults_validates_and_is_independent(ctx, pkg):
    fresh = pkg.Context(width=0, height=0)
    assert fresh.get_pnp_mse_loss() == fresh.get_ba_loss() == fresh.get_pose_graph_loss() == (pkg.BA_LOSS_NONE, 0.0)
    fresh.close()
    ctx.set_pnp_mse_loss("huber", 2.0)
    assert ctx.get_pnp_mse_loss() == (pkg.BA_LOSS_HUBER, 2.0) and ctx.get_ba_loss() == (0, 0.0) and ctx.get_pose_graph_loss() == (0, 0.0)
    for bad in ((3, 1.0), (-1, 1.0), ("huber", 0.0), ("cauchy", -2.0), ("huber", np.nan), ("cauchy", np.inf), ("tukey", 1.0)):
        with pytest.raises(pkg.MslamHipError) as e:
            ctx.set_pnp_mse_loss(*bad)
        assert e.value.code == pkg.E_INVALID and ctx.get_pnp_mse_loss() == (pkg.BA_LOSS_HUBER, 2.0), bad
    ctx.set_ba_loss("cauchy", 0.02)
    ctx.set_pose_graph_loss("cauchy", 0.1)
    assert ctx.get_pnp_mse_loss() == (pkg.BA_LOSS_HUBER, 2.0)
    ctx.set_pnp_mse_loss("none", 5.0)
    assert ctx.get_pnp_mse_loss() == (0, 0.0) and ctx.get_ba_loss() == (pkg.BA_LOSS_CAUCHY, 0.02)
    assert ctx.get_pose_graph_loss() == (pkg.BA_LOSS_CAUCHY, 0.1)
    # the other two settings do not reach the PnP: the bits of a solve without a loss
    c = ml.case("mixed:65:1")
    with_others = _single(ctx, c["obj"], c["img"], c["start"])
    ctx.set_ba_loss("none")
    ctx.set_pose_graph_loss("none")
    alone = _single(ctx, c["obj"], c["img"], c["start"])
    assert with_others[1].tobytes() == alone[1].tobytes() and with_others[2:] == alone[2:]
    k, s = C.c_int(-1), C.c_double(-1)
    assert ctx.L.mslam_hip_get_pnp_mse_loss(ctx._h, None, C.byref(s)) == 0 and s.value == 0.0
    assert ctx.L.mslam_hip_get_pnp_mse_loss(ctx._h, C.byref(k), None) == 0 and k.value == 0


# ---- the plugin --------------------------------------------------------------------------------------------------------------

def _quat_of_rvec(r):
    th = np.linalg.norm(r)
    return np.concatenate([[np.cos(th / 2)], np.sin(th / 2) * r / th])


def _rvec_of_quat(q):
    nv = np.linalg.norm(q[1:])
    d = -nv if q[0] < 0 else nv
    return q[1:] / d * (2 * np.arctan2(nv, abs(q[0])))


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", HOST])
    return True


@pytest.mark.parametrize("kind", ml.LOSSES)
def test_plugin_min_mse_tracker_with_a_loss(ctx, built, tmp_path, kind):
    """hipMinMseTrackerFactory through the loader with IRobustPnp::setLoss: its result is the C call's under
    mslam_hip_set_pnp_mse_loss from the same start, through the reference's float conversions (tests/test_gpu_mse_pnp.py): one
    float ulp of a value near 1 is 1.2e-7"""
    c = ml.case("mixed:129:0")
    q0 = _quat_of_rvec(c["start"][:3])
    path = tmp_path / "scene.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(c["obj"])))
        for P, uv in zip(c["obj"], c["img"]):
            f.write(struct.pack("<5d", *P, *uv))
        f.write(struct.pack("<7d", *c["start"][3:], *q0))
        f.write(struct.pack("<4d", *CAM))
    lines = {}
    for flags in ((), ("--loss", "%s:%r" % (kind, ml.SCALE))):
        r = subprocess.run([HARNESS, PLUGIN, "--pnp-mse", str(path), *flags], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        lines[bool(flags)] = [l for l in r.stdout.splitlines() if l.startswith("pnp ")][0]
    assert lines[True] != lines[False]
    for with_loss, line in lines.items():
        f = line.split()
        pos, q = np.array([float(v) for v in f[2:5]]), np.array([float(v) for v in f[6:10]])
        rc, x, term, _, _ = _single(ctx, c["obj"], c["img"], np.concatenate([_rvec_of_quat(q0), c["start"][3:]]),
                                    (kind, ml.SCALE) if with_loss else None)
        assert rc == 0
        angle = np.float32(np.sqrt(x[:3] @ x[:3]))
        axis = x[:3].astype(np.float32).astype(np.float64) / np.float64(angle)
        q_ref = np.concatenate([[np.cos(0.5 * np.float64(angle))], np.sin(0.5 * np.float64(angle)) * axis])
        pos_ref = x[3:].astype(np.float32).astype(np.float64)
        assert np.abs(pos - pos_ref).max() < 1e-6 and np.abs(q - q_ref).max() < 1e-6, (with_loss, pos - pos_ref, q - q_ref)
    # the loss is what brings the plugin's pose to the truth: the position is the translation itself
    err = {k: np.abs(np.array([float(v) for v in l.split()[2:5]]) - c["truth"][3:]).max() for k, l in lines.items()}
    assert err[True] < err[False]
