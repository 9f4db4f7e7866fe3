"""The loss of min-MSE PnP (mslam_hip_set_pnp_mse_loss), on the CPU: the symbols, the restatement tests/mse_pnp_loss_ref.py
against its own stated cost and against tests/mse_pnp_ref.py, that every case is what its name says, and that the restatement
alone shows what the loss is for.  The kernel is compared with it in tests/test_gpu_mse_pnp_loss.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mse_pnp_loss_ref as ml  # noqa: E402
import mse_pnp_ref as mr  # noqa: E402
from test_mse_pnp import CAM, perturbed, scene64  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mslam_hip_set_pnp_mse_loss", "mslam_hip_get_pnp_mse_loss"]


def test_symbols_are_exported_declared_and_listed(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mslam_hip.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "modular-slam_amd", "libmslam_hip.so")]).decode()
    exported = {l.split()[-1] for l in out.splitlines()}
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in pkg.ABI_SYMBOLS and name in exported and hasattr(pkg.lib(), name), name
    assert pkg.lib().mslam_hip_abi_version() == 5
    assert callable(pkg.Context.set_pnp_mse_loss) and callable(pkg.Context.get_pnp_mse_loss)


@pytest.mark.parametrize("n,noise,outliers", [(6, 0.0, 0.0), (50, 0.5, 0.2), (400, 0.5, 0.0)])
@pytest.mark.parametrize("solver", ["qr", "normal"])
def test_without_a_loss_it_is_mse_pnp_ref_bit_for_bit(n, noise, outliers, solver):
    obj, img, x = scene64(100 * n, n=n, outliers=outliers, noise=noise)
    x0 = perturbed(x, 0)
    a, b = mr.min_mse_pnp(obj, img, CAM, x0, solver), ml.min_mse_pnp(obj, img, CAM, x0, solver, None)
    assert a["x"].tobytes() == b["x"].tobytes() and a["trace"] == b["trace"]
    for k in ("termination", "iterations", "reason"):
        assert a[k] == b[k]
    for k in ("initial_cost", "final_cost"):
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes()


@pytest.mark.parametrize("name", ["mixed:64:0", "from64", "all_bad"])
@pytest.mark.parametrize("kind", ml.LOSSES)
def test_gradient_is_the_central_difference_of_half_sum_rho(name, kind):
    """the corrected pair's J^T f against central differences of 1/2 sum rho at the start, where the bad points are far out
    on both losses and the others near the branch point of Huber.  h = 1e-6 on parameters of order 1 with gradients of
    order 1e4: the truncation term is h^2 times a third derivative, the rounding term eps cost / h"""
    c = ml.case(name)
    how = (kind, ml.SCALE)
    x = c["start"]
    ok, cost, f, g, J = ml.evaluate(x, c["obj"], c["img"], CAM, ml.KINDS[kind], ml.SCALE)
    assert ok and abs(cost - ml.cost(x, c["obj"], c["img"], CAM, how)) <= 1e-12 * cost
    h = 1e-6
    num = np.zeros(6)
    for j in range(6):
        d = np.zeros(6)
        d[j] = h
        num[j] = (ml.cost(x + d, c["obj"], c["img"], CAM, how) - ml.cost(x - d, c["obj"], c["img"], CAM, how)) / (2.0 * h)
    assert np.max(np.abs(num - g)) <= 1e-6 * max(1.0, float(np.max(np.abs(g)))), (num, g)


def test_every_case_is_what_its_name_says():
    for name in ml.CASES:
        c = ml.case(name)
        n = len(c["obj"])
        if n == 0:
            continue
        res = c["img"] - mr.project(c["truth"], c["obj"], CAM)
        d = np.sqrt(np.sum(res * res, 1))
        good = np.setdiff1d(np.arange(n), c["bad"])
        # half a pixel of noise per coordinate: 3 px is more than four sigma of the norm; a uniform point is frames away
        assert (len(good) == 0 or d[good].max() < 3.0) and (len(c["bad"]) == 0 or d[c["bad"]].min() > 10.0), name
    for n in ml.SIZES:
        for seed in ml.SEEDS:
            c = ml.case("mixed:%d:%d" % (n, seed))
            obj, img, x = scene64(100 * n + seed, n=n, outliers=0.2, noise=0.5)
            assert len(c["obj"]) == n and c["img"].tobytes() == img.tobytes() and c["start"].tobytes() == perturbed(x, seed).tobytes()
            assert len(c["bad"]) >= 1
    assert ml.case("from64")["bad"].min() >= 64 and len(ml.case("from64")["obj"]) == 129 and 128 in ml.case("from64")["bad"]
    assert ml.case("last")["bad"].tolist() == [len(ml.case("last")["obj"]) - 1] == [64]
    assert len(ml.case("all_bad")["bad"]) == len(ml.case("all_bad")["obj"]) == 30
    assert len(ml.case("n1")["obj"]) == 1 and len(ml.case("n0")["obj"]) == 0


@pytest.mark.parametrize("name", ml.CASES)
@pytest.mark.parametrize("kind", ml.LOSSES)
def test_the_two_solvers_agree(name, kind):
    c, qr, nm = ml.reference(name, kind)
    assert qr["termination"] == nm["termination"] != mr.FAILURE and qr["iterations"] == nm["iterations"]
    assert qr["trace"]["invalid"] == nm["trace"]["invalid"] == 0 and qr["trace"]["rejected"] == nm["trace"]["rejected"] == 0
    assert np.abs(qr["x"] - nm["x"]).max() <= 1e-11 if len(c["obj"]) else True
    assert np.all(np.isfinite(qr["x"])) and np.isfinite(qr["final_cost"])
    # the jets' projection and the plain one differ by d = 1e-12 px in rounding (a few ulp of a pixel coordinate below 640):
    # rho / 2 of a residual r moves by at most r d, r at most sqrt(2 cost / n) on average
    n = max(len(c["obj"]), 1)
    slack = 1e-12 * qr["final_cost"] + n * 1e-12 * (np.sqrt(2.0 * qr["final_cost"] / n) + 1e-12)
    assert abs(qr["final_cost"] - ml.cost(qr["x"], c["obj"], c["img"], CAM, (kind, ml.SCALE))) <= slack
    if (name, kind) in (("mixed:6:0", "huber"), ("all_bad", "huber")):  # the 50-iteration cap: wanted
        assert qr["termination"] == mr.NO_CONVERGENCE and qr["iterations"] == mr.MAX_NUM_ITERATIONS
    elif name != "n0":
        assert qr["termination"] == mr.CONVERGENCE and 1 <= qr["iterations"] < mr.MAX_NUM_ITERATIONS


@pytest.mark.parametrize("name", [m for m in ml.MIXED if int(m.split(":")[1]) >= 64] + ["from64", "last"])
def test_what_it_is_for_holds_in_the_restatement_alone(name):
    """on the scenes with n >= 64, max |x - x_true| with each loss is below that without"""
    c, none, _ = ml.reference(name, "none")
    err0 = np.abs(none["x"] - c["truth"]).max()
    for kind in ml.LOSSES:
        err = np.abs(ml.reference(name, kind)[1]["x"] - c["truth"]).max()
        print("%s %s: max |x - x_true| %.3g (none %.3g)" % (name, kind, err, err0))
        assert err < err0


def test_threshold_case_sits_on_hubers_branch_point():
    obj, img, x0 = ml.threshold_case()
    a = ml.THRESHOLD_A
    at = ml.min_mse_pnp(obj, img, CAM, x0, "qr", ("huber", a))
    lo = float(np.nextafter(a, 0.0))
    below = ml.min_mse_pnp(obj, img, CAM, x0, "qr", ("huber", lo))
    assert at["initial_cost"] == a * a / 2.0
    assert below["initial_cost"] == 0.5 * (2.0 * lo * 2.0 - lo * lo) and lo * lo < a * a
