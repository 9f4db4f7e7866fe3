"""Min-MSE PnP on the MI355X (k_pnp_mse.hip), the edges: rejected steps and the reset of the decrease factor, the
iteration cap, the first-order rotation branch and solves that cross its boundary, fx != fy, ill-conditioned geometry,
n around the multiples of the 64 lanes, the batch call's guards, and the costs it reports.

Every case is built and proved on the CPU in tests/test_mse_pnp.py (section 3): there the reference's own path counters
show that a case takes the path it is named for, and two CPU solvers written apart (QR, normal equations) agree on it.
Here the kernel is compared with the QR solve.  The bound on the pose is max(1e-9, 1000 |x_normal - x_qr|_inf), both
solves computed by the test: the distance of two correct solvers, times 1000 for the kernel's other summation order (64
lane sums and a butterfly against numpy's pairwise sum).  The reported costs are checked against 50-digit arithmetic.

The one place where the kernel is known to leave Ceres (include/mslam_hip.h, `evaluation valid`) is pinned at the end."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mse_pnp_ref as mr  # noqa: E402
import test_mse_pnp as cpu  # noqa: E402

pytestmark = pytest.mark.gpu

CAPACITY = 65
GUARD = 4                # problems' worth of sentinel space past the batch, in n, pose and info
SENTINEL = -7.25


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(width=0, height=0)
    yield c
    c.close()


_singles = {}


def single(ctx, name):
    """the single C call on a named case, once: dict(rc, x, termination, iterations, cost)"""
    if name not in _singles:
        obj, img, cam, x0, _ = cpu.edge_case(name)
        _singles[name] = _single(ctx, obj, img, cam, x0)
    return _singles[name]


def _single(ctx, obj, img, cam, x0):
    obj = np.ascontiguousarray(obj, np.float64).reshape(-1, 3)
    img = np.ascontiguousarray(img, np.float64).reshape(-1, 2)
    r = np.array(x0[:3], np.float64)
    t = np.array(x0[3:6], np.float64)
    term, iters, cost = C.c_int(-1), C.c_int(-1), C.c_double(-1)
    rc = ctx.L.mslam_hip_pnp_min_mse(ctx._h, obj.ctypes.data_as(C.c_void_p), img.ctypes.data_as(C.c_void_p), len(obj),
                                     *[C.c_double(v) for v in cam], r.ctypes.data_as(C.c_void_p),
                                     t.ctypes.data_as(C.c_void_p), C.byref(term), C.byref(iters), C.byref(cost))
    return dict(rc=rc, x=np.concatenate([r, t]), termination=term.value, iterations=iters.value, cost=cost.value)


def _batch(ctx, problems, cam=cpu.CAM, capacity=CAPACITY, n_problems=None, launches=1):
    """one batch launch over `problems` = [(obj, img, x0, n)], n the count handed to the kernel (it may lie outside
    [0, capacity]); rows at or past n are NaN in both arrays.  n, pose and info carry GUARD problems' worth of sentinel
    past the batch.  -> (pose, info, n) as they come back, sentinel space included, once per launch"""
    import torch
    P = len(problems)
    obj = np.full((P, capacity, 3), np.nan)
    img = np.full((P, capacity, 2), np.nan)
    pose = np.full((P + GUARD, 6), SENTINEL)
    ns = np.zeros(P + GUARD, np.int32)
    for p, (o, i, x0, n) in enumerate(problems):
        live = n if 0 <= n <= capacity else 0
        obj[p, :live], img[p, :live] = np.asarray(o).reshape(-1, 3)[:live], np.asarray(i).reshape(-1, 2)[:live]
        pose[p], ns[p] = x0, n
    dev = torch.device("cuda")
    d_obj, d_img, d_n = (torch.from_numpy(a).to(dev) for a in (obj, img, ns))
    out = []
    for _ in range(launches):
        d_pose = torch.from_numpy(pose).to(dev)
        d_info = torch.full((P + GUARD, 4), SENTINEL, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ctx.pnp_min_mse_batch_dev(d_obj.data_ptr(), d_img.data_ptr(), d_n.data_ptr(), P if n_problems is None else n_problems,
                                  capacity, d_pose.data_ptr(), d_info.data_ptr(), cam[:2], cam[2:])
        ctx.sync()
        out.append((d_pose.cpu().numpy(), d_info.cpu().numpy(), d_n.cpu().numpy()))
    return (pose, ns), out


_ones = {}


def batch_of_one(ctx, name):
    """info = (termination, iterations, initial cost, final cost) and pose of a named case through a batch of one: the
    single call does not return the initial cost"""
    if name not in _ones:
        obj, img, cam, x0, _ = cpu.edge_case(name)
        _, [(pose, info, _)] = _batch(ctx, [(obj, img, x0, len(obj))], cam=cam, capacity=len(obj))
        assert np.all(pose[1:] == SENTINEL) and np.all(info[1:] == SENTINEL)
        _ones[name] = pose[0], info[0]
    return _ones[name]


# ---- the single call against the QR solve -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cpu.EDGE_CASES)
def test_edge_case_matches_the_qr_solve(ctx, name):
    obj, img, cam, x0, x = cpu.edge_case(name)
    ref, _ = cpu.edge_solves(name)
    got = single(ctx, name)
    bound = max(1e-9, 1000.0 * cpu.solver_drift(name))
    dev = np.abs(got["x"] - ref["x"]).max()
    print("%s: termination %d / %d, iterations %d / %d, |x_gpu - x_qr| %.3g (bound %.3g), cost %.17g / %.17g" % (
        name, got["termination"], ref["termination"], got["iterations"], ref["iterations"], dev, bound, got["cost"],
        ref["final_cost"]))
    assert got["rc"] == 0
    assert got["termination"] == ref["termination"], (got, ref)
    assert abs(got["iterations"] - ref["iterations"]) <= 1, (got, ref)
    assert abs(got["cost"] - ref["final_cost"]) <= 1e-6 * max(ref["final_cost"], 1e-12) + 1e-15, (got, ref)
    assert dev <= bound, (got["x"] - ref["x"], bound)
    family = name.split(":")[0]
    if name in cpu.MAX_ITERATION_CASES:
        # NO_CONVERGENCE is a usable result: the return code is OK (asserted above), the pose came back, the cost fell
        assert got["termination"] == mr.NO_CONVERGENCE and got["iterations"] == 50
        assert np.abs(got["x"] - x0).max() > 1e-3
        pose, info = batch_of_one(ctx, name)
        assert np.array_equal(pose, got["x"]) and info[3] == got["cost"] and info[3] < info[2], info
    if family == "full":
        assert np.linalg.norm(got["x"][:3]) > np.pi      # the rotation vectors as they are: a whole turn away, unwrapped
    if family in ("cam2", "boundary"):
        assert np.abs(got["x"] - x).max() < 1e-9, got["x"] - x


@pytest.mark.parametrize("name", cpu.COST_CASES)
def test_reported_costs_match_50_digit_arithmetic(ctx, name):
    """info[2] at the start pose and info[3] at the returned pose against the cost in 50 digits, within
    max(8 e_ref, n 2^-50) relative, e_ref the numpy restatement's own relative error at the same pose; where the final
    cost has all but vanished (noise-free, below 1e-12) the same expression times the initial cost, absolutely."""
    obj, img, cam, x0, _ = cpu.edge_case(name)
    pose, info = batch_of_one(ctx, name)
    n = len(obj)
    exact0 = float(cpu.mp_cost(x0, obj, img, cam))
    for at, reported in ((x0, info[2]), (pose, info[3])):
        exact = float(cpu.mp_cost(at, obj, img, cam))
        scale = exact if exact >= 1e-12 else exact0
        e_ref = cpu.cost_error(mr.cost(at, obj, img, cam), at, obj, img, cam) / scale
        err = cpu.cost_error(reported, at, obj, img, cam) / scale
        tol = max(8 * e_ref, n * 2.0 ** -50)
        print("%s: cost %.17g, error %.3g of %.3g, numpy's %.3g, tolerance %.3g" % (name, reported, err, scale, e_ref, tol))
        assert err <= tol, (name, reported, exact, err, tol)


# ---- the batch call -------------------------------------------------------------------------------------------------------------
BATCH_CASES = [name for name in cpu.EDGE_CASES if name != "cam2" and len(cpu.edge_case(name)[0]) <= CAPACITY]
BAD_N = {3: 0, 9: -1, 18: CAPACITY + 1, 36: 2 ** 31 - 1}          # position in the batch -> n (36: the last live wave)


def _batch_problems():
    """37 problems: the edge cases of at most 65 points under the TUM intrinsics, three of them again with fewer points
    than they have (their later rows are then NaN like all padding), and four entries whose n is 0 or invalid"""
    probs = []
    for name in BATCH_CASES:
        obj, img, _, x0, _ = cpu.edge_case(name)
        probs.append((obj, img, x0, len(obj)))
    for name, n in (("large:10:0", 33), ("stride:64", 1), ("large:100:1", 64)):
        obj, img, _, x0, _ = cpu.edge_case(name)
        probs.append((obj[:n], img[:n], x0, n))
    obj, img, _, x0, _ = cpu.edge_case("large:10:1")
    for p in sorted(BAD_N):
        probs.insert(p, (obj, img, x0 + p, BAD_N[p]))
    assert len(probs) == 37 and len(probs) % 4 == 1
    return probs


def test_batch_guards_padding_and_bit_identity(ctx):
    probs = _batch_problems()
    P = len(probs)
    (pose0, ns), runs = _batch(ctx, probs, launches=2)
    for a, b in zip(runs[0], runs[1]):                   # two launches: the same bits, NaN for NaN
        assert np.array_equal(a, b, equal_nan=True)
    pose, info, n_back = runs[0]
    assert np.array_equal(n_back, ns)
    # nothing was written past the batch
    assert np.all(pose[P:] == SENTINEL) and np.all(info[P:] == SENTINEL)
    for p, (obj, img, x0, n) in enumerate(probs):
        if p in BAD_N and n != 0:
            assert info[p, 0] == mr.FAILURE and info[p, 1] == 0 and np.isnan(info[p, 2]) and np.isnan(info[p, 3]), (p, info[p])
            assert pose[p].tobytes() == pose0[p].tobytes(), p
        elif n == 0:
            assert np.array_equal(info[p], [mr.CONVERGENCE, 0, 0.0, 0.0]) and pose[p].tobytes() == pose0[p].tobytes()
        else:
            # the NaN padding never shows, and the problem gives the bits of its single call, which
            # test_edge_case_matches_the_qr_solve ties to the reference
            assert np.all(np.isfinite(pose[p])) and np.all(np.isfinite(info[p])), (p, pose[p], info[p])
            got = _single(ctx, obj[:n], img[:n], cpu.CAM, x0)
            assert got["rc"] == 0
            assert info[p, 0] == got["termination"] and info[p, 1] == got["iterations"] and info[p, 3] == got["cost"], (p, info[p], got)
            assert pose[p].tobytes() == got["x"].tobytes(), p
    live = [p for p in range(P) if p not in BAD_N]
    for p, name in zip(live, BATCH_CASES):                     # the named ones are the cached single calls themselves
        got = single(ctx, name)
        assert pose[p].tobytes() == got["x"].tobytes() and info[p, 3] == got["cost"], name
    # every termination kind is in the batch
    assert {mr.CONVERGENCE, mr.NO_CONVERGENCE, mr.FAILURE} == set(info[:P, 0].astype(int))
    # shorter batches over the first problems: the last workgroup has 1, 2, 3 and 1 live waves
    for k in (1, 2, 3, 5):
        _, [(pk, ik, _)] = _batch(ctx, probs[:k])
        assert np.array_equal(pk[:k], pose[:k], equal_nan=True) and np.array_equal(ik[:k], info[:k], equal_nan=True), k
        assert np.all(pk[k:] == SENTINEL) and np.all(ik[k:] == SENTINEL), k


def test_batch_empty_and_invalid_calls(ctx, pkg):
    probs = _batch_problems()[:5]
    # n_problems = 0: OK, nothing written, not even to the first problem
    (pose0, _), [(pose, info, _)] = _batch(ctx, probs, n_problems=0)
    assert np.array_equal(pose, pose0) and np.all(info == SENTINEL)
    # capacity 0 and every n = 0: no point arrays at all
    import torch
    x0 = np.arange(30, dtype=np.float64).reshape(5, 6) / 8
    d_pose = torch.from_numpy(np.vstack([x0, np.full((GUARD, 6), SENTINEL)])).cuda()
    d_info = torch.full((5 + GUARD, 4), SENTINEL, dtype=torch.float64, device="cuda")
    d_n = torch.zeros(5 + GUARD, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.pnp_min_mse_batch_dev(0, 0, d_n.data_ptr(), 5, 0, d_pose.data_ptr(), d_info.data_ptr(), cpu.CAM[:2], cpu.CAM[2:])
    ctx.sync()
    pose, info = d_pose.cpu().numpy(), d_info.cpu().numpy()
    assert np.array_equal(pose[:5], x0) and np.all(pose[5:] == SENTINEL) and np.all(info[5:] == SENTINEL)
    assert np.array_equal(info[:5], np.tile([mr.CONVERGENCE, 0, 0.0, 0.0], (5, 1)))
    # negative counts are refused before anything is launched
    for n_problems, capacity in ((-1, CAPACITY), (5, -1)):
        d_info.fill_(SENTINEL)
        torch.cuda.synchronize()
        with pytest.raises(pkg.MslamHipError) as e:
            ctx.pnp_min_mse_batch_dev(0, 0, d_n.data_ptr(), n_problems, capacity, d_pose.data_ptr(), d_info.data_ptr(),
                                      cpu.CAM[:2], cpu.CAM[2:])
        assert e.value.code == pkg.E_INVALID
        ctx.sync()
        assert np.all(d_info.cpu().numpy() == SENTINEL)


# ---- where the kernel leaves Ceres: a finite derivative whose square is not --------------------------------------------------
def test_overflowing_square_of_a_finite_derivative_is_a_failed_evaluation(ctx, pkg):
    """include/mslam_hip.h, DEVIATES `evaluation valid`.  The kernel judges an evaluation by the cost and the diagonal of
    J^T J; a derivative above about 1.3e154 is finite and its square is not, so the start counts as failed: FAILURE at
    iteration 0, E_NO_MODEL, the pose unchanged.  Ceres looks at the entries and carries on: the reference converges in 3
    iterations (tests/test_mse_pnp.py::test_overflow_case_does_not_fail_in_the_reference).  No scene reaches such values;
    the behaviour is pinned here so that a change to it is a decision."""
    obj, img, cam, x0, _ = cpu.edge_case(cpu.OVERFLOW)
    assert cpu.edge_solves(cpu.OVERFLOW)[0]["termination"] == mr.CONVERGENCE
    got = _single(ctx, obj, img, cam, x0)
    assert got["rc"] == pkg.E_NO_MODEL and got["termination"] == mr.FAILURE and got["iterations"] == 0, got
    assert got["x"].tobytes() == np.asarray(x0).tobytes()
    pose, info = batch_of_one(ctx, cpu.OVERFLOW)
    assert info[0] == mr.FAILURE and info[1] == 0 and np.isfinite(info[2]) and info[2] == info[3], info
    assert pose.tobytes() == np.asarray(x0).tobytes()
    # the context works on
    obj, img, cam, x0, x = cpu.edge_case("cam2")
    got = _single(ctx, obj, img, cam, x0)
    assert got["rc"] == 0 and got["termination"] == mr.CONVERGENCE and np.abs(got["x"] - x).max() < 1e-9
