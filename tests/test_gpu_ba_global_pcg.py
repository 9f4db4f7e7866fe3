"""mslam_hip_bundle_adjust_global with mslam_hip_set_ba_global_pcg on the MI355X (k_bag_schur_pairs of k_ba.hip writing the
covisible pairs' Schur blocks, the block-Jacobi preconditioned conjugate gradients of k_pcg.hip) through
Context.set_ba_global_pcg and Context.bundle_adjust_global.

Bounds.  Tight tier (tolerance 1e-12, cap 2000): tests/test_gpu_ba_global.py's _check as it is, |x_gpu - x_ref|_inf <=
max(1e-9, 1000 dist) with dist the larger of the two direct CPU solvers' distance and the CPU PCG reference's
(tests/ba_global_pcg_ref.py) distance to the direct solution: nothing from the GPU.  Default tier (1e-6, 500): both the GPU
and the CPU PCG reference are inexact solutions whose error the tolerance sets; d is the CPU PCG reference's own distance to
the direct solution and the bound max(1e-9, 10 d), the factor for a stopping index that differs by one or two.  Above every
other solver's ground: against the truth on the noise-free scenes, max(1e-7, 10 x the CPU PCG reference's own distance to
it), and against the CPU PCG reference with _check at dist = 0 (its floor, 1e-9).  No test asserts a time.

The boundaries of the kernels (k_pcg.hip): the vector kernels take 256 entries per workgroup, so 6 n_free = 252 / 258 (n_free
42 / 43) is one workgroup / two; k_pcg_product takes 4 block rows per workgroup (n_free 43, 44, 45) and 10 neighbours per pass
(rows of 9, 10, 11 blocks: complete:10 / 11 / 12); every scalar is a sum of per-workgroup partials taken 256 at a time, so more
than 256 partials of the product is n_free > 1024 (revisit:1025 / 1026: 256 and 257 of them)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_cases  # noqa: E402
import ba_global_cases as bg  # noqa: E402
import ba_global_pcg_cases as pc  # noqa: E402
import ba_global_sparse_cases as bc  # noqa: E402
import ba_global_sparse_ref as bs  # noqa: E402
import ba_loss_ref as lr  # noqa: E402
import ba_ref  # noqa: E402
import loop_walk  # noqa: E402
import pose_graph_sparse_cases as psc  # noqa: E402
import test_gpu_ba_global as tg  # noqa: E402
import test_gpu_pose_graph as tpg  # noqa: E402

pytestmark = pytest.mark.gpu
TIGHT = (2000, 1e-12)
DEFAULT = (500, 1e-6)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(width=0, height=0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def off_again(ctx):
    yield
    ctx.set_ba_global_pcg(False)
    ctx.set_ba_global_solver("dense")
    ctx.set_ba_loss("none")


def _solve(ctx, sc, setting=TIGHT, **kw):
    ctx.set_ba_global_pcg(True, *setting)
    got = tg._solve(ctx, sc, **kw)
    got["pcg"] = ctx.ba_global_pcg_stats()
    return got


def _ran_clean(got, cap):
    st = got["pcg"]
    print("     CG: %d solves, %d iterations, longest %d, at the cap %d, breakdowns %d" % (
        st["solves"], st["iterations"], st["longest"], st["at_cap"], st["breakdowns"]))
    assert st["at_cap"] == 0 and st["breakdowns"] == 0 and st["longest"] < cap
    assert st["solves"] in (0, got["iterations"])               # one linear solve per iteration, none without a free keyframe
    assert st["iterations"] >= st["longest"]


def _tight(ctx, tag, name, sc, ref, dist, mask, loss=None):
    """the tight tier on one scene: dist from the CPU alone"""
    cpu = pc.pcg_reference(name, *TIGHT, loss=loss)[1]
    assert cpu["at_cap"] == 0 and cpu["breakdowns"] == 0
    got = _solve(ctx, sc)
    tg._check(tag, name, got, sc, ref, max(dist, bs.distance(cpu, ref)), mask)
    _ran_clean(got, TIGHT[0])
    return got


# ---- 1. the tight tier -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", bg.WITH_QR)
def test_tight_against_the_qr_reference(ctx, name):
    sc, qr, sch, dist, mask, margin = bg.reference(name)
    got = _tight(ctx, "PCG", name, sc, qr, dist, mask)
    if sc["fixed"][0]:
        assert got["poses"][0].tobytes() == sc["poses"][0].tobytes()
    if name == "hard66":
        assert got["rejected_steps"] > 0
    if name == "gross80":
        assert got["n_outliers"] == 2


@pytest.mark.parametrize("name", tg.OLD_GROUND)
def test_tight_on_the_old_ground(ctx, name):
    sc, qr, sch, dist, mask, margin = ba_cases.reference(name)
    got = _tight(ctx, "PCG old", name, sc, qr, dist, mask)
    if name in ("all_fixed", "k1_fixed", "empty"):
        assert np.array_equal(got["poses"], sc["poses"]) and got["pcg"]["solves"] == 0      # no reduced system
    if name == "empty":
        assert got["final_cost"] == 0.0
    if name.startswith("cap"):
        assert got["iterations"] == qr["iterations"]
    if name in ("cap0", "at_minimum"):
        assert got["iterations"] == 0 and got["pcg"]["iterations"] == 0
        assert got["poses"].tobytes() == np.asarray(sc["poses"], np.float64).tobytes()
        assert got["landmarks"].tobytes() == np.asarray(sc["landmarks"], np.float64).tobytes()
    if name in ("fixed_middle", "fixed_two"):
        for k in (1,) + tuple(np.flatnonzero(sc["fixed"])):
            assert got["poses"][k].tobytes() == sc["poses"][k].tobytes(), k


@pytest.mark.parametrize("name", bc.NEW)
def test_tight_on_the_sparse_scenes(ctx, name):
    """isolated: a row of its diagonal block alone; two_rings: two components; complete12: every row full; loop_row: one
    long row"""
    sc, ref, aug, dist, mask = bc.reference(name)
    _tight(ctx, "PCG new", name, sc, ref, dist, mask)


# ---- 2. the default tier ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["traj:66", "traj:130", "hard66", "gross80", "revisit:130", "revisit:400"])
def test_default_tolerance(ctx, name):
    sc, ref, dist, mask = pc.direct_reference(name)
    cpu = pc.pcg_reference(name, *DEFAULT)[1]
    d = bs.distance(cpu, ref)
    got = _solve(ctx, sc, DEFAULT)
    reached = bs.distance(got, ref)
    bound = max(1e-9, 10.0 * d)
    st = got["pcg"]
    print("PCG default %-12s term %d/%d it %d/%d/%d cost %.9g/%.9g  d(cpu pcg, direct) %.3e  reached %.3e  bound %.3e  CG longest %d/%d total %d" % (
        name, got["termination"], ref["termination"], got["iterations"], cpu["iterations"], ref["iterations"], got["final_cost"],
        ref["final_cost"], d, reached, bound, st["longest"], max(cpu["cg"]), st["iterations"]))
    assert cpu["termination"] == ref["termination"] and cpu["iterations"] == ref["iterations"]      # the reference itself
    assert got["termination"] == ref["termination"] and abs(got["iterations"] - ref["iterations"]) <= 1
    assert got["invalid_steps"] == 0 and st["at_cap"] == 0 and st["breakdowns"] == 0
    assert np.array_equal(got["outlier"], mask) and got["n_outliers"] == int(mask.sum())
    M = len(sc["obs_kf"])
    assert abs(got["final_cost"] - ref["final_cost"]) <= 1e-6 * ref["final_cost"] + M * (12.0 * bound) ** 2 / 2.0
    assert reached <= bound


# ---- 3. the ground no other solver takes -------------------------------------------------------------------------------------------------

def _raw(ctx, pkg, sc):
    """the C call on copies -> (rc, poses, landmarks, outlier array, the copies before)"""
    x, lm = np.ascontiguousarray(sc["poses"], np.float64).copy(), np.ascontiguousarray(sc["landmarks"], np.float64).copy()
    out = np.full(len(sc["obs_kf"]), 7, np.uint8)
    before = (x.copy(), lm.copy())
    summary = pkg.BaSummary()
    rc = ctx.L.mslam_hip_bundle_adjust_global(ctx._h, pkg._p(x), pkg._p(sc["fixed"]), len(x), pkg._p(lm), len(lm), pkg._p(sc["obs_kf"]),
                                              pkg._p(sc["obs_lm"]), pkg._p(sc["obs_cam"]), len(sc["obs_kf"]), 100, pkg.C.c_double(0.15),
                                              pkg._p(out), pkg.C.byref(summary))
    return rc, x, lm, out, before


@pytest.mark.parametrize("K", [1900, 2800])
def test_the_ground_no_other_solver_takes(ctx, pkg, K):
    """a noise-free map that revisits its ground: DENSE rejects K, SPARSE the envelope, both with nothing touched; PCG reaches
    the truth.  2800: 6 n_free = 16794 entries, 66 workgroups of the vector kernels, 700 of the product"""
    name = "revisit0:%d" % K
    sc, cpu = pc.pcg_reference(name, *TIGHT)
    ctx.set_ba_global_solver("dense")
    rc, x, lm, out, before = _raw(ctx, pkg, sc)
    assert rc == pkg.E_INVALID and x.tobytes() == before[0].tobytes() and lm.tobytes() == before[1].tobytes() and np.all(out == 7)
    ctx.set_ba_global_solver("sparse")
    rc, x, lm, out, before = _raw(ctx, pkg, sc)
    assert rc == pkg.E_CAPACITY and x.tobytes() == before[0].tobytes() and lm.tobytes() == before[1].tobytes() and np.all(out == 7)
    got = _solve(ctx, sc)
    assert ctx.get_ba_global_solver() == pkg.BA_GLOBAL_SOLVER_SPARSE         # PCG ran whatever that setting says, and left it
    err, cpu_err = pc.truth_error(got, sc), pc.truth_error(cpu, sc)
    print("PCG %s err %.3e, the CPU PCG reference's %.3e" % (name, err, cpu_err))
    mask = ba_ref.outliers(cpu["poses"], cpu["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"])
    tg._check("PCG", name, got, sc, cpu, 0.0, mask)
    _ran_clean(got, TIGHT[0])
    assert err <= max(1e-7, 10.0 * cpu_err) and not got["outlier"].any()


def test_revisit_1900_with_noise(ctx):
    sc, cpu = pc.pcg_reference("revisit:1900", *TIGHT)
    got = _solve(ctx, sc)
    mask = ba_ref.outliers(cpu["poses"], cpu["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"])
    tg._check("PCG", "revisit:1900", got, sc, cpu, 0.0, mask)
    _ran_clean(got, TIGHT[0])


@pytest.mark.parametrize("K", [10, 11, 12, 64])
def test_complete_maps(ctx, K):
    """every row of the reduced system holds K - 1 blocks: 9, 10 and 11 either side of k_pcg_product's pass of 10, and 63"""
    name = "complete:%d" % K
    sc, ref, dist, mask = pc.direct_reference(name)
    _tight(ctx, "PCG", name, sc, ref, dist, mask)


# ---- 4. shapes --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [43, 44, 45, 46])
def test_workgroup_boundaries_of_the_vector_and_product_kernels(ctx, K):
    """n_free = K - 1 = 42 .. 45: 6 n_free = 252 (one workgroup of 256 entries), 258, 264, 270 (two); 42 .. 45 block rows in
    workgroups of 4: 11 workgroups with 2 rows in the last, 11 with 3, 11 full, 12 with 1"""
    name = "traj:%d" % K
    sc, ref, dist, mask = pc.direct_reference(name)
    _tight(ctx, "PCG shape", name, sc, ref, dist, mask)


@pytest.mark.parametrize("K", [1025, 1026])
def test_more_partial_sums_than_one_pass_takes(ctx, K):
    """n_free = 1024 / 1025: 256 partials of the product (one pass of pcg_sum) and 257 (a second pass); against the CPU PCG
    reference"""
    name = "revisit:%d" % K
    sc, cpu = pc.pcg_reference(name, *TIGHT)
    got = _solve(ctx, sc)
    mask = ba_ref.outliers(cpu["poses"], cpu["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"])
    tg._check("PCG shape", name, got, sc, cpu, 0.0, mask)
    _ran_clean(got, TIGHT[0])


# ---- 5. edges ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [1, 3])
def test_a_small_cap_takes_the_iterate(ctx, cap):
    sc = bg.scene("traj:66")
    got = _solve(ctx, sc, (cap, 1e-12))
    st = got["pcg"]
    print("PCG cap %d: term %d it %d cost %.6g -> %.6g, %d solves, %d at the cap, longest %d" % (
        cap, got["termination"], got["iterations"], got["initial_cost"], got["final_cost"], st["solves"], st["at_cap"], st["longest"]))
    assert got["termination"] in (0, 1) and st["at_cap"] > 0 and st["longest"] == cap and st["breakdowns"] == 0
    assert st["iterations"] == cap * st["solves"]
    assert np.all(np.isfinite(got["poses"])) and np.all(np.isfinite(got["landmarks"]))
    assert np.isfinite(got["final_cost"]) and got["final_cost"] <= got["initial_cost"]
    tg._same_bits(got, _solve(ctx, sc, (cap, 1e-12)))


def test_failure_leaves_the_state_as_dense_does(ctx, pkg):
    for name in ("traj:66", "gross80"):
        clean = bg.scene(name)
        sc = {k: np.array(v) for k, v in clean.items()}
        sc["obs_cam"][5, 1] = np.nan
        dense = tg._solve(ctx, sc)
        got = _solve(ctx, sc)
        ctx.set_ba_global_pcg(False)
        assert got["termination"] == 2 and got["iterations"] == 0 and not np.isfinite(got["initial_cost"])
        assert got["poses"].tobytes() == sc["poses"].tobytes() and got["landmarks"].tobytes() == sc["landmarks"].tobytes()
        assert np.array_equal(got["outlier"], dense["outlier"]) and got["n_outliers"] == dense["n_outliers"]
        assert (dense["termination"], dense["iterations"]) == (2, 0) and got["pcg"]["iterations"] == 0
    c = pkg.Context(width=0, height=0)
    tg._same_bits(_solve(ctx, clean), _solve(c, clean))         # the context is usable afterwards
    c.close()


def test_huber_against_the_corrector_on_the_pcg_reference(ctx):
    loss = ("huber", lr.SCALE)
    sc, ref, aug, dist, mask = bc.reference("gross80", loss)
    ctx.set_ba_loss(*loss)
    got = _tight(ctx, "PCG huber", "gross80", sc, ref, dist, mask, loss=loss)
    tg._same_bits(got, _solve(ctx, sc))
    cpu = pc.pcg_reference("gross80", *TIGHT, loss=loss)[1]
    assert cpu["final_cost"] < 0.5 * pc.pcg_reference("gross80", *TIGHT)[1]["final_cost"]       # the loss is active


# ---- 6. state ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,setting", [("traj:66", TIGHT), ("hard66", DEFAULT), ("loop_row", DEFAULT), ("complete12", TIGHT),
                                          ("revisit:400", DEFAULT), ("revisit0:1900", DEFAULT)])
def test_a_second_call_returns_the_same_bits(ctx, name, setting):
    sc = pc.scene(name)
    a = _solve(ctx, sc, setting)
    assert a["termination"] == 0
    b = _solve(ctx, sc, setting)
    tg._same_bits(a, b)
    assert a["pcg"] == b["pcg"]


@pytest.mark.parametrize("other", ["dense", "sparse"])
def test_the_other_solvers_keep_their_bits_around_pcg(ctx, pkg, other):
    sc = bg.scene("traj:66")
    ctx.set_ba_global_solver(other)
    first = tg._solve(ctx, sc)
    assert ctx.ba_global_pcg_stats()["solves"] == 0
    p0 = _solve(ctx, sc)
    assert ctx.get_ba_global_solver() == (pkg.BA_GLOBAL_SOLVER_SPARSE if other == "sparse" else pkg.BA_GLOBAL_SOLVER_DENSE)
    ctx.set_ba_global_pcg(False)
    assert ctx.get_ba_global_pcg() == (False,) + DEFAULT
    again = tg._solve(ctx, sc)
    tg._same_bits(first, again)
    assert ctx.ba_global_pcg_stats()["solves"] == 0                 # the last global solve ran without PCG
    tg._same_bits(p0, _solve(ctx, sc))
    fresh = pkg.Context(width=0, height=0)
    assert fresh.get_ba_global_pcg() == (False,) + DEFAULT
    fresh.set_ba_global_solver(other)
    tg._same_bits(tg._solve(fresh, sc), first)
    tg._same_bits(_solve(fresh, sc), p0)
    fresh.close()


def test_a_sparse_pose_graph_solve_and_a_covariance_in_between(ctx, pkg):
    """the blocks share one buffer with both envelopes; the local solve does not read the setting"""
    sc = bc.scene("loop_row")
    a = _solve(ctx, sc, DEFAULT)
    graph = psc.scene("revisit200")
    ctx.set_pose_graph_solver("sparse")
    try:
        pg = ctx.pose_graph(graph["poses"], graph["edge_a"], graph["edge_b"], graph["edge_meas"], graph["sqrt_info"], graph["fixed"])
        free = int(np.flatnonzero(np.asarray(graph["fixed"]) == 0)[0])
        cov = ctx.pose_graph_covariance(pg["poses"], graph["edge_a"], graph["edge_b"], graph["edge_meas"], graph["sqrt_info"], graph["fixed"],
                                        poses_of=[free])
    finally:
        ctx.set_pose_graph_solver("dense")
    assert pg["termination"] == 0 and cov is not None
    tg._same_bits(a, _solve(ctx, sc, DEFAULT))
    small = bg.scene("traj:34")
    ctx.set_ba_global_pcg(False)
    local = ctx.bundle_adjust(*tg._args(small))
    ctx.set_ba_global_pcg(True, *DEFAULT)
    tg._same_bits(local, ctx.bundle_adjust(*tg._args(small)))


def test_capacity_then_a_small_solve(ctx, pkg):
    """a complete map of 1500 keyframes: 1500 x 1501 / 2 blocks (the library's own count, analyze's n_pairs), above the bound:
    E_CAPACITY, the count in the message, nothing touched; the context then solves as a fresh one does"""
    sc = bc.scene("wide:1500")
    n_pairs = pkg.ba_global_analyze(sc["fixed"], 1500, sc["obs_kf"], sc["obs_lm"], len(sc["landmarks"]))["n_pairs"]
    assert n_pairs == 1500 * 1501 // 2 > pkg.POSE_GRAPH_MAX_ENVELOPE_BLOCKS
    moved = dict(sc, poses=np.array(sc["poses"], np.float64))
    moved["poses"][:, 4] = 1e-3 * np.arange(1500)                # off the minimum: a solve would move them
    ctx.set_ba_global_pcg(True, *DEFAULT)
    rc, x, lm, out, before = _raw(ctx, pkg, moved)
    assert rc == pkg.E_CAPACITY and x.tobytes() == before[0].tobytes() and lm.tobytes() == before[1].tobytes() and np.all(out == 7)
    with pytest.raises(pkg.MslamHipError) as e:
        _solve(ctx, sc, DEFAULT)
    assert e.value.code == pkg.E_CAPACITY and str(n_pairs) in str(e.value)
    small = bc.scene("shuffled:66")
    got = _solve(ctx, small, DEFAULT)
    c = pkg.Context(width=0, height=0)
    tg._same_bits(got, _solve(c, small, DEFAULT))
    c.close()


def test_the_cap_on_keyframes(ctx, pkg):
    ctx.set_ba_global_pcg(True)
    over = np.tile([0, 0, 0, 1.0, 0, 0, 0], (pkg.BA_GLOBAL_MAX_KEYFRAMES_SPARSE + 1, 1))
    none = np.zeros(0, np.int32)
    with pytest.raises(pkg.MslamHipError) as e:
        ctx.bundle_adjust_global(over, np.zeros((1, 3)), none, none, np.zeros((0, 3)))
    assert e.value.code == pkg.E_INVALID
    ok = ctx.bundle_adjust_global(over[:-1], np.zeros((1, 3)), none, none, np.zeros((0, 3)))
    assert ok["termination"] == 0 and ok["final_cost"] == 0.0


def test_the_setter_rejects_bad_values_and_the_setting_stays(ctx, pkg):
    ctx.set_ba_global_pcg(True, 40, 1e-3)
    assert ctx.get_ba_global_pcg() == (True, 40, 1e-3)
    L, h, D = ctx.L, ctx._h, pkg.C.c_double
    for enable, it, tol in ((2, 500, 1e-6), (-1, 500, 1e-6), (1, 0, 1e-6), (1, -5, 1e-6), (1, 500, 0.0), (1, 500, 1.0), (1, 500, -1e-6),
                            (1, 500, 2.0), (1, 500, float("nan")), (1, 500, float("inf")), (0, 0, 1e-6), (0, 500, 1.0)):
        assert L.mslam_hip_set_ba_global_pcg(h, enable, it, D(tol)) == pkg.E_INVALID, (enable, it, tol)
        assert ctx.get_ba_global_pcg() == (True, 40, 1e-3)
    for bad in (dict(enable=2), dict(max_iterations=0), dict(max_iterations=2 ** 31), dict(tolerance=1.0), dict(enable="yes")):
        with pytest.raises(pkg.MslamHipError) as e:
            ctx.set_ba_global_pcg(**bad)
        assert e.value.code == pkg.E_INVALID and ctx.get_ba_global_pcg() == (True, 40, 1e-3)
    assert L.mslam_hip_get_ba_global_pcg(h, None, None, None) == pkg.OK and L.mslam_hip_get_ba_global_pcg_stats(h, None) == pkg.OK
    assert L.mslam_hip_set_ba_global_pcg(None, 1, 500, D(1e-6)) == pkg.E_INVALID
    ctx.set_ba_global_pcg(True, 1, 0.5)
    assert ctx.get_ba_global_pcg() == (True, 1, 0.5)
    ctx.set_ba_global_pcg(False)
    assert ctx.get_ba_global_pcg() == (False,) + DEFAULT
    # the other setter keeps its two kinds
    assert L.mslam_hip_set_ba_global_solver(h, 2) == pkg.E_INVALID and ctx.get_ba_global_solver() == pkg.BA_GLOBAL_SOLVER_DENSE
    assert ctx.get_pose_graph_solver() == pkg.PG_SOLVER_DENSE


def test_stage_names(pkg):
    sc = bg.scene("traj:66")
    c = pkg.Context(width=0, height=0)
    plain = _solve(c, sc, DEFAULT)
    c.set_profiling(2)
    c.stage_times()
    timed = _solve(c, sc, DEFAULT)
    names = {n for n, ms in c.stage_times()}
    c.set_profiling(0)
    assert {"solver_schur", "solver_precond", "solver_cg", "ba_iterations", "ba_start_cost"} <= names
    assert not names & {"solver_factor", "solver_subst"}
    tg._same_bits(plain, timed)
    c.close()


# ---- 7. above the ABI -----------------------------------------------------------------------------------------------------------------------

def test_backend_global_ba_on_revisit_1900(pkg):
    """HipBackend(global_solver=True, global_pcg=...) on a map no other solver takes, on a context whose own setting is off
    and stays off; without global_pcg the same map is E_CAPACITY"""
    sc, cpu = pc.pcg_reference("revisit:1900", *TIGHT)
    K = len(sc["poses"])
    c = pkg.Context(width=0, height=0, max_keypoints=64)
    c.set_ba_global_pcg(False, 77, 1e-2)
    be = pkg.HipBackend(c, global_solver=True, global_pcg=TIGHT)
    order = np.argsort(sc["obs_kf"], kind="stable")
    start = np.searchsorted(sc["obs_kf"][order], np.arange(K + 1))
    for k in range(K):                                        # ids = indices, keyframe 0 first: it is the constant one
        m = order[start[k]:start[k + 1]]
        be.add_keyframe(k, sc["poses"][k], sc["obs_lm"][m].astype(np.int64), sc["obs_cam"][m])
    for l in list(be.landmarks):
        be.landmarks[l] = sc["landmarks"][l].copy()
    got = be.global_ba()
    assert c.get_ba_global_pcg() == (False, 77, 1e-2) and c.get_ba_global_solver() == pkg.BA_GLOBAL_SOLVER_DENSE
    dx = max(float(np.max(np.abs(got["poses"] - cpu["poses"]))),
             float(np.max(np.abs(got["landmarks"] - cpu["landmarks"][got["landmark_ids"]]))))
    print("PCG backend revisit:1900 term %d it %d/%d cost %.6g -> %.6g / %.6g dx %.3e CG %s" % (
        got["termination"], got["iterations"], cpu["iterations"], got["initial_cost"], got["final_cost"], cpu["final_cost"], dx, got["pcg"]))
    assert got["termination"] == 0 and abs(got["iterations"] - cpu["iterations"]) <= 1 and got["invalid_steps"] == 0
    assert got["keyframes"] == list(range(K)) and dx <= 1e-9
    assert got["pcg"]["solves"] > 0 and got["pcg"]["at_cap"] == 0 and got["pcg"]["breakdowns"] == 0
    assert be.poses[0].tobytes() == sc["poses"][0].tobytes() and be.poses[7].tobytes() == got["poses"][7].tobytes()
    be.global_pcg = None
    for kind, code in (("dense", pkg.E_CAPACITY), ("sparse", pkg.E_CAPACITY)):
        be.global_linear_solver = pkg._pg_solver_kind(kind, "test")
        with pytest.raises(pkg.MslamHipError) as e:
            be.global_ba()
        assert e.value.code == code
        assert c.get_ba_global_solver() == pkg.BA_GLOBAL_SOLVER_DENSE
    c.close()


def test_tracker_ring_walk_with_pcg(pkg):
    """tests/test_gpu_pose_graph.py's ring walk with loop_global_ba and ba_global_pcg: the loop closes, the global solve runs
    by PCG and ends usable, the context's own setting stays off"""
    seq = loop_walk.ring_sequence()
    c, t, rows = tpg._run_ring(pkg, seq, loop_closure=True, loop_min_gap=5, loop_global_ba=True, ba_global_pcg=DEFAULT)
    assert t.backend.global_pcg == DEFAULT and t.backend.global_solver
    closed = [a for a in t.loop_results if a["loop"] is not None]
    assert len(closed) == 1 and all(r["tracked"] for r in rows)
    res, ba = closed[0]["result"], closed[0]["global_ba"]
    print("PCG ring walk: closure %s, global BA term %d it %d cost %.6g -> %.6g, CG %s" % (
        closed[0]["loop"], ba["termination"], ba["iterations"], ba["initial_cost"], ba["final_cost"], ba["pcg"]))
    assert res["termination"] == 0
    assert ba["termination"] in (0, 1) and ba["invalid_steps"] == 0 and ba["final_cost"] <= ba["initial_cost"]
    assert ba["pcg"]["solves"] > 0 and ba["pcg"]["breakdowns"] == 0
    assert ba["keyframes"] == res["keyframes"] and ba["n_written"] >= len(ba["landmark_ids"]) > 0
    assert c.get_ba_global_pcg() == (False,) + DEFAULT
    c.close()
