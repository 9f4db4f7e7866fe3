"""mslam_hip_pose_graph with mslam_hip_set_pose_graph_pcg on the MI355X (k_pg_assemble_pairs of k_posegraph.hip writing the
non-zero blocks of the damped normal equations, the block-Jacobi preconditioned conjugate gradients of k_pcg.hip) through
Context.set_pose_graph_pcg and Context.pose_graph.

Bounds, every one from the CPU alone.  Tight tier (cap 2000, tolerance 1e-12): tests/test_gpu_pose_graph_sparse.py's _against as
it is, |x_gpu - x_ref|_inf <= max(1e-9, 1000 dist) with dist the larger of the two direct CPU solvers' distance and the CPU
PCG reference's (tests/pose_graph_pcg_ref.py) distance to the direct solution.  Default tier (500, 1e-6) and at the cap: both
the GPU and the CPU PCG reference are inexact solutions whose error the tolerance (or the cap) sets; d is the CPU PCG
reference's own distance to the direct solution and the bound max(1e-9, 10 d), the factor for a stopping index that differs
by one or two.  Above every other solver's ground: within 1e-9 of the CPU PCG reference at the tight tier (the project's floor
for two solves of the same tolerance), and against the truth on the noise-free scene, max(1e-7, 10 x the CPU PCG reference's
own distance to it).  No test asserts a time.

The boundaries of the kernels (k_pcg.hip): the vector kernels take 256 entries per workgroup, so 6 n_free = 252 / 258 (n_free
42 / 43) is one workgroup / two; k_pcg_product takes 4 block rows per workgroup (n_free 42 .. 45: 2, 3, 4, 1 rows in the last)
and 10 neighbours per pass (rows of 9, 10, 11 blocks: complete:10 / 11 / 12, whose constant pose 0 leaves K - 1 free poses with
K - 2 neighbours and the diagonal); every scalar is a sum of per-workgroup partials taken 256 at a time, so more than 256
partials of the product is n_free > 1024 (walk:1025 / 1026: 256 and 257 of them).

loops:257 and loops:258 of pose_graph_sparse_cases.ENVELOPE are left out of the tight tier by name: a thin chain needs about
nine CG iterations per pose, the CPU PCG reference itself ends 7 of 9 solves of loops:258 at the cap of 2000
(tests/test_pose_graph_pcg.py), and a solve that ends at the cap does not make the direct solver's decisions to the last bit.
loops:258 is the at-the-cap test instead.

A complete graph of 1500 poses, above the block bound as a bundle adjustment's map, cannot reach it here: its 1124250 edges
are above MSLAM_HIP_POSE_GRAPH_MAX_EDGES (65536), which mslam_hip_pose_graph checks first (E_INVALID, as before this setting),
and with E <= 65536 and K <= 16384 the stored blocks are at most 81920 < 1048576.  The test asserts what the call does."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_global_cases as bg  # noqa: E402
import loop_walk  # noqa: E402
import pose_graph_cases as pc  # noqa: E402
import pose_graph_loss_ref as pl  # noqa: E402
import pose_graph_pcg_cases as pcc  # noqa: E402
import pose_graph_pcg_ref as pr  # noqa: E402
import pose_graph_ref as pg  # noqa: E402
import pose_graph_sparse_cases as psc  # noqa: E402
import test_gpu_ba_global as tg  # noqa: E402
import test_gpu_pose_graph as tpg  # noqa: E402
import test_gpu_pose_graph_sparse as tps  # noqa: E402

pytestmark = pytest.mark.gpu
TIGHT, DEFAULT = pcc.TIGHT, pcc.DEFAULT


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(width=0, height=0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def off_again(ctx):
    yield
    ctx.set_pose_graph_pcg(False)
    ctx.set_pose_graph_solver("dense")
    ctx.set_pose_graph_loss("none")
    ctx.set_ba_global_pcg(False)


def _solve(ctx, sc, setting=TIGHT, **over):
    ctx.set_pose_graph_pcg(True, *setting)
    got = tps._solve(ctx, sc, **over)
    got["pcg"] = ctx.pose_graph_pcg_stats()
    return got


def _ran_clean(got, cap):
    st = got["pcg"]
    print("     CG: %d solves, %d iterations, longest %d, at the cap %d, breakdowns %d" % (
        st["solves"], st["iterations"], st["longest"], st["at_cap"], st["breakdowns"]))
    assert st["at_cap"] == 0 and st["breakdowns"] == 0 and st["longest"] < cap
    assert st["solves"] in (0, got["iterations"])               # one linear solve per iteration, none without a free pose
    assert st["iterations"] >= st["longest"]


def _tight(ctx, name, sc, ref, dist):
    """the tight tier on one scene: dist from the CPU alone"""
    cpu = pcc.pcg(name, TIGHT)[1]
    assert cpu["at_cap"] == 0 and cpu["breakdowns"] == 0
    got = _solve(ctx, sc)
    tps._against("PCG " + name, sc, got, ref, max(dist, pc.same_rotation_distance(cpu["poses"], ref["poses"])))
    _ran_clean(got, TIGHT[0])
    return got


# ---- 1. the tight tier -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", pcc.TIGHT_TIER)
def test_tight_against_the_direct_references(ctx, name):
    sc, ref, other, dist = pcc.direct(name)
    got = _tight(ctx, name, sc, ref, dist)
    start = np.asarray(sc["poses"], np.float64)
    if name in ("all_fixed", "empty", "cap0"):                  # no system, or no iteration: the statistics are zero
        assert got["pcg"] == dict(solves=0, iterations=0, longest=0, at_cap=0, breakdowns=0)
        assert got["poses"].tobytes() == start.tobytes()
    else:
        assert got["pcg"]["solves"] == got["iterations"] >= 1
    if name in ("pair_component", "two_components"):           # the component with a free gauge moves and stays finite
        assert np.all(np.isfinite(got["poses"])) and not np.array_equal(got["poses"][5], start[5])
    if name == "rejected":
        assert got["rejected_steps"] == ref["trace"]["rejected"] >= 1
    if name == "cap1":
        assert got["termination"] == 1 and got["iterations"] == 1 and got["pcg"]["solves"] == 1


# ---- 2. at the cap ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("setting", [TIGHT, DEFAULT])
def test_at_the_cap(ctx, setting):
    """loops:258, a thin chain of 257 free poses: CG ends most solves at the cap, the iterate is taken, and the trust region
    still ends where the direct solver ends.  d (CPU): 1.5e-10 at (2000, 1e-12), 3.2e-5 at the defaults"""
    sc, ref, other, dist = pcc.direct("loops:258")
    cpu = pcc.pcg("loops:258", setting)[1]
    d = pcc.distance("loops:258", setting)
    got = _solve(ctx, sc, setting)
    reached = pc.same_rotation_distance(got["poses"], ref["poses"])
    bound = max(1e-9, 10.0 * d)
    st = got["pcg"]
    print("PCG at the cap %s term %d/%d it %d/%d/%d at cap %d/%d of %d solves  d(cpu pcg, direct) %.3e  reached %.3e  bound %.3e" % (
        setting, got["termination"], ref["termination"], got["iterations"], cpu["iterations"], ref["iterations"], st["at_cap"],
        cpu["at_cap"], st["solves"], d, reached, bound))
    assert cpu["at_cap"] > 0                                   # the reference itself
    assert st["at_cap"] > 0 and st["longest"] == setting[0] and st["breakdowns"] == 0 and got["invalid_steps"] == 0
    assert got["termination"] == ref["termination"] and abs(got["iterations"] - ref["iterations"]) <= 1
    assert reached <= bound


# ---- 3. the default tier ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", pcc.DEFAULT_TIER)
def test_default_tolerance(ctx, name):
    sc, ref, other, dist = pcc.direct(name)
    cpu = pcc.pcg(name, DEFAULT)[1]
    d = pcc.distance(name, DEFAULT)
    got = _solve(ctx, sc, DEFAULT)
    reached = pc.same_rotation_distance(got["poses"], ref["poses"])
    bound = max(1e-9, 10.0 * d)
    st = got["pcg"]
    print("PCG default %-12s term %d/%d it %d/%d/%d cost %.9g/%.9g  d(cpu pcg, direct) %.3e  reached %.3e  bound %.3e  CG longest %d/%d total %d" % (
        name, got["termination"], ref["termination"], got["iterations"], cpu["iterations"], ref["iterations"], got["final_cost"],
        ref["final_cost"], d, reached, bound, st["longest"], max(cpu["cg"]), st["iterations"]))
    assert cpu["at_cap"] == 0 and cpu["termination"] == ref["termination"] and cpu["iterations"] == ref["iterations"]   # the reference itself
    assert got["termination"] == ref["termination"] and abs(got["iterations"] - ref["iterations"]) <= 1
    assert got["invalid_steps"] == 0 and st["at_cap"] == 0 and st["breakdowns"] == 0
    second_order = len(sc["edge_a"]) * (pc.jacobian_row_bound(sc) * bound) ** 2 / 2.0
    assert abs(got["final_cost"] - ref["final_cost"]) <= 1e-6 * ref["final_cost"] + second_order
    assert reached <= bound


# ---- 4. the ground no other solver takes -------------------------------------------------------------------------------------------------

def _raw(ctx, pkg, sc):
    """the C call on a copy -> (rc, poses, the copy before)"""
    x = np.ascontiguousarray(sc["poses"], np.float64).copy()
    before = x.copy()
    ea, eb = np.ascontiguousarray(sc["edge_a"], np.int32), np.ascontiguousarray(sc["edge_b"], np.int32)
    z, fx = np.ascontiguousarray(sc["edge_meas"], np.float64), np.ascontiguousarray(sc["fixed"], np.uint8)
    rc = ctx.L.mslam_hip_pose_graph(ctx._h, pkg._p(x), pkg._p(fx), len(x), pkg._p(ea), pkg._p(eb), pkg._p(z), None, len(ea), 100, None)
    return rc, x, before


def _against_the_cpu_pcg(name, sc, got, cpu):
    dx = pc.same_rotation_distance(got["poses"], cpu["poses"])
    print("PCG %-12s term %d/%d it %d/%d cost %.9g/%.9g dx %.3e CG %s / longest %d" % (
        name, got["termination"], cpu["termination"], got["iterations"], cpu["iterations"], got["final_cost"], cpu["final_cost"], dx,
        got["pcg"], max(cpu["cg"])))
    tps._against("PCG " + name, sc, got, cpu, 0.0)             # dist = 0: the floor, 1e-9
    _ran_clean(got, TIGHT[0])


def test_random2048_that_no_other_solver_takes(ctx, pkg):
    """20000 random pairs among 2048 poses, "chosen: None" in pose_graph_sparse_cases.table(): DENSE rejects K, SPARSE the
    envelope (1704117 blocks in the better order), both with nothing touched; PCG ends within 1e-9 of the CPU PCG reference
    and leaves the solver setting as it was"""
    sc, cpu = pcc.pcg("random2048", TIGHT)
    ctx.set_pose_graph_solver("dense")
    rc, x, before = _raw(ctx, pkg, sc)
    assert rc == pkg.E_INVALID and x.tobytes() == before.tobytes()
    ctx.set_pose_graph_solver("sparse")
    rc, x, before = _raw(ctx, pkg, sc)
    assert rc == pkg.E_CAPACITY and x.tobytes() == before.tobytes()
    assert ctx.pose_graph_pcg_stats()["solves"] == 0
    got = _solve(ctx, sc)
    assert ctx.get_pose_graph_solver() == pkg.PG_SOLVER_SPARSE          # PCG ran whatever that setting says, and left it
    assert cpu["at_cap"] == 0 and cpu["termination"] == 0
    _against_the_cpu_pcg("random2048", sc, got, cpu)


def test_a_noise_free_walk_reaches_the_truth(ctx, pkg):
    """walk0:2800: both orders of the envelope are above the bound (tests/test_pose_graph_pcg.py), the measurements are exact,
    so the minimum is the truth.  6 n_free = 16794 entries: 66 workgroups of the vector kernels, 700 of the product"""
    name = "walk0:%d" % pcc.WALK0_K
    sc, cpu = pcc.pcg(name, TIGHT)
    assert min(pcc.envelope(sc)) > pkg.POSE_GRAPH_MAX_ENVELOPE_BLOCKS
    got = _solve(ctx, sc)
    err, cpu_err = pc.same_rotation_distance(got["poses"], sc["truth_poses"]), pc.same_rotation_distance(cpu["poses"], sc["truth_poses"])
    print("PCG %s err %.3e, the CPU PCG reference's %.3e" % (name, err, cpu_err))
    _against_the_cpu_pcg(name, sc, got, cpu)
    assert err <= max(1e-7, 10.0 * cpu_err)


# ---- 5. shapes --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", pcc.SHAPES)
def test_workgroup_and_pass_boundaries(ctx, name):
    """chain:43 .. 46: n_free 42 .. 45; complete:10 / 11 / 12: rows either side of the pass of 10; duplicates: a pair with
    several edges, both directions"""
    sc, ref, other, dist = pcc.direct(name)
    _tight(ctx, name, sc, ref, dist)


@pytest.mark.parametrize("name", pcc.PARTIALS)
def test_more_partial_sums_than_one_pass_takes(ctx, name):
    """n_free = 1024 / 1025: 256 partials of the product (one pass of pcg_sum) and 257 (a second pass); against the CPU PCG
    reference (a direct CPU solve of this graph takes 40 s)"""
    sc, cpu = pcc.pcg(name, TIGHT)
    got = _solve(ctx, sc)
    assert cpu["at_cap"] == 0
    _against_the_cpu_pcg(name, sc, got, cpu)


# ---- 6. edges ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [1, 3])
def test_a_small_cap_takes_the_iterate(ctx, cap):
    sc = pcc.scene("loops:66")
    got = _solve(ctx, sc, (cap, 1e-12))
    st = got["pcg"]
    print("PCG cap %d: term %d it %d cost %.6g -> %.6g, %d solves, %d at the cap, longest %d" % (
        cap, got["termination"], got["iterations"], got["initial_cost"], got["final_cost"], st["solves"], st["at_cap"], st["longest"]))
    assert got["termination"] in (0, 1) and st["at_cap"] > 0 and st["longest"] == cap and st["breakdowns"] == 0
    assert st["iterations"] == cap * st["solves"]
    assert np.all(np.isfinite(got["poses"]))
    assert np.isfinite(got["final_cost"]) and got["final_cost"] <= got["initial_cost"]
    again = _solve(ctx, sc, (cap, 1e-12))
    tps._same_bits(got, again)
    assert again["pcg"] == st


def test_failure_leaves_the_state_as_dense_does(ctx, pkg):
    clean = pcc.scene("loops:66")
    sc = {k: (np.array(v) if v is not None else None) for k, v in clean.items()}
    sc["edge_meas"][5, 5] = np.nan                              # a position: the quaternion check passes
    dense = tps._solve(ctx, sc)
    got = _solve(ctx, sc)
    ctx.set_pose_graph_pcg(False)
    assert got["termination"] == 2 and got["iterations"] == 0 and not np.isfinite(got["initial_cost"])
    assert got["poses"].tobytes() == sc["poses"].tobytes()
    assert (dense["termination"], dense["iterations"]) == (2, 0) and dense["poses"].tobytes() == got["poses"].tobytes()
    assert got["pcg"]["iterations"] == 0 and got["pcg"]["solves"] == 0
    c = pkg.Context(width=0, height=0)
    a, b = _solve(ctx, clean), _solve(c, clean)                 # the context is usable afterwards
    tps._same_bits(a, b)
    assert a["pcg"] == b["pcg"]
    c.close()


def test_huber_against_the_corrector_on_the_pcg_reference(ctx):
    """a chain of 40 poses with 10 loop edges and 3 grossly wrong ones (tests/pose_graph_loss_ref.py): k_pg_edges_loss corrects
    the rows before k_pg_assemble_pairs reads them"""
    name, loss = "false:40,10,3,2", ("huber", pl.SCALE)
    sc, ref, ch, dist = pl.reference(name, "huber")
    cpu = pr.solve(sc, cg_max_iterations=TIGHT[0], cg_tolerance=TIGHT[1], loss=loss)
    plain = pr.solve(sc, cg_max_iterations=TIGHT[0], cg_tolerance=TIGHT[1])
    assert cpu["at_cap"] == 0 and cpu["breakdowns"] == 0
    assert cpu["termination"] == ref["termination"] and cpu["iterations"] == ref["iterations"]
    ctx.set_pose_graph_loss(*loss)
    got = _solve(ctx, sc)
    tps._against("PCG huber " + name, sc, got, ref, max(dist, pc.same_rotation_distance(cpu["poses"], ref["poses"])))
    _ran_clean(got, TIGHT[0])
    again = _solve(ctx, sc)
    tps._same_bits(got, again)
    assert cpu["final_cost"] < 0.5 * plain["final_cost"]          # the loss is active
    chi2, weight = ctx.pose_graph_edge_weights(got["poses"], sc["edge_a"], sc["edge_b"], sc["edge_meas"], sc["sqrt_info"])
    assert np.all(weight[sc["bad"]] < 1.0)


def test_the_cap_on_keyframes(ctx, pkg):
    ctx.set_pose_graph_solver("dense")
    ctx.set_pose_graph_pcg(True)
    K = pkg.POSE_GRAPH_MAX_KEYFRAMES_SPARSE + 1
    over = psc.identity_scene(K, pc.chain(K))
    with pytest.raises(pkg.MslamHipError) as e:
        tps._solve(ctx, over)
    assert e.value.code == pkg.E_INVALID and str(pkg.POSE_GRAPH_MAX_KEYFRAMES_SPARSE) in str(e.value)
    unit = np.tile([0, 0, 0, 1.0, 0, 0, 0], (K - 1, 1))
    none = np.zeros(0, np.int32)
    ok = ctx.pose_graph(unit, none, none, np.zeros((0, 7)))
    assert ok["termination"] == 0 and ok["final_cost"] == 0.0 and ctx.pose_graph_pcg_stats()["solves"] == 0


def test_complete_1500_is_rejected_by_the_edge_cap_first(ctx, pkg):
    """see the module's docstring: 1500 x 1499 / 2 edges are above the edge cap, which is checked before any block is counted,
    so the call is E_INVALID with nothing touched, as it is without PCG; the context then solves as a fresh one does"""
    sc = psc.identity_scene(1500, psc.complete(1500))
    assert len(sc["edge_a"]) == 1500 * 1499 // 2 > pkg.POSE_GRAPH_MAX_EDGES
    assert pkg.POSE_GRAPH_MAX_EDGES + pkg.POSE_GRAPH_MAX_KEYFRAMES_SPARSE < pkg.POSE_GRAPH_MAX_ENVELOPE_BLOCKS
    moved = dict(sc, poses=np.array(sc["poses"], np.float64))
    moved["poses"][:, 4] = 1e-3 * np.arange(1500)
    ctx.set_pose_graph_pcg(True, *DEFAULT)
    rc, x, before = _raw(ctx, pkg, moved)
    assert rc == pkg.E_INVALID and x.tobytes() == before.tobytes()
    small = pcc.scene("walk:130")
    got = _solve(ctx, small, DEFAULT)
    c = pkg.Context(width=0, height=0)
    tps._same_bits(got, _solve(c, small, DEFAULT))
    c.close()


def test_the_most_blocks_a_call_can_store(ctx, pkg):
    """the edge cap: 65536 distinct pairs among 16384 poses, 81919 stored blocks, the most mslam_hip_pose_graph can ask for;
    identity poses and measurements, so the start is the minimum and the solve ends at once"""
    K = pkg.POSE_GRAPH_MAX_KEYFRAMES_SPARSE
    edges = psc.band(K, 4)[:pkg.POSE_GRAPH_MAX_EDGES]
    sc = psc.identity_scene(K, edges)
    got = _solve(ctx, sc, DEFAULT)
    assert got["termination"] == 0 and got["final_cost"] == 0.0 and got["poses"].tobytes() == np.asarray(sc["poses"]).tobytes()
    assert got["pcg"]["breakdowns"] == 0


def test_the_setter_rejects_bad_values_and_the_setting_stays(ctx, pkg):
    ctx.set_pose_graph_pcg(True, 40, 1e-3)
    assert ctx.get_pose_graph_pcg() == (True, 40, 1e-3)
    L, h, D = ctx.L, ctx._h, pkg.C.c_double
    for enable, it, tol in ((2, 500, 1e-6), (-1, 500, 1e-6), (1, 0, 1e-6), (1, -5, 1e-6), (1, 500, 0.0), (1, 500, 1.0), (1, 500, -1e-6),
                            (1, 500, 2.0), (1, 500, float("nan")), (1, 500, float("inf")), (0, 0, 1e-6), (0, 500, 1.0)):
        assert L.mslam_hip_set_pose_graph_pcg(h, enable, it, D(tol)) == pkg.E_INVALID, (enable, it, tol)
        assert ctx.get_pose_graph_pcg() == (True, 40, 1e-3)
    for bad in (dict(enable=2), dict(max_iterations=0), dict(max_iterations=2 ** 31), dict(tolerance=1.0), dict(enable="yes")):
        with pytest.raises(pkg.MslamHipError) as e:
            ctx.set_pose_graph_pcg(**bad)
        assert e.value.code == pkg.E_INVALID and ctx.get_pose_graph_pcg() == (True, 40, 1e-3)
    assert L.mslam_hip_get_pose_graph_pcg(h, None, None, None) == pkg.OK and L.mslam_hip_get_pose_graph_pcg_stats(h, None) == pkg.OK
    assert L.mslam_hip_set_pose_graph_pcg(None, 1, 500, D(1e-6)) == pkg.E_INVALID
    assert L.mslam_hip_get_pose_graph_pcg(None, None, None, None) == pkg.E_INVALID
    assert L.mslam_hip_get_pose_graph_pcg_stats(None, None) == pkg.E_INVALID
    ctx.set_pose_graph_pcg(True, 1, 0.5)
    assert ctx.get_pose_graph_pcg() == (True, 1, 0.5)
    # a setting of its own: neither the solver's kind nor the bundle adjustment's PCG moves with it, nor it with them
    assert ctx.get_pose_graph_solver() == pkg.PG_SOLVER_DENSE and ctx.get_ba_global_pcg() == (False, pkg.BA_GLOBAL_PCG_MAX_ITERATIONS,
                                                                                             pkg.BA_GLOBAL_PCG_TOLERANCE)
    ctx.set_ba_global_pcg(True, 7, 0.25)
    assert ctx.get_pose_graph_pcg() == (True, 1, 0.5)
    ctx.set_pose_graph_pcg(False)
    assert ctx.get_pose_graph_pcg() == (False,) + DEFAULT == (False, pkg.POSE_GRAPH_PCG_MAX_ITERATIONS, pkg.POSE_GRAPH_PCG_TOLERANCE)
    assert ctx.get_ba_global_pcg() == (True, 7, 0.25)
    for bad in ((0, 1e-6), (500, 1.0), "yes"):
        with pytest.raises(pkg.MslamHipError) as e:
            pkg.HipBackend(None, pose_graph_pcg=bad)
        assert e.value.code == pkg.E_INVALID
    with pytest.raises(pkg.MslamHipError) as e:
        pkg.HipKeyframeTracker(ctx, pose_graph_pcg=True)         # needs loop_closure
    assert e.value.code == pkg.E_INVALID


def test_stage_names(pkg):
    sc = pcc.scene("complete40")
    c = pkg.Context(width=0, height=0)
    plain = _solve(c, sc, DEFAULT)
    c.set_profiling(2)
    c.stage_times()
    timed = _solve(c, sc, DEFAULT)
    names = {n for n, ms in c.stage_times()}
    c.set_profiling(0)
    assert {"solver_schur", "solver_precond", "solver_cg", "pg_iterations", "pg_start_cost", "pg_blocks", "pg_step"} <= names
    assert not names & {"solver_factor", "solver_subst"}
    tps._same_bits(plain, timed)
    c.close()


# ---- 7. state ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,setting", [("loops:66", TIGHT), ("revisit200", DEFAULT), ("complete:12", TIGHT), ("star70", DEFAULT),
                                          ("walk:400", DEFAULT), ("loops:258", DEFAULT)])
def test_a_second_call_returns_the_same_bits(ctx, name, setting):
    sc = pcc.scene(name)
    a = _solve(ctx, sc, setting)
    assert a["termination"] == 0
    b = _solve(ctx, sc, setting)
    tps._same_bits(a, b)
    assert a["pcg"] == b["pcg"]


@pytest.mark.parametrize("other", ["dense", "sparse"])
def test_the_other_solvers_keep_their_bits_around_pcg(ctx, pkg, other):
    sc = pcc.scene("loops:66")
    ctx.set_pose_graph_solver(other)
    first = tps._solve(ctx, sc)
    assert ctx.pose_graph_pcg_stats()["solves"] == 0
    p0 = _solve(ctx, sc)
    assert ctx.get_pose_graph_solver() == (pkg.PG_SOLVER_SPARSE if other == "sparse" else pkg.PG_SOLVER_DENSE)
    ctx.set_pose_graph_pcg(False)
    assert ctx.get_pose_graph_pcg() == (False,) + DEFAULT
    again = tps._solve(ctx, sc)
    tps._same_bits(first, again)
    assert ctx.pose_graph_pcg_stats()["solves"] == 0                 # the last pose-graph solve ran without PCG
    p1 = _solve(ctx, sc)
    tps._same_bits(p0, p1)
    assert p0["pcg"] == p1["pcg"]
    fresh = pkg.Context(width=0, height=0)
    assert fresh.get_pose_graph_pcg() == (False,) + DEFAULT
    fresh.set_pose_graph_solver(other)
    tps._same_bits(tps._solve(fresh, sc), first)
    tps._same_bits(_solve(fresh, sc), p0)
    fresh.close()


def test_a_global_ba_with_pcg_and_a_covariance_in_between(ctx, pkg):
    """the blocks share d_ba_S with the bundle adjustment's blocks and the covariance's envelope; the two PCG settings and
    their statistics are apart"""
    graph = pcc.scene("revisit200")
    a = _solve(ctx, graph, DEFAULT)
    sc = bg.scene("traj:66")
    ctx.set_ba_global_pcg(True, 300, 1e-8)
    ba0 = tg._solve(ctx, sc)
    ba_stats = ctx.ba_global_pcg_stats()
    assert ba_stats["solves"] > 0 and ctx.pose_graph_pcg_stats() == a["pcg"] and ctx.get_pose_graph_pcg() == (True,) + DEFAULT
    free = int(np.flatnonzero(np.asarray(graph["fixed"]) == 0)[0])
    cov0 = ctx.pose_graph_covariance(a["poses"], graph["edge_a"], graph["edge_b"], graph["edge_meas"], graph["sqrt_info"], graph["fixed"],
                                     poses_of=[free])
    assert ctx.pose_graph_pcg_stats() == a["pcg"]                  # the covariance and the edge weights do not read the setting
    b = _solve(ctx, graph, DEFAULT)
    tps._same_bits(a, b)
    assert a["pcg"] == b["pcg"] and ctx.ba_global_pcg_stats() == ba_stats and ctx.get_ba_global_pcg() == (True, 300, 1e-8)
    tg._same_bits(ba0, tg._solve(ctx, sc))
    cov1 = ctx.pose_graph_covariance(a["poses"], graph["edge_a"], graph["edge_b"], graph["edge_meas"], graph["sqrt_info"], graph["fixed"],
                                     poses_of=[free])
    assert cov0["cov"].tobytes() == cov1["cov"].tobytes()
    ctx.set_pose_graph_pcg(False)
    ctx.set_pose_graph_solver("sparse")
    cov2 = ctx.pose_graph_covariance(a["poses"], graph["edge_a"], graph["edge_b"], graph["edge_meas"], graph["sqrt_info"], graph["fixed"],
                                     poses_of=[free])
    assert cov0["cov"].tobytes() == cov2["cov"].tobytes()          # under any setting
    w0 = ctx.pose_graph_edge_weights(a["poses"], graph["edge_a"], graph["edge_b"], graph["edge_meas"], graph["sqrt_info"])
    ctx.set_pose_graph_pcg(True)
    w1 = ctx.pose_graph_edge_weights(a["poses"], graph["edge_a"], graph["edge_b"], graph["edge_meas"], graph["sqrt_info"])
    assert w0[0].tobytes() == w1[0].tobytes() and w0[1].tobytes() == w1[1].tobytes()


# ---- 8. above the ABI -----------------------------------------------------------------------------------------------------------------------

def test_backend_close_loop_on_a_revisiting_map_above_1024_keyframes(pkg):
    """HipBackend(pose_graph_pcg=...) on walk:1100's graph as the covisibility graph, on a context whose own setting is off and
    stays off, against the CPU PCG reference on loop_problem()'s arrays; without pose_graph_pcg the same map is E_CAPACITY
    before the context is touched"""
    sc = pcc.scene("walk:1100")
    K = len(sc["poses"])
    c = pkg.Context(width=0, height=0)
    c.set_pose_graph_pcg(False, 77, 1e-2)
    be = pkg.HipBackend(c, pose_graph_pcg=TIGHT)
    rng = np.random.default_rng(9)
    for k in range(K):                                        # ids = indices, keyframe 0 first: it is the constant one
        be.add_keyframe(k, sc["poses"][k], [10 * k, 10 * k + 1], rng.uniform([-1, -1, 1.5], [1, 1, 3.0], (2, 3)))
    graph = {k: set() for k in range(K)}
    for a, b in zip(sc["edge_a"].tolist(), sc["edge_b"].tolist()):
        graph[a].add(b), graph[b].add(a)
    T = sc["truth_poses"][-1]
    R = pg.q_matrix(T[:4]).T
    rvec, tvec = tps._rvec(R), -R @ T[4:]
    ids, poses, fixed, ea, eb, meas, info = be.loop_problem(K - 1, 0, rvec, tvec, graph)
    cpu = pr.pose_graph(poses, ea, eb, meas, info, fixed, be.max_iterations, *TIGHT)
    lm_before = {l: be.landmarks[l].copy() for l in (10 * (K - 1), 10 * 7 + 1)}
    got = be.close_loop(K - 1, 0, rvec, tvec, graph)
    assert c.get_pose_graph_pcg() == (False, 77, 1e-2) and c.get_pose_graph_solver() == pkg.PG_SOLVER_DENSE
    dx = pc.same_rotation_distance(got["poses"], cpu["poses"])
    print("PCG close_loop walk:1100 term %d/%d it %d/%d cost %.6g -> %.6g / %.6g dx %.3e CG %s" % (
        got["termination"], cpu["termination"], got["iterations"], cpu["iterations"], got["initial_cost"], got["final_cost"],
        cpu["final_cost"], dx, got["pcg"]))
    assert cpu["at_cap"] == 0 and cpu["termination"] == 0
    assert got["termination"] == 0 and abs(got["iterations"] - cpu["iterations"]) <= 1 and got["invalid_steps"] == 0
    assert got["keyframes"] == list(range(K)) and dx <= 1e-9
    assert got["pcg"]["solves"] > 0 and got["pcg"]["at_cap"] == 0 and got["pcg"]["breakdowns"] == 0
    assert be.poses[0].tobytes() == sc["poses"][0].tobytes() and be.poses[7].tobytes() == got["poses"][7].tobytes()
    assert not np.array_equal(got["poses"][K - 1], poses[K - 1])
    for l, X in lm_before.items():                              # a landmark moves rigidly with its anchor keyframe
        k = l // 10
        local = pg.q_matrix(poses[k, :4]).T @ (X - poses[k, 4:])
        assert np.max(np.abs(be.landmarks[l] - (pg.q_matrix(got["poses"][k, :4]) @ local + got["poses"][k, 4:]))) <= 1e-12
    be.pose_graph_pcg = None
    with pytest.raises(pkg.MslamHipError) as e:
        be.close_loop(K - 1, 0, rvec, tvec, graph)
    assert e.value.code == pkg.E_CAPACITY
    c.close()


def test_tracker_ring_walk_with_both_pcg_settings(pkg):
    """tests/test_gpu_pose_graph.py's ring walk with pose_graph_pcg and ba_global_pcg together: the loop closes by PCG, the
    global solve behind it runs by PCG, and the context's own settings stay off"""
    seq = loop_walk.ring_sequence()
    c, t, rows = tpg._run_ring(pkg, seq, loop_closure=True, loop_min_gap=5, loop_global_ba=True, ba_global_pcg=DEFAULT,
                               pose_graph_pcg=DEFAULT)
    assert t.backend.pose_graph_pcg == DEFAULT and t.backend.global_pcg == DEFAULT
    closed = [a for a in t.loop_results if a["loop"] is not None]
    assert len(closed) == 1 and all(r["tracked"] for r in rows)
    res, ba = closed[0]["result"], closed[0]["global_ba"]
    print("PCG ring walk: closure %s, pose graph term %d it %d cost %.6g -> %.6g CG %s; global BA term %d it %d CG %s" % (
        closed[0]["loop"], res["termination"], res["iterations"], res["initial_cost"], res["final_cost"], res["pcg"], ba["termination"],
        ba["iterations"], ba["pcg"]))
    assert res["termination"] == 0 and res["invalid_steps"] == 0 and res["iterations"] >= 1
    assert res["initial_cost"] > res["final_cost"] >= 0.0
    assert res["pcg"]["solves"] > 0 and res["pcg"]["breakdowns"] == 0
    assert ba["termination"] in (0, 1) and ba["invalid_steps"] == 0 and ba["pcg"]["solves"] > 0 and ba["pcg"]["breakdowns"] == 0
    assert c.get_pose_graph_pcg() == (False,) + DEFAULT and c.get_ba_global_pcg() == (False,) + DEFAULT
    assert c.get_pose_graph_solver() == pkg.PG_SOLVER_DENSE
    c.close()
