"""mslam_hip_pose_graph with the SPARSE linear solver (k_pg_sparse.hip: a Cholesky factor on the block envelope after a NATURAL
or reverse Cuthill-McKee order) on the MI355X, through Context.set_pose_graph_solver("sparse") and Context.pose_graph.

  * every case of pose_graph_cases.ALL and .EDGES under the assertions and bounds of
    tests/test_gpu_pose_graph.py::test_against_the_qr_reference, unchanged: state within max(1e-9, 1000 |x_chol - x_qr|_inf) of
    the QR solve (the distance of two correct CPU solvers, times 1000 for the kernels' other summation orders), costs 1e-6
    relative plus the second-order term E (J B)^2 / 2 the state bound allows at a minimum, |iterations - qr| <= 1; constant
    poses and poses without an edge bit for bit;
  * the envelope's edges and the sizes beyond the dense cap (tests/pose_graph_sparse_cases.py) under the same rule with the
    two sparse CPU solvers of tests/pose_graph_sparse_ref.py in the places of QR and Cholesky.  The 16384-pose chain has exact
    measurements (with the default noise it sits at the iteration cap after 100 iterations) and its two CPU solves are
    recorded under tests/golden/; the noisy chain of that size runs under a cap of two iterations against the two solvers
    solved in the test;
  * capacity, the size checks, determinism, DENSE -> SPARSE -> DENSE on one context, global bundle adjustment after a SPARSE
    solve (the factor lives in the buffer it factors in), the setter; HipBackend(pose_graph_solver="sparse").close_loop and
    HipKeyframeTracker(loop_closure=True, pose_graph_solver="sparse") on the ring walk."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth  # noqa: E402  (tools/, on the path through conftest.py)

import ba_global_cases as bg  # noqa: E402
import loop_walk  # noqa: E402
import pose_graph_cases as pc  # noqa: E402
import pose_graph_ref as pg  # noqa: E402
import pose_graph_sparse_cases as psc  # noqa: E402
import reloc_ref as rr  # noqa: E402
import track_ref as tr  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(width=0, height=0)
    c.set_pose_graph_solver("sparse")
    yield c
    c.close()


def _solve(ctx, sc, **over):
    a = dict(sc)
    a.update(over)
    return ctx.pose_graph(a["poses"], a["edge_a"], a["edge_b"], a["edge_meas"], a["sqrt_info"], a["fixed"],
                          max_iterations=a.get("max_iterations", 100))


def _outside(sc):
    """the poses outside the problem: constant, or without an edge"""
    seen = np.zeros(len(sc["poses"]), bool)
    seen[sc["edge_a"]], seen[sc["edge_b"]] = True, True
    return np.flatnonzero(~seen | (sc["fixed"] != 0))


def _against(name, sc, got, ref, dist):
    """test_against_the_qr_reference's assertions with `ref` in the place of the QR solve -> the state bound"""
    bound = max(1e-9, 1000.0 * dist)
    dx = pc.same_rotation_distance(got["poses"], ref["poses"])
    second_order = len(sc["edge_a"]) * (pc.jacobian_row_bound(sc) * bound) ** 2 / 2.0
    print("PGS %-22s term %d/%d it %d/%d rejected %d/%d cost0 %.17g/%.17g cost %.6g/%.6g dx %.3e bound %.3e" % (
        name, got["termination"], ref["termination"], got["iterations"], ref["iterations"], got["rejected_steps"],
        ref["trace"]["rejected"], got["initial_cost"], ref["initial_cost"], got["final_cost"], ref["final_cost"], dx, bound))
    assert got["termination"] == ref["termination"]
    assert abs(got["iterations"] - ref["iterations"]) <= 1
    assert got["invalid_steps"] == 0 and got["n_outliers"] == 0
    assert abs(got["initial_cost"] - ref["initial_cost"]) <= 1e-6 * ref["initial_cost"]
    assert abs(got["final_cost"] - ref["final_cost"]) <= 1e-6 * ref["final_cost"] + second_order
    assert dx <= bound
    start = np.asarray(sc["poses"], np.float64)
    for k in _outside(sc):                                    # constant poses and poses without an edge come back bit for bit
        assert got["poses"][k].tobytes() == start[k].tobytes(), k
    return bound


@pytest.mark.parametrize("name", pc.ALL + pc.EDGES)
def test_existing_cases_against_the_qr_reference(ctx, name):
    sc, qr, ch, dist = pc.reference(name)
    got = _solve(ctx, sc)
    bound = _against(name, sc, got, qr, dist)
    start = np.asarray(sc["poses"], np.float64)
    kind, _, rest = name.partition(":")
    if name == "isolated_fixed_middle":
        assert got["poses"][4].tobytes() == start[4].tobytes() and not np.array_equal(got["poses"][5], start[5])
    if name in ("all_fixed", "empty", "zero_start"):
        assert got["poses"].tobytes() == start.tobytes() and got["iterations"] == 0 and got["termination"] == 0
    if name in ("empty", "zero_start"):
        assert got["final_cost"] == 0.0 and got["initial_cost"] == 0.0
    if name.startswith("cap"):                                # the cap is exact
        assert got["termination"] == 1 and got["iterations"] == qr["iterations"] == sc["max_iterations"]
    if name == "cap0":                                        # nothing may move
        assert got["final_cost"] == got["initial_cost"] and got["poses"].tobytes() == start.tobytes()
    if name == "cap1":                                        # NO_CONVERGENCE, and the state reached is written
        assert np.max(np.abs(got["poses"] - start)) > 1e-3
    if name == "rejected":
        assert got["rejected_steps"] == qr["trace"]["rejected"] >= 1
    if name == "neg_q":                                       # no sign fix: the signs entered are the signs returned
        assert np.all(np.sum(got["poses"][:, :4] * start[:, :4], 1) > 0.0)
        assert np.max(np.abs(got["poses"] - qr["poses"])) <= bound
    if name == "pair":                                        # T_0 o Z
        want = pg.compose(start[0], sc["edge_meas"][0])
        assert got["final_cost"] < 1e-20 and pc.same_rotation_distance(got["poses"][1], want) <= 1e-9
    if kind == "sparse1024":
        for k in (1, 64, 256, 1023):
            assert not np.array_equal(got["poses"][k], start[k]), k
    if kind == "rejected" and rest:
        cap = int(rest[3:])
        assert got["termination"] == 1 and got["iterations"] == qr["iterations"] == cap
        assert got["rejected_steps"] == qr["trace"]["rejected"] == min(cap, 4)


@pytest.mark.parametrize("name", psc.ENVELOPE)
def test_envelope_edges_against_the_sparse_reference(ctx, pkg, name):
    sc, ref, aug, dist = psc.reference(name)
    got = _solve(ctx, sc)
    _against(name, sc, got, ref, dist)
    assert got["termination"] == 0 and aug["termination"] == 0 and aug["iterations"] == ref["iterations"]
    an = pkg.pose_graph_analyze(sc["fixed"], len(sc["poses"]), sc["edge_a"], sc["edge_b"])
    if name == "revisit200":                                  # the order that writes blocks transposed
        assert an["ordering"] == pkg.PG_ORDER_RCM and an["envelope_blocks"] == 984
    if name == "complete40":                                  # the whole triangle
        assert an["envelope_blocks"] == 39 * 40 // 2
    if name == "chain2":
        assert an["envelope_blocks"] == 1
    if name.startswith("loops:"):                             # the long row of the second loop edge
        K = int(name[6:])
        assert an["ordering"] == pkg.PG_ORDER_NATURAL and an["first"][K - 5] == 0 and an["envelope_blocks"] == 3 * K - 9


def test_beyond_the_dense_cap(ctx, pkg):
    """1025 keyframes: DENSE rejects the call as before, SPARSE agrees with the sparse reference"""
    sc, ref, aug, dist = psc.reference("loops:1025")
    ctx.set_pose_graph_solver("dense")
    try:
        with pytest.raises(pkg.MslamHipError) as e:
            _solve(ctx, sc)
        assert e.value.code == pkg.E_INVALID
    finally:
        ctx.set_pose_graph_solver("sparse")
    got = _solve(ctx, sc)
    _against("loops:1025", sc, got, ref, dist)
    assert got["termination"] == ref["termination"] == aug["termination"] == 0


def test_the_sparse_cap(ctx, pkg):
    """16384 keyframes, the new cap, against the recorded sparse reference and the ground truth; 16385 is rejected"""
    sc, ref, aug, dist = psc.reference("loops:16384")
    got = _solve(ctx, sc)
    _against("loops:16384", sc, got, ref, dist)
    assert got["termination"] == ref["termination"] == aug["termination"] == 0
    assert abs(got["iterations"] - aug["iterations"]) <= 1
    assert pc.same_rotation_distance(got["poses"], sc["truth_poses"]) <= 1e-6      # exact measurements: the minimum is the truth
    # the same graph with the default measurement noise, which no solver brings to convergence in 100 iterations: the first
    # two iterations under a cap, NO_CONVERGENCE with the state reached, against the two sparse solvers solved here
    noisy, nref, naug, ndist = psc.reference("noisy16384:cap2")
    ngot = _solve(ctx, noisy)
    _against("noisy16384:cap2", noisy, ngot, nref, ndist)
    assert ngot["termination"] == nref["termination"] == naug["termination"] == 1 and ngot["iterations"] == nref["iterations"] == 2
    assert ngot["final_cost"] < ngot["initial_cost"] and np.max(np.abs(ngot["poses"] - noisy["poses"])) > 1e-3
    over = psc.identity_scene(pkg.POSE_GRAPH_MAX_KEYFRAMES_SPARSE + 1, pc.chain(pkg.POSE_GRAPH_MAX_KEYFRAMES_SPARSE + 1))
    with pytest.raises(pkg.MslamHipError) as e:
        _solve(ctx, over)
    assert e.value.code == pkg.E_INVALID


def _same_bits(a, b):
    assert a["poses"].tobytes() == b["poses"].tobytes()
    for k in ("termination", "iterations", "rejected_steps", "invalid_steps", "n_outliers"):
        assert a[k] == b[k], k
    for k in ("initial_cost", "final_cost"):
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), k


def test_capacity_then_a_small_solve(ctx, pkg):
    """neither order of 20000 random pairs among 2048 poses fits the envelope: E_CAPACITY, the message names the blocks needed,
    the poses stay; the context then solves a small problem as a fresh one does"""
    K, edges, natural, rcm, chosen = psc.table()["random2048"]
    sc = psc.identity_scene(K, edges)
    x = np.ascontiguousarray(sc["poses"], np.float64)
    before = x.copy()
    ea, eb = np.ascontiguousarray(sc["edge_a"], np.int32), np.ascontiguousarray(sc["edge_b"], np.int32)
    z, fx = np.ascontiguousarray(sc["edge_meas"], np.float64), np.ascontiguousarray(sc["fixed"], np.uint8)
    rc = ctx.L.mslam_hip_pose_graph(ctx._h, pkg._p(x), pkg._p(fx), K, pkg._p(ea), pkg._p(eb), pkg._p(z), None, len(ea), 100, None)
    assert rc == pkg.E_CAPACITY and x.tobytes() == before.tobytes()
    with pytest.raises(pkg.MslamHipError) as e:
        _solve(ctx, sc)
    assert e.value.code == pkg.E_CAPACITY and str(min(natural, rcm)) in str(e.value)
    small, ref, aug, dist = psc.reference("loops:66")
    got = _solve(ctx, small)
    _against("loops:66 after E_CAPACITY", small, got, ref, dist)
    c = pkg.Context(width=0, height=0)
    c.set_pose_graph_solver("sparse")
    _same_bits(got, _solve(c, small))
    c.close()


@pytest.mark.parametrize("name", ["loops:258", "revisit200", "complete40", "star70", "rejected", "info65"])
def test_a_second_call_returns_the_same_bits(ctx, name):
    sc = psc.scene(name) if name in psc.ENVELOPE else pc.scene(name)
    _same_bits(_solve(ctx, sc), _solve(ctx, sc))


def test_dense_sparse_dense_on_one_context(ctx, pkg):
    sc, ref, aug, dist = psc.reference("loops:257")
    try:
        ctx.set_pose_graph_solver("dense")
        assert ctx.get_pose_graph_solver() == pkg.PG_SOLVER_DENSE
        d0 = _solve(ctx, sc)
        ctx.set_pose_graph_solver("sparse")
        assert ctx.get_pose_graph_solver() == pkg.PG_SOLVER_SPARSE
        s0 = _solve(ctx, sc)
        ctx.set_pose_graph_solver(pkg.PG_SOLVER_DENSE)
        d1 = _solve(ctx, sc)
    finally:
        ctx.set_pose_graph_solver("sparse")
    _same_bits(d0, d1)
    bound = max(1e-9, 1000.0 * dist)
    assert s0["termination"] == d0["termination"] and abs(s0["iterations"] - d0["iterations"]) <= 1
    assert pc.same_rotation_distance(s0["poses"], d0["poses"]) <= bound
    assert pc.same_rotation_distance(d0["poses"], ref["poses"]) <= bound
    fresh = pkg.Context(width=0, height=0)                    # a fresh context is DENSE and returns the bits of d0
    assert fresh.get_pose_graph_solver() == pkg.PG_SOLVER_DENSE
    _same_bits(_solve(fresh, sc), d0)
    fresh.close()


def test_global_bundle_adjustment_after_a_sparse_solve(ctx):
    """the envelope lives in the buffer global bundle adjustment factors in: what a SPARSE solve left there must not reach it"""
    _solve(ctx, psc.scene("revisit200"))
    sc, qr, sch, dist, mask, margin = bg.reference("traj:17")
    got = ctx.bundle_adjust_global(sc["poses"], sc["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"], sc["fixed"])
    bound = max(1e-9, 1000.0 * dist)
    dx = max(float(np.max(np.abs(got["poses"] - qr["poses"]))), float(np.max(np.abs(got["landmarks"] - qr["landmarks"]))))
    assert got["termination"] == qr["termination"] and abs(got["iterations"] - qr["iterations"]) <= 1 and got["invalid_steps"] == 0
    assert abs(got["final_cost"] - qr["final_cost"]) <= 1e-6 * qr["final_cost"] + len(sc["obs_kf"]) * (12.0 * bound) ** 2 / 2.0
    assert dx <= bound and np.array_equal(got["outlier"], mask)
    small, ref, aug, d2 = psc.reference("loops:65")
    _against("loops:65 after global BA", small, _solve(ctx, small), ref, d2)


def test_the_setter_rejects_an_unknown_kind(ctx, pkg):
    for bad in (2, -1, "skyline"):
        with pytest.raises(pkg.MslamHipError) as e:
            ctx.set_pose_graph_solver(bad)
        assert e.value.code == pkg.E_INVALID
        assert ctx.get_pose_graph_solver() == pkg.PG_SOLVER_SPARSE
    assert ctx.L.mslam_hip_set_pose_graph_solver(ctx._h, 2) == pkg.E_INVALID
    assert ctx.get_pose_graph_solver() == pkg.PG_SOLVER_SPARSE
    with pytest.raises(pkg.MslamHipError) as e:
        pkg.HipBackend(ctx, pose_graph_solver="skyline")
    assert e.value.code == pkg.E_INVALID


# ---- HipBackend.close_loop --------------------------------------------------------------------------------------------------------

def _rvec(R):
    q = pg.matrix_to_quaternion(R)
    n = np.linalg.norm(q[:3])
    return 2.0 * np.arctan2(n, q[3]) * q[:3] / n


def test_backend_close_loop_sparse_against_the_numpy_close_loop(pkg):
    """the scene of tests/test_gpu_pose_graph.py's backend test (the 40-keyframe drift scene, ids with gaps, the chain as the
    covisibility graph) with pose_graph_solver = "sparse" on a context whose own setting is DENSE and stays DENSE; the caps"""
    ctx = pkg.Context(width=0, height=0)
    sc = pc.scene("drift40")
    K = len(sc["poses"])
    ids = [3 * k + 1 for k in range(K)]
    rng = np.random.default_rng(8)
    be = pkg.HipBackend(ctx, pose_graph_solver="sparse")
    for k in range(K):
        own = rng.uniform([-1, -1, 1.5], [1, 1, 3.0], (3, 3))
        lids, cam = [1000 + 3 * k + i for i in range(3)], own
        if k:
            lids, cam = lids + [1000 + 3 * (k - 1)], np.concatenate([own, rng.uniform([-1, -1, 1.5], [1, 1, 3.0], (1, 3))])
        be.add_keyframe(ids[k], sc["poses"][k], lids, cam)
    graph = {ids[k]: set(ids[j] for j in (k - 1, k + 1) if 0 <= j < K) for k in range(K)}
    T = sc["truth_poses"][-1]
    R = pg.q_matrix(T[:4]).T
    rvec, tvec = _rvec(R), -R @ T[4:]
    state = (dict(be.poses), be.first, graph, dict(be.anchor), dict(be.landmarks), ids[-1], ids[0], rvec, tvec)
    qr, ch = pg.close_loop(*state, linear_solver="qr"), pg.close_loop(*state, linear_solver="chol")
    bound = max(1e-9, 1000.0 * max(pc.same_rotation_distance(qr["poses"], ch["poses"]),
                                   float(np.max(np.abs(qr["landmarks"] - ch["landmarks"])))))
    got = be.close_loop(ids[-1], ids[0], rvec, tvec, graph)
    assert ctx.get_pose_graph_solver() == pkg.PG_SOLVER_DENSE
    dx, dl = pc.same_rotation_distance(got["poses"], qr["poses"]), float(np.max(np.abs(got["landmarks"] - qr["landmarks"])))
    print("PGS close_loop term %d/%d it %d/%d cost %.6g -> %.6g / %.6g dx %.3e dl %.3e bound %.3e" % (
        got["termination"], qr["termination"], got["iterations"], qr["iterations"], got["initial_cost"], got["final_cost"],
        qr["final_cost"], dx, dl, bound))
    assert got["termination"] == qr["termination"] == 0 and abs(got["iterations"] - qr["iterations"]) <= 1 and got["invalid_steps"] == 0
    assert got["keyframes"] == ids and got["poses_before"].tobytes() == qr["poses_before"].tobytes()
    assert got["landmark_ids"].tolist() == qr["landmark_ids"].tolist() and len(got["landmark_ids"]) == 3 * K
    assert dx <= bound and dl <= bound
    assert abs(got["initial_cost"] - qr["initial_cost"]) <= 1e-6 * qr["initial_cost"]
    assert abs(got["final_cost"] - qr["final_cost"]) <= 1e-6 * qr["final_cost"] + 40 * (18.0 * bound) ** 2 / 2.0
    for k, id in enumerate(ids):
        assert be.poses[id].tobytes() == got["poses"][k].tobytes()
    # the caps, raised before the context is touched: 1024 when dense, 16384 when sparse
    unit = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
    for solver, cap in (("dense", pkg.POSE_GRAPH_MAX_KEYFRAMES), ("sparse", pkg.POSE_GRAPH_MAX_KEYFRAMES_SPARSE)):
        big = pkg.HipBackend(None, pose_graph_solver=solver)
        big.poses = {k: unit for k in range(cap + 1)}
        with pytest.raises(pkg.MslamHipError) as e:
            big.close_loop(cap, 0, np.zeros(3), np.zeros(3), {})
        assert e.value.code == pkg.E_CAPACITY and str(cap) in str(e.value)
    ctx.close()


# ---- the tracker ------------------------------------------------------------------------------------------------------------------

def test_tracker_closes_the_ring_walk_with_the_sparse_solver(pkg):
    """tests/test_gpu_pose_graph.py's ring walk with pose_graph_solver = "sparse": the loop closes with CONVERGENCE and every
    keyframe and frame stays within that test's 0.1 degree / 0.02 m of the ground truth"""
    seq = loop_walk.ring_sequence()
    c = pkg.Context(width=0, height=0, max_keypoints=4096)
    c.bow_load(synth.make_vocabulary(10, 3))
    t = pkg.HipKeyframeTracker(c, focal=tr.CAM[:2], principal=tr.CAM[2:], local_map_depth=2, local_ba=True,
                               new_keyframe_min_landmarks=200, loop_closure=True, loop_min_gap=5, pose_graph_solver="sparse")
    assert t.backend.pose_graph_solver == pkg.PG_SOLVER_SPARSE
    rows = [t.processSensorData(fr["desc"], fr["xy"], fr["depth"]) for fr in seq["frames"]]
    kf_frames = {r["keyframe"]: f for f, r in enumerate(rows) if r["keyframe"] >= 0}
    fired = [(f, r["loop"]) for f, r in enumerate(rows) if r["loop"] is not None]
    assert len(fired) == 1 and fired[0][1][1] == 0 and all(r["tracked"] for r in rows)
    closed = [a for a in t.loop_results if a["loop"] is not None]
    assert len(closed) == 1
    res = closed[0]["result"]
    print("PGS ring walk: loop %s, cost %.6g -> %.6g in %d iterations" % (fired, res["initial_cost"], res["final_cost"], res["iterations"]))
    assert res["termination"] == 0 and res["invalid_steps"] == 0 and res["iterations"] >= 1
    assert res["initial_cost"] > res["final_cost"] >= 0.0
    assert res["poses"][0].tobytes() == res["poses_before"][0].tobytes()
    assert not np.array_equal(res["poses"][-1], res["poses_before"][-1])
    assert c.get_pose_graph_solver() == pkg.PG_SOLVER_DENSE
    for k in t.ids:                                           # every keyframe against the ground truth of its frame
        q, p = t.backend.poses[k][:4], t.backend.poses[k][4:]
        R = pg.q_matrix(q).T
        fr = seq["frames"][kf_frames[k]]
        err_deg, err_m = rr.rot_err(R, fr["R"]), float(np.linalg.norm(-R @ p - fr["t"]))
        assert err_deg < 0.1 and err_m < 0.02, (k, err_deg, err_m)
    for f, r in enumerate(rows):
        assert rr.rot_err(r["R"], seq["frames"][f]["R"]) < 0.1 and np.linalg.norm(r["tvec"] - seq["frames"][f]["t"]) < 0.02, f
    c.close()
