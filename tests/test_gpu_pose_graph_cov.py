"""mslam_hip_pose_graph_covariance (k_pg_cov.hip: the blocks of (J^T J)^-1 inside the block envelope, by the Takahashi recursion
over k_pg_sparse.hip's factor) on the MI355X, through Context.pose_graph_covariance.

The rule is test_against_the_qr_reference's, on relative differences: with d = max|Sigma_chol - Sigma_qr| / max|Sigma_qr| of
the two dense CPU references of tests/pose_graph_cov_ref.py, every entry of every returned block lies within
max(1e-9, 1000 d) max|Sigma_qr| of Sigma_qr (1000 for the kernels' other summation orders).  Every test prints d and the
distance it reached ("PGC ..." lines).

  * every case of pose_graph_cov_cases.CASES at the scene's start and at the poses Context.pose_graph returns: all free poses
    that have an edge, and for every edge between two of them the pair in both orientations;
  * loops:16384 against sparse LU solves of unit vectors;
  * constant poses (zeros), poses without an edge, pairs no edge joins, a == b (E_INVALID), the two rank cases (E_NO_MODEL),
    capacity (E_CAPACITY): on every error the output arrays keep the bytes the test put there;
  * Huber and Cauchy at a robust solve's result, and NONE again afterwards;
  * determinism, symmetry and transposes bit for bit, `poses` read only, and a DENSE solve, a SPARSE solve and a global bundle
    adjustment returning the bytes they return without a covariance call on the same context;
  * HipBackend.close_loop(covariance=True) and HipKeyframeTracker(loop_closure=True, loop_covariance=True) on the ring walk."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth  # noqa: E402  (tools/, on the path through conftest.py)

import ba_global_cases as bg  # noqa: E402
import loop_walk  # noqa: E402
import pose_graph_cases as pc  # noqa: E402
import pose_graph_cov_cases as cc  # noqa: E402
import pose_graph_cov_ref as cr  # noqa: E402
import pose_graph_loss_ref as pl  # noqa: E402
import pose_graph_ref as pg  # noqa: E402
import pose_graph_sparse_cases as psc  # noqa: E402
import track_ref as tr  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(width=0, height=0)
    yield c
    c.close()


def _cov(ctx, sc, poses_of, pairs, poses=None):
    return ctx.pose_graph_covariance(sc["poses"] if poses is None else poses, sc["edge_a"], sc["edge_b"], sc["edge_meas"],
                                     sc["sqrt_info"], sc["fixed"], poses_of=poses_of, pairs=pairs)


def _within(tag, got, ref):
    """the rule, on cov and cross of a reference_at() dict"""
    dist = max(float(np.max(np.abs(got["cov"] - ref["cov"]), initial=0.0)), float(np.max(np.abs(got["cross"] - ref["cross"]), initial=0.0)))
    top = float(np.max(np.abs(ref["sigma"])))
    print("PGC %-32s P %4d Q %4d d %.3e reached %.3e (relative) bound %.3e" % (tag, len(ref["cov"]), len(ref["cross"]), ref["d"], dist / top,
                                                                               ref["bound"] / top))
    assert ref["d"] <= cr.MAX_D
    assert got["cov"].shape == ref["cov"].shape and got["cross"].shape == ref["cross"].shape
    assert np.all(np.isfinite(got["cov"])) and np.all(np.isfinite(got["cross"]))
    assert dist <= ref["bound"]


def _bitwise_structure(got, pairs):
    """cov blocks equal their transposes and cross(a, b) equals cross(b, a)^T, bit for bit"""
    assert got["cov"].tobytes() == np.ascontiguousarray(got["cov"].transpose(0, 2, 1)).tobytes()
    where = {}
    for q, (a, b) in enumerate(pairs):
        where.setdefault((int(a), int(b)), q)
    for (a, b), q in where.items():
        assert got["cross"][q].tobytes() == np.ascontiguousarray(got["cross"][where[(b, a)]].T).tobytes(), (a, b)


@pytest.mark.parametrize("name", cc.CASES)
def test_at_the_start_against_the_qr_reference(ctx, name):
    sc, ref = cc.reference(name)
    got = _cov(ctx, sc, ref["poses_of"], ref["pairs"])
    _within(name, got, ref)
    _bitwise_structure(got, ref["pairs"])
    for p in range(len(ref["poses_of"])):      # a covariance: positive diagonal
        assert np.all(np.diag(got["cov"][p]) > 0.0)


@pytest.mark.parametrize("name", cc.CASES)
def test_at_the_solution_against_the_qr_reference(ctx, name):
    sc, _ = cc.reference(name)
    solved = ctx.pose_graph(sc["poses"], sc["edge_a"], sc["edge_b"], sc["edge_meas"], sc["sqrt_info"], sc["fixed"])
    assert solved["termination"] in (0, 1)
    ref = cc.reference_at(sc, solved["poses"])
    got = _cov(ctx, sc, ref["poses_of"], ref["pairs"], poses=solved["poses"])
    _within(name + " solved", got, ref)
    _bitwise_structure(got, ref["pairs"])


def test_sixteen_thousand_poses_against_sparse_lu(ctx):
    sc, cov, cross, d, bound = cc.big_reference()
    got = _cov(ctx, sc, cc.BIG_POSES, cc.BIG_PAIRS)
    dist = max(float(np.max(np.abs(got["cov"] - cov))), float(np.max(np.abs(got["cross"] - cross))))
    print("PGC %-32s d %.3e reached %.3e bound %.3e (absolute)" % (cc.BIG, d, dist, bound))
    assert d <= cr.MAX_D
    assert dist <= bound
    assert not got["cov"][0].any() and not got["cross"][0].any() and not got["cross"][1].any()    # pose 0 is constant
    assert got["cross"][2].tobytes() == np.ascontiguousarray(got["cross"][3].T).tobytes()


# ---- requests and errors: the raw entry, so that the test owns the output arrays ----------------------------------------------
SENTINEL = 0x5A


def _raw(ctx, pkg, sc, poses_of, pairs, poses=None):
    """-> (rc, cov bytes untouched?, cross bytes untouched?, cov, cross) with outputs the test filled with SENTINEL"""
    x = np.ascontiguousarray(sc["poses"] if poses is None else poses, np.float64).reshape(-1, 7)
    ea, eb = np.ascontiguousarray(sc["edge_a"], np.int32), np.ascontiguousarray(sc["edge_b"], np.int32)
    z = np.ascontiguousarray(sc["edge_meas"], np.float64)
    w = None if sc["sqrt_info"] is None else np.ascontiguousarray(sc["sqrt_info"], np.float64)
    fx = np.ascontiguousarray(sc["fixed"], np.uint8)
    idx = np.ascontiguousarray(poses_of, np.int32).reshape(-1)
    pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    pa, pb = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
    cov, cross = np.full((len(idx) + 1) * 288, SENTINEL, np.uint8), np.full((len(pr) + 1) * 288, SENTINEL, np.uint8)
    p = pkg._p
    rc = ctx.L.mslam_hip_pose_graph_covariance(ctx._h, p(x), p(fx), len(x), p(ea), p(eb), p(z), p(w), len(ea), p(idx), len(idx), p(cov),
                                               p(pa), p(pb), len(pr), p(cross))
    return rc, bool(np.all(cov == SENTINEL)), bool(np.all(cross == SENTINEL)), cov, cross


def _refused(ctx, pkg, sc, poses_of, pairs, code):
    rc, cov_kept, cross_kept, _, _ = _raw(ctx, pkg, sc, poses_of, pairs)
    assert rc == code, (rc, ctx.L.mslam_hip_last_error(ctx._h))
    assert cov_kept and cross_kept


def test_constant_poses_give_zeros(ctx, pkg):
    sc, ref = cc.reference("isolated_fixed_middle")       # poses 0 and 3 are constant; (2, 3) and (3, 5) are edges
    rc, _, _, cov, cross = _raw(ctx, pkg, sc, [3, 2, 0], [(2, 3), (3, 5), (3, 2), (1, 2)])
    assert rc == pkg.OK
    cov, cross = cov[:3 * 288].view(np.float64).reshape(3, 6, 6), cross[:4 * 288].view(np.float64).reshape(4, 6, 6)
    assert not cov[0].any() and not cov[2].any() and cov[1].any()
    assert not cross[0].any() and not cross[1].any() and not cross[2].any() and cross[3].any()
    assert np.max(np.abs(cov[1] - cr.block(ref["sigma"], ref["prob"], 2, 2))) <= ref["bound"]
    # beyond the blocks asked for nothing is written
    rc, _, _, cov, cross = _raw(ctx, pkg, sc, [2], [(1, 2)])
    assert rc == pkg.OK and np.all(cov[288:] == SENTINEL) and np.all(cross[288:] == SENTINEL)


def test_requests_that_are_refused(ctx, pkg):
    sc, _ = cc.reference("isolated_fixed_middle")
    _refused(ctx, pkg, sc, [1, 4], [], pkg.E_INVALID)              # pose 4 is free and has no edge
    _refused(ctx, pkg, sc, [1], [(1, 2), (4, 5)], pkg.E_INVALID)
    _refused(ctx, pkg, sc, [1], [(1, 2), (1, 5)], pkg.E_INVALID)   # no edge joins 1 and 5
    _refused(ctx, pkg, sc, [1], [(1, 2), (2, 2)], pkg.E_INVALID)   # a == b
    _refused(ctx, pkg, sc, [1], [(3, 3)], pkg.E_INVALID)           # also for a constant pose
    _refused(ctx, pkg, sc, [8], [], pkg.E_INVALID)                 # out of range
    _refused(ctx, pkg, sc, [1], [(1, -1)], pkg.E_INVALID)
    with pytest.raises(pkg.MslamHipError) as e:
        _cov(ctx, sc, [4], [])
    assert e.value.code == pkg.E_INVALID and "no edge" in str(e.value)


@pytest.mark.parametrize("name", cc.RANK)
def test_rank_deficient_problems_give_no_model(ctx, pkg, name):
    sc = cc.scene(name)
    poses_of, pairs = cr.requests(sc)
    _refused(ctx, pkg, sc, poses_of, pairs, pkg.E_NO_MODEL)
    with pytest.raises(pkg.MslamHipError) as e:
        _cov(ctx, sc, poses_of[:1], [])
    assert e.value.code == pkg.E_NO_MODEL
    if name == "two_components":
        assert "pose 4" in str(e.value)          # the least pose of the component 4-5-6
    if name == "pair_component":
        assert "pose 5" in str(e.value)
    if name == "zero_info":
        assert "pivot" in str(e.value)


def test_an_envelope_above_the_bound_is_capacity(ctx, pkg):
    K, edges, _, _, chosen = psc.table()["random2048"]
    assert chosen is None
    sc = psc.identity_scene(K, edges)
    _refused(ctx, pkg, sc, [1, 2], [], pkg.E_CAPACITY)


# ---- loss -------------------------------------------------------------------------------------------------------------------
def test_under_a_loss_the_corrected_jacobians_are_used(ctx):
    name = "false:12,4,1,1"
    sc = pl.scene(name)
    poses_of, pairs = cr.requests(sc)
    first = _cov(ctx, sc, poses_of, pairs)
    try:
        for kind in pl.LOSSES:
            ctx.set_pose_graph_loss(kind, pl.SCALE)
            solved = ctx.pose_graph(sc["poses"], sc["edge_a"], sc["edge_b"], sc["edge_meas"], sc["sqrt_info"], sc["fixed"])
            ref = cc.reference_at(sc, solved["poses"], loss=(kind, pl.SCALE))
            got = _cov(ctx, sc, poses_of, pairs, poses=solved["poses"])
            _within("%s %s" % (name, kind), got, ref)
            plain = cc.reference_at(sc, solved["poses"])       # the loss matters: without it the blocks are elsewhere
            assert np.max(np.abs(plain["cov"] - ref["cov"])) > 100.0 * ref["bound"]
    finally:
        ctx.set_pose_graph_loss("none")
    again = _cov(ctx, sc, poses_of, pairs)
    assert again["cov"].tobytes() == first["cov"].tobytes() and again["cross"].tobytes() == first["cross"].tobytes()


# ---- determinism and the shared buffers -----------------------------------------------------------------------------------------
def test_two_calls_return_the_same_bytes_and_poses_are_read_only(ctx):
    for name in ("revisit200", "complete:45"):
        sc, ref = cc.reference(name)
        x = np.array(sc["poses"], np.float64)
        before = x.tobytes()
        a = _cov(ctx, sc, ref["poses_of"], ref["pairs"], poses=x)
        b = _cov(ctx, sc, ref["poses_of"], ref["pairs"], poses=x)
        assert a["cov"].tobytes() == b["cov"].tobytes() and a["cross"].tobytes() == b["cross"].tobytes()
        assert x.tobytes() == before


def test_no_requests_is_a_valid_call(ctx):
    sc, _ = cc.reference("chain:9")
    got = _cov(ctx, sc, [], [])
    assert got["cov"].shape == (0, 6, 6) and got["cross"].shape == (0, 6, 6)
    sc = pc.scene("all_fixed")
    got = _cov(ctx, sc, [0, 1], [(0, 1)])
    assert not got["cov"].any() and not got["cross"].any()


def test_later_solves_keep_their_bits(ctx, pkg):
    """a DENSE solve, a SPARSE solve and a global bundle adjustment return the same bytes before and after a covariance call"""
    sc, ref = cc.reference("loops:65")
    ba = bg.scene("traj:17")

    def solves():
        out = []
        try:
            for kind in ("dense", "sparse"):
                ctx.set_pose_graph_solver(kind)
                r = ctx.pose_graph(sc["poses"], sc["edge_a"], sc["edge_b"], sc["edge_meas"], sc["sqrt_info"], sc["fixed"])
                out.append(r["poses"].tobytes() + np.float64(r["final_cost"]).tobytes())
        finally:
            ctx.set_pose_graph_solver("dense")
        r = ctx.bundle_adjust_global(ba["poses"], ba["landmarks"], ba["obs_kf"], ba["obs_lm"], ba["obs_cam"], ba["fixed"])
        out.append(r["poses"].tobytes() + r["landmarks"].tobytes() + np.float64(r["final_cost"]).tobytes())
        return out
    before = solves()
    _cov(ctx, sc, ref["poses_of"], ref["pairs"])
    big, bref = cc.reference("complete:45")
    _cov(ctx, big, bref["poses_of"], bref["pairs"])
    assert solves() == before


# ---- HipBackend.close_loop and the tracker --------------------------------------------------------------------------------------
def _rvec(R):
    q = pg.matrix_to_quaternion(R)
    n = np.linalg.norm(q[:3])
    return 2.0 * np.arctan2(n, q[3]) * q[:3] / n


def _drift_backend(pkg, ctx):
    """tests/test_gpu_pose_graph.py's backend scene: the 40-keyframe drift scene, ids with gaps, the chain as the graph"""
    sc = pc.scene("drift40")
    K = len(sc["poses"])
    ids = [3 * k + 1 for k in range(K)]
    rng = np.random.default_rng(8)
    be = pkg.HipBackend(ctx)
    for k in range(K):
        be.add_keyframe(ids[k], sc["poses"][k], [1000 + 3 * k + i for i in range(3)], rng.uniform([-1, -1, 1.5], [1, 1, 3.0], (3, 3)))
    graph = {ids[k]: set(ids[j] for j in (k - 1, k + 1) if 0 <= j < K) for k in range(K)}
    T = sc["truth_poses"][-1]
    R = pg.q_matrix(T[:4]).T
    return be, graph, ids, _rvec(R), -R @ T[4:]


def _loop_blocks_within(tag, cv, problem, poses, cur, loop):
    """the covariance dict of a closure against the dense references on `problem` (loop_problem's arrays) at `poses`"""
    ids, _, fixed, ea, eb, meas, info = problem
    sc = dict(poses=poses, fixed=fixed, edge_a=ea, edge_b=eb, edge_meas=meas, sqrt_info=info)
    ref = cc.reference_at(sc, poses)
    kc, kl = ids.index(cur), ids.index(loop)
    want = dict(cov=np.array([cr.block(ref["sigma"], ref["prob"], kc, kc), cr.block(ref["sigma"], ref["prob"], kl, kl)]),
                cross=cr.block(ref["sigma"], ref["prob"], kc, kl)[None], sigma=ref["sigma"], d=ref["d"], bound=ref["bound"])
    _within(tag, dict(cov=np.array([cv["cur"], cv["loop"]]), cross=cv["cross"][None]), want)


def test_backend_close_loop_with_covariance(pkg, ctx):
    be, graph, ids, rvec, tvec = _drift_backend(pkg, ctx)
    problem = pg.loop_problem(dict(be.poses), be.first, graph, ids[-1], ids[0], rvec, tvec)
    got = be.close_loop(ids[-1], ids[0], rvec, tvec, graph, covariance=True)
    assert got["termination"] == 0
    cv = got["covariance"]
    assert sorted(cv) == ["cross", "cur", "loop"]
    _loop_blocks_within("close_loop drift40", cv, problem, got["poses"], ids[-1], ids[0])
    assert not cv["loop"].any() and not cv["cross"].any() and cv["cur"].any()      # the loop keyframe is the constant first one
    # a loop between two free keyframes: the cross block is there, rows from the current keyframe
    be2, graph, ids, rvec, tvec = _drift_backend(pkg, ctx)
    T = pg.compose(be2.poses[ids[5]], pg.relative(pc.scene("drift40")["truth_poses"][5], pc.scene("drift40")["truth_poses"][-1]))
    R = pg.q_matrix(T[:4]).T
    rvec, tvec = _rvec(R), -R @ T[4:]
    problem = pg.loop_problem(dict(be2.poses), be2.first, graph, ids[-1], ids[5], rvec, tvec)
    got2 = be2.close_loop(ids[-1], ids[5], rvec, tvec, graph, covariance=True)
    assert got2["termination"] == 0 and got2["covariance"]["cross"].any()
    _loop_blocks_within("close_loop drift40 free", got2["covariance"], problem, got2["poses"], ids[-1], ids[5])
    # the flag off: what a call without the argument returns
    off, plain = _drift_backend(pkg, ctx), _drift_backend(pkg, ctx)
    a = off[0].close_loop(ids[-1], ids[0], off[3], off[4], off[1], covariance=False)
    b = plain[0].close_loop(ids[-1], ids[0], plain[3], plain[4], plain[1])
    assert sorted(a) == sorted(b) and "covariance" not in a
    assert a["poses"].tobytes() == b["poses"].tobytes() == got["poses"].tobytes() and a["landmarks"].tobytes() == b["landmarks"].tobytes()


def test_tracker_puts_the_covariance_into_the_attempt_record(pkg):
    seq = loop_walk.ring_sequence()
    records = {}
    for flag in (True, False):
        c = pkg.Context(width=0, height=0, max_keypoints=4096)
        c.bow_load(synth.make_vocabulary(10, 3))
        t = pkg.HipKeyframeTracker(c, focal=tr.CAM[:2], principal=tr.CAM[2:], local_map_depth=2, local_ba=True,
                                   new_keyframe_min_landmarks=200, loop_closure=True, loop_min_gap=5, loop_covariance=flag)
        seen = []
        inner = c.pose_graph_covariance
        c.pose_graph_covariance = lambda *a, **k: (seen.append((a, k)), inner(*a, **k))[1]      # what the closure asked for
        rows = [t.processSensorData(fr["desc"], fr["xy"], fr["depth"]) for fr in seq["frames"]]
        closed = [a for a in t.loop_results if a["loop"] is not None]
        assert len(closed) == 1 and all(r["tracked"] for r in rows)
        records[flag] = (closed[0], seen, [r["tvec"].tobytes() + r["R"].tobytes() for r in rows])
        c.close()
    (on, asked, rows_on), (off, none, rows_off) = records[True], records[False]
    assert len(asked) == 1 and not none
    assert "covariance" not in off and "covariance" not in off["result"]
    assert sorted(k for k in on if k != "covariance") == sorted(off)
    assert on["result"]["poses"].tobytes() == off["result"]["poses"].tobytes() and rows_on == rows_off
    (poses, ea, eb, meas, info, fixed), kw = asked[0]
    assert poses.tobytes() == on["result"]["poses"].tobytes()
    ids = on["result"]["keyframes"]
    cv = on["covariance"]
    assert cv is on["result"]["covariance"] and list(kw["poses_of"]) == [ids.index(on["keyframe"]), ids.index(on["loop"])]
    _loop_blocks_within("ring walk", cv, (ids, None, fixed, ea, eb, meas, info), poses, on["keyframe"], on["loop"])
    assert cv["cur"].any() and np.all(np.diag(cv["cur"]) > 0.0)
    with pytest.raises(pkg.MslamHipError) as e:
        pkg.HipKeyframeTracker(None, focal=tr.CAM[:2], principal=tr.CAM[2:], loop_covariance=True)
    assert e.value.code == pkg.E_INVALID
