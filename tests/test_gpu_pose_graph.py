"""Pose-graph optimisation on the MI355X (k_posegraph.hip) through Context.pose_graph, against tests/pose_graph_ref.py's QR
solve on the cases of tests/pose_graph_cases.py (tests/test_pose_graph.py shows on the CPU that every case takes the path it
is named for); blocks outside the problem, determinism, also of a small solve after a large one on one context, the shared
normal-equation buffer with global bundle adjustment, FAILURE, the argument checks; a 300-keyframe chain against ground
truth; HipBackend.close_loop against the numpy close_loop; HipKeyframeTracker(loop_closure) on a walk that returns to its
start (tests/loop_walk.py) and on one that never leaves its own local map (tests/track_ref.py).

Bounds, taken from tests/test_gpu_ba.py.  State: |x_gpu - x_qr|_inf <= max(1e-9, 1000 |x_chol - x_qr|_inf), quaternions
compared up to sign: the distance of two correct CPU solvers, times 1000 for the kernels' other summation orders.  Costs:
1e-6 relative, plus what the state bound itself allows at a minimum: there the cost is stationary, so two states B apart
differ in cost by the second-order term only, at most E (J B)^2 / 2 with J the largest row norm of an edge's Jacobian.  The
rows of [2 R^T [v]x, -R^T | 0, R^T] have norm at most 2 |v| + 2 and those of [2 M | -2 M] norm 2 sqrt(2) (M is a rotation for
unit quaternions); the scenes keep every position in [-2, 2]^3 and start within 1 m of the truth, so |v| = |p_b - p_a| < 8 m
and J <= 18 without sqrt_info; sqrt_info multiplies a row by at most its largest absolute row sum (below 3.5 in info_upper).
pose_graph_cases.jacobian_row_bound computes J per scene by this rule.  The kernels divide by |q|^2 where the reference's jets
multiply by its reciprocal, so a start cost of exactly 0 would have no relative precision; no case here has one."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth  # noqa: E402  (tools/, on the path through conftest.py)

import ba_global_cases as bg  # noqa: E402
import local_map_ref as lm  # noqa: E402
import loop_walk  # noqa: E402
import pose_graph_cases as pc  # noqa: E402
import pose_graph_ref as pg  # noqa: E402
import reloc_ref as rr  # noqa: E402
import track_ref as tr  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(width=0, height=0)
    yield c
    c.close()


def _solve(ctx, sc, **over):
    a = dict(sc)
    a.update(over)
    return ctx.pose_graph(a["poses"], a["edge_a"], a["edge_b"], a["edge_meas"], a["sqrt_info"], a["fixed"],
                          max_iterations=a.get("max_iterations", 100))


@pytest.mark.parametrize("name", pc.ALL)
def test_against_the_qr_reference(ctx, name):
    sc, qr, ch, dist = pc.reference(name)
    got = _solve(ctx, sc)
    bound = max(1e-9, 1000.0 * dist)
    dx = pc.same_rotation_distance(got["poses"], qr["poses"])
    second_order = len(sc["edge_a"]) * (pc.jacobian_row_bound(sc) * bound) ** 2 / 2.0
    print("PG %-22s term %d/%d it %d/%d rejected %d/%d cost0 %.17g/%.17g cost %.6g/%.6g dx %.3e bound %.3e" % (
        name, got["termination"], qr["termination"], got["iterations"], qr["iterations"], got["rejected_steps"],
        qr["trace"]["rejected"], got["initial_cost"], qr["initial_cost"], got["final_cost"], qr["final_cost"], dx, bound))
    assert got["termination"] == qr["termination"]
    assert abs(got["iterations"] - qr["iterations"]) <= 1
    assert got["invalid_steps"] == 0 and got["n_outliers"] == 0
    assert abs(got["initial_cost"] - qr["initial_cost"]) <= 1e-6 * qr["initial_cost"]
    assert abs(got["final_cost"] - qr["final_cost"]) <= 1e-6 * qr["final_cost"] + second_order
    assert dx <= bound
    start = np.asarray(sc["poses"], np.float64)
    for k in np.flatnonzero(sc["fixed"]):                     # a constant pose comes back bit for bit
        assert got["poses"][k].tobytes() == start[k].tobytes(), k
    if name == "isolated_fixed_middle":                       # so does a pose without an edge
        assert got["poses"][4].tobytes() == start[4].tobytes()
        assert not np.array_equal(got["poses"][5], start[5])
    if name in ("all_fixed", "empty"):
        assert got["poses"].tobytes() == start.tobytes() and got["iterations"] == 0 and got["termination"] == 0
    if name == "empty":
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


def _same_bits(a, b):
    assert a["poses"].tobytes() == b["poses"].tobytes()
    for k in ("termination", "iterations", "rejected_steps", "invalid_steps", "n_outliers"):
        assert a[k] == b[k], k
    for k in ("initial_cost", "final_cost"):
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), k


@pytest.mark.parametrize("name", ["chain:17", "star70", "duplicates", "rejected", "info_upper"])
def test_a_second_call_returns_the_same_bits(ctx, name):
    sc = pc.scene(name)
    _same_bits(_solve(ctx, sc), _solve(ctx, sc))


def test_fixed_none_is_no_constant_pose(ctx):
    sc = pc.scene("two_components")
    free = dict(sc, fixed=np.zeros(len(sc["poses"]), np.uint8))
    a, b = _solve(ctx, free), _solve(ctx, free, fixed=None)
    _same_bits(a, b)
    assert a["termination"] == 0 and not np.array_equal(a["poses"][0], sc["poses"][0])


@pytest.fixture(scope="module")
def chain300():
    """300 keyframes on a loop walked once, exact measurements, loop edges every 50 keyframes and one that closes the walk"""
    K = 300
    tp = np.zeros((K, 7))
    tp[0, 3] = 1.0
    rng = np.random.default_rng(300)
    for k in range(K - 1):
        step = np.concatenate([[0.0, np.sin(np.pi / K), 0.0, np.cos(np.pi / K)], [0.1, 0.01 * rng.normal(), 0.0]])
        tp[k + 1] = pg.compose(tp[k], step)
    edges = pc.chain(K, 0) + [(k, (k + 150) % K) for k in range(0, K, 50)] + [(K - 1, 0)]
    return pc.make_scene(K, edges, 301, noise=0.0, angle=0.02, shift=0.05, truth=tp)


def test_chain_of_300_against_ground_truth(ctx, chain300):
    """exact measurements: the minimum is the truth at cost 0.  1794 unknowns: 38 panels of the blocked factor.  The solve ends
    by the gradient or function tolerance with the last step's leftover: 1e-6 m is three orders above what the noise-free
    cases of pose_graph_cases leave (1e-12 in cost) and four below the start's 0.05 m."""
    sc = chain300
    got = _solve(ctx, sc)
    dx = pc.same_rotation_distance(got["poses"], sc["truth_poses"])
    print("PG chain300 term %d it %d cost %.6g -> %.6g dx to truth %.3e" % (
        got["termination"], got["iterations"], got["initial_cost"], got["final_cost"], dx))
    assert got["termination"] == 0 and got["invalid_steps"] == 0
    assert got["final_cost"] <= 1e-12 * got["initial_cost"]
    assert dx <= 1e-6
    _same_bits(got, _solve(ctx, sc))


def test_a_smaller_problem_after_a_larger_one_and_the_shared_buffer(ctx, pkg, chain300):
    """the workspaces only grow and are carved afresh per call: what the 300-keyframe solve left in them — the normal
    equations live in the buffer global bundle adjustment factors in — must reach neither a smaller pose graph nor a global
    bundle adjustment after it"""
    small = pc.scene("chain:10")
    c = pkg.Context(width=0, height=0)
    fresh = _solve(c, small)
    c.close()
    _solve(ctx, chain300)
    _same_bits(_solve(ctx, small), fresh)
    _solve(ctx, chain300)
    sc, qr, sch, dist, mask, margin = bg.reference("traj:17")
    got = ctx.bundle_adjust_global(sc["poses"], sc["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"], sc["fixed"])
    bound = max(1e-9, 1000.0 * dist)
    dx = max(float(np.max(np.abs(got["poses"] - qr["poses"]))), float(np.max(np.abs(got["landmarks"] - qr["landmarks"]))))
    assert got["termination"] == qr["termination"] and abs(got["iterations"] - qr["iterations"]) <= 1 and got["invalid_steps"] == 0
    assert abs(got["final_cost"] - qr["final_cost"]) <= 1e-6 * qr["final_cost"] + len(sc["obs_kf"]) * (12.0 * bound) ** 2 / 2.0
    assert dx <= bound and np.array_equal(got["outlier"], mask)
    _same_bits(_solve(ctx, small), fresh)


def test_failure_leaves_the_poses(ctx):
    """a NaN in a measurement's position passes the argument checks (they look at quaternions and sqrt_info): the cost at
    the start is not finite, termination 2 (MSLAM_HIP_E_NO_MODEL) is the result, nothing moves"""
    clean = pc.scene("chain:9")
    for spoil in ("meas", "pose"):
        sc = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in clean.items()}
        if spoil == "meas":
            sc["edge_meas"][3, 5] = np.nan
        else:
            sc["poses"][4, 6] = np.inf
        got = _solve(ctx, sc)
        with np.errstate(all="ignore"):
            ref = pc.solve(sc)
        assert ref["termination"] == pg.FAILURE and ref["reason"] == "initial evaluation failed"
        assert got["termination"] == 2 and got["iterations"] == 0 and not np.isfinite(got["initial_cost"])
        assert got["poses"].tobytes() == sc["poses"].tobytes()
    _same_bits(_solve(ctx, clean), _solve(ctx, clean))


def test_invalid_arguments_then_a_clean_call(ctx, pkg):
    sc = pc.scene("chain:9")
    E, K = len(sc["edge_a"]), len(sc["poses"])

    def at(a, i, v):
        a = np.array(a)
        a[i] = v
        return a
    off_q = sc["poses"].copy()
    off_q[2, :4] *= 1.0 + 3e-6
    off_z = sc["edge_meas"].copy()
    off_z[1, :4] *= 1.0 - 3e-6
    bad_info = np.tile(np.eye(6), (E, 1, 1))
    bad_info[E - 1, 2, 4] = np.inf
    many = np.tile([0, 0, 0, 1.0, 0, 0, 0], (pkg.POSE_GRAPH_MAX_KEYFRAMES + 1, 1))
    n_big = pkg.POSE_GRAPH_MAX_EDGES + 1
    for bad in (dict(edge_a=at(sc["edge_a"], 0, -1)), dict(edge_b=at(sc["edge_b"], E - 1, K)), dict(edge_a=at(sc["edge_a"], 2, K)),
                dict(edge_a=at(sc["edge_a"], 4, sc["edge_b"][4])), dict(max_iterations=-1), dict(poses=off_q), dict(edge_meas=off_z),
                dict(sqrt_info=bad_info), dict(sqrt_info=at(bad_info, (0, 0, 0), np.nan)), dict(poses=many, fixed=None),
                dict(edge_a=np.zeros(n_big, np.int32), edge_b=np.ones(n_big, np.int32),
                     edge_meas=np.tile([0, 0, 0, 1.0, 0, 0, 0], (n_big, 1)))):
        with pytest.raises(pkg.MslamHipError) as e:
            _solve(ctx, sc, **bad)
        assert e.value.code == pkg.E_INVALID, bad.keys()
    qr = pc.reference("chain:9")[1]
    got = _solve(ctx, sc)
    assert got["termination"] == qr["termination"] and pc.same_rotation_distance(got["poses"], qr["poses"]) <= 1e-9
    off_q[2, :4] = sc["poses"][2, :4] * (1.0 + 5e-7)          # inside the 1e-6 band: accepted
    assert _solve(ctx, sc, poses=off_q)["termination"] == 0


# ---- HipBackend.close_loop ------------------------------------------------------------------------------------------------------

def _rvec(R):
    q = pg.matrix_to_quaternion(R)
    n = np.linalg.norm(q[:3])
    return 2.0 * np.arctan2(n, q[3]) * q[:3] / n


def test_backend_close_loop_against_the_numpy_close_loop(ctx, pkg):
    """the 40-keyframe drift scene in a HipBackend (ids with gaps, the chain as the covisibility graph, landmarks seen from
    their own keyframe and the next), the loop between the last and the first keyframe measured at the truth.  Poses and
    landmarks stay within the state bound, formed over both: max(1e-9, 1000 x the distance of the two CPU close_loop results
    in poses and in landmarks)."""
    sc = pc.scene("drift40")
    K = len(sc["poses"])
    ids = [3 * k + 1 for k in range(K)]
    rng = np.random.default_rng(8)
    be = pkg.HipBackend(ctx)
    for k in range(K):
        own = rng.uniform([-1, -1, 1.5], [1, 1, 3.0], (3, 3))
        lids, cam = [1000 + 3 * k + i for i in range(3)], own
        if k:                                                 # the previous keyframe's first landmark, seen again: not re-anchored
            lids, cam = lids + [1000 + 3 * (k - 1)], np.concatenate([own, rng.uniform([-1, -1, 1.5], [1, 1, 3.0], (1, 3))])
        be.add_keyframe(ids[k], sc["poses"][k], lids, cam)
    graph = {ids[k]: set(ids[j] for j in (k - 1, k + 1) if 0 <= j < K) for k in range(K)}
    assert all(be.anchor[1000 + 3 * k + i] == ids[k] for k in range(K) for i in range(3))
    T = sc["truth_poses"][-1]
    R = pg.q_matrix(T[:4]).T
    rvec, tvec = _rvec(R), -R @ T[4:]
    state = (dict(be.poses), be.first, graph, dict(be.anchor), dict(be.landmarks), ids[-1], ids[0], rvec, tvec)
    qr, ch = pg.close_loop(*state, linear_solver="qr"), pg.close_loop(*state, linear_solver="chol")
    bound = max(1e-9, 1000.0 * max(pc.same_rotation_distance(qr["poses"], ch["poses"]),
                                   float(np.max(np.abs(qr["landmarks"] - ch["landmarks"])))))
    got = be.close_loop(ids[-1], ids[0], rvec, tvec, graph)
    dx, dl = pc.same_rotation_distance(got["poses"], qr["poses"]), float(np.max(np.abs(got["landmarks"] - qr["landmarks"])))
    print("PG close_loop term %d/%d it %d/%d cost %.6g -> %.6g / %.6g dx %.3e dl %.3e bound %.3e" % (
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
    for i, l in enumerate(got["landmark_ids"].tolist()):
        assert be.landmarks[l].tobytes() == got["landmarks"][i].tobytes()
    assert be.poses[ids[0]].tobytes() == sc["poses"][0].tobytes()
    end = lambda x: float(np.linalg.norm(x[-1, 4:] - sc["truth_poses"][-1, 4:]))
    assert end(got["poses"]) < end(got["poses_before"]) / 5.0
    # FAILURE keeps the stored state
    be.poses[ids[5]][5] = np.nan
    before = ({k: v.tobytes() for k, v in be.poses.items()}, {l: v.tobytes() for l, v in be.landmarks.items()})
    bad = be.close_loop(ids[-1], ids[0], rvec, tvec, graph)
    assert bad["termination"] == 2
    assert before == ({k: v.tobytes() for k, v in be.poses.items()}, {l: v.tobytes() for l, v in be.landmarks.items()})


# ---- the tracker ----------------------------------------------------------------------------------------------------------------

def test_tracker_with_loop_closure_off_and_on_without_a_loop(pkg):
    """tests/track_ref.py's out-and-back walk.  It tracks the way back on the local map of the keyframes of the way out, so
    every keyframe is a covisibility neighbour of the place it returns to and no loop event may fire: with loop_closure on,
    every keyframe goes through the database and every frame equals the frame without it, apart from the `loop` key, which
    loop_closure = False does not add."""
    seq = tr.make_sequence()
    runs = []
    for kw in (dict(loop_closure=False), dict(loop_closure=True, loop_min_gap=2)):
        c = pkg.Context(width=0, height=0, max_keypoints=4096)
        c.bow_load(synth.make_vocabulary(10, 3))
        t = pkg.HipKeyframeTracker(c, focal=tr.CAM[:2], principal=tr.CAM[2:], local_map_depth=2, local_ba=True, **dict(tr.SEQ_PARAMS, **kw))
        rows = [t.processSensorData(fr["desc"], fr["xy"], fr["depth"]) for fr in seq["frames"]]
        runs.append((c, t, rows))
    (c0, t0, a), (c2, t2, on) = runs
    assert all("loop" not in r for r in a) and all(r["loop"] is None for r in on)
    assert len(t0.ids) >= 3 and c2.bow_db_size() == len(t2.ids) and c0.bow_db_size() == 0
    assert sorted(t2._bow_entry.values()) == t2.ids
    assert t2.ids == t0.ids and [r["termination"] for r in t2.ba_results] == [r["termination"] for r in t0.ba_results]
    for f, (x, y) in enumerate(zip(a, on)):
        assert (x["tracked"], x["n_inliers"], x["keyframe"], x["reference"], x["relocalized"]) == \
               (y["tracked"], y["n_inliers"], y["keyframe"], y["reference"], y["relocalized"]), f
        assert x["R"].tobytes() == y["R"].tobytes() and x["tvec"].tobytes() == y["tvec"].tobytes() and x["rvec"].tobytes() == y["rvec"].tobytes(), f
    for k in t0.ids:
        assert c0.kf_read(k)[1].tobytes() == c2.kf_read(k)[1].tobytes()
    for r in t2.loop_results:                                 # an attempt, if the database offered one, found no loop
        assert r["loop"] is None
    with pytest.raises(pkg.MslamHipError) as e:
        pkg.HipKeyframeTracker(c0, local_map_depth=2, loop_closure=True)      # needs local_ba
    assert e.value.code == pkg.E_INVALID
    bare = pkg.Context(width=0, height=0)
    with pytest.raises(pkg.MslamHipError) as e:
        pkg.HipKeyframeTracker(bare, local_map_depth=2, local_ba=True, loop_closure=True)   # needs a vocabulary
    assert e.value.code == pkg.E_INVALID
    for c in (c0, c2, bare):
        c.close()


RING_PARAMS = dict(local_map_depth=2, local_ba=True, new_keyframe_min_landmarks=200)


def _expected_loop(seq, min_gap, min_inliers):
    """the CPU trackers on the ring walk (tests/local_map_ref.py, tests/reloc_ref.py): the first keyframe that verifies, with
    at least min_inliers, against a keyframe at least min_gap older that is not in its neighbourhood -> (cur, loop, frames
    of the keyframes)"""
    trk = lm.LocalMapTracker(depth=2, cam=seq["cam"], new_keyframe_min_landmarks=200)
    frames = {}
    for f, fr in enumerate(seq["frames"]):
        k = trk.process(fr["desc"], fr["xy"], fr["depth"])["keyframe"]
        if k < 0:
            continue
        frames[k] = f
        near = lm.neighbours(trk.graph, k, 2)
        cands = [j for j in trk.ids if k - j >= min_gap and j not in near]
        if cands and "loop" not in frames:
            best = rr.relocalize(fr["desc"], fr["xy"], trk.store, cands, seq["cam"], seed=f, min_inliers=min_inliers)["best"]
            if best >= 0:
                frames["loop"] = (k, cands[best])
    return frames.pop("loop"), frames


def _run_ring(pkg, seq, **kw):
    c = pkg.Context(width=0, height=0, max_keypoints=4096)
    c.bow_load(synth.make_vocabulary(10, 3))
    t = pkg.HipKeyframeTracker(c, focal=tr.CAM[:2], principal=tr.CAM[2:], **dict(RING_PARAMS, **kw))
    return c, t, [t.processSensorData(fr["desc"], fr["xy"], fr["depth"]) for fr in seq["frames"]]


@pytest.mark.parametrize("global_ba", [False, True])
def test_tracker_closes_the_loop_of_the_ring_walk(pkg, global_ba):
    """the camera turns once round in a ring of landmarks.  The keyframe inserted when the first keyframe's landmarks come
    back into view was tracked on a local map that does not reach the first keyframe, so it shares no landmark id with it:
    the database names the first keyframe, the verification accepts it, closeLoop runs.  The scene has no noise but the
    depth quantisation, so the loop edge agrees with the odometry edges and the correction must leave every keyframe within
    the ground-truth tolerance of tests/test_gpu_track.py (0.1 degree, 0.02 m)."""
    seq = loop_walk.ring_sequence()
    (cur, loop), kf_frames = _expected_loop(seq, min_gap=5, min_inliers=60)
    assert loop == 0 and cur >= 5 and len(kf_frames) > cur
    c, t, rows = _run_ring(pkg, seq, loop_closure=True, loop_min_gap=5, loop_global_ba=global_ba)
    fired = [(f, r["loop"]) for f, r in enumerate(rows) if r["loop"] is not None]
    print("ring walk: keyframes at frames %s, loop events %s, attempts %s" % (
        [f for f, r in enumerate(rows) if r["keyframe"] >= 0], fired,
        [(a["keyframe"], a["candidates"], a["inliers"], a["loop"]) for a in t.loop_results]))
    assert fired == [(kf_frames[cur], (cur, loop))]
    assert all(r["tracked"] for r in rows) and [f for f, r in enumerate(rows) if r["keyframe"] >= 0] == [kf_frames[k] for k in sorted(kf_frames)]
    closed = [a for a in t.loop_results if a["loop"] is not None]
    assert len(closed) == 1 and closed[0]["keyframe"] == cur and closed[0]["loop"] == loop
    res = closed[0]["result"]
    assert res["termination"] == 0 and res["invalid_steps"] == 0 and res["keyframes"] == list(range(cur + 1))
    # a correction was applied: the loop edge disagrees with the odometry edges by what the depth quantisation left, the
    # solve takes that cost down and moves free poses (the first keyframe stays)
    moved = float(np.max(np.abs(res["poses"] - res["poses_before"])))
    print("ring walk: closure cost %.6g -> %.6g in %d iterations, largest pose change %.3e" % (
        res["initial_cost"], res["final_cost"], res["iterations"], moved))
    assert res["initial_cost"] > res["final_cost"] >= 0.0 and res["iterations"] >= 1
    assert moved > 0.0 and res["poses"][0].tobytes() == res["poses_before"][0].tobytes()
    assert not np.array_equal(res["poses"][cur], res["poses_before"][cur])
    assert res["n_written"] >= len(res["landmark_ids"]) > 0
    assert ("global_ba" in closed[0]) == global_ba
    if global_ba:                                             # the global solve after the closure, over every keyframe so far
        ba = closed[0]["global_ba"]
        assert ba["termination"] in (0, 1) and ba["keyframes"] == list(range(cur + 1)) and ba["final_cost"] <= ba["initial_cost"]
        assert ba["n_written"] >= len(ba["landmark_ids"]) > 0
    assert c.bow_db_size() == len(t.ids) and sorted(t._bow_entry.values()) == t.ids
    for k in t.ids:                                           # every keyframe against the ground truth of its frame
        q, p = t.backend.poses[k][:4], t.backend.poses[k][4:]
        R = pg.q_matrix(q).T
        fr = seq["frames"][kf_frames[k]]
        err_deg, err_m = rr.rot_err(R, fr["R"]), float(np.linalg.norm(-R @ p - fr["t"]))
        assert err_deg < 0.1 and err_m < 0.02, (k, err_deg, err_m)
    for f, r in enumerate(rows):                              # and every frame's pose, the frame of the closure included
        assert rr.rot_err(r["R"], seq["frames"][f]["R"]) < 0.1 and np.linalg.norm(r["tvec"] - seq["frames"][f]["t"]) < 0.02, f
    for l in res["landmark_ids"][:50].tolist():               # the store holds the moved landmarks that no later solve touched
        assert l in t.backend.landmarks
    c.close()


def test_tracker_ring_walk_loop_closure_false_is_the_default_and_repeats(pkg):
    """loop_closure = False is the default: the constructor call with the switch named and the one without it take the
    same path, nothing reaches the database, no frame gains the `loop` key, and two runs return the same bits.  That the
    default path computes what it computed before this feature is shown by tests/test_gpu_track.py, tests/test_gpu_ba.py and
    tests/test_gpu_local_map.py, which run untouched."""
    seq = loop_walk.ring_sequence(n_frames=40)
    c0, t0, a = _run_ring(pkg, seq)
    c1, t1, b = _run_ring(pkg, seq, loop_closure=False)
    assert t1.loop_results == [] and c1.bow_db_size() == 0 and len(t0.ids) >= 5
    for f, (x, y) in enumerate(zip(a, b)):
        assert sorted(x) == sorted(y) and "loop" not in y
        assert (x["tracked"], x["n_inliers"], x["keyframe"], x["reference"], x["relocalized"]) == \
               (y["tracked"], y["n_inliers"], y["keyframe"], y["reference"], y["relocalized"]), f
        assert x["R"].tobytes() == y["R"].tobytes() and x["tvec"].tobytes() == y["tvec"].tobytes() and x["rvec"].tobytes() == y["rvec"].tobytes(), f
    for k in t0.ids:
        assert c0.kf_read(k)[1].tobytes() == c1.kf_read(k)[1].tobytes() and t0.backend.poses[k].tobytes() == t1.backend.poses[k].tobytes()
    c0.close()
    c1.close()
