"""The pose-graph reference (tests/pose_graph_ref.py) on the CPU: the analytic derivatives DESIGN.md 4.17 writes down against
the jets, the closed-form two-pose problem, that every case of tests/pose_graph_cases.py takes the path it is named for and
that the two linear solvers agree on it, the drift a loop edge takes out of a chain, the numpy close_loop, the loop logic of
HipKeyframeTracker and HipBackend.close_loop on a stub context (no GPU: the stub solves with the reference), and what
build() left of the feature."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_cases as pc  # noqa: E402
import pose_graph_ref as pg  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "modular-slam_amd", "host")


@pytest.mark.parametrize("name", ["chain:9", "star70", "duplicates", "rot170", "neg_q", "info_upper", "rejected"])
def test_analytic_jacobians_equal_the_jets(name):
    sc = pc.scene(name)
    r, Ja, Jb = pg.tangent_jacobians(sc["poses"], sc["edge_a"], sc["edge_b"], sc["edge_meas"], sc["sqrt_info"])
    Aa, Ab = pg.analytic_jacobians(sc["poses"], sc["edge_a"], sc["edge_b"], sc["edge_meas"], sc["sqrt_info"])
    assert np.max(np.abs(Ja - Aa)) <= 1e-10 and np.max(np.abs(Jb - Ab)) <= 1e-10
    assert np.max(np.abs(Ja)) > 0.5 and np.max(np.abs(Jb)) > 0.5


def test_jets_equal_central_differences():
    sc = pc.scene("info_upper")
    args = (sc["edge_a"], sc["edge_b"], sc["edge_meas"], sc["sqrt_info"])
    r, Ja, Jb = pg.tangent_jacobians(sc["poses"], *args)
    h = 1e-6
    for k in (1, 4):
        for j in range(6):
            d = np.zeros(6)
            d[j] = h
            hi, lo = sc["poses"].copy(), sc["poses"].copy()
            hi[k, :4], lo[k, :4] = pg.quaternion_plus(hi[k, :4], d[:3]), pg.quaternion_plus(lo[k, :4], -d[:3])
            hi[k, 4:] += d[3:]
            lo[k, 4:] -= d[3:]
            num = (pg.residuals(hi, *args) - pg.residuals(lo, *args)) / (2.0 * h)
            for e in range(len(r)):
                want = Ja[e, :, j] if sc["edge_a"][e] == k else Jb[e, :, j] if sc["edge_b"][e] == k else np.zeros(6)
                assert np.max(np.abs(num[e] - want)) <= 1e-7, (k, j, e)


@pytest.mark.parametrize("solver", ["qr", "chol"])
def test_two_poses_one_edge_reach_the_measurement(solver):
    sc = pc.scene("pair")
    res = pc.solve(sc, solver)
    assert res["termination"] == pg.CONVERGENCE and res["final_cost"] < 1e-20
    assert pc.same_rotation_distance(res["poses"][1], pg.compose(sc["poses"][0], sc["edge_meas"][0])) <= 1e-10
    assert res["poses"][0].tobytes() == sc["poses"][0].tobytes()


@pytest.mark.parametrize("name", pc.ALL)
def test_every_case_takes_its_path_and_the_solvers_agree(name):
    sc, qr, ch, dist = pc.reference(name)
    tr = qr["trace"]
    assert qr["termination"] == ch["termination"] and qr["iterations"] == ch["iterations"]
    assert tr["rejected"] == ch["trace"]["rejected"] and tr["invalid"] == ch["trace"]["invalid"] == 0
    assert dist <= 1e-9
    start = np.asarray(sc["poses"], np.float64)
    for k in np.flatnonzero(sc["fixed"]):
        assert qr["poses"][k].tobytes() == start[k].tobytes()
    kind = name.partition(":")[0]
    if kind == "chain":
        assert tr["free_poses"] == int(name.partition(":")[2]) - 1 and qr["termination"] == pg.CONVERGENCE
    if kind == "star70":
        hub = int(np.sum(sc["edge_a"] == 0) + np.sum(sc["edge_b"] == 0))
        assert hub == 70 > 64 and not sc["fixed"][0] and tr["free_poses"] == 70
    if kind == "duplicates":
        pairs = list(zip(sc["edge_a"].tolist(), sc["edge_b"].tolist()))
        assert pairs.count((1, 2)) == 2 and (2, 3) in pairs and (3, 2) in pairs and pairs.count((0, 1)) == 2
    if kind == "two_components":
        assert not sc["fixed"][4:].any() and not np.array_equal(qr["poses"][4:], start[4:]) and qr["termination"] == pg.CONVERGENCE
    if kind == "isolated_fixed_middle":
        assert 4 not in sc["edge_a"] and 4 not in sc["edge_b"] and qr["poses"][4].tobytes() == start[4].tobytes()
        assert sc["fixed"][3] and tr["free_poses"] == 5
    if kind == "all_fixed":
        assert tr["free_poses"] == 0 and qr["iterations"] == 0 and qr["termination"] == pg.CONVERGENCE and qr["initial_cost"] > 0.0
    if kind == "empty":
        assert qr["reason"] == "no parameter blocks" and qr["final_cost"] == 0.0
    if kind == "rot170":
        z = sc["edge_meas"][0]
        assert abs(np.rad2deg(2.0 * np.arccos(abs(z[3]))) - 170.0) < 2.0
    if kind == "neg_q":
        assert np.all(np.sum(qr["poses"][:, :4] * start[:, :4], 1) > 0.0) and start[2, 3] * pc.scene("chain:9")["poses"][2, 3] != 0.0
        plain = pc.scene("neg_q")
        plain["poses"][[0, 2], :4] *= -1.0
        assert pc.same_rotation_distance(pc.solve(plain)["poses"], qr["poses"]) <= 1e-9
    if kind == "info_upper":
        W = sc["sqrt_info"]
        assert np.all(np.tril(W, -1) == 0.0) and np.max(np.abs(np.triu(W, 1))) > 0.1
    if kind == "rejected":
        assert tr["rejected"] >= 1 and tr["accepted_after_rejected"] >= 1 and qr["termination"] == pg.CONVERGENCE
    if kind in ("cap0", "cap1"):
        n = int(kind[3])
        assert qr["termination"] == pg.NO_CONVERGENCE and qr["iterations"] == n and qr["reason"] == "max iterations"
        assert (qr["poses"].tobytes() == start.tobytes()) == (n == 0)
    if kind not in ("cap0", "cap1", "all_fixed", "empty"):
        assert qr["final_cost"] < 0.1 * qr["initial_cost"]


def _end_error(poses, truth):
    return float(np.linalg.norm(poses[-1, 4:] - truth[-1, 4:]))


def test_a_loop_edge_takes_the_drift_out_of_a_chain():
    """39 drifted odometry edges and one ground-truth loop edge, identity information: against the loop edge's weight 1 the
    chain acts as one edge of weight 1 / 39 (39 unit springs in series), so about 1 / 40 of the end pose's translation error
    stays"""
    sc, qr, ch, dist = pc.reference("drift40")
    before, after = _end_error(sc["poses"], sc["truth_poses"]), _end_error(qr["poses"], sc["truth_poses"])
    print("drift: end error %.4f m -> %.4f m, ratio %.4f (1 / 40 = 0.025)" % (before, after, after / before))
    assert len(sc["edge_a"]) == 40 and before > 0.1
    assert after < before / 5.0


def _drift_backend_state(sc):
    """the drift scene as a backend holds it: poses by id, the chain as the covisibility graph, three landmarks per
    keyframe anchored there"""
    K = len(sc["poses"])
    ids = [3 * k + 1 for k in range(K)]                      # ids with gaps, the first is the constant one
    poses = {ids[k]: sc["poses"][k].copy() for k in range(K)}
    graph = {ids[k]: set(ids[j] for j in (k - 1, k + 1) if 0 <= j < K) for k in range(K)}
    rng = np.random.default_rng(8)
    cam = {ids[k]: rng.uniform([-1, -1, 1.5], [1, 1, 3.0], (3, 3)) for k in range(K)}
    lids = {ids[k]: [1000 + 3 * k + i for i in range(3)] for k in range(K)}
    T = sc["truth_poses"][-1]
    R = pg.q_matrix(T[:4]).T                                 # world -> camera of the last keyframe, at the truth
    return ids, poses, graph, cam, lids, -R @ T[4:], R


def _rvec(R):
    q = pg.matrix_to_quaternion(R)
    n = np.linalg.norm(q[:3])
    return 2.0 * np.arctan2(n, q[3]) * q[:3] / n


def test_numpy_close_loop_measurement_and_landmarks():
    sc = pc.scene("drift40")
    ids, poses, graph, cam, lids, tvec, R = _drift_backend_state(sc)
    rvec = _rvec(R)
    anchor, landmarks = {}, {}
    for k in ids:
        for l, c in zip(lids[k], cam[k]):
            anchor[l], landmarks[l] = k, pg.q_matrix(poses[k][:4]) @ c + poses[k][4:]
    # Z = T_loop^-1 o T_cur*: with the true pose of the last keyframe and the first keyframe at the origin, Z is the truth's
    Z = pg.loop_measurement(poses[ids[0]], rvec, tvec)
    assert pc.same_rotation_distance(Z, pg.relative(sc["truth_poses"][0], sc["truth_poses"][-1])) <= 1e-12
    res = pg.close_loop(poses, ids[0], graph, anchor, landmarks, ids[-1], ids[0], rvec, tvec)
    assert res["keyframes"] == ids and res["termination"] == pg.CONVERGENCE
    assert len(res["edge_a"]) == 40 and (res["edge_a"][-1], res["edge_b"][-1]) == (0, 39)
    assert [(a, b) for a, b in zip(res["edge_a"][:-1], res["edge_b"][:-1])] == [(k, k + 1) for k in range(39)]
    # the odometry edges are measured on the current poses: only the loop edge has a residual at the start
    r0 = pg.residuals(res["poses_before"], res["edge_a"], res["edge_b"], res["edge_meas"])
    assert np.max(np.abs(r0[:-1])) <= 1e-12 and np.linalg.norm(r0[-1]) > 0.1
    before, after = _end_error(res["poses_before"], sc["truth_poses"]), _end_error(res["poses"], sc["truth_poses"])
    assert after < before / 5.0
    # a landmark keeps its place in its anchor keyframe's frame
    for i, l in enumerate(res["landmark_ids"].tolist()):
        k = ids.index(anchor[l])
        T = res["poses"][k]
        local = pg.q_matrix(pg.q_inv(T[:4])) @ (res["landmarks"][i] - T[4:])
        assert np.max(np.abs(local - cam[anchor[l]][lids[anchor[l]].index(l)])) <= 1e-12


# ---- the package's host logic on a stub context ---------------------------------------------------------------------------

class StubContext:
    """what HipKeyframeTracker's loop logic and HipBackend.close_loop ask of a Context, without a device: the pose graph is
    solved by the numpy reference, the database and the verification answer what the test scripted"""

    def __init__(self, pkg, vocabulary=True):
        self.pkg, self.vocabulary = pkg, vocabulary
        self.hits, self.verdict = ([], []), None
        self.db, self.calls, self.written = [], [], []

    def bow_info(self):
        if not self.vocabulary:
            raise self.pkg.MslamHipError(self.pkg.E_NO_VOCABULARY, "no vocabulary")
        return dict(k=10, L=3)

    def bow_db_query(self, desc, max_results=4):
        self.calls.append(("query", len(self.db), max_results))
        return np.array(self.hits[0], np.int32)[:max_results], np.array(self.hits[1], np.float64)[:max_results]

    def bow_db_add(self, desc):
        self.calls.append(("add", len(self.db)))
        self.db.append(desc)
        return 100 + len(self.db) - 1                         # entry ids are not keyframe ids

    def relocalize(self, desc, xy, cand_ids, focal, principal, valid, ratio, iterations, reprojection_error, seed, rvec=None,
                   tvec=None, min_inliers=60):
        self.calls.append(("relocalize", list(cand_ids), rvec, min_inliers))
        best, rv, tv, inl = self.verdict(list(cand_ids))
        cands = [dict(n_inliers=inl if i == best else 3, rvec=np.array(rv, np.float64), tvec=np.array(tv, np.float64), status=1)
                 for i in range(len(cand_ids))]
        return dict(best=best, candidates=cands)

    def pose_graph(self, poses, edge_a, edge_b, edge_meas, sqrt_info=None, fixed=None, max_iterations=100):
        res = pg.pose_graph(poses, edge_a, edge_b, edge_meas, sqrt_info, fixed, max_iterations)
        self.calls.append(("pose_graph", len(edge_a)))
        return dict(poses=res["poses"], termination=res["termination"], iterations=res["iterations"], rejected_steps=0,
                    invalid_steps=0, n_outliers=0, initial_cost=res["initial_cost"], final_cost=res["final_cost"])

    def kf_update_world(self, landmark_ids, world_xyz):
        self.written.append((np.array(landmark_ids), np.array(world_xyz)))
        return len(landmark_ids)


def _loop_tracker(pkg, **kw):
    """a tracker whose map is the drift scene: 40 keyframes 0..39 on a chain, fed to its backend"""
    sc = pc.scene("drift40")
    ctx = StubContext(pkg)
    t = pkg.HipKeyframeTracker(ctx, local_map_depth=1, local_ba=True, loop_closure=True, **kw)
    K = len(sc["poses"])
    rng = np.random.default_rng(8)
    for k in range(K):
        t.backend.add_keyframe(k, sc["poses"][k], [1000 + 2 * k, 1001 + 2 * k], rng.uniform([-1, -1, 1.5], [1, 1, 3.0], (2, 3)))
        t.graph[k] = set(j for j in (k - 1, k + 1) if 0 <= j < K)
        t._bow_entry[100 + k] = k
    t.ids, t.reference = list(range(K)), K - 1
    ctx.db = [None] * K
    return sc, ctx, t


def test_tracker_needs_local_ba_and_a_vocabulary(pkg):
    for ctx, kw in ((StubContext(pkg), dict(local_map_depth=1)), (StubContext(pkg), dict()),
                    (StubContext(pkg, vocabulary=False), dict(local_map_depth=1, local_ba=True))):
        with pytest.raises(pkg.MslamHipError) as e:
            pkg.HipKeyframeTracker(ctx, loop_closure=True, **kw)
        assert e.value.code == pkg.E_INVALID
    t = pkg.HipKeyframeTracker(StubContext(pkg, vocabulary=False), local_map_depth=1, local_ba=True)   # off: nothing is asked
    assert not t.loop_closure and t.loop_results == []


def test_tracker_loop_candidate_filters(pkg):
    sc, ctx, t = _loop_tracker(pkg, loop_min_gap=10, loop_min_score=0.05, loop_max_candidates=3)
    entries = [100 + k for k in (38, 37, 30, 29, 5, 2, 0, 20, 999)]
    scores = [0.9, 0.8, 0.5, 0.3, 0.2, 0.049, 0.6, 0.05, 0.7]
    # 38 is a neighbour and 37 its neighbour (depth 1 expands two hops), 30 is 9 keyframes back, 2 scores too little, entry
    # 999 is no keyframe; 29, 5, 0, 20 pass: best score first, three of them
    assert t.neighbours(39) == [37, 38, 39]
    assert t.loop_candidates(39, entries, scores) == [0, 29, 5]
    t.loop_max_candidates = 8
    assert t.loop_candidates(39, entries, scores) == [0, 29, 5, 20]
    t.graph[39].add(0)                                      # covisible already: no loop to close
    t.graph[0].add(39)
    assert t.loop_candidates(39, entries, scores) == [29, 5, 20]
    t._last_closure = 30                                    # the cool-down: 9 keyframes after a closure
    assert t.loop_candidates(39, entries, scores) == []
    t._last_closure = 29
    assert t.loop_candidates(39, entries, scores) == [29, 5, 20]


def test_tracker_closes_a_loop_on_the_stub(pkg):
    sc, ctx, t = _loop_tracker(pkg, loop_min_inliers=77)
    truth = sc["truth_poses"]
    R = pg.q_matrix(truth[39, :4]).T
    rvec, tvec = _rvec(R), -R @ truth[39, 4:]
    ctx.hits = ([100 + 38, 100 + 1, 100 + 0], [0.9, 0.2, 0.4])
    ctx.verdict = lambda cands: (cands.index(0), rvec, tvec, 120)
    before = {k: v.copy() for k, v in t.backend.poses.items()}
    lm_before = {l: v.copy() for l, v in t.backend.landmarks.items()}
    desc, xy = np.zeros((5, 32), np.uint8), np.zeros((5, 2), np.float32)
    assert t._close_loops(39, desc, xy, seed=4) == (39, 0)
    # the order: query before add; the verification without a guess, best score first, with the loop's own inlier floor
    assert [c[0] for c in ctx.calls] == ["query", "add", "relocalize", "pose_graph"]
    assert ctx.calls[0][1] == 40 and ctx.calls[2][1:] == ([0, 1], None, 77) and ctx.calls[3][1] == 40
    assert t._bow_entry[140] == 39 and t._last_closure == 39 and t._local_map_of is None
    att = t.loop_results[-1]
    assert att["keyframe"] == 39 and att["candidates"] == [0, 1] and att["loop"] == 0 and att["result"]["termination"] == 0
    # the reference's close_loop on the same state gives the same poses and landmarks
    ref = pg.close_loop(before, 0, t.graph, t.backend.anchor, lm_before, 39, 0, rvec, tvec)
    got = att["result"]
    assert got["keyframes"] == ref["keyframes"] and np.max(np.abs(got["poses_before"] - ref["poses_before"])) == 0.0
    assert pc.same_rotation_distance(got["poses"], ref["poses"]) <= 1e-12
    assert got["landmark_ids"].tolist() == ref["landmark_ids"].tolist() and np.max(np.abs(got["landmarks"] - ref["landmarks"])) <= 1e-12
    for k in range(40):
        assert t.backend.poses[k].tobytes() == got["poses"][k].tobytes()
    assert t.backend.poses[0].tobytes() == before[0].tobytes()                     # the first keyframe is constant
    assert _end_error(got["poses"], truth) < _end_error(got["poses_before"], truth) / 5.0
    # the store gets the moved landmarks, the tracker the corrected pose of the new keyframe (world -> camera)
    assert len(ctx.written) == 1 and ctx.written[0][0].tolist() == got["landmark_ids"].tolist()
    assert ctx.written[0][1].tobytes() == got["landmarks"].tobytes()
    T = t.backend.poses[39]
    assert np.max(np.abs(t.R - pg.q_matrix(T[:4]).T)) <= 1e-12 and np.max(np.abs(t.tvec + t.R @ T[4:])) <= 1e-12
    assert np.max(np.abs(pg.rodrigues(t.rvec) - t.R)) <= 1e-12
    # every landmark kept its place in its anchor keyframe
    for l, x in t.backend.landmarks.items():
        a = t.backend.anchor[l]
        old = pg.q_matrix(pg.q_inv(before[a][:4])) @ (lm_before[l] - before[a][4:])
        new = pg.q_matrix(pg.q_inv(t.backend.poses[a][:4])) @ (x - t.backend.poses[a][4:])
        assert np.max(np.abs(old - new)) <= 1e-12
    # loop_global_ba: the global solve follows the closure, and its landmarks go to the store as well
    t._last_closure, t.loop_global_ba = None, True
    t.backend.global_ba = lambda: (ctx.calls.append(("global_ba",)), dict(termination=0, landmark_ids=np.array([1000]), landmarks=np.ones((1, 3))))[1]
    del ctx.calls[:]
    assert t._close_loops(39, desc, xy, seed=4) == (39, 0)
    assert [c[0] for c in ctx.calls] == ["query", "add", "relocalize", "pose_graph", "global_ba"]
    assert len(ctx.written) == 3 and ctx.written[2][0].tolist() == [1000] and t.loop_results[-1]["global_ba"]["n_written"] == 1
    t.loop_global_ba = False
    del ctx.written[1:], t.loop_results[1:]
    # no winner: the attempt is recorded, nothing moves; no candidate: no attempt
    state = {k: v.tobytes() for k, v in t.backend.poses.items()}
    t._last_closure = None
    ctx.verdict = lambda cands: (-1, rvec, tvec, 0)
    assert t._close_loops(39, desc, xy, seed=5) is None and t.loop_results[-1]["loop"] is None and len(t.loop_results) == 2
    ctx.hits = ([100 + 38], [0.9])
    assert t._close_loops(39, desc, xy, seed=6) is None and len(t.loop_results) == 2
    assert state == {k: v.tobytes() for k, v in t.backend.poses.items()} and len(ctx.written) == 1


def test_backend_close_loop_arguments(pkg):
    be = pkg.HipBackend(StubContext(pkg))
    be.add_keyframe(4, [0, 0, 0, 1, 0, 0, 0], [7], [[0.0, 0.0, 2.0]])
    be.add_keyframe(9, [0, 0, 0, 1, 1.0, 0, 0], [7, 8], [[-1.0, 0.0, 2.0], [0.5, 0.0, 2.0]])
    assert be.anchor == {7: 4, 8: 9}                        # the keyframe that created the landmark, not the last to see it
    for cur, loop in ((9, 9), (9, 5), (5, 4)):
        with pytest.raises(pkg.MslamHipError) as e:
            be.close_loop(cur, loop, np.zeros(3), np.zeros(3), {})
        assert e.value.code == pkg.E_INVALID
    # the loop edge alone, weighted: keyframe 9 goes where the measurement says (identity rotation, camera centre (2, 0, 0))
    # (to 1e-6: the solve ends by the function tolerance, with the last step's leftover)
    res = be.close_loop(9, 4, np.zeros(3), [-2.0, 0.0, 0.0], {}, sqrt_info=2.0 * np.eye(6))
    assert res["termination"] == 0 and np.max(np.abs(res["poses"][1] - [0, 0, 0, 1, 2.0, 0, 0])) <= 1e-6
    assert abs(res["initial_cost"] - 0.5 * 4.0 * 1.0) <= 1e-12          # |2 I (1, 0, 0, 0, 0, 0)|^2 / 2
    assert np.max(np.abs(be.landmarks[8] - [2.5, 0.0, 2.0])) <= 1e-6 and np.max(np.abs(be.landmarks[7] - [0.0, 0.0, 2.0])) == 0.0


def test_the_build_knows_the_pose_graph(pkg):
    """what build() left: nothing is compiled here"""
    out = subprocess.check_output(["nm", "-DC", pkg.LIB_PATH]).decode()
    assert "mslam_hip_pose_graph" in out
    out = subprocess.check_output(["nm", "-DC", os.path.join(HOST, "libmslam_hip_plugin.so")]).decode()
    assert "mslam_hip_pose_graph" in out and "hipBundleAdjustBackendFactory" in out
    src = open(os.path.join(HOST, "harness.cpp")).read()
    assert "--pose-graph" in src and "ILoopClosingBackend" in src and "closeLoop" in src
    hdr = open(os.path.join(HOST, "mslam_interfaces.hpp")).read()
    assert "class ILoopClosingBackend : public IGlobalBackend" in hdr and "closeLoop" in hdr
    assert b"--pose-graph" in open(os.path.join(HOST, "mslam_harness"), "rb").read()
    assert "mslam_hip_pose_graph" in pkg.ABI_SYMBOLS and hasattr(pkg.Context, "pose_graph")
