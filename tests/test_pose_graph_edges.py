"""The second, edge-focused set of pose-graph scenes (pose_graph_cases.EDGES) on the CPU: for every name, both linear solvers
of tests/pose_graph_ref.py agree on termination, reason, iterations and rejected count, no step is invalid, and the case takes
the path it is named for: the block, stride and list lengths k_posegraph.hip's kernels see, the termination test that ends the
run with the margin it has (trace["steps"] records the two ratios and the decision of every iteration), exact zeros, exact sign
symmetry.  tests/test_gpu_pose_graph_edges.py compares the kernels on the same names.

Looked at and left out: the invalid-step branch, the five-in-a-row FAILURE it leads to and the minimum-radius exit.  They need
a non-positive pivot or model_cost_change <= 0, and no input was found that reaches either through both solvers alike (QR does
not fail where Cholesky does), so the reference could not pin what the kernels do there."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_cases as pc  # noqa: E402
import pose_graph_ref as pg  # noqa: E402


def _decisions(res):
    return [s["decision"] for s in res["trace"]["steps"]]


def _pair_lists(sc):
    """what the host of k_posegraph.hip builds: incidences per pose, edges per unordered pair of free poses"""
    K = len(sc["poses"])
    ea, eb = sc["edge_a"].astype(np.int64), sc["edge_b"].astype(np.int64)
    inc = np.bincount(ea, minlength=K) + np.bincount(eb, minlength=K)
    free = ~sc["fixed"].astype(bool) & (inc > 0)
    both = free[ea] & free[eb]
    per_pair = np.unique(np.minimum(ea, eb)[both] * K + np.maximum(ea, eb)[both], return_counts=True)[1]
    return inc, free, per_pair


@pytest.mark.parametrize("name", pc.EDGES)
def test_every_edge_case_takes_its_path_and_the_solvers_agree(name):
    sc, qr, ch, dist = pc.reference(name)
    tr, steps = qr["trace"], qr["trace"]["steps"]
    print("PG ref %-20s term %d (%s) it %d rejected %d dist %.3e last ratios %s" % (
        name, qr["termination"], qr["reason"], qr["iterations"], tr["rejected"], dist,
        (steps[-1]["parameter_ratio"], steps[-1]["function_ratio"]) if steps else None))
    assert qr["termination"] == ch["termination"] and qr["reason"] == ch["reason"] and qr["iterations"] == ch["iterations"]
    assert tr["rejected"] == ch["trace"]["rejected"] and tr["invalid"] == ch["trace"]["invalid"] == 0
    assert _decisions(qr) == _decisions(ch) and len(steps) == qr["iterations"]
    assert tr["rejected"] == _decisions(qr).count("rejected") and "invalid" not in _decisions(qr)
    assert dist <= 1e-9
    start = np.asarray(sc["poses"], np.float64)
    K, E = len(start), len(sc["edge_a"])
    inc, free, per_pair = _pair_lists(sc)
    assert np.all(sc["edge_a"] != sc["edge_b"]) and tr["free_poses"] == int(free.sum())
    for k in np.flatnonzero(~free):
        assert qr["poses"][k].tobytes() == start[k].tobytes() and ch["poses"][k].tobytes() == start[k].tobytes()
    kind, _, rest = name.partition(":")
    if kind == "edges":
        assert E == int(rest) and qr["termination"] == pg.CONVERGENCE and qr["final_cost"] < 0.1 * qr["initial_cost"]
        pairs = set(zip(sc["edge_a"].tolist(), sc["edge_b"].tolist()))
        assert any((b, a) in pairs for a, b in pairs)         # both directions between one pair of poses
    if name == "edges:16641":                                  # 66 blocks, the last with one edge: the second trip of b += 64
        assert K == 12 and (E + 255) // 256 == 66 > 64 and E % 256 == 1
        assert len(per_pair) == 55 and per_pair.min() > 200    # all pairs among the 11 free poses, hundreds of edges each
        assert inc.min() > 40 * 64                             # more than 40 lane strides of every incidence list
        assert pairs == set((a, b) for a in range(K) for b in range(K) if a != b)
    if name == "edges:256":                                    # an exactly full block
        assert K == 20 and E == 256
    if name == "edges:257":                                    # a full block and one lane
        assert K == 20 and (E + 255) // 256 == 2 and E % 256 == 1
    if kind == "sparse1024":
        assert K == 1024 and sorted(np.flatnonzero(inc).tolist()) == pc.SPARSE_NODES and E == 11
        assert sc["fixed"][0] and sc["fixed"][700] and inc[700] == 0 and sc["fixed"].sum() == 2 and int(free.sum()) == 9
        assert np.max(np.abs(np.linalg.norm(start[:, :4], axis=1) - 1.0)) <= 1e-15
        assert len(np.unique(start[:, :4], axis=0)) == K       # every pose its own quaternion: a copy from the wrong row shows
        for k in (1, 64, 256, 1023):                           # one pose per block of k_pg_candidate, and lanes 0, 1, 63 of the k += 64 loops
            assert not np.array_equal(qr["poses"][k], start[k])
        assert qr["termination"] == pg.CONVERGENCE and qr["final_cost"] < 0.1 * qr["initial_cost"]
    if kind == "far":
        # the margins: a later edit to the scenes cannot move the case to another exit without this failing
        assert qr["reason"] == "parameter tolerance" and qr["iterations"] >= 2
        for res in (qr, ch):
            last, before = res["trace"]["steps"][-1], res["trace"]["steps"][-2]
            assert last["decision"] == "converged" and before["decision"] == "accepted"
            assert before["parameter_ratio"] >= 5.0 and last["parameter_ratio"] <= 1.0 / 5.0
            assert last["function_ratio"] > 5.0              # the function test would not have fired: only the parameter test can
        plain = pc.make_scene(9, pc.chain(9), pc.FAR_SEED)
        assert np.array_equal(sc["poses"][:, :4], plain["poses"][:, :4]) and np.array_equal(sc["edge_meas"], plain["edge_meas"])
        assert np.all(sc["poses"][:, 4:] - plain["poses"][:, 4:] == pc.FAR_OFFSET)
    elif qr["termination"] == pg.CONVERGENCE and steps:        # every other converging case ends by the function test, with the
        assert qr["reason"] == "function tolerance"            # parameter test far from firing
        assert steps[-1]["function_ratio"] <= 1.0 and steps[-1]["parameter_ratio"] > 5.0
    if kind == "zero_start":
        r = pg.residuals(start, sc["edge_a"], sc["edge_b"], sc["edge_meas"])
        assert r.shape == (4, 6) and np.all(r == 0.0)
        assert qr["termination"] == pg.CONVERGENCE and qr["iterations"] == 0 and qr["reason"] == "gradient tolerance"
        assert qr["initial_cost"] == 0.0 and qr["final_cost"] == 0.0 and qr["gradient_max_norm"] == 0.0
        assert qr["poses"].tobytes() == start.tobytes() and ch["poses"].tobytes() == start.tobytes() and free.sum() == 4
    if kind == "neg_meas":
        plain = dict(sc, edge_meas=sc["edge_meas"].copy())
        plain["edge_meas"][pc.NEG_MEAS_EDGES, :4] *= -1.0
        assert E == 6 and len(pc.NEG_MEAS_EDGES) == 3 and sc["sqrt_info"] is None
        assert np.array_equal(plain["edge_meas"], pc.make_scene(6, pc.chain(6, 2), 33)["edge_meas"])
        r0 = pg.residuals(start, sc["edge_a"], sc["edge_b"], sc["edge_meas"])
        r1 = pg.residuals(start, sc["edge_a"], sc["edge_b"], plain["edge_meas"])
        flip = np.ones((E, 6))
        flip[pc.NEG_MEAS_EDGES, 3:] = -1.0                     # vec(delta) turns round, the position part stays
        assert np.array_equal(r0, flip * r1) and np.min(np.abs(r1[pc.NEG_MEAS_EDGES, 3:])) > 0.0
        for solver, res in (("qr", qr), ("chol", ch)):         # squares and products of two flipped quantities: the same bits
            other = pc.solve(plain, solver)
            assert other["poses"].tobytes() == res["poses"].tobytes() and other["iterations"] == res["iterations"]
            assert other["initial_cost"] == res["initial_cost"] and other["final_cost"] == res["final_cost"]
    if kind in ("info_dense", "info_dense_dropped"):
        W = sc["sqrt_info"]
        assert W.shape == (E, 6, 6) and E == (8 if kind == "info_dense" else 7)
        live = [e for e in range(E) if e != 2 and not (kind == "info_dense" and e == E - 1)]
        assert np.min(np.abs(np.tril(W[live], -1)[:, np.tril_indices(6, -1)[0], np.tril_indices(6, -1)[1]])) > 0.0
        assert np.max(np.abs(np.tril(W, -1))) > 0.2 and np.max(np.abs(np.triu(W, 1))) > 0.2
        d = W[live][:, np.arange(6), np.arange(6)]
        assert np.all((np.abs(d) >= 0.5) & (np.abs(d) <= 2.0)) and np.any(d < 0.0) and np.any(d > 0.0)
        assert np.all(W[2, 3:] == 0.0) and np.all(W[2, :3] != 0.0)           # a position-only edge
        if kind == "info_dense":
            assert np.all(W[E - 1] == 0.0)                                     # an edge without weight
            other = pc.reference("info_dense_dropped")
            assert np.array_equal(W[:-1], other[0]["sqrt_info"]) and np.array_equal(sc["poses"], other[0]["poses"])
            assert pc.same_rotation_distance(qr["poses"], other[1]["poses"]) <= 1e-12
            assert qr["iterations"] == other[1]["iterations"]
    if kind == "rejected":
        cap = int(rest[3:])
        assert sc["max_iterations"] == cap and np.array_equal(start, pc.scene("rejected")["poses"])
        for res in (qr, ch):                                   # four rejected steps, then accepted ones: a cap of 2 to 4 arrives
            want = (["rejected"] * 4 + ["accepted"] * 4)[:cap]  # while the Jacobians are not re-evaluated
            assert _decisions(res) == want
            assert res["termination"] == pg.NO_CONVERGENCE and res["reason"] == "max iterations" and res["iterations"] == cap
            assert (res["poses"].tobytes() == start.tobytes()) == (cap <= 4)
            assert (res["final_cost"] == res["initial_cost"]) == (cap <= 4)
        if cap == 5:
            assert np.max(np.abs(qr["poses"] - start)) > 1e-3


def test_the_uncapped_rejected_scene_passes_the_batch_boundaries():
    """the caps of EDGES cut a run that goes on: without a cap it rejects iterations 1 to 4, accepts from 5 on and converges
    after more than two batches of four"""
    sc, qr, ch, dist = pc.reference("rejected")
    for res in (qr, ch):
        assert [s["decision"] for s in res["trace"]["steps"]][:8] == ["rejected"] * 4 + ["accepted"] * 4
        assert res["iterations"] > 8 and res["termination"] == pg.CONVERGENCE


def test_the_step_trace_adds_to_the_old_one():
    """one entry per iteration; the counters the first tests use are what they were"""
    for name in pc.ALL:
        qr = pc.reference(name)[1]
        tr = qr["trace"]
        assert sorted(tr) == ["accepted_after_rejected", "dbl_max", "free_poses", "invalid", "rejected", "steps"]
        assert len(tr["steps"]) == qr["iterations"]
        assert [s["decision"] for s in tr["steps"]].count("rejected") == tr["rejected"]
        ended = qr["reason"] in ("parameter tolerance", "function tolerance")
        assert [s["decision"] for s in tr["steps"]].count("converged") == int(ended)
        if ended:
            last = tr["steps"][-1]
            assert last["decision"] == "converged"
            assert (last["parameter_ratio"] <= 1.0) == (qr["reason"] == "parameter tolerance")
            assert qr["reason"] == "parameter tolerance" or last["function_ratio"] <= 1.0
