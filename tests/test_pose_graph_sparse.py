"""The SPARSE pose-graph solver's CPU side: tests/pose_graph_sparse_ref.py (the Levenberg-Marquardt loop on a scipy.sparse
Jacobian, two sparse linear solvers) pinned to tests/pose_graph_ref.py on every case of pose_graph_cases.ALL, and the
symbolic phase of the library (pose_graph_analyze: no context, no GPU) pinned to the ordering rule restated in plain Python:
the six graphs of the ordering table with their envelope sizes, the edge cases of the rule, the argument errors."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_cases as pc  # noqa: E402
import pose_graph_sparse_cases as psc  # noqa: E402
import pose_graph_sparse_ref as ps  # noqa: E402


@pytest.mark.parametrize("name", pc.ALL)
def test_sparse_reference_is_the_dense_reference(name):
    """the same termination, iteration count and per-iteration decisions; poses within max(1e-9, 1000 x the distance of the two
    dense CPU solvers) of the QR solve"""
    sc, qr, ch, dist = pc.reference(name)
    for solver in ("normal", "augmented"):
        got = ps.solve(sc, solver)
        assert got["termination"] == qr["termination"] and got["iterations"] == qr["iterations"], solver
        assert [s["decision"] for s in got["trace"]["steps"]] == [s["decision"] for s in qr["trace"]["steps"]], solver
        for k in ("rejected", "invalid", "dbl_max", "free_poses"):
            assert got["trace"][k] == qr["trace"][k], (solver, k)
        assert pc.same_rotation_distance(got["poses"], qr["poses"]) <= max(1e-9, 1000.0 * dist), solver
        assert abs(got["initial_cost"] - qr["initial_cost"]) <= 1e-12 * qr["initial_cost"]


def _fixed0(K):
    fx = np.zeros(K, np.uint8)
    if K:
        fx[0] = 1
    return fx


def _same_analysis(pkg, fixed, K, edges):
    e = np.array(edges, np.int32).reshape(-1, 2)
    got, want = pkg.pose_graph_analyze(fixed, K, e[:, 0], e[:, 1]), ps.analyze(fixed, K, e[:, 0], e[:, 1])
    assert got["n_free"] == want["n_free"] and got["ordering"] == want["ordering"]
    assert got["envelope_blocks"] == want["envelope_blocks"] and got["fits"] == want["fits"]
    assert got["order"].tolist() == want["order"].tolist() and got["first"].tolist() == want["first"].tolist()
    return got, want


@pytest.mark.parametrize("name", ["chain1025", "chain16384", "sparse1024", "revisit200", "revisit3000", "random2048"])
def test_ordering_table(pkg, name):
    K, edges, natural, rcm, chosen = psc.table()[name]
    got, want = _same_analysis(pkg, _fixed0(K), K, edges)
    assert (want["natural_blocks"], want["rcm_blocks"]) == (natural, rcm)
    if chosen is None:                                        # neither order fits: E_CAPACITY
        assert not got["fits"] and min(natural, rcm) > pkg.POSE_GRAPH_MAX_ENVELOPE_BLOCKS
        assert got["envelope_blocks"] == min(natural, rcm)
    else:
        assert got["fits"] and got["ordering"] == chosen
        assert got["envelope_blocks"] == (rcm if chosen == ps.RCM else natural)
    if name == "revisit3000":                                 # fits only under RCM
        assert natural > pkg.POSE_GRAPH_MAX_ENVELOPE_BLOCKS >= rcm


def test_ordering_edge_cases(pkg):
    # two components, the second a ring without a constant pose; the component of least degree starts
    got, _ = _same_analysis(pkg, _fixed0(7), 7, [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 4)])
    assert got["n_free"] == 6 and sorted(got["order"].tolist()) == [1, 2, 3, 4, 5, 6]
    # a constant pose in the middle of a chain: two runs, no block joins them
    fx = _fixed0(9)
    fx[4] = 1
    got, _ = _same_analysis(pkg, fx, 9, pc.chain(9, 0))
    assert got["order"].tolist() == [1, 2, 3, 5, 6, 7, 8] and got["first"].tolist() == [0, 0, 1, 3, 3, 4, 5]
    assert got["envelope_blocks"] == 12 and got["ordering"] == ps.NATURAL
    # every pose constant; no edge at all; K = 0
    got, _ = _same_analysis(pkg, np.ones(4, np.uint8), 4, pc.chain(4))
    assert got["n_free"] == 0 and got["envelope_blocks"] == 0 and len(got["order"]) == 0 and got["fits"]
    got, _ = _same_analysis(pkg, _fixed0(3), 3, [])
    assert got["n_free"] == 0 and got["envelope_blocks"] == 0
    got, _ = _same_analysis(pkg, None, 0, [])
    assert got["n_free"] == 0
    # a duplicate edge and both directions count once: degrees, order and envelope are those of the plain path
    plain, _ = _same_analysis(pkg, _fixed0(5), 5, [(0, 1), (1, 2), (2, 3), (3, 4)])
    twice, _ = _same_analysis(pkg, _fixed0(5), 5, [(0, 1), (1, 2), (1, 2), (2, 1), (2, 3), (3, 4), (3, 4)])
    assert plain["order"].tolist() == twice["order"].tolist() and plain["envelope_blocks"] == twice["envelope_blocks"] == 7
    # an edge to a constant pose joins nothing: 1 and 3 are both tied to pose 0 only
    got, _ = _same_analysis(pkg, _fixed0(4), 4, [(0, 1), (0, 3), (3, 0)])
    assert got["order"].tolist() == [1, 3] and got["first"].tolist() == [0, 1] and got["envelope_blocks"] == 2
    # fixed = None: no constant pose; a pose without an edge is no node
    got, _ = _same_analysis(pkg, None, 5, [(0, 1), (1, 3)])
    assert got["order"].tolist() == [0, 1, 3]
    # a star whose hub has the largest index: NATURAL keeps the hub last (7 blocks + 4 diagonals), and RCM cannot do better
    got, want = _same_analysis(pkg, None, 5, [(4, 0), (4, 1), (4, 2), (4, 3)])
    assert got["ordering"] == ps.NATURAL and want["natural_blocks"] == 9 and want["rcm_blocks"] >= 9
    # the hub first: NATURAL fills every row back to column 0; RCM starts at leaf 1, visits 1, 0, 2, 3, 4 and reverses
    got, want = _same_analysis(pkg, None, 5, [(0, 1), (0, 2), (0, 3), (0, 4)])
    assert got["ordering"] == ps.RCM and want["natural_blocks"] == 15 and got["envelope_blocks"] == 9
    assert got["order"].tolist() == [4, 3, 2, 0, 1] and got["first"].tolist() == [0, 1, 2, 0, 3]


def test_analyze_argument_errors(pkg):
    ok = pkg.pose_graph_analyze(None, 3, [0, 1], [1, 2])
    assert ok["n_free"] == 3 and ok["envelope_blocks"] == 5
    big = pkg.POSE_GRAPH_MAX_EDGES + 1
    for K, ea, eb in ((3, [0, 3], [1, 2]), (3, [0, 1], [1, -1]), (3, [0, 2], [1, 2]), (-1, [], []),
                      (pkg.POSE_GRAPH_MAX_KEYFRAMES_SPARSE + 1, [0], [1]), (2, np.zeros(big, np.int32), np.ones(big, np.int32)),
                      (3, [0, 1], [1])):
        with pytest.raises(pkg.MslamHipError) as e:
            pkg.pose_graph_analyze(None, K, ea, eb)
        assert e.value.code == pkg.E_INVALID, (K, len(ea))
    with pytest.raises(pkg.MslamHipError) as e:
        pkg.pose_graph_analyze(np.zeros(4, np.uint8), 3, [0], [1])
    assert e.value.code == pkg.E_INVALID
    assert pkg.pose_graph_analyze(None, pkg.POSE_GRAPH_MAX_KEYFRAMES_SPARSE, [0], [pkg.POSE_GRAPH_MAX_KEYFRAMES_SPARSE - 1])["n_free"] == 2
    assert pkg.POSE_GRAPH_MAX_KEYFRAMES_SPARSE == 16384 and pkg.POSE_GRAPH_MAX_ENVELOPE_BLOCKS == 1048576
    assert (pkg.PG_SOLVER_DENSE, pkg.PG_SOLVER_SPARSE) == (0, 1)


def test_recorded_reference_belongs_to_its_scene():
    """the recorded solves of the 16384-pose chain carry the digest of the scene this tree builds"""
    sc = psc.scene("loops:16384")
    rec = psc._recorded("loops:16384", sc)
    assert rec is not None
    a, b, dist = rec
    assert a["termination"] == b["termination"] == 0 and a["iterations"] == b["iterations"] and dist < 1e-9
    # exact measurements: the minimum is the truth
    assert pc.same_rotation_distance(a["poses"], sc["truth_poses"]) <= 1e-6
