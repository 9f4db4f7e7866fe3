"""The scenes of the SPARSE pose-graph solver's tests beyond tests/pose_graph_cases.py: the envelope's edges (row widths at
wave and workgroup boundaries, a reverse Cuthill-McKee order with transposed blocks, a full triangle, components, a constant
pose inside a chain), the sizes beyond the dense solver's cap, the graphs of the ordering table of include/mslam_hip.h's rule,
and their reference solutions by the two sparse CPU solvers of tests/pose_graph_sparse_ref.py, solved once per process.
Every scene holds pose 0 constant unless it says otherwise.  This is test infrastructure like pose_graph_cases.py (not a
conftest.py, not under oracle/)."""
import functools
import hashlib
import os

import numpy as np

import pose_graph_cases as pc
import pose_graph_sparse_ref as ps


def band(K, width):
    """(k, k + 1) .. (k, k + width) for every k"""
    return [(k, k + d) for k in range(K) for d in range(1, width + 1) if k + d < K]


def revisit(K, width, n):
    """a band of `width` over K poses and the way back over the first n: (K - 1 - i, i + c) for i < n, c < 2"""
    return band(K, width) + [(K - 1 - i, i + c) for i in range(n) for c in range(2)]


def complete(K):
    return [(j, i) for i in range(K) for j in range(i + 1, K)]


def identity_scene(K, edges, fixed=(0,)):
    """every pose and measurement the identity: for the calls that end before any arithmetic (capacity, the size checks)"""
    e = np.array(edges, np.int32).reshape(-1, 2)
    unit = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
    fx = np.zeros(K, np.uint8)
    fx[list(fixed)] = 1
    return dict(poses=np.tile(unit, (K, 1)), fixed=fx, edge_a=e[:, 0].copy(), edge_b=e[:, 1].copy(), edge_meas=np.tile(unit, (len(e), 1)),
                sqrt_info=None)


# the graphs of the ordering table: name -> (K, edges, NATURAL blocks, RCM blocks, chosen or None for E_CAPACITY)
def table():
    return {
        "chain1025": (1025, pc.chain(1025), 2047, 2047, ps.NATURAL),
        "chain16384": (16384, pc.chain(16384), 32765, 32765, ps.NATURAL),
        "sparse1024": (1024, pc.SPARSE_EDGES, 21, 24, ps.NATURAL),
        "revisit200": (200, revisit(200, 2, 60), 8873, 984, ps.RCM),
        "revisit3000": (3000, revisit(3000, 3, 1200), 2168389, 20970, ps.RCM),
        "random2048": (2048, pc.random_pairs(2048, 20000, 5), 1892011, 1704117, None),
    }


LOOP_WIDTHS = [64, 65, 66, 257, 258]   # chain(K, loops = 2): the second loop edge (K - 4, 1) makes row K - 5 K - 4 blocks wide
ENVELOPE = ["chain2"] + ["loops:%d" % K for K in LOOP_WIDTHS] + ["revisit200", "complete40", "pair_component", "fixed_middle", "info65"]
BEYOND = ["loops:1025", "loops:16384", "noisy16384:cap2"]


def scene(name):
    kind, _, rest = name.partition(":")
    if kind == "chain2":               # one free pose: a 1 x 1 envelope
        return pc.make_scene(2, pc.chain(2), 41)
    if kind == "loops":                # loops:K -> chain(K, loops = 2)
        K = int(rest)
        # at 16384 poses the default measurement noise leaves the chain at the iteration cap after 100 slow iterations; with
        # exact measurements the minimum is the truth at cost 0 and the solve converges in about 15
        return pc.make_scene(K, pc.chain(K, 2), 50 + K % 1000, **(dict(noise=0.0) if K >= 4096 else {}))
    if kind == "noisy16384":           # noisy16384:capN -> chain(16384, loops = 2) with the default noise under a cap of N
        return dict(pc.make_scene(16384, pc.chain(16384, 2), 435), max_iterations=int(rest[3:]))
    if kind == "revisit200":           # RCM is chosen: blocks are written transposed
        return pc.make_scene(200, revisit(200, 2, 60), 42)
    if kind == "revisit3000":
        return pc.make_scene(3000, revisit(3000, 3, 1200), 43)
    if kind == "complete40":           # the envelope is the whole triangle
        return pc.make_scene(40, complete(40), 44)
    if kind == "pair_component":       # 0-1-2-3-4 with the constant pose 0, and the pair 5-6 on its own: its gauge is free
        return pc.make_scene(7, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0), (5, 6)], 45)
    if kind == "fixed_middle":         # pose 4 of a chain of 9 is constant as well: two runs of free poses
        return pc.make_scene(9, pc.chain(9), 46, fixed=(0, 4))
    if kind == "info65":               # full sqrt_info on the K = 65 chain
        sc = pc.make_scene(65, pc.chain(65, 2), 47)
        sc["sqrt_info"] = pc.dense_info(len(sc["edge_a"]), 48)
        return sc
    raise KeyError(name)


# The two CPU solves of loops:16384 take a quarter of a minute, so their results are recorded under tests/golden/ (the normal
# solution, the distance of the two, the summaries) with a digest of the scene they belong to; a scene that no longer matches
# the digest is solved afresh.  `python tests/pose_graph_sparse_cases.py` writes the file.
RECORDED = {"loops:16384": os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_graph_sparse_loops16384.npz")}
_SUMMARY = ("termination", "iterations", "initial_cost", "final_cost")


def _digest(sc):
    h = hashlib.sha256()
    for k in ("poses", "fixed", "edge_a", "edge_b", "edge_meas"):
        h.update(np.ascontiguousarray(sc[k]).tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def _recorded(name, sc):
    path = RECORDED.get(name)
    if path is None or not os.path.exists(path):
        return None
    with np.load(path) as z:
        if not np.array_equal(z["digest"], _digest(sc)):
            return None
        a = dict(poses=z["poses"], trace=dict(rejected=int(z["rejected"][0])), **{k: z["normal"][i] for i, k in enumerate(_SUMMARY)})
        b = dict(poses=None, trace=dict(rejected=int(z["rejected"][1])), **{k: z["augmented"][i] for i, k in enumerate(_SUMMARY)})
        for r in (a, b):
            r["termination"], r["iterations"] = int(r["termination"]), int(r["iterations"])
        return a, b, float(z["dist"])


def record(name):
    sc = scene(name)
    a, b, dist = ps.solve_pair(sc)
    np.savez_compressed(RECORDED[name], digest=_digest(sc), poses=a["poses"], dist=np.float64(dist),
             normal=np.array([a[k] for k in _SUMMARY], np.float64), augmented=np.array([b[k] for k in _SUMMARY], np.float64),
             rejected=np.array([a["trace"]["rejected"], b["trace"]["rejected"]], np.int64))
    return a, b, dist


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (scene, normal solution, augmented solution, |x_augmented - x_normal|_inf up to the quaternions' signs); of a
    recorded case the augmented solution has its summary only (poses None)"""
    sc = scene(name)
    return (sc,) + (_recorded(name, sc) or ps.solve_pair(sc))


if __name__ == "__main__":
    for name in RECORDED:
        a, b, dist = record(name)
        print(name, [a[k] for k in _SUMMARY], [b[k] for k in _SUMMARY], dist)
