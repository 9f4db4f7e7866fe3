"""The scenes of the pose graph's PCG tests (mslam_hip_set_pose_graph_pcg) beyond tests/pose_graph_cases.py and
tests/pose_graph_sparse_cases.py, and the CPU references they are compared with, solved once per process:

  walk:K      band(K, 2) plus K random pairs, deduplicated: a trajectory that keeps meeting its own past, the sparsity of a
              covisibility graph on a map that revisits its ground.  walk0:K: the same with exact measurements, so the truth
              is the minimum.
  complete:K  every pair: rows of K - 1 blocks in k_pcg_product.
  random2048  the graph of pose_graph_sparse_cases.table() that neither DENSE (K > 1024) nor SPARSE (1704117 envelope blocks
              in the better order) takes.
  chain:K and every other name: pose_graph_cases.scene / pose_graph_sparse_cases.scene.

direct(name) is the pair of direct CPU solves and their distance (QR / Cholesky of pose_graph_ref for pose_graph_cases.ALL, the
two sparse LU solves of pose_graph_sparse_ref otherwise); pcg(name, tier) is tests/pose_graph_pcg_ref.py's solve.  No PCG
reference takes more than four seconds (random2048 3.4 s, walk0:2800 2.3 s at the tight tier), so none is recorded under
tests/golden/; the direct solves of walk:1025 / 1026 take 40 s each and no test asks for them.  This is test infrastructure (not a conftest.py, not under oracle/)."""
import functools

import numpy as np

import pose_graph_cases as pc
import pose_graph_pcg_ref as pr
import pose_graph_sparse_cases as psc
import pose_graph_sparse_ref as ps

DEFAULT = (pr.MAX_ITERATIONS, pr.TOLERANCE)
TIGHT = pr.TIGHT

# the CPU PCG reference ends solves at the cap on these two even at (2000, 1e-12) (loops:258: 7 of 9), so its decisions are
# not the direct solver's to the last bit and the tight tier's rule does not hold for them; loops:258 is the at-the-cap test
AT_CAP = ("loops:257", "loops:258")
TIGHT_TIER = [n for n in pc.ALL + psc.ENVELOPE if n not in AT_CAP]
DEFAULT_TIER = ["chain:17", "loops:66", "complete40", "walk:130", "walk:400"]
SHAPES = ["chain:43", "chain:44", "chain:45", "chain:46", "complete:10", "complete:11", "complete:12", "duplicates"]
PARTIALS = ["walk:1025", "walk:1026"]     # 1024 and 1025 free poses: 256 and 257 workgroups of k_pcg_product (4 block rows each),
                                          # so 256 and 257 partial sums of p . q; 24 and 25 of the 256-entry vector kernels
WALK0_K = 2800


def walk_edges(K, seed):
    """band(K, 2) and K random pairs, every unordered pair once"""
    seen, out = set(), []
    for a, b in psc.band(K, 2) + pc.random_pairs(K, K, seed):
        key = (min(a, b), max(a, b))
        if key not in seen:
            seen.add(key)
            out.append((a, b))
    return out


def scene(name):
    kind, _, rest = name.partition(":")
    if kind in ("walk", "walk0"):
        K = int(rest)
        return pc.make_scene(K, walk_edges(K, 700 + K % 1000), 800 + K % 1000, **(dict(noise=0.0) if kind == "walk0" else {}))
    if kind == "complete":
        K = int(rest)
        return pc.make_scene(K, psc.complete(K), 900 + K)
    if kind == "random2048":
        K, edges = psc.table()["random2048"][:2]
        return pc.make_scene(K, edges, 61)
    try:
        return pc.scene(name)
    except KeyError:
        return psc.scene(name)


def envelope(sc):
    """-> (NATURAL blocks, RCM blocks) by the restated ordering rule"""
    an = ps.analyze(sc["fixed"], len(sc["poses"]), sc["edge_a"], sc["edge_b"])
    return an["natural_blocks"], an["rcm_blocks"]


@functools.lru_cache(maxsize=None)
def direct(name):
    """-> (scene, a direct solution, the other direct solution, their distance)"""
    if name in pc.ALL:
        return pc.reference(name)
    if name in psc.ENVELOPE:
        return psc.reference(name)
    sc = scene(name)
    return (sc,) + ps.solve_pair(sc)


@functools.lru_cache(maxsize=None)
def pcg(name, tier=DEFAULT):
    """-> (scene, the CPU PCG reference at tier = (max_iterations, tolerance))"""
    sc = scene(name)
    return sc, pr.solve(sc, cg_max_iterations=tier[0], cg_tolerance=tier[1])


def distance(name, tier):
    """the CPU PCG reference's distance to the direct solution"""
    return pc.same_rotation_distance(pcg(name, tier)[1]["poses"], direct(name)[1]["poses"])

