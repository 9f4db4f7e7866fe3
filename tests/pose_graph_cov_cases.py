"""The scenes of the tests of mslam_hip_pose_graph_covariance: those of tests/pose_graph_cases.py and
tests/pose_graph_sparse_cases.py by their names there, and three of its own:

  complete:44, complete:45   the whole triangle; column 0 of the envelope has 42 / 43 rows, so the 6 x rows items of
                             k_pgs_selinv's first step are 252 / 258: either side of one pass of its 256 threads.  Both are
                             NATURAL with 946 / 990 blocks;
  zero_info                  a chain whose last pose's only edge has sqrt_info = 0: that pose's diagonal block of J^T J is
                             exactly 0 and the pivot test fires, whatever the rounding.

and their references (tests/pose_graph_cov_ref.py), computed once per process.  This is test infrastructure like
pose_graph_cases.py (not a conftest.py, not under oracle/)."""
import functools

import numpy as np

import pose_graph_cases as pc
import pose_graph_cov_ref as cr
import pose_graph_sparse_cases as psc
import pose_graph_sparse_ref as ps

# the cases under the tolerance rule, at the scene's start and at the solve's result
CASES = ["pair", "chain:9", "chain:17", "duplicates", "star70", "isolated_fixed_middle", "rot170", "info_upper", "info_dense",
         "edges:257", "sparse1024", "loops:65", "loops:258", "revisit200", "complete40", "complete:44", "complete:45", "info65"]
RANK = ["two_components", "pair_component", "zero_info"]     # MSLAM_HIP_E_NO_MODEL
RCM = ["star70", "edges:257", "revisit200"]                  # the cases whose chosen order is reverse Cuthill-McKee
BIG = "loops:16384"
_SPARSE_KINDS = ("loops", "revisit200", "complete40", "pair_component", "info65")


def scene(name):
    kind, _, rest = name.partition(":")
    if kind == "complete":
        K = int(rest)
        return pc.make_scene(K, psc.complete(K), 900 + K)
    if kind == "zero_info":
        sc = pc.make_scene(6, pc.chain(6, 0), 61)
        sc["sqrt_info"] = np.tile(np.eye(6), (len(sc["edge_a"]), 1, 1))
        sc["sqrt_info"][-1] = 0.0       # the edge (4, 5), pose 5's only one
        return sc
    return psc.scene(name) if kind in _SPARSE_KINDS else pc.scene(name)


def analysis(sc):
    return ps.analyze(sc["fixed"], len(sc["poses"]), sc["edge_a"], sc["edge_b"])


def reference_at(sc, poses, loss=None):
    """-> dict(prob, sigma (the QR reference), d, bound, cov, cross, poses_of, pairs) at `poses`"""
    prob = cr.problem(sc, loss)
    s_qr, _, d = cr.dense_pair(cr.jacobian(prob, poses))
    poses_of, pairs = cr.requests(sc)
    cov, cross = cr.expected(s_qr, prob, poses_of, pairs)
    return dict(prob=prob, sigma=s_qr, d=d, bound=cr.bound(d, float(np.max(np.abs(s_qr)))), cov=cov, cross=cross, poses_of=poses_of,
                pairs=pairs)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (scene, reference_at the scene's start).  Computed once and shared: do not write into what this returns"""
    sc = scene(name)
    return sc, reference_at(sc, sc["poses"])


# loops:16384 = chain(16384, 2): the loop edges are (16383, 0) and (16380, 1), pose 0 is constant.  The 0-side ends of both
# loop edges, their other ends, a neighbour of each, the middle
BIG_POSES = [0, 1, 2, 8191, 8192, 16380, 16382, 16383]
BIG_PAIRS = [(16383, 0), (0, 16383), (16380, 1), (1, 16380)]


@functools.lru_cache(maxsize=None)
def big_reference():
    """-> (scene, cov [8, 6, 6], cross [4, 6, 6], d, bound): the splu solves of BIG_POSES; d is their distance from the
    restated recursion over the requested blocks, relative to the largest entry of the solved columns"""
    sc = scene(BIG)
    prob = cr.problem(sc, sparse=True)
    J = cr.jacobian(prob, sc["poses"])
    cols = cr.splu_columns(J, prob, [k for k in BIG_POSES if prob.col[k] >= 0])
    an = analysis(sc)
    Z = cr.selected_inverse(J.T @ J, prob, an)

    def from_cols(a, b):
        if prob.col[a] < 0 or prob.col[b] < 0:
            return np.zeros((6, 6))
        return cols[b][prob.col[a]:prob.col[a] + 6, :]
    cov = np.array([from_cols(k, k) for k in BIG_POSES])
    cross = np.array([from_cols(a, b) for a, b in BIG_PAIRS])
    rec = np.concatenate([[cr.envelope_block(Z, an, prob, k, k) for k in BIG_POSES],
                          [cr.envelope_block(Z, an, prob, a, b) for a, b in BIG_PAIRS]])
    top = max(float(np.max(np.abs(c))) for c in cols.values())
    d = float(np.max(np.abs(rec - np.concatenate([cov, cross])))) / top
    return sc, cov, cross, d, cr.bound(d, top)
