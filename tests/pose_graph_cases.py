"""The pose-graph scenes the tests of mslam_hip_pose_graph share, their reference solutions (tests/pose_graph_ref.py), solved
once per process, and the scene file `mslam_harness --pose-graph` reads.  tests/test_pose_graph.py shows on the CPU that
every named case takes the path it is named for.

A scene: K truth poses with positions in [-2, 2]^3 and random orientations, edges whose measurements are the truth's relative
poses with a little noise, and a start that is the truth moved per free pose (Plus with a tangent of length `angle`, a shift
of `shift` m).  So |p_b - p_a| <= 4 sqrt(3) < 7 m at the truth and below 8 m at every point a solve visits (`far` adds one
offset to every position, which leaves the differences where they were).  ALL are the cases of the first tests; EDGES, of
tests/test_pose_graph_edges.py and tests/test_gpu_pose_graph_edges.py, reach the index ranges and branches ALL leaves out.
This is test infrastructure like ba_cases.py (not a conftest.py, not under oracle/)."""
import functools

import numpy as np

import pose_graph_ref as pg
from ba_ref import quaternion_plus, random_rotation_quaternion


def _truth(K, rng):
    tp = np.zeros((K, 7))
    for k in range(K):
        tp[k, :4] = random_rotation_quaternion(rng, rng.uniform(0.0, np.pi))
        tp[k, 4:] = rng.uniform(-2.0, 2.0, 3)
    return tp


def _perturb(T, rng, angle, shift):
    d, s = rng.normal(size=3), rng.normal(size=3)
    q = quaternion_plus(T[:4], angle * d / np.linalg.norm(d))
    return np.concatenate([q / np.linalg.norm(q), T[4:] + shift * s / np.linalg.norm(s)])


def make_scene(K, edges, seed, fixed=(0,), noise=0.01, angle=0.05, shift=0.1, truth=None):
    """edges: list of (a, b).  -> dict(truth_poses, poses, fixed, edge_a, edge_b, edge_meas, sqrt_info=None)"""
    rng = np.random.default_rng(seed)
    tp = _truth(K, rng) if truth is None else truth
    fx = np.zeros(K, np.uint8)
    fx[list(fixed)] = 1
    meas = np.array([_perturb(pg.relative(tp[a], tp[b]), rng, noise, noise) if noise else pg.relative(tp[a], tp[b])
                     for a, b in edges]).reshape(-1, 7)
    sp = np.array([tp[k] if fx[k] else _perturb(tp[k], rng, angle, shift) for k in range(K)]).reshape(-1, 7)
    e = np.array(edges, np.int32).reshape(-1, 2)
    return dict(truth_poses=tp, poses=sp, fixed=fx, edge_a=e[:, 0].copy(), edge_b=e[:, 1].copy(), edge_meas=meas, sqrt_info=None)


def chain(K, loops=1):
    """odometry 0-1-...-(K-1) and `loops` loop edges back towards the start"""
    return [(k, k + 1) for k in range(K - 1)] + [(K - 1 - 3 * i, i) for i in range(loops) if K - 1 - 3 * i > i + 1]


def upper_info(E, seed):
    """upper-triangular sqrt_info with a diagonal in [0.5, 2] and off-diagonal entries in [-0.3, 0.3]"""
    rng = np.random.default_rng(seed)
    W = np.triu(rng.uniform(-0.3, 0.3, (E, 6, 6)), 1)
    W[:, np.arange(6), np.arange(6)] = rng.uniform(0.5, 2.0, (E, 6))
    return W


def dense_info(E, seed):
    """full sqrt_info: off-diagonal entries in [-0.3, 0.3] above and below the diagonal, a diagonal of magnitude in [0.5, 2]
    with random signs; edge 2 has rows 3 to 5 zero (it weighs the position only), the last edge's matrix is zero"""
    rng = np.random.default_rng(seed)
    W = rng.uniform(-0.3, 0.3, (E, 6, 6))
    W[:, np.arange(6), np.arange(6)] = rng.uniform(0.5, 2.0, (E, 6)) * rng.choice([-1.0, 1.0], (E, 6))
    W[2, 3:, :] = 0.0
    W[E - 1] = 0.0
    return W


def random_pairs(K, E, seed):
    """E ordered pairs (a, b), a != b, uniform over the K (K - 1) of them: both directions of every pair of poses"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, K, E)
    b = (a + rng.integers(1, K, E)) % K
    return list(zip(a.tolist(), b.tolist()))


SPARSE_NODES = [0, 1, 63, 64, 65, 255, 256, 511, 1022, 1023]
SPARSE_EDGES = list(zip(SPARSE_NODES[:-1], SPARSE_NODES[1:])) + [(1023, 0), (511, 63)]
FAR_SEED, FAR_OFFSET = 19, 5e4
NEG_MEAS_EDGES = [1, 3, 5]   # two odometry edges and the loop edge


def drift_scene(N=39, seed=3, step_noise=0.05, angle_noise=0.03):
    """a walk of N + 1 keyframes: odometry edges with an error per step (so the chained start drifts) and one exact loop
    edge from the first to the last keyframe.  The start is the chained odometry; pose 0 is constant."""
    rng = np.random.default_rng(seed)
    tp = np.zeros((N + 1, 7))
    tp[0, 3] = 1.0
    for k in range(N):
        step = np.concatenate([random_rotation_quaternion(rng, 0.15), [0.25, 0.0, 0.02] + 0.01 * rng.normal(size=3)])
        tp[k + 1] = pg.compose(tp[k], step)
    edges = [(k, k + 1) for k in range(N)]
    meas = [_perturb(pg.relative(tp[a], tp[b]), rng, angle_noise, step_noise) for a, b in edges]
    sp = tp.copy()
    for k in range(N):
        sp[k + 1] = pg.compose(sp[k], meas[k])
    edges.append((0, N))
    meas.append(pg.relative(tp[0], tp[N]))
    e = np.array(edges, np.int32)
    fx = np.zeros(N + 1, np.uint8)
    fx[0] = 1
    return dict(truth_poses=tp, poses=sp, fixed=fx, edge_a=e[:, 0].copy(), edge_b=e[:, 1].copy(), edge_meas=np.array(meas), sqrt_info=None)


def scene(name):
    kind, _, rest = name.partition(":")
    if kind == "pair":                 # two poses, one edge, the first constant: the solution is T_0 o Z
        return make_scene(2, [(0, 1)], 1, angle=0.3, shift=0.5)
    if kind == "chain":                # chain:K -> 6 (K - 1) unknowns: 48 = one panel, 54 = a pad, 96 = two panels
        K = int(rest)
        return make_scene(K, chain(K), 10 + K)
    if kind == "star70":               # the hub (pose 0, free) has 70 edges: its incidence sum crosses a wave; leaf 1 is constant
        return make_scene(71, [(0, k) if k % 2 else (k, 0) for k in range(1, 71)], 5, fixed=(1,))
    if kind == "duplicates":           # an edge listed twice, and both directions between one pair
        return make_scene(5, [(0, 1), (1, 2), (1, 2), (2, 3), (3, 2), (3, 4), (4, 0), (0, 1)], 6)
    if kind == "two_components":       # 0-1-2-3 holds the constant pose 0; 4-5-6 has none: its gauge is free
        return make_scene(7, [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 4)], 7)
    if kind == "isolated_fixed_middle":   # pose 4 has no edge, pose 3 (in the middle of the chain) is constant as well
        return make_scene(8, [(0, 1), (1, 2), (2, 3), (3, 5), (5, 6), (6, 7), (7, 0)], 8, fixed=(0, 3))
    if kind == "all_fixed":
        return make_scene(4, chain(4), 9, fixed=(0, 1, 2, 3))
    if kind == "empty":
        return make_scene(3, [], 10)
    if kind == "rot170":               # pose 1 is pose 0 turned by 170 degrees: delta's scalar part is near 0 along the way
        sc = make_scene(4, chain(4), 11)
        tp = sc["truth_poses"].copy()
        tp[1, :4] = pg.q_mul(tp[0, :4], random_rotation_quaternion(np.random.default_rng(2), np.deg2rad(170.0)))
        return make_scene(4, chain(4), 11, truth=tp)
    if kind == "neg_q":                # a free pose and a constant one entered as -q: no sign fix, the signs are kept
        sc = make_scene(6, chain(6), 12)
        sc["poses"][2, :4] *= -1.0
        sc["poses"][0, :4] *= -1.0
        return sc
    if kind == "info_upper":
        sc = make_scene(6, chain(6, 2), 13)
        sc["sqrt_info"] = upper_info(len(sc["edge_a"]), 14)
        return sc
    if kind == "rejected":             # a start far from the truth: the reference trace shows rejected steps
        sc = make_scene(8, chain(8, 2), 4, angle=1.2, shift=2.0)
        return dict(sc, max_iterations=int(rest[3:])) if rest else sc       # rejected:capN -> the same under a cap
    if kind == "cap0":
        return dict(make_scene(6, chain(6), 15), max_iterations=0)
    if kind == "cap1":
        return dict(make_scene(6, chain(6), 15), max_iterations=1)
    if kind == "drift40":
        return drift_scene()
    if kind == "edges":                # edges:E -> E random ordered pairs a != b among few poses: whole blocks of 256 edges
        E = int(rest)
        K = 12 if E > 4096 else 20
        return make_scene(K, random_pairs(K, E, 20 + E % 1000), 21 + E % 1000)
    if kind == "sparse1024":           # the cap of K; ten poses carry edges, 700 is constant without one
        return make_scene(1024, SPARSE_EDGES, 31, fixed=(0, 700))
    if kind == "far":                  # chain:9's shape, moved away from the origin: |x| is large, the parameter test ends it
        sc = make_scene(9, chain(9), FAR_SEED)
        sc["poses"][:, 4:] += FAR_OFFSET
        sc["truth_poses"] = sc["truth_poses"] + np.concatenate([np.zeros(4), np.full(3, FAR_OFFSET)])
        return sc
    if kind == "zero_start":           # the start is the truth and the measurements are exact: every residual is exactly 0
        tp = np.zeros((5, 7))
        tp[:, 3], tp[:, 4] = 1.0, 0.5 * np.arange(5)
        sc = make_scene(5, chain(5, 0), 32, noise=0.0, truth=tp)
        sc["poses"] = tp.copy()
        return sc
    if kind == "neg_meas":             # three measurements entered as -q_meas: vec(delta) turns round on these edges
        sc = make_scene(6, chain(6, 2), 33)
        sc["edge_meas"][NEG_MEAS_EDGES, :4] *= -1.0
        return sc
    if kind in ("info_dense", "info_dense_dropped"):   # full sqrt_info, a position-only edge, an all-zero last edge (or none)
        sc = make_scene(7, chain(7, 2), 34)
        sc["sqrt_info"] = dense_info(len(sc["edge_a"]), 35)
        if kind == "info_dense_dropped":
            for key in ("edge_a", "edge_b", "edge_meas", "sqrt_info"):
                sc[key] = sc[key][:-1].copy()
        return sc
    raise KeyError(name)


ALL = ["pair", "chain:9", "chain:10", "chain:17", "star70", "duplicates", "two_components", "isolated_fixed_middle", "all_fixed",
       "empty", "rot170", "neg_q", "info_upper", "rejected", "cap0", "cap1", "drift40"]


# the second pass over the kernels' index ranges and branches: tests/test_pose_graph_edges.py shows on the CPU that each takes
# the path it is named for, tests/test_gpu_pose_graph_edges.py compares them.  ALL stays: the host-harness test runs its names.
EDGES = ["edges:16641", "edges:256", "edges:257", "sparse1024", "far", "zero_start", "neg_meas", "info_dense", "info_dense_dropped",
         "rejected:cap2", "rejected:cap3", "rejected:cap4", "rejected:cap5", "rejected:cap8"]


def solve(sc, linear_solver="qr", **kw):
    return pg.pose_graph(sc["poses"], sc["edge_a"], sc["edge_b"], sc["edge_meas"], sc["sqrt_info"], sc["fixed"],
                         sc.get("max_iterations", 100), linear_solver=linear_solver, **kw)


def same_rotation_distance(a, b):
    """|a - b|_inf over poses [K, 7] with every quaternion compared up to sign"""
    a, b = np.asarray(a, np.float64).reshape(-1, 7), np.asarray(b, np.float64).reshape(-1, 7)
    if len(a) == 0:
        return 0.0
    sign = np.where(np.sum(a[:, :4] * b[:, :4], 1) < 0.0, -1.0, 1.0)
    return float(max(np.max(np.abs(a[:, :4] - sign[:, None] * b[:, :4])), np.max(np.abs(a[:, 4:] - b[:, 4:]))))


def jacobian_row_bound(sc):
    """a bound on the largest row norm of an edge's Jacobian: the rows of [2 R^T [v]x, -R^T | 0, R^T] have norm at most
    2 |v| + 2 and those of [2 M | -2 M] norm 2 sqrt(2); |v| = |p_b - p_a| is taken at the start plus 1 m for the way to the
    solution; sqrt_info multiplies a row by at most its largest absolute row sum"""
    v = sc["poses"][sc["edge_b"], 4:] - sc["poses"][sc["edge_a"], 4:]
    extent = float(np.max(np.linalg.norm(v, axis=1), initial=0.0)) + 1.0
    w = 1.0 if sc["sqrt_info"] is None else max(1.0, float(np.max(np.sum(np.abs(sc["sqrt_info"]), 2))))
    return w * (2.0 * extent + 2.0)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (scene, qr solution, chol solution, |x_chol - x_qr|_inf up to the quaternions' signs)"""
    sc = scene(name)
    qr, ch = solve(sc, "qr"), solve(sc, "chol")
    return sc, qr, ch, same_rotation_distance(qr["poses"], ch["poses"])


def write_scene(path, sc):
    """the scene file `mslam_harness --pose-graph` reads: "MSPG", i32 version 1, K, E, max_iterations, has_info; K x i32
    keyframe id (the adapter holds keyframe id 1 constant: the constant pose, if any, must be the first); K x 7 f64; E x i32 a;
    E x i32 b; E x 7 f64 measurement; has_info: E x 36 f64"""
    K, E = len(sc["poses"]), len(sc["edge_a"])
    assert not sc["fixed"][1:].any()
    ids = np.arange(K, dtype="<i4") + (1 if sc["fixed"][0] else 2)
    with open(path, "wb") as f:
        f.write(b"MSPG" + np.array([1, K, E, sc.get("max_iterations", 100), sc["sqrt_info"] is not None], "<i4").tobytes())
        f.write(ids.tobytes())
        for a, dt in ((sc["poses"], "<f8"), (sc["edge_a"], "<i4"), (sc["edge_b"], "<i4"), (sc["edge_meas"], "<f8")):
            f.write(np.ascontiguousarray(a, dt).tobytes())
        if sc["sqrt_info"] is not None:
            f.write(np.ascontiguousarray(sc["sqrt_info"], "<f8").tobytes())
    return ids
