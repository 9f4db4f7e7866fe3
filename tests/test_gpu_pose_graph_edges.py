"""k_posegraph.hip on the MI355X at its block, stride, batch, sign and termination edges: the scenes of pose_graph_cases.EDGES
(tests/test_pose_graph_edges.py shows on the CPU that each takes the path it is named for) against tests/pose_graph_ref.py's QR
solve, under the bounds of tests/test_gpu_pose_graph.py, unchanged:

  termination equal, iterations within 1, no invalid step; initial_cost within 1e-6 relative (zero_start: equal to 0.0);
  final_cost within 1e-6 relative plus E (J B)^2 / 2 with J = pose_graph_cases.jacobian_row_bound; the state within
  B = max(1e-9, 1000 |x_chol - x_qr|_inf) up to the quaternions' signs; constant and edgeless poses bit for bit.

`far` keeps that state bound as it stands: its positions lie near 5e4, where an ulp is 7.3e-12, the two CPU solvers return the
same position bits, and the 1e-9 floor is 137 ulp.

What the names reach in the kernels: edges:16641 is 66 blocks of k_pg_edges / k_pg_eval, the last with one edge (the second
trip of the b += 64 loops of k_pg_check and k_pg_control, a partly filled block), 43 lane strides of k_pg_poses and 250 trips
of k_pg_assemble's serial loop; edges:256 / edges:257 a full block and a full block plus a lane; sparse1024 the cap of K, all
four blocks of k_pg_candidate and sixteen trips of the k += 64 loops, with 1 014 poses to copy; far the parameter-tolerance exit
and the xn / sn sums; zero_start a cost of exactly 0; neg_meas the sign of q_meas; info_dense the whole 6 x 6 sqrt_info;
rejected:capN a cap that arrives after rejected steps, at and past the host's batch of four iterations.  Further: a second call
returns the same bits, the argument forms Context.pose_graph converts, K = 0.

Found by the Fortran-ordered form: Context.pose_graph copied `poses` with np.array(poses, np.float64), which keeps a column-major
argument's layout, and handed that memory to the library as row-major ("the quaternion of pose 0 is not unit").  The copy now
asks for row-major order; Context._bundle_adjust had the same two lines and has a test here as well.

Not covered, on purpose: the invalid-step branch, the five-in-a-row FAILURE and the minimum-radius exit need a non-positive
pivot or model_cost_change <= 0; no input reaches either through both CPU solvers alike, so no reference pins them.  E at its
cap of 65 536 is left out as well.

One-line breaks of k_posegraph.hip, each built once in a scratch copy and run against tests/test_gpu_pose_graph.py and this
file: the block-partial loops of k_pg_check / k_pg_control stopping after one trip (the old tests pass; edges:16641 fails here),
k_pg_candidate handling its first block only (chain300 fails there, sparse1024 here), |x| summed over the quaternions only (old
pass; far fails), sqrt_info's strict lower triangle ignored (old pass; info_dense and info_dense_dropped fail), the iteration cap
looked at only when the Jacobians were re-evaluated (old pass; rejected:cap2, cap3, cap4 fail).

The loop's decisions, reductions and quaternions now live once in csrc/trust_region.hpp, shared with k_ba.hip, so a break there
shows in both solvers' tests.  Built and run in the same way against tests/test_gpu_ba.py and tests/test_gpu_pose_graph.py: the
function tolerance compared without `* x_cost` (37 and 19 tests fail), the sign of w flipped in the quaternion inverse (54 and
22 fail); the radius left undivided after an invalid step fails nothing in either file, for the reason given above: no case
reaches the invalid-step branch.

Measured on an MI355X (GPU / reference; dx = distance to the QR reference, beside the bound B):
  edges:16641          term 0/0  it 3/3  rejected 0/0  dx 6.661e-16  B 1.000e-09
  edges:256            term 0/0  it 3/3  rejected 0/0  dx 1.554e-15  B 1.000e-09
  edges:257            term 0/0  it 3/3  rejected 0/0  dx 6.661e-16  B 1.000e-09
  sparse1024           term 0/0  it 4/4  rejected 0/0  dx 3.553e-15  B 1.000e-09
  far                  term 0/0  it 3/3  rejected 0/0  dx 1.110e-16  B 1.000e-09
  zero_start           term 0/0  it 0/0  rejected 0/0  dx 0.000e+00  B 1.000e-09
  neg_meas             term 0/0  it 4/4  rejected 0/0  dx 5.551e-16  B 1.000e-09
  info_dense           term 0/0  it 4/4  rejected 0/0  dx 4.885e-15  B 1.000e-09
  info_dense_dropped   term 0/0  it 4/4  rejected 0/0  dx 2.442e-15  B 1.000e-09
  rejected:cap2        term 1/1  it 2/2  rejected 2/2  dx 0.000e+00  B 1.000e-09
  rejected:cap3        term 1/1  it 3/3  rejected 3/3  dx 0.000e+00  B 1.000e-09
  rejected:cap4        term 1/1  it 4/4  rejected 4/4  dx 0.000e+00  B 1.000e-09
  rejected:cap5        term 1/1  it 5/5  rejected 4/4  dx 2.220e-15  B 1.000e-09
  rejected:cap8        term 1/1  it 8/8  rejected 4/4  dx 1.137e-13  B 1.000e-09
  neg_meas against the plain scene: the same bits (poses, costs, counts)
  info_dense against info_dense_dropped: dx 0.000e+00, the same final cost bits
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_cases  # noqa: E402
import pose_graph_cases as pc  # noqa: E402

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


def _same_bits(a, b):
    assert a["poses"].tobytes() == b["poses"].tobytes()
    for k in ("termination", "iterations", "rejected_steps", "invalid_steps", "n_outliers"):
        assert a[k] == b[k], k
    for k in ("initial_cost", "final_cost"):
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), k


def _outside(sc):
    """the poses outside the problem: constant, or without an edge"""
    seen = np.zeros(len(sc["poses"]), bool)
    seen[sc["edge_a"]], seen[sc["edge_b"]] = True, True
    return np.flatnonzero(~seen | (sc["fixed"] != 0))


@pytest.mark.parametrize("name", pc.EDGES)
def test_edge_cases_against_the_qr_reference(ctx, name):
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
    if name == "zero_start":
        assert got["initial_cost"] == 0.0 and qr["initial_cost"] == 0.0
    else:
        assert abs(got["initial_cost"] - qr["initial_cost"]) <= 1e-6 * qr["initial_cost"]
    assert abs(got["final_cost"] - qr["final_cost"]) <= 1e-6 * qr["final_cost"] + second_order
    assert dx <= bound
    start = np.asarray(sc["poses"], np.float64)
    outside = _outside(sc)
    assert len(outside) >= 1
    for k in outside:                                         # constant and edgeless poses come back bit for bit
        assert got["poses"][k].tobytes() == start[k].tobytes(), k
    kind, _, rest = name.partition(":")
    if kind in ("edges", "sparse1024", "far", "neg_meas", "info_dense", "info_dense_dropped"):
        assert got["termination"] == 0 and got["rejected_steps"] == qr["trace"]["rejected"] == 0
    if kind == "sparse1024":
        assert len(outside) == 1015 and 700 in outside        # 1 014 poses without an edge (700 constant as well) and pose 0
        for k in (1, 64, 256, 1023):
            assert not np.array_equal(got["poses"][k], start[k]), k
    if kind == "far":                                         # the margins are 5 x either way: the same iteration ends it
        assert got["iterations"] == qr["iterations"] and qr["reason"] == "parameter tolerance"
    if kind == "zero_start":
        assert got["termination"] == 0 and got["iterations"] == 0 and got["rejected_steps"] == 0
        assert got["final_cost"] == 0.0 and got["poses"].tobytes() == start.tobytes()
    if kind == "rejected":
        cap = int(rest[3:])
        assert got["termination"] == 1 and got["iterations"] == qr["iterations"] == cap
        assert got["rejected_steps"] == qr["trace"]["rejected"] == min(cap, 4)
        if cap <= 4:                                          # every step so far was rejected: nothing may have moved
            assert got["poses"].tobytes() == start.tobytes()
            assert got["final_cost"] == got["initial_cost"]
        else:
            assert np.max(np.abs(got["poses"] - start)) > 1e-3 and got["final_cost"] < got["initial_cost"]


@pytest.mark.parametrize("name", ["edges:16641", "sparse1024", "far", "info_dense"])
def test_a_second_call_returns_the_same_bits(ctx, name):
    sc = pc.reference(name)[0]
    _same_bits(_solve(ctx, sc), _solve(ctx, sc))


def test_a_negated_measurement_returns_the_bits_of_the_plain_one(ctx):
    """-q_meas flips delta, and with it rows 3 to 5 of r, J_a and J_b of that edge, exactly (identity sqrt_info adds exact
    zeros).  The normal equations, the gradient, the model cost change and the cost are sums of products of two such
    quantities, so every sum gets the same terms: the same bits, as in the reference."""
    sc = pc.reference("neg_meas")[0]
    plain = dict(sc, edge_meas=sc["edge_meas"].copy())
    plain["edge_meas"][pc.NEG_MEAS_EDGES, :4] *= -1.0
    a, b = _solve(ctx, sc), _solve(ctx, plain)
    print("PG neg_meas vs plain: it %d/%d cost %.17g/%.17g dx %.3e" % (
        a["iterations"], b["iterations"], a["final_cost"], b["final_cost"], float(np.max(np.abs(a["poses"] - b["poses"])))))
    _same_bits(a, b)


def test_an_edge_of_zero_weight_is_no_edge(ctx):
    """info_dense's last edge has sqrt_info = 0; info_dense_dropped is the scene without it.  The zero edge still makes the
    pair (1, 3) a block of the normal equations, an incidence of poses 1 and 3 and a lane of the edge kernels."""
    sc, qr, ch, dist = pc.reference("info_dense")
    dropped = pc.reference("info_dense_dropped")[0]
    a, b = _solve(ctx, sc), _solve(ctx, dropped)
    bound = max(1e-9, 1000.0 * dist)
    dx = pc.same_rotation_distance(a["poses"], b["poses"])
    print("PG info_dense vs dropped: it %d/%d cost %.17g/%.17g dx %.3e bound %.3e" % (
        a["iterations"], b["iterations"], a["final_cost"], b["final_cost"], dx, bound))
    assert a["termination"] == b["termination"] == 0 and a["iterations"] == b["iterations"]
    assert dx <= bound
    assert abs(a["final_cost"] - b["final_cost"]) <= 1e-6 * qr["final_cost"]


def test_argument_forms_return_the_bits_of_the_plain_call(ctx):
    """what Context.pose_graph converts: chain:9 with values that f32 holds exactly, poses 0 and 4 constant, an upper
    sqrt_info; as f32, with int64 edge arrays, in Fortran order, as strided views, fixed as bool and as bytes 0 / 2 / 255"""
    sc = pc.scene("chain:9")
    K, E = len(sc["poses"]), len(sc["edge_a"])
    x32, z32 = sc["poses"].astype(np.float32), sc["edge_meas"].astype(np.float32)
    w32 = pc.upper_info(E, 41).astype(np.float32)
    fx = np.zeros(K, np.uint8)
    fx[[0, 4]] = 1
    plain = dict(poses=x32.astype(np.float64), edge_a=sc["edge_a"], edge_b=sc["edge_b"], edge_meas=z32.astype(np.float64),
                 sqrt_info=w32.astype(np.float64), fixed=fx)
    want = _solve(ctx, plain)
    assert want["termination"] == 0 and want["iterations"] >= 2
    assert want["poses"][4].tobytes() == plain["poses"][4].tobytes() and not np.array_equal(want["poses"][5], plain["poses"][5])

    def strided(a, step):
        big = np.zeros((len(a) * step,) + a.shape[1:], a.dtype)
        big[::step] = a
        view = big[::step]
        assert not view.flags["C_CONTIGUOUS"] or len(a) <= 1
        return view

    def reversed_view(a):
        return np.ascontiguousarray(a[::-1])[::-1]

    odd = fx.copy()
    odd[0], odd[4] = 2, 255
    forms = dict(
        f32=dict(poses=x32, edge_meas=z32, sqrt_info=w32),
        int64=dict(edge_a=sc["edge_a"].astype(np.int64), edge_b=sc["edge_b"].astype(np.int64)),
        fortran=dict(poses=np.asfortranarray(plain["poses"]), edge_meas=np.asfortranarray(plain["edge_meas"]),
                     sqrt_info=np.asfortranarray(plain["sqrt_info"])),
        strided=dict(poses=strided(plain["poses"], 2), edge_a=strided(sc["edge_a"], 3), edge_b=strided(sc["edge_b"], 2),
                     edge_meas=strided(plain["edge_meas"], 3), sqrt_info=strided(plain["sqrt_info"], 2), fixed=strided(fx, 5)),
        reversed=dict(poses=reversed_view(plain["poses"]), edge_a=reversed_view(sc["edge_a"]), sqrt_info=reversed_view(plain["sqrt_info"])),
        columns=dict(poses=np.zeros((K, 9))[:, 1:8], edge_meas=np.zeros((E, 8))[:, :7]),
        lists=dict(poses=plain["poses"].tolist(), edge_a=sc["edge_a"].tolist(), edge_b=sc["edge_b"].tolist(), fixed=fx.tolist()),
        fixed_bool=dict(fixed=fx.astype(bool)),
        fixed_bytes=dict(fixed=odd),
    )
    forms["columns"]["poses"][...] = plain["poses"]
    forms["columns"]["edge_meas"][...] = plain["edge_meas"]
    assert forms["fortran"]["sqrt_info"].flags["F_CONTIGUOUS"] and not forms["fortran"]["poses"].flags["C_CONTIGUOUS"]
    for form, over in forms.items():
        before = {k: np.array(v) for k, v in over.items()}
        got = _solve(ctx, plain, **over)
        _same_bits(got, want)
        assert got["poses"].dtype == np.float64 and got["poses"].shape == (K, 7), form
        for k, v in over.items():                             # the arguments are read, never written
            assert np.array_equal(np.array(v), before[k]), (form, k)


@pytest.mark.parametrize("entry", ["bundle_adjust", "bundle_adjust_global"])
def test_bundle_adjustment_takes_its_state_in_fortran_order(ctx, entry):
    """Context._bundle_adjust copied its poses and landmarks the way Context.pose_graph did (the copy kept a column-major
    argument's layout, and the library read it as row-major); the Fortran form above found it, so both are pinned"""
    sc = ba_cases.scene("fixed:3,65,5")
    solve = getattr(ctx, entry)
    want = solve(sc["poses"], sc["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"], sc["fixed"])
    got = solve(np.asfortranarray(sc["poses"]), np.asfortranarray(sc["landmarks"]), sc["obs_kf"], sc["obs_lm"],
                np.asfortranarray(sc["obs_cam"]), sc["fixed"])
    assert want["termination"] == 0 and want["iterations"] >= 1
    for k in ("poses", "landmarks", "outlier"):
        assert got[k].tobytes() == want[k].tobytes(), k
    for k in ("termination", "iterations", "initial_cost", "final_cost"):
        assert got[k] == want[k], k


def test_no_poses_and_no_edges(ctx):
    got = ctx.pose_graph(np.zeros((0, 7)), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 7)))
    assert got["termination"] == 0 and got["iterations"] == 0 and got["poses"].shape == (0, 7)
    assert got["initial_cost"] == 0.0 and got["final_cost"] == 0.0
    got = ctx.pose_graph([], [], [], [], None, [])
    assert got["termination"] == 0 and got["poses"].shape == (0, 7)
