"""mslam_hip_pose_graph_covariance on the CPU: the references of tests/pose_graph_cov_ref.py among themselves, on every case
the GPU tests list (tests/pose_graph_cov_cases.py), and what the header, the library and the Python mirror declare.

  * the two dense references, R^-1 R^-T of a QR of J and L^-T L^-1 of a Cholesky of J^T J, agree to d <= 1e-6 on every listed
    case: the condition under which a case may be in the lists (a case beyond it tests nothing);
  * the Takahashi recursion restated on analyze()'s envelope equals the dense inverse on every block of the envelope, for
    NATURAL and RCM orders;
  * a loop edge never enlarges a marginal (Sigma_open - Sigma_closed is positive semi-definite per pose).  The trace along the
    chain is NOT monotone in this parameterisation (36.6 then 35.9 on this scene), so that is not tested;
  * delta is half a rotation vector, applied on the left."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_cases as pc  # noqa: E402
import pose_graph_cov_cases as cc  # noqa: E402
import pose_graph_cov_ref as cr  # noqa: E402
import pose_graph_loss_ref as pl  # noqa: E402
import pose_graph_ref as pg  # noqa: E402
import pose_graph_sparse_ref as ps  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", cc.CASES)
def test_the_references_agree_and_the_recursion_equals_the_dense_inverse(name):
    sc, ref = cc.reference(name)
    print("PGC-CPU %-24s n %5d d %.3e" % (name, ref["prob"].n, ref["d"]))
    assert ref["d"] <= cr.MAX_D
    an = cc.analysis(sc)
    assert (an["ordering"] == ps.RCM) == (name in cc.RCM)
    J = cr.jacobian(ref["prob"], sc["poses"])
    Z = cr.selected_inverse(J.T @ J, ref["prob"], an)
    assert len(Z) == an["envelope_blocks"]
    worst = 0.0
    for (i, j), B in Z.items():
        worst = max(worst, float(np.max(np.abs(B - cr.block(ref["sigma"], ref["prob"], an["order"][i], an["order"][j])))))
    assert worst <= ref["bound"], (worst, ref["bound"])
    # every requested block is a block of the envelope
    for a, b in ref["pairs"]:
        assert np.max(np.abs(cr.envelope_block(Z, an, ref["prob"], a, b) - cr.block(ref["sigma"], ref["prob"], a, b))) <= ref["bound"]


def test_the_new_scenes_are_what_they_are_named_for():
    for K, rows, blocks in ((44, 42, 946), (45, 43, 990)):
        an = cc.analysis(cc.scene("complete:%d" % K))
        assert an["ordering"] == ps.NATURAL and an["envelope_blocks"] == blocks
        assert int(np.sum(an["first"][1:] <= 0)) == rows                 # column 0's rows below the diagonal
    assert 6 * 42 <= 256 < 6 * 43
    sc = cc.scene("zero_info")
    prob = cr.problem(sc)
    A = (lambda J: J.T @ J)(cr.jacobian(prob, sc["poses"]))
    c = prob.col[5]
    assert not A[c:c + 6, :].any() and A[:c, :c].any()                    # pose 5's rows of J^T J are exactly zero
    for name in cc.RANK[:2]:                                              # a component without a constant pose: singular
        s = cc.scene(name)
        J = cr.jacobian(cr.problem(s), s["poses"])
        assert np.linalg.matrix_rank(J) <= J.shape[1] - 6


def test_the_big_case_meets_the_condition():
    sc, cov, cross, d, bound = cc.big_reference()
    print("PGC-CPU %-24s d %.3e bound %.3e" % (cc.BIG, d, bound))
    assert d <= cr.MAX_D and cov.shape == (8, 6, 6) and cross.shape == (4, 6, 6)
    assert not cov[0].any() and cov[1].any()


@pytest.mark.parametrize("kind", pl.LOSSES)
def test_the_loss_references_agree(kind):
    sc = pl.scene("false:12,4,1,1")
    _, qr, _, _ = pl.reference("false:12,4,1,1", kind)
    ref = cc.reference_at(sc, qr["poses"], loss=(kind, pl.SCALE))
    plain = cc.reference_at(sc, qr["poses"])
    assert ref["d"] <= cr.MAX_D
    assert np.max(np.abs(plain["cov"] - ref["cov"])) > 100.0 * ref["bound"]       # a down-weighted edge gives less information


def test_a_loop_edge_never_enlarges_a_marginal():
    open_, closed = pc.make_scene(12, pc.chain(12, 0), 77), pc.make_scene(12, pc.chain(12, 1), 77)
    # the same truth and the same odometry measurements; the starts differ (the generator has drawn one measurement more), so
    # both are evaluated at one of them
    assert np.array_equal(open_["edge_meas"], closed["edge_meas"][:-1]) and len(closed["edge_a"]) == len(open_["edge_a"]) + 1
    ro, rc = cc.reference_at(open_, closed["poses"]), cc.reference_at(closed, closed["poses"])
    bound = ro["bound"] + rc["bound"]
    for p in range(len(ro["poses_of"])):
        diff = ro["cov"][p] - rc["cov"][p]
        assert np.min(np.linalg.eigvalsh((diff + diff.T) / 2.0)) >= -6.0 * bound, p       # |E|_2 <= 6 max|E_ij| for a 6 x 6 block


def test_delta_is_half_a_rotation_vector_on_the_left():
    """the header's statement about the tangent: Plus(q, delta) = q_delta (x) q with q_delta the rotation by 2 |delta| about
    delta, so the covariance of a rotation vector is 4 x the delta block"""
    rng = np.random.default_rng(3)
    q = np.array([pg.matrix_to_quaternion(pg.rodrigues(rng.normal(size=3)))])
    d = 1e-3 * rng.normal(size=(1, 3))
    got = ps._quaternion_plus(q, d)[0]
    want = pg.q_mul(pg.matrix_to_quaternion(pg.rodrigues(2.0 * d[0])), q[0])
    assert np.max(np.abs(got - want)) <= 1e-15
    assert np.max(np.abs(pg.q_matrix(got) - pg.rodrigues(2.0 * d[0]) @ pg.q_matrix(q[0]))) <= 1e-15
    hdr = open(os.path.join(ROOT, "include", "mslam_hip.h")).read()
    assert "delta is HALF a rotation vector" in hdr


def test_header_library_and_mirror_declare_the_entry(pkg):
    hdr = open(os.path.join(ROOT, "include", "mslam_hip.h")).read()
    assert re.search(r"#define MSLAM_HIP_ABI_VERSION 5\b", hdr)
    decl = hdr[hdr.index("int mslam_hip_pose_graph_covariance("):]
    decl = " ".join(decl[:decl.index(";")].split())
    for piece in ("const double* poses", "const int32_t* pose_idx, int P", "double* cov", "const int32_t* pair_a, const int32_t* pair_b, int Q",
                  "double* cross"):
        assert piece in decl, piece
    assert "PARITY UNPINNED" in hdr[hdr.index("Marginal covariances of mslam_hip_pose_graph"):hdr.index("int mslam_hip_pose_graph_covariance(")]
    assert "mslam_hip_pose_graph_covariance" in pkg.ABI_SYMBOLS and hasattr(pkg.Context, "pose_graph_covariance")
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH]).decode()
    assert " T mslam_hip_pose_graph_covariance" in out
    import inspect
    assert "covariance" in inspect.signature(pkg.HipBackend.close_loop).parameters
    assert "loop_covariance" in inspect.signature(pkg.HipKeyframeTracker.__init__).parameters
    with pytest.raises(pkg.MslamHipError) as e:
        pkg.HipKeyframeTracker(None, focal=(500.0, 500.0), principal=(320.0, 240.0), loop_covariance=True)
    assert e.value.code == pkg.E_INVALID and "loop_closure" in str(e.value)
