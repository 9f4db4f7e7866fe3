"""Bundle adjustment, CPU side: tests/ba_ref.py (the numpy restatement of CeresBackend::bundleAdjustment's solve) against
central differences, against ground truth, and its two linear solvers against each other, on the cases of tests/ba_cases.py
that the GPU tests (tests/test_gpu_ba.py) run on the kernels."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_cases  # noqa: E402
import ba_ref  # noqa: E402


def test_tangent_jacobian_against_central_differences():
    """J_q * PlusJacobian, J_p and J_X against central differences of residual(Plus(q, d)), residual(p + d),
    residual(X + d).  Step 1e-6 on quantities of order 1: truncation ~1e-12 (third derivatives are O(1)), rounding
    ~1e-16 / 1e-6 = 1e-10 per unit of residual magnitude (up to ~5 m here); the bound is 5e-9."""
    sc = ba_cases.scene("fixed:3,65,5")
    P, X, kf, lm, cam = sc["poses"], sc["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"]
    r, Jd, Jp, JX = ba_ref.tangent_jacobians(P, X, kf, lm, cam)
    h = 1e-6
    for m in (0, 7, 100, 194):
        k, l = kf[m], lm[m]

        def res(dq=np.zeros(3), dp=np.zeros(3), dX=np.zeros(3)):
            P2, X2 = P.copy(), X.copy()
            P2[k, :4] = ba_ref.quaternion_plus(P[k, :4], dq)
            P2[k, 4:] += dp
            X2[l] += dX
            return ba_ref.residuals(P2, X2, kf, lm, cam)[m]
        for j in range(3):
            e = np.zeros(3)
            e[j] = h
            for name, J, num in (("delta", Jd, (res(dq=e) - res(dq=-e)) / (2 * h)), ("p", Jp, (res(dp=e) - res(dp=-e)) / (2 * h)),
                                 ("X", JX, (res(dX=e) - res(dX=-e)) / (2 * h))):
                assert np.max(np.abs(num - J[m][:, j])) < 5e-9, (m, name, j)
    assert np.allclose(r, ba_ref.residuals(P, X, kf, lm, cam), rtol=0, atol=0)


def test_plus_keeps_unit_norm_and_zero_is_identity():
    q = np.array([0.1, -0.2, 0.3, 0.9])
    q /= np.linalg.norm(q)
    assert np.array_equal(ba_ref.quaternion_plus(q, np.zeros(3)), q)
    assert abs(np.linalg.norm(ba_ref.quaternion_plus(q, [0.3, -0.1, 0.2])) - 1.0) < 1e-15


@pytest.mark.parametrize("name", [c for c in ba_cases.FAMILIES["fixed"] if c.endswith(",0")] + ["rejected"])
def test_ground_truth_on_noise_free_scenes(name):
    sc, qr, sch, dist, mask, margin = ba_cases.reference(name)
    for sol in (qr, sch):
        assert sol["termination"] == ba_ref.CONVERGENCE
        assert np.max(np.abs(sol["poses"] - sc["truth_poses"])) < 1e-7
        assert np.max(np.abs(sol["landmarks"] - sc["truth_landmarks"])) < 1e-7
    assert not mask.any()


@pytest.mark.parametrize("name", ba_cases.ALL)
def test_two_solvers_agree(name):
    sc, qr, sch, dist, mask, margin = ba_cases.reference(name)
    assert qr["termination"] == sch["termination"]
    assert abs(qr["iterations"] - sch["iterations"]) <= 1
    assert dist <= 1e-9
    assert qr["final_cost"] <= qr["initial_cost"]
    assert margin > 1e-6        # the outlier mask of the case does not hang on rounding


def test_families_take_their_paths():
    for name in ba_cases.FAMILIES["fixed"] + ba_cases.FAMILIES["free"]:
        sc, qr = ba_cases.reference(name)[:2]
        K = len(sc["poses"])
        assert 3 <= qr["iterations"] <= 6 and qr["trace"]["rejected"] == 0 and qr["trace"]["invalid"] == 0, name
        assert qr["trace"]["free_poses"] == (K - 1 if name.startswith("fixed") else K), name
        assert qr["trace"]["constant_poses"] == (1 if name.startswith("fixed") else 0), name


def test_named_cases_take_their_paths():
    t = {n: ba_cases.reference(n)[1] for n in ("rejected", "all_fixed", "k1_fixed", "fixed_only_landmarks", "cap3", "empty",
                                               "k64", "keyframe_one_observation", "gross_outliers", "twice_in_keyframe")}
    assert t["rejected"]["trace"]["rejected"] >= 4 and t["rejected"]["trace"]["accepted_after_rejected"] >= 1
    assert t["rejected"]["iterations"] > 10
    assert t["all_fixed"]["trace"]["free_poses"] == 0 and t["all_fixed"]["trace"]["constant_poses"] == 3
    assert t["all_fixed"]["iterations"] <= 3
    assert t["k1_fixed"]["trace"]["free_poses"] == 0 and t["k1_fixed"]["trace"]["landmarks_fixed_only"] == 30
    assert t["fixed_only_landmarks"]["trace"]["landmarks_fixed_only"] == 10
    assert t["cap3"]["termination"] == ba_ref.NO_CONVERGENCE and t["cap3"]["iterations"] == 3
    assert t["cap3"]["final_cost"] < t["cap3"]["initial_cost"]
    assert t["empty"]["termination"] == ba_ref.CONVERGENCE and t["empty"]["final_cost"] == 0.0
    assert t["k64"]["trace"]["free_poses"] == 63 and t["k64"]["trace"]["landmarks"] == 513
    assert t["keyframe_one_observation"]["trace"]["free_poses"] == 3
    assert ba_cases.reference("gross_outliers")[4].sum() >= 3
    sc = ba_cases.scene("twice_in_keyframe")
    pairs = list(zip(sc["obs_kf"].tolist(), sc["obs_lm"].tolist()))
    assert pairs.count((1, 3)) == 3 and pairs.count((1, 17)) == 2
    sc = ba_cases.scene("keyframe_one_observation")
    assert np.sum(sc["obs_kf"] == 3) == 1
    # the iteration cap next to the host's batch of four, and a start that is the minimum
    t = {n: ba_cases.reference(n)[1] for n in ("cap0", "cap1", "cap4_converges", "cap4_stops", "at_minimum")}
    for n, its in (("cap0", 0), ("cap1", 1), ("cap4_stops", 4)):
        assert (t[n]["termination"], t[n]["iterations"], t[n]["reason"]) == (ba_ref.NO_CONVERGENCE, its, "max iterations"), n
    assert t["cap0"]["final_cost"] == t["cap0"]["initial_cost"] and t["cap1"]["final_cost"] < t["cap1"]["initial_cost"]
    assert (t["cap4_converges"]["termination"], t["cap4_converges"]["iterations"], t["cap4_converges"]["reason"]) == \
           (ba_ref.CONVERGENCE, 4, "function tolerance")
    assert ba_ref.solve_scene(ba_cases.scene("free:5,150,10"))["iterations"] == 5      # what cap4_stops is cut short of
    assert (t["at_minimum"]["termination"], t["at_minimum"]["iterations"], t["at_minimum"]["reason"]) == \
           (ba_ref.CONVERGENCE, 0, "gradient tolerance")
    assert t["at_minimum"]["final_cost"] == 0.0
    # gaps in the block numbering: keyframe 1 unobserved, keyframe 3 (and 0) constant
    for n, free, const, fixed_only in (("fixed_middle", 4, 1, 0), ("fixed_two", 3, 2, 1)):
        sc, qr = ba_cases.reference(n)[:2]
        tr = qr["trace"]
        assert (tr["free_poses"], tr["constant_poses"], tr["landmarks_fixed_only"]) == (free, const, fixed_only), n
        assert not np.any(sc["obs_kf"] == 1) and sc["fixed"].tolist() == [n == "fixed_two", 0, 0, 1, 0, 0], n
        assert np.bincount(sc["obs_lm"], minlength=80).min() >= 2, n
        assert qr["termination"] == ba_ref.CONVERGENCE and qr["iterations"] == 4, n
    # 64 and 65 blocks of 256 observations, long rows, long runs of one landmark in one keyframe
    for n, blocks in (("blocks:16384", 64), ("blocks:16385", 65)):
        sc, qr, _, _, mask, _ = ba_cases.reference(n)
        M = len(sc["obs_kf"])
        assert (M + 255) // 256 == blocks, n
        assert np.bincount(sc["obs_kf"], minlength=4).min() >= 4000, n
        assert np.bincount(sc["obs_kf"] * 48 + sc["obs_lm"], minlength=192).min() >= 85, n
        assert mask[0] and mask[16383] and mask[M - 1] and np.flatnonzero(mask).max() >= 16383, n
        assert int(mask.sum()) == blocks - 62, n
        assert qr["termination"] == ba_ref.CONVERGENCE and qr["iterations"] == 4 and qr["trace"]["rejected"] == 0, n
    # a dense reduced system: every pair of keyframes shares a landmark
    sc, qr = ba_cases.reference("k64_dense")[:2]
    assert qr["trace"]["free_poses"] == 63 and qr["termination"] == ba_ref.CONVERGENCE and qr["iterations"] == 4
    seen = np.zeros((64, 120), np.int64)
    seen[sc["obs_kf"], sc["obs_lm"]] = 1
    assert (seen @ seen.T).min() >= 1
