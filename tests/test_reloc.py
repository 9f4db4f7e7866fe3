"""Verified relocalisation, CPU part: the reference composition (tests/reloc_ref.py: oracle matcher + ratio test, PnP oracle
with seed + position, ranking) is pinned on the synthetic scene the GPU tests compare the product with, and the library
exports the new entry points without an ABI bump."""
import numpy as np

import reloc_ref as rr
from reloc_ref import po

NEW_SYMBOLS = ["mslam_hip_kf_add", "mslam_hip_kf_add_from_batch_dev", "mslam_hip_kf_remove", "mslam_hip_kf_clear",
               "mslam_hip_kf_size", "mslam_hip_kf_reserve", "mslam_hip_kf_read", "mslam_hip_relocalize"]


def test_library_exports_the_store_and_relocalize(pkg):
    lib = pkg.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in pkg.ABI_SYMBOLS, name
    assert lib.mslam_hip_abi_version() == 5          # new functions only: no struct changed
    for method in ("kf_add", "kf_add_from_batch_dev", "kf_remove", "kf_clear", "kf_size", "kf_read", "kf_reserve", "relocalize"):
        assert callable(getattr(pkg.Context, method)), method
    assert callable(pkg.HipOrbRelocalizer.addKeyframeLandmarks) and callable(pkg.HipOrbRelocalizer.relocalizePose)
    assert callable(pkg.HipLoopDetector.detectLoopVerified)
    import ctypes
    assert ctypes.sizeof(pkg.RelocCandidate) == 64


def test_reference_picks_the_keyframe_and_rejects_the_decoy(orc):
    sc = rr.make_scene(seed=0)
    cand = [sc["decoy"]] + sc["ids"]                 # the decoy first: it must not win by position
    ref = rr.relocalize(sc["desc"], sc["xy"], sc["store"], cand, seed=5)
    j = cand.index(sc["target_id"])
    assert ref["best"] == j
    win = ref["candidates"][j]
    # every match of the target is a true one, and every one is an inlier
    fi, ti = win["pairs"]
    assert len(fi) > 450 and np.array_equal(sc["from_landmark"][fi], ti)
    assert win["status"] == 1 and win["n_inliers"] == win["n_correspondences"] == win["n_matches"]
    # noise-free image points: the pose is the truth (tests/test_pnp.py's noise-free tolerance)
    rv_true = _rvec(sc["R"])
    print("pose error:", np.abs(_rvec(win["R"]) - rv_true).max(), np.abs(win["t"] - sc["t"]).max())
    assert np.abs(_rvec(win["R"]) - rv_true).max() < 1e-6 and np.abs(win["t"] - sc["t"]).max() < 1e-6
    # the decoy carries the same descriptors: the same matches, but its permuted world points support no pose
    dec = ref["candidates"][0]
    assert np.array_equal(dec["pairs"][0], fi) and np.array_equal(dec["pairs"][1], ti)
    assert dec["n_correspondences"] == len(fi) and (dec["status"] == 0 or dec["n_inliers"] < 60)
    # unrelated keyframes: random descriptors fail the ratio test, fewer than 4 correspondences, status 0
    for k, cid in enumerate(cand):
        if cid not in (sc["decoy"], sc["target_id"]):
            c = ref["candidates"][k]
            assert c["n_matches"] < 4 and c["status"] == 0 and c["n_inliers"] == 0


def test_reference_ties_and_min_inliers(orc):
    assert rr.rank([1, 1, 1], [70, 90, 90], 60) == 1         # first maximum (max_element)
    assert rr.rank([0, 1, 1], [0, 59, 30], 60) == -1          # winner below min_inliers
    assert rr.rank([0, 1], [500, 61], 60) == 1                # a candidate without a model never wins
    assert rr.rank([0, 0], [0, 0], 0) == -1 and rr.rank([], [], 0) == -1
    assert rr.rank([1], [60], 60) == 0
    sc = rr.make_scene(seed=1, target=0)
    tid = sc["target_id"]
    # the target listed twice: different sampling seeds (seed + position), the same consensus set — the first one wins
    ref = rr.relocalize(sc["desc"], sc["xy"], sc["store"], [sc["ids"][1], tid, tid], seed=9)
    a, b = ref["candidates"][1], ref["candidates"][2]
    assert a["status"] == b["status"] == 1 and a["n_inliers"] == b["n_inliers"] > 400 and ref["best"] == 1
    n_in = a["n_inliers"]
    assert rr.relocalize(sc["desc"], sc["xy"], sc["store"], [tid], seed=9, min_inliers=n_in)["best"] == 0
    assert rr.relocalize(sc["desc"], sc["xy"], sc["store"], [tid], seed=9, min_inliers=n_in + 1)["best"] == -1
    # no candidates, one query keypoint: no model
    assert rr.relocalize(sc["desc"], sc["xy"], sc["store"], [], seed=9)["best"] == -1
    one = rr.relocalize(sc["desc"][:1], sc["xy"][:1], sc["store"], [tid], seed=9)
    assert one["best"] == -1 and one["candidates"][0]["n_matches"] == 0


def test_reference_depth_mask_and_guess(orc):
    """track()'s form (rgbd_feature_frontend.cpp:317-334): masked query keypoints are dropped from the correspondences, and
    the guess is the refinement's start"""
    sc = rr.make_scene(seed=2, noise=0.5)
    rng = np.random.default_rng(3)
    valid = rng.random(len(sc["desc"])) < 0.8
    tid = sc["target_id"]
    guess = (po.rodrigues([0.01, -0.02, 0.015]) @ sc["R"], sc["t"] + 0.03)
    ref = rr.relocalize(sc["desc"], sc["xy"], sc["store"], [tid], valid=valid, guess=guess, seed=4)
    c = ref["candidates"][0]
    fi = c["pairs"][0]
    assert c["n_correspondences"] == int(valid[fi].sum()) < c["n_matches"]
    assert ref["best"] == 0 and rr.rot_err(c["R"], sc["R"]) < 0.1 and np.linalg.norm(c["t"] - sc["t"]) < 0.02


def test_reference_lift_is_add_new_landmarks():
    rng = np.random.default_rng(7)
    n = 50
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    xyz = rng.uniform(-1, 1, (n, 3)) + [0, 0, 2.6]
    valid = rng.random(n) < 0.7
    R, t = po.rodrigues([0.1, 0.2, -0.3]), np.array([0.5, -0.25, 1.0])
    d, w = rr.lift(desc, xyz, valid, R, t, 3.0)
    keep = valid & (xyz[:, 2] <= 3.0)
    assert 5 < keep.sum() < valid.sum() and np.array_equal(d, desc[keep])
    assert np.allclose(w, xyz[keep] @ R.T + t, rtol=0, atol=1e-14)


def _rvec(R):
    th = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    return th / (2 * np.sin(th)) * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
