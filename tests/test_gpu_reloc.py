"""Verified relocalisation on the GPU, through the C ABI: the keyframe store, the device lift, and mslam_hip_relocalize
against the reference composition of tests/reloc_ref.py (oracle matcher + ratio test, PnP oracle with seed + position,
ranking) — with both matcher kinds."""
import os
import sys

import numpy as np
import pytest

import reloc_ref as rr
from reloc_ref import po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = rr.CAM
pytestmark = pytest.mark.gpu


def _ctx(pkg, kind, **kw):
    c = pkg.Context(width=0, height=0, max_keypoints=kw.pop("max_keypoints", 1024), **kw)
    c.set_matcher(kind)
    return c


def _fill(c, store):
    for cid, (d, w) in store.items():
        c.kf_add(cid, d, w)


def _rvec(R):
    th = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    return th / (2 * np.sin(th)) * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])


def _compare(got, ref, what=""):
    """pairs, counts, masks and best equal; poses within 1e-7 (the kernel against its own hypothesis-sequence oracle)"""
    assert got["best"] == ref["best"], (what, got["best"], ref["best"])
    assert len(got["candidates"]) == len(ref["candidates"])
    for k, (g, r) in enumerate(zip(got["candidates"], ref["candidates"])):
        tag = (what, k)
        assert np.array_equal(got["pairs"][k][0], r["pairs"][0]) and np.array_equal(got["pairs"][k][1], r["pairs"][1]), tag
        assert (g["n_matches"], g["n_correspondences"]) == (r["n_matches"], r["n_correspondences"]), tag
        assert g["status"] == r["status"], (tag, g["n_inliers"], r["n_inliers"])
        assert g["n_inliers"] == r["n_inliers"] and np.array_equal(got["inliers"][k], r["mask"]), (tag, g["n_inliers"], r["n_inliers"])
        if r["status"]:
            dR, dt = np.abs(po.rodrigues(g["rvec"]) - r["R"]).max(), np.abs(g["tvec"] - r["t"]).max()
            print("candidate", tag, "inliers", g["n_inliers"], "pose difference", dR, dt)
            assert dR < 1e-7 and dt < 1e-7, (tag, dR, dt)
        else:
            assert not g["rvec"].any() and not g["tvec"].any()


@pytest.mark.parametrize("kind", [0, 1], ids=["auto", "popcount"])
def test_store_round_trip(pkg, kind):
    c = _ctx(pkg, kind)
    rng = np.random.default_rng(1)
    entries = {i: (rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.normal(size=(n, 3))) for i, n in ((3, 600), (-7, 1), (40, 0), (41, 1024))}
    _fill(c, entries)
    assert c.kf_size() == 4
    for i, (d, w) in entries.items():
        gd, gw = c.kf_read(i)
        assert np.array_equal(gd, d) and np.array_equal(gw, w), i
    # an existing id is replaced
    d2, w2 = rng.integers(0, 256, (10, 32), dtype=np.uint8), rng.normal(size=(10, 3))
    c.kf_add(3, d2, w2)
    gd, gw = c.kf_read(3)
    assert c.kf_size() == 4 and np.array_equal(gd, d2) and np.array_equal(gw, w2)
    c.kf_remove(3)
    assert c.kf_size() == 3
    for call in (lambda: c.kf_read(3), lambda: c.kf_remove(3), lambda: c.kf_remove(12345)):
        with pytest.raises(pkg.MslamHipError) as e:
            call()
        assert e.value.code == pkg.E_INVALID
    c.kf_clear()
    assert c.kf_size() == 0
    c.close()


def test_store_grows_past_its_reservation_and_rejects_oversized_entries(pkg):
    c = _ctx(pkg, 0, max_keypoints=100)
    c.kf_reserve(2)
    rng = np.random.default_rng(2)
    entries = {i: (rng.integers(0, 256, (20 + i, 32), dtype=np.uint8), rng.normal(size=(20 + i, 3))) for i in range(70)}
    _fill(c, entries)                          # 70 entries: the store doubles several times, the early entries move with it
    assert c.kf_size() == 70
    for i, (d, w) in entries.items():
        gd, gw = c.kf_read(i)
        assert np.array_equal(gd, d) and np.array_equal(gw, w), i
    with pytest.raises(pkg.MslamHipError) as e:
        c.kf_add(500, rng.integers(0, 256, (101, 32), dtype=np.uint8), rng.normal(size=(101, 3)))
    assert e.value.code == pkg.E_CAPACITY
    c.kf_add(501, rng.integers(0, 256, (100, 32), dtype=np.uint8), rng.normal(size=(100, 3)))
    c.close()


def test_device_lift_equals_add_new_landmarks(pkg):
    """kf_add_from_batch_dev on a detected and back-projected synthetic batch against the reference lift, bit for bit (f64
    multiply / add in a fixed order, the library is built with -ffp-contract=off: no fused multiply-add)"""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth
    B, K = 3, 4096
    frames = synth.make_stream(B, 640, 480, seed=21)
    # depth: 1 m .. 4.2 m across the columns (so z <= 3 m cuts), with a band of invalid (zero) depth
    depth = np.tile((np.linspace(1.0, 4.2, 640) * 5000).astype(np.uint16), (B, 480, 1))
    depth[:, 100:180, :] = 0
    c = pkg.Context(width=640, height=480, max_batch=B, max_keypoints=K)
    d_frames = torch.from_numpy(np.stack(frames)).cuda()   # held until the sync: detection is only enqueued here, and a freed
    c.detect_batch_dev(d_frames.data_ptr(), B)              # tensor's block is what the depth upload below would be given
    d_depth = torch.from_numpy(depth.view(np.int16)).cuda()
    with pytest.raises(pkg.MslamHipError) as e:      # not back-projected yet
        c.kf_add_from_batch_dev(1, 0)
    assert e.value.code == pkg.E_INVALID
    c.backproject_batch_dev(d_depth.data_ptr(), focal=CAM[:2], principal=CAM[2:])
    poses = [(po.rodrigues([0.1 * f, -0.2, 0.05]), np.array([0.3, -0.1 * f, 1.5])) for f in range(B)]
    for f, (R, t) in enumerate(poses):
        c.kf_add_from_batch_dev(100 + f, f, R, t, 3.0)
    with pytest.raises(pkg.MslamHipError) as e:
        c.kf_add_from_batch_dev(1, B)
    assert e.value.code == pkg.E_INVALID
    c.sync()
    v, pv = c.batch_view(), c.points_view()
    cnt = pkg.read_device(c, v.count, (B,), np.int32)
    desc = pkg.read_device(c, v.desc, (B, K, 32), np.uint8)
    xyz = pkg.read_device(c, pv.xyz, (B, K, 3), np.float64)
    ok = pkg.read_device(c, pv.valid, (B, K), np.uint8)
    for f, (R, t) in enumerate(poses):
        n = int(cnt[f])
        rd, rw = rr.lift(desc[f, :n], xyz[f, :n], ok[f, :n], R, t, 3.0)
        gd, gw = c.kf_read(100 + f)
        print("frame", f, "keypoints", n, "valid", int(ok[f, :n].sum()), "landmarks", len(rd))
        assert 50 < len(rd) < int(ok[f, :n].sum()) < n            # both filters cut
        assert np.array_equal(gd, rd) and np.array_equal(gw, rw), f
    c.close()


@pytest.mark.parametrize("kind", [0, 1], ids=["auto", "popcount"])
def test_relocalize_equals_the_reference(pkg, orc, kind):
    sc = rr.make_scene(seed=0)
    c = _ctx(pkg, kind)
    _fill(c, sc["store"])
    # 5 candidates (the batched matcher shape) with the decoy first, and 4 (the few-pairs shape) with the target last
    for cand, seed in (([sc["decoy"]] + sc["ids"], 5), ([i for i in sc["ids"] if i != sc["target_id"]] + [sc["target_id"]], 11)):
        ref = rr.relocalize(sc["desc"], sc["xy"], sc["store"], cand, seed=seed)
        got = c.relocalize(sc["desc"], sc["xy"], cand, seed=seed, with_pairs=True)
        _compare(got, ref, (kind, len(cand)))
        j = cand.index(sc["target_id"])
        assert got["best"] == j and c.last_match_kernel() == ("matrix", "popcount")[kind]
        w = got["candidates"][j]
        assert np.abs(w["rvec"] - _rvec(sc["R"])).max() < 1e-6 and np.abs(w["tvec"] - sc["t"]).max() < 1e-6   # ground truth
        # the call without the optional outputs gives the same records
        bare = c.relocalize(sc["desc"], sc["xy"], cand, seed=seed)
        assert bare["best"] == got["best"]
        for a, b in zip(bare["candidates"], got["candidates"]):
            assert all(np.array_equal(a[k], b[k]) for k in a)
    # ties: the target twice — the first one wins; min_inliers at and above the winner's count
    tid = sc["target_id"]
    cand = [sc["ids"][0] if sc["ids"][0] != tid else sc["ids"][1], tid, tid]
    ref = rr.relocalize(sc["desc"], sc["xy"], sc["store"], cand, seed=9)
    got = c.relocalize(sc["desc"], sc["xy"], cand, seed=9, with_pairs=True)
    _compare(got, ref, "tie")
    n_in = got["candidates"][1]["n_inliers"]
    assert got["best"] == 1 and got["candidates"][2]["n_inliers"] == n_in
    assert c.relocalize(sc["desc"], sc["xy"], [tid], seed=9, min_inliers=n_in)["best"] == 0
    assert c.relocalize(sc["desc"], sc["xy"], [tid], seed=9, min_inliers=n_in + 1)["best"] == -1
    c.close()


@pytest.mark.parametrize("kind", [0, 1], ids=["auto", "popcount"])
def test_track_form_mask_and_guess(pkg, orc, kind):
    """one candidate, the depth mask of track() (rgbd_feature_frontend.cpp:317-334) and an extrinsic guess, 0.5 px noise"""
    sc = rr.make_scene(seed=2, noise=0.5)
    rng = np.random.default_rng(3)
    valid = rng.random(len(sc["desc"])) < 0.8
    tid = sc["target_id"]
    R0, t0 = po.rodrigues([0.01, -0.02, 0.015]) @ sc["R"], sc["t"] + 0.03
    c = _ctx(pkg, kind)
    _fill(c, sc["store"])
    ref = rr.relocalize(sc["desc"], sc["xy"], sc["store"], [tid], valid=valid, guess=(R0, t0), seed=4)
    got = c.relocalize(sc["desc"], sc["xy"], [tid], valid=valid, rvec=_rvec(R0), tvec=t0, seed=4, with_pairs=True)
    _compare(got, ref, "track")
    w = got["candidates"][0]
    assert got["best"] == 0 and w["n_correspondences"] < w["n_matches"]
    err_r, err_t = rr.rot_err(po.rodrigues(w["rvec"]), sc["R"]), np.linalg.norm(w["tvec"] - sc["t"])
    print("track form: ground-truth error", err_r, "deg", err_t, "m")
    assert err_r < 0.1 and err_t < 0.02
    c.close()


@pytest.mark.parametrize("kind", [0, 1], ids=["auto", "popcount"])
def test_relocalize_edges(pkg, orc, kind):
    sc = rr.make_scene(seed=4)
    rng = np.random.default_rng(8)
    store = dict(sc["store"])
    for i in range(70):                                    # small unrelated keyframes: the store grows past 64 entries
        n = 30 + i
        store[200 + i] = (rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.normal(size=(n, 3)) + [0, 0, 4])
    store[300] = (np.empty((0, 32), np.uint8), np.empty((0, 3)))                      # no landmark
    store[301] = (sc["store"][sc["target_id"]][0][:1].copy(), sc["store"][sc["target_id"]][1][:1].copy())   # one landmark
    c = _ctx(pkg, kind)
    _fill(c, store)
    tid = sc["target_id"]
    # no candidate
    got = c.relocalize(sc["desc"], sc["xy"], [], seed=1, with_pairs=True)
    assert got["best"] == -1 and got["candidates"] == []
    # one candidate
    _compare(c.relocalize(sc["desc"], sc["xy"], [tid], seed=1, with_pairs=True),
             rr.relocalize(sc["desc"], sc["xy"], store, [tid], seed=1), "one")
    # 64 candidates, the target at position 40, candidates with 0 and 1 landmarks among them
    cand = [200 + i for i in range(64)]
    cand[40], cand[3], cand[63] = tid, 300, 301
    ref = rr.relocalize(sc["desc"], sc["xy"], store, cand, seed=2)
    got = c.relocalize(sc["desc"], sc["xy"], cand, seed=2, with_pairs=True)
    _compare(got, ref, "64")
    assert got["best"] == 40 and got["candidates"][3]["n_matches"] == 0 and got["candidates"][63]["status"] == 0
    with pytest.raises(pkg.MslamHipError) as e:
        c.relocalize(sc["desc"], sc["xy"], cand + [tid], seed=2)        # 65 candidates
    assert e.value.code == pkg.E_INVALID
    # a query with one keypoint: no matches, no model
    one = c.relocalize(sc["desc"][:1], sc["xy"][:1], [tid], seed=1, with_pairs=True)
    assert one["best"] == -1 and one["candidates"][0]["n_matches"] == 0 and one["candidates"][0]["status"] == 0
    # an id that is not in the store; remove, then query
    for bad in ([tid, 77777], [77777]):
        with pytest.raises(pkg.MslamHipError) as e:
            c.relocalize(sc["desc"], sc["xy"], bad, seed=1)
        assert e.value.code == pkg.E_INVALID
    c.kf_remove(tid)
    with pytest.raises(pkg.MslamHipError) as e:
        c.relocalize(sc["desc"], sc["xy"], [tid], seed=1)
    assert e.value.code == pkg.E_INVALID
    # the others are untouched by the removal
    others = [i for i in sc["ids"] if i != tid] + [sc["decoy"]]
    _compare(c.relocalize(sc["desc"], sc["xy"], others, seed=3, with_pairs=True),
             rr.relocalize(sc["desc"], sc["xy"], store, others, seed=3), "after remove")
    c.close()


def test_python_adapters_verify_their_candidates(pkg, orc):
    """HipOrbRelocalizer.relocalizePose / HipLoopDetector.detectLoopVerified: the BoW candidates of relocalize() /
    detectLoop(), verified against the landmarks addKeyframeLandmarks stored; existing methods unchanged"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth
    sc = rr.make_scene(seed=6, n_landmarks=500, n_distractors=300)
    reloc = pkg.HipOrbRelocalizer(synth.make_vocabulary(10, 4, seed=5), ctx=pkg.Context(width=0, height=0, max_keypoints=1024))
    loop = pkg.HipLoopDetector(reloc, min_score=0.0, exclude_recent=0)
    kfs = {}
    for cid in sc["ids"]:
        d, w = sc["store"][cid]
        kps = [pkg.OrbKeypoint(i, (0.0, 0.0), d[i]) for i in range(len(d))]
        kfs[cid] = object()
        loop.feed(kfs[cid], kps)
        reloc.addKeyframeLandmarks(kfs[cid], kps, w)
    query = [pkg.OrbKeypoint(i, (float(x), float(y)), d) for i, ((x, y), d) in enumerate(zip(sc["xy"], sc["desc"]))]
    plain = reloc.relocalize(query)
    kf, pose, n_in, table = reloc.relocalizePose(query, seed=3)
    assert [row["keyframe"] for row in table] == plain and kf is kfs[sc["target_id"]]
    assert n_in > 300 and np.abs(pose[0] - _rvec(sc["R"])).max() < 1e-6 and np.abs(pose[1] - sc["t"]).max() < 1e-6
    entries = [e for row in table for e, k in reloc._entry_to_keyframe.items() if k is row["keyframe"]]
    store = {e: sc["store"][sc["ids"][e]] for e in entries}          # entry e = the e-th keyframe fed
    ref = rr.relocalize(sc["desc"], sc["xy"], store, entries, seed=3)
    assert [r["n_inliers"] for r in table] == [r["n_inliers"] for r in ref["candidates"]]
    loop.feed(object(), query)
    kf2, pose2, n2, _ = loop.detectLoopVerified(seed=3)
    assert loop.detectLoop() is kfs[sc["target_id"]] and kf2 is kfs[sc["target_id"]] and n2 > 300
    reloc.removeKeyframe(kfs[sc["target_id"]])
    kf3, _, _, table3 = reloc.relocalizePose(query, seed=3)
    assert kf3 is None and all(row["keyframe"] is not kfs[sc["target_id"]] for row in table3)
    assert reloc.ctx.kf_size() == len(sc["ids"]) - 1
    reloc.ctx.close()
