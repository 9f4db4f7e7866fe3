"""Guided matching on the GPU, through the C ABI, against tests/guided_match_ref.py: everything the matcher returns is
compared bit for bit (indices, distances, candidate counts, pairs); the mode of mslam_hip_set_guided_match against the
reference composition record for record, poses within 1e-7 (the PnP kernel against its hypothesis-sequence oracle, the
bound tests/test_gpu_reloc.py and tests/test_gpu_track.py use).  tests/test_guided_match.py proves the planted scenes."""
import numpy as np
import pytest

import guided_match_ref as gr
import reloc_ref as rr
from reloc_ref import po

CAM = gr.CAM
pytestmark = pytest.mark.gpu
FRAMES = [(640, 480), (100, 80), (20, 20), (4114, 102)]      # 20 x 20: smaller than a cell; 4114: the detector's own limit
RADII = [0.5, 15.0, 47.5]
N_KP = [0, 1, 2, 63, 64, 65, 700]
N_LM = [0, 1, 7, 8, 9, 64, 65, 513]
# every keypoint count with 65 landmarks, every landmark count with 65 keypoints, and the corners
SIZES = sorted({(k, 65) for k in N_KP} | {(65, l) for l in N_LM} | {(0, 0), (700, 513), (1, 1), (0, 513), (700, 0)})


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(width=0, height=0, max_keypoints=2048)
    yield c
    c.close()


def _args(sc):
    return sc["kp_desc"], sc["kp_xy"], sc["lm_desc"], sc["lm_world"], sc["R"], sc["t"]


def _kw(sc):
    return dict(focal=sc["cam"][:2], principal=sc["cam"][2:], width=sc["width"], height=sc["height"])


def _check_knn2(c, sc, radius, what=""):
    got = c.match_guided_knn2(*_args(sc), radius, **_kw(sc))
    ref = gr.knn2(*_args(sc), radius, sc["cam"], sc["width"], sc["height"])
    for name, g, r in zip(("idx0", "idx1", "dist0", "dist1", "n_cand"), got, ref):
        assert g.dtype == np.int32 and np.array_equal(g, r), (what, name, np.flatnonzero(g != r)[:8])
    assert c.last_match_kernel() == "guided" or len(sc["lm_desc"]) == 0
    return got


def _check_match(c, sc, radius, max_distance=256, ratio=0.7, what=""):
    fi, ti = c.match_guided(*_args(sc), radius, max_distance, ratio, **_kw(sc))
    rfi, rti = gr.match(*_args(sc), radius, max_distance, ratio, sc["cam"], sc["width"], sc["height"])
    assert np.array_equal(fi, rfi) and np.array_equal(ti, rti), (what, max_distance, len(fi), len(rfi))
    return fi, ti


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("size", FRAMES, ids=["%dx%d" % s for s in FRAMES])
def test_sizes(ctx, size, radius):
    seen = 0
    for n_kp, n_lm in SIZES:
        sc = gr.random_scene(1000 * n_kp + n_lm + size[0], n_kp, n_lm, *size)
        got = _check_knn2(ctx, sc, radius, (n_kp, n_lm))
        fi, _ = _check_match(ctx, sc, radius, what=(n_kp, n_lm))
        seen += int(got[4].sum())
    assert seen > 0                                    # the comparison is not one of empty windows only


@pytest.mark.parametrize("kind", [0, 1], ids=["auto", "popcount"])
@pytest.mark.parametrize("size", FRAMES, ids=["%dx%d" % s for s in FRAMES])
def test_whole_frame_radius_is_the_brute_force_matcher(pkg, size, kind):
    """every keypoint in the frame, every landmark in front of the camera and at most 10 px beyond the frame, radius = the
    larger extent + 10: the candidates are all keypoints, and knn-2 and the accepted pairs are match_knn2's and match's"""
    c = pkg.Context(width=0, height=0, max_keypoints=2048)
    c.set_matcher(kind)
    radius = float(max(size)) + 10.0
    for n_kp, n_lm in ((2, 9), (65, 64), (700, 65), (64, 513)):
        sc = gr.random_scene(7 + n_kp + n_lm, n_kp, n_lm, *size)
        i0, i1, d0, d1, nc = c.match_guided_knn2(*_args(sc), radius, **_kw(sc))
        assert (nc == n_kp).all()
        b = c.match_knn2(sc["kp_desc"], sc["lm_desc"])
        assert c.last_match_kernel() == ("popcount" if kind else "matrix")
        for g, r in zip((i0, i1, d0, d1), b):
            assert np.array_equal(g, r), (n_kp, n_lm)
        fi, ti = c.match_guided(*_args(sc), radius, **_kw(sc))
        bfi, bti = c.match(sc["kp_desc"], sc["lm_desc"])
        assert np.array_equal(fi, bfi) and np.array_equal(ti, bti) and (n_kp < 65 or len(fi) > 0)
    c.close()


@pytest.mark.parametrize("radius", RADII)
def test_exact_edges(ctx, radius):
    sc = gr.edge_scene(radius)
    i0, i1, d0, d1, nc = _check_knn2(ctx, sc, radius)
    assert nc.tolist() == [len(sc["expect"][j]) for j in range(len(nc))]
    for j, want in sc["expect"].items():              # with at most two candidates the pair IS the window
        if len(want) <= 2:
            assert sorted(k for k in (i0[j], i1[j]) if k >= 0) == want, j
    _check_match(ctx, sc, radius)


def test_ties_and_extremes(ctx):
    sc = gr.tie_scene()
    i0, i1, d0, d1, nc = _check_knn2(ctx, sc, sc["radius"])
    A = int(gr.ABSENT)
    assert d0.tolist() == [3, 0, 200, 255, 256, 0, 9] and d1.tolist() == [3, 256, A, 256, A, A, 10]
    assert i1[0] == i0[0] + 1                          # equal descriptors: the lower index first
    for md, want in ((0, [1, 5]), (255, [1, 2, 5]), (256, [1, 2, 4, 5])):
        fi, ti = _check_match(ctx, sc, sc["radius"], md)
        assert ti.tolist() == want                     # a lone candidate passes without a ratio test; d0 == d1 does not
    for ratio in (0.9, 0.91, 1.0, 1.01):               # the table of the ratio at its integer edges
        _check_match(ctx, sc, sc["radius"], 256, ratio)


def test_a_crowded_cell(ctx):
    sc = gr.crowded_scene()
    i0, i1, d0, d1, nc = _check_knn2(ctx, sc, sc["radius"])
    assert nc.tolist() == [0, 3000, 0] and i0[0] == -1 and i0[2] == -1 and i0[1] >= 0 and i1[1] >= 0
    _check_match(ctx, sc, sc["radius"])


def test_errors_leave_the_context_usable(pkg, ctx):
    sc = gr.random_scene(1, 65, 9, 100, 80)
    a, kw = _args(sc), _kw(sc)
    bad = [lambda: ctx.match_guided_knn2(*a, float("nan"), **kw), lambda: ctx.match_guided_knn2(*a, 0.0, **kw),
           lambda: ctx.match_guided_knn2(*a, -1.0, **kw), lambda: ctx.match_guided(*a, 5.0, -1, **kw),
           lambda: ctx.match_guided(*a, 5.0, 257, **kw), lambda: ctx.match_guided(*a, 5.0, **dict(kw, width=0)),
           lambda: ctx.match_guided(*a, 5.0, **dict(kw, height=8193)), lambda: ctx.match_guided(*a, 5.0, **dict(kw, focal=(0.0, 1.0))),
           lambda: ctx.match_guided_knn2(*a, 5.0, **dict(kw, focal=(1.0, float("nan")))),
           lambda: ctx.set_guided_match(float("nan"), 256, 640, 480), lambda: ctx.set_guided_match(15.0, 257, 640, 480),
           lambda: ctx.set_guided_match(15.0, -1, 640, 480), lambda: ctx.set_guided_match(15.0, 256, 0, 480),
           lambda: ctx.set_guided_match(15.0, 256, 640, 8193)]
    for k, call in enumerate(bad):
        with pytest.raises(pkg.MslamHipError) as e:
            call()
        assert e.value.code == pkg.E_INVALID, k
    assert ctx.get_guided_match() == (0.0, 256, 0, 0)              # a refused setter changes nothing
    ctx.set_guided_match(-3.0, 7, 0, 0)                            # off: the extent is not checked
    assert ctx.get_guided_match() == (0.0, 7, 0, 0)
    ctx.set_guided_match(0.0, 256, 0, 0)
    big = gr.random_scene(2, 4, 4, 8192, 8192)                     # the largest extent: 128-px cells
    _check_knn2(ctx, big, 3000.0)
    _check_knn2(ctx, sc, 15.0)


# ---- the mode -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mode(orc):
    m = gr.mode_frames()
    m["rvec"], m["tvec"] = gr.rvec_of(m["guess"][0]), m["guess"][1]
    return m


def _mode_ctx(pkg, m, radius=None, max_distance=256, kind=0):
    c = pkg.Context(width=0, height=0, max_keypoints=2048)
    c.set_matcher(kind)
    for cid, (d, w) in m["store"].items():
        c.kf_add(cid, d, w)
    if radius is not None:
        c.set_guided_match(radius, max_distance, 640, 480)
    return c


def _same_pose(got_R, got_t, ref, what):
    d = max(np.abs(got_R - ref["R"]).max(), np.abs(got_t - ref["t"]).max())
    print(what, "pose difference", d)
    assert d < 1e-7, (what, d)


def _compare_counts(got, ref, what):
    assert (got["n_matches"], got["n_correspondences"], got["status"], got["n_inliers"]) == \
        (ref["n_matches"], ref["n_correspondences"], ref["status"], ref["n_inliers"]), (what, got, ref["n_matches"])


@pytest.mark.parametrize("radius,max_distance", [(15.0, 256), (47.5, 64)])
def test_mode_relocalize(pkg, mode, radius, max_distance):
    c = _mode_ctx(pkg, mode, radius, max_distance)
    fr = mode["frames"][0]
    valid = (np.arange(len(fr["desc"])) % 7 != 0).astype(np.uint8)
    ids = [1, 0, 2]
    got = c.relocalize(fr["desc"], fr["xy"], ids, valid=valid, seed=5, rvec=mode["rvec"], tvec=mode["tvec"], min_inliers=30,
                       with_pairs=True)
    assert c.last_match_kernel() == "guided"
    ref = gr.relocalize(fr["desc"], fr["xy"], mode["store"], ids, mode["guess"], radius, max_distance, valid=valid, seed=5,
                        min_inliers=30)
    print("matches", [k["n_matches"] for k in ref["candidates"]], "inliers", [k["n_inliers"] for k in ref["candidates"]])
    assert got["best"] == ref["best"] == 1 and ref["candidates"][1]["n_inliers"] > 100
    for k, (g, r) in enumerate(zip(got["candidates"], ref["candidates"])):
        _compare_counts(g, r, ("candidate", k))
        assert np.array_equal(got["pairs"][k][0], r["pairs"][0]) and np.array_equal(got["pairs"][k][1], r["pairs"][1]), k
        assert np.array_equal(got["inliers"][k], r["mask"]), k
        if r["status"]:
            _same_pose(po.rodrigues(g["rvec"]), g["tvec"], r, ("candidate", k))
    c.close()


def _compare_step(got, ref, what):
    _compare_counts(got, ref, what)
    assert bool(got["tracked"]) == ref["tracked"] and bool(got["keyframe_required"]) == ref["keyframe_required"], what
    assert np.array_equal(got["vote_counts"], ref["vote_counts"]), what
    assert (got["vote_best"], got["vote_best_count"]) == (ref["vote_best"], ref["vote_best_count"]), what
    if ref["status"]:
        _same_pose(got["R"], got["tvec"], ref, what)
    else:
        assert not got["R"].any() and not got["tvec"].any()


@pytest.fixture(scope="module")
def window_steps(mode):
    """the reference composition of the 17-frame window, computed once: a shorter window is its prefix (frame s has the
    seed 40 + s and the shared guess whatever the window's length).  max_distance = 64: a lone stranger in a window (about
    128 bits away) is not a match, so the far frame 12 has none and is the window's first event"""
    fr = mode["frames"]
    return gr.track_window([f["desc"] for f in fr], [f["xy"] for f in fr], [f["depth"] for f in fr], mode["store"], 0, mode["guess"],
                           15.0, 64, [0, 1], 0, seed=40)


def test_mode_track(pkg, mode, window_steps):
    c = _mode_ctx(pkg, mode, 15.0, 64)
    for s in (0, 12):                                  # a frame that is tracked, and the far one
        fr = mode["frames"][s]
        got = c.track(fr["desc"], fr["xy"], fr["depth"], 0, [0, 1], -1, seed=40 + s, rvec=mode["rvec"], tvec=mode["tvec"],
                      with_pairs=True)
        assert c.last_match_kernel() == "guided"
        ref = window_steps[0][s]
        _compare_step(got, ref, ("track", s))
        assert np.array_equal(got["pairs"][0], ref["pairs"][0]) and np.array_equal(got["pairs"][1], ref["pairs"][1])
        assert np.array_equal(got["inliers"], ref["mask"])
        assert bool(got["tracked"]) == (s == 0)
    c.close()


@pytest.mark.parametrize("S", [1, 5, 17])
def test_mode_track_window(pkg, mode, window_steps, S):
    c = _mode_ctx(pkg, mode, 15.0, 64)
    fr = mode["frames"][:S]
    recs, first = c.track_window([f["desc"] for f in fr], [f["xy"] for f in fr], [f["depth"] for f in fr], 0, [0, 1], -1, 0,
                                 seed=40, rvec=mode["rvec"], tvec=mode["tvec"])
    assert c.last_match_kernel() == "guided"
    steps, ref_first = window_steps
    assert first == min(ref_first, S) and ref_first == 12 and len(recs) == S
    for s in range(S):
        _compare_step(recs[s], steps[s], ("window", S, s))
    c.close()


def test_mode_track_window_dev(pkg, orc):
    """the device form on a detected batch: the guess is the identity (rvec = 0 becomes R = I exactly), the reference
    composition runs on the batch's own arrays read back"""
    import torch
    import synth
    B, K, radius = 4, 2048, 47.5
    stream = synth.make_stream(B, 640, 480, seed=1234)
    depth = np.ascontiguousarray(synth.make_depth(B, 640, 480))
    c = pkg.Context(width=640, height=480, max_batch=B, max_keypoints=K)
    c.set_guided_match(radius)                         # the context's own frame size
    assert c.get_guided_match() == (radius, 256, 640, 480)
    d_frames = torch.from_numpy(stream).cuda()
    d_depth = torch.from_numpy(depth.view(np.int16)).cuda()
    c.detect_batch_dev(d_frames.data_ptr(), B)
    c.backproject_batch_dev(d_depth.data_ptr(), focal=CAM[:2], principal=CAM[2:])
    c.kf_add_from_batch_dev(0, 0, np.eye(3), np.zeros(3), 3.0)
    c.sync()
    v = c.batch_view()
    cnt = pkg.read_device(c, v.count, (B,), np.int32)
    desc = pkg.read_device(c, v.desc, (B, K, 32), np.uint8)
    xy = pkg.read_device(c, v.xy, (B, K, 2), np.float32)
    store = {0: c.kf_read(0)}
    recs, first = c.track_window_dev(1, B - 1, 0, [0], -1, 0, focal=CAM[:2], principal=CAM[2:], seed=7, rvec=np.zeros(3),
                                     tvec=np.zeros(3))
    assert c.last_match_kernel() == "guided"
    steps, ref_first = gr.track_window([desc[f, :cnt[f]] for f in range(1, B)], [xy[f, :cnt[f]] for f in range(1, B)],
                                       [depth[f] for f in range(1, B)], store, 0, (np.eye(3), np.zeros(3)), radius, 256, [0], 0,
                                       seed=7)
    print("dev window", [(r["n_matches"], r["n_correspondences"], r["n_inliers"], r["tracked"]) for r in recs])
    assert first == ref_first and max(r["n_matches"] for r in recs) > 0
    for s in range(B - 1):
        _compare_step(recs[s], steps[s], ("dev", s))
    c.close()


def _bytes_of(x):
    if isinstance(x, dict):
        return {k: _bytes_of(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_bytes_of(v) for v in x]
    return np.asarray(x).tobytes()


@pytest.mark.parametrize("kind", [0, 1], ids=["auto", "popcount"])
def test_mode_off_and_calls_without_a_guess_are_byte_identical(pkg, mode, kind):
    plain = _mode_ctx(pkg, mode, None, kind=kind)                  # never set
    unset = _mode_ctx(pkg, mode, 15.0, 64, kind=kind)              # set, then switched off
    unset.set_guided_match(0.0, 64, 640, 480)
    on = _mode_ctx(pkg, mode, 15.0, 64, kind=kind)                 # on
    fr = mode["frames"][:3]
    guess = dict(rvec=mode["rvec"], tvec=mode["tvec"])
    kernel = "popcount" if kind else "matrix"

    def calls(c, **g):
        f = fr[0]
        out = [c.relocalize(f["desc"], f["xy"], [1, 0, 2], seed=5, min_inliers=30, with_pairs=True, **g),
               c.track(f["desc"], f["xy"], f["depth"], 0, [0, 1], -1, seed=40, with_pairs=True, **g),
               c.track_window([x["desc"] for x in fr], [x["xy"] for x in fr], [x["depth"] for x in fr], 0, [0, 1], -1, 0, seed=40, **g)]
        return _bytes_of(out), c.last_match_kernel()

    base_guess, k0 = calls(plain, **guess)
    base_bare, k1 = calls(plain)
    assert k0 == k1 == kernel
    assert calls(unset, **guess) == (base_guess, kernel) and calls(unset) == (base_bare, kernel)
    assert calls(on) == (base_bare, kernel)                        # no guess: the brute-force stage, the same bytes
    got, k = calls(on, **guess)
    assert k == "guided" and got != base_guess                     # (and with one, the mode does change the matches)
    for c in (plain, unset, on):
        c.close()


# ---- what the feature is for ------------------------------------------------------------------------------------------------

def test_twins_scene_tracks_where_brute_force_cannot(pkg, orc):
    tw = gr.twins_scene()
    guess = gr.perturbed(tw["R"], tw["t"], 0.5, 0.01)
    kw = dict(seed=3, rvec=gr.rvec_of(guess[0]), tvec=guess[1], with_pairs=True)
    c = pkg.Context(width=0, height=0, max_keypoints=1024)
    c.kf_add(0, *tw["store"][0])
    brute = c.track(tw["desc"], tw["xy"], tw["depth"], 0, [0], -1, **kw)
    assert brute["n_matches"] == 0 and not brute["tracked"] and not brute["status"]          # E_NO_MODEL
    c.set_guided_match(tw["radius"], 256, 640, 480)
    got = c.track(tw["desc"], tw["xy"], tw["depth"], 0, [0], -1, **kw)
    ref = gr.track(tw["desc"], tw["xy"], tw["depth"], tw["store"], 0, guess, tw["radius"], 256, [0], seed=3)
    assert got["tracked"] and ref["tracked"] and got["n_matches"] == len(tw["own"])
    assert np.array_equal(got["pairs"][0], tw["own"]) and np.array_equal(got["pairs"][1], np.arange(len(tw["own"])))
    _compare_step(got, ref, "twins")
    assert np.array_equal(got["inliers"], ref["mask"])
    err_deg, err_m = rr.rot_err(got["R"], tw["R"]), float(np.linalg.norm(got["tvec"] - tw["t"]))
    print("twins: inliers", got["n_inliers"], "of", got["n_matches"], "pose error", err_deg, "deg", err_m, "m")
    assert err_deg < 0.1 and err_m < 0.02
    c.close()


def test_create_set_mode_track_destroy_returns_device_memory(pkg, mode):
    """Four create / set mode / track / destroy cycles on growing sizes.  tests/test_gpu_lifetime.py's own criterion: what
    free device memory loses from the end of cycle 2 to the end of cycle 4 is at most one driver granule (the smallest
    step in which free memory is seen to move in this run) — that file's bound with its parent drift of 0."""
    import torch
    readings, free = [], []
    for k in range(4):
        readings.append(torch.cuda.mem_get_info()[0])
        c = _mode_ctx(pkg, mode, 15.0 + 10 * k)
        readings.append(torch.cuda.mem_get_info()[0])
        fr = mode["frames"][:1 + 4 * k]
        n = 200 * (k + 1)
        got = c.track(fr[0]["desc"][:n], fr[0]["xy"][:n], fr[0]["depth"], 0, [0, 1], -1, seed=1, rvec=mode["rvec"], tvec=mode["tvec"])
        c.track_window([f["desc"][:n] for f in fr], [f["xy"][:n] for f in fr], [f["depth"] for f in fr], 0, [0, 1], -1, 0, seed=1,
                       rvec=mode["rvec"], tvec=mode["tvec"])
        assert c.last_match_kernel() == "guided" and got["n_matches"] > 0
        readings.append(torch.cuda.mem_get_info()[0])
        c.close()
        free.append(torch.cuda.mem_get_info()[0])
        readings.append(free[-1])
    steps = [abs(b - a) for a, b in zip(readings, readings[1:]) if b != a]
    assert steps, "free device memory never moved: the cycles allocated nothing"
    drift = free[1] - free[3]
    print("free after each close", free, "drift(2 -> 4)", drift, "granule", min(steps))
    assert drift <= min(steps), (drift, min(steps))
