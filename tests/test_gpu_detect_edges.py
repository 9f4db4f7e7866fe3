"""GPU parity of the native front end (k_level / k_pyramid / k_blur, k_fast, k_quadtree, k_describe and build_geometry)
where test_gpu_parity.py's natural frames never go: cell remainders and the size limits of build_geometry, frames
narrower than one 64-px tile, sparse and ragged batches through k_describe (and the matcher and the packer behind it),
exact symmetries of the intensity centroid, and quadtree ties.  Every comparison is bit-exact against the oracle, stage
by stage and end to end; a detection that differs is attributed to one keypoint and one stage by explain().
tests/test_detect_edge_frames.py proves on the CPU that the inputs (tests/detect_edge_frames.py) reach those regimes."""
import numpy as np
import pytest

import detect_edge_frames as F

pytestmark = pytest.mark.gpu

def _ctx(pkg, W, H, p, **kw):
    return pkg.Context(width=W, height=H, n_levels=p["n_levels"], scale_factor=p["scale_factor"], ini_fast_thr=p["ini_fast_thr"],
                       min_fast_thr=p["min_fast_thr"], min_node_area=p["min_node_area"], **kw)


def _ref(orc, frame, p):
    d = orc.detect(frame, F.oparams(orc, p))
    for a in d.values():
        a.setflags(write=False)
    return d


def explain(ctx, frame_index, frame, params, got, orc):
    """Turns "desc differs" into "keypoint 412, level 3, (x, y): angle ok, descriptor bytes 8-15 differ": reads DBG_SELECTED
    of every level, recomputes orientation and descriptor of every selected keypoint from the oracle's planes and names
    the first keypoint that differs and which of selection / angle / descriptor / xy scaling / octave is wrong."""
    op = F.oparams(orc, params)
    H, W = frame.shape[:2]
    pyr = orc.pyramid(orc.gray(frame), op)
    _, _, scale = orc.level_geometry(W, H, op)
    ref_sel = F.level_selected(orc, frame, params)
    k = 0
    for l in range(params["n_levels"]):
        sel = ctx.debug_keypoints(F.DBG_SELECTED, frame_index, l)
        if not F.same_bits(sel, ref_sel[l]):
            n = min(len(sel), len(ref_sel[l]))
            bad = np.nonzero((sel[:n] != ref_sel[l][:n]).any(1))[0]
            i = int(bad[0]) if len(bad) else n
            return "selection: level %d has %d keypoints, the oracle %d; first difference at entry %d (%s vs %s)" % (
                l, len(sel), len(ref_sel[l]), i, sel[i].tolist() if i < len(sel) else None,
                ref_sel[l][i].tolist() if i < len(ref_sel[l]) else None)
        blurred = orc.gaussian_blur7(pyr[l]) if len(sel) else None
        for x, y, resp in sel:
            px, py = int(x) + F.BORDER, int(y) + F.BORDER
            where = "keypoint %d, level %d, (%d, %d)" % (k, l, px, py)
            if k >= len(got["xy"]):
                return "count: %d keypoints returned, %s is missing" % (len(got["xy"]), where)
            ang = np.float32(orc.ic_angle(pyr[l], px, py))
            if got["octave"][k] != l:
                return "%s: octave %d" % (where, got["octave"][k])
            fx, fy = np.float32(px), np.float32(py)
            if l:
                fx, fy = fx * scale[l], fy * scale[l]
            if not F.same_bits(got["xy"][k], np.array([fx, fy], np.float32)):
                return "%s: xy scaling %s, expected %s" % (where, got["xy"][k].tolist(), [float(fx), float(fy)])
            if got["response"][k] != resp:
                return "%s: response %s, selected %s" % (where, got["response"][k], resp)
            if got["angle"][k].view(np.uint32) != ang.view(np.uint32):
                return "%s: angle %r, expected %r" % (where, float(got["angle"][k]), float(ang))
            d = orc.orb_descriptor(blurred, px, py, ang)
            if not np.array_equal(got["desc"][k], d):
                bad = np.nonzero(got["desc"][k] != d)[0]
                return "%s: angle ok, descriptor bytes %s differ" % (where, bad.tolist())
            k += 1
    if k != len(got["xy"]):
        return "count: %d keypoints returned, %d selected" % (len(got["xy"]), k)
    return "stages agree with the oracle's primitives (the difference is between orc.detect and its own stages)"


def _assert_same(got, ref, what, ctx, slot, frame, p, orc):
    ok = len(got["xy"]) == len(ref["xy"]) and all(F.same_bits(got[k], ref[k]) for k in F.KEYS)
    if not ok:
        bad = ["count"] if len(got["xy"]) != len(ref["xy"]) else [k for k in F.KEYS if not F.same_bits(got[k], ref[k])]
        why = explain(ctx, slot, frame, p, got, orc)
        raise AssertionError("%s: %s differ (%d vs %d keypoints); %s" % (what, bad, len(got["xy"]), len(ref["xy"]), why))


def _assert_planes(pkg, orc, c, frame, p, slot, what):
    for l, img in enumerate(orc.pyramid(orc.gray(frame), F.oparams(orc, p))):
        assert np.array_equal(c.debug_image(pkg.DBG_PYRAMID, slot, l), img), (what, "pyramid level %d" % l)
        assert np.array_equal(c.debug_image(pkg.DBG_BLURRED, slot, l), orc.gaussian_blur7(img)), (what, "blurred level %d" % l)


def _assert_lists(pkg, c, cand, sel, slot, what):
    for l in range(len(cand)):
        got = c.debug_keypoints(pkg.DBG_CANDIDATES, slot, l)
        assert len(got) == len(cand[l]) and F.same_bits(got, cand[l]), (what, "FAST level %d" % l, len(got), len(cand[l]))
        got = c.debug_keypoints(pkg.DBG_SELECTED, slot, l)
        assert len(got) == len(sel[l]) and F.same_bits(got, sel[l]), (what, "selection level %d" % l, len(got), len(sel[l]))


def _run_batch(c, frames):
    import torch
    dev = torch.from_numpy(np.ascontiguousarray(np.stack(frames))).cuda()
    c.detect_batch_dev(dev.data_ptr(), len(frames))
    c.sync()
    return dev      # (kept alive by the caller until the results are read)


def _read_batch(pkg, c, n):
    """the first n frames of the batch view as a list of detect()-shaped dicts"""
    K = c.params.max_keypoints
    v = c.batch_view()
    cnt = pkg.read_device(c, v.count, (n,), np.int32)
    assert (cnt >= 0).all() and (cnt <= K).all(), cnt
    arr = dict(xy=pkg.read_device(c, v.xy, (n, K, 2), np.float32), desc=pkg.read_device(c, v.desc, (n, K, 32), np.uint8),
               octave=pkg.read_device(c, v.octave, (n, K), np.int32), angle=pkg.read_device(c, v.angle, (n, K), np.float32),
               response=pkg.read_device(c, v.response, (n, K), np.float32))
    return [{k: a[t, :cnt[t]] for k, a in arr.items()} for t in range(n)]


def _capacities(W, H):
    return dict(max_keypoints=32768, max_candidates=min(1 << 18, max(4096, W * H // 2)))


_GEOMETRY = F.geometry_cases()


@pytest.mark.parametrize("case", _GEOMETRY, ids=["%dx%d-%d" % c[:3] for c in _GEOMETRY])
def test_geometry_sizes(pkg, orc, case):
    """every cell remainder (7-px and dropped columns and rows), frames narrower than a tile, and the accepted side of
    each limit of build_geometry: level sizes and the FAST cell table, every pyramid and blurred plane, DBG_CANDIDATES,
    DBG_SELECTED and the detection — of a single call and of the first, middle and last member of a 9-frame batch"""
    W, H, n, frame = case
    p = F.P(n_levels=n, **F.GEOMETRY_P)
    ref, cand, sel = _ref(orc, frame, p), F.level_candidates(orc, frame, p), F.level_selected(orc, frame, p)
    c = _ctx(pkg, W, H, p, max_batch=9, **_capacities(W, H))
    try:
        w, h, s = orc.level_geometry(W, H, F.oparams(orc, p))
        gw, gh, gs = c.level_geometry()
        assert (gw, gh) == (w, h) and F.same_bits(gs, s)
        for l in range(n):
            assert np.array_equal(c.debug_cells(l), F.reference_cells(w[l], h[l])), "FAST cells of level %d" % l
        got = c.detect(frame, max_out=32768)
        _assert_planes(pkg, orc, c, frame, p, 0, "single")
        _assert_lists(pkg, c, cand, sel, 0, "single")
        _assert_same(got, ref, "single", c, 0, frame, p, orc)
        dev = _run_batch(c, [frame] * 9)
        batch = _read_batch(pkg, c, 9)
        for t in (0, 4, 8):
            _assert_planes(pkg, orc, c, frame, p, t, "batch member %d" % t)
            _assert_lists(pkg, c, cand, sel, t, "batch member %d" % t)
            _assert_same(batch[t], ref, "batch member %d" % t, c, t, frame, p, orc)
        del dev
    finally:
        c.close()


_FORMS = [("fused-0", {"MSLAM_HIP_FUSED_LEVELS": "0"}, False), ("fused-16", {"MSLAM_HIP_FUSED_LEVELS": "16"}, False),
          ("rows", {"MSLAM_HIP_TILED_BLUR": "0"}, False), ("tiled", {"MSLAM_HIP_TILED_BLUR": "1"}, False),
          ("chain-1-4", {"MSLAM_HIP_LEVEL_CHAIN": "1", "MSLAM_HIP_LEVEL_CHAIN_FRAMES": "1", "MSLAM_HIP_LEVEL_CHAIN_WAVES": "4"}, True),
          ("chain-3-8", {"MSLAM_HIP_LEVEL_CHAIN": "1", "MSLAM_HIP_LEVEL_CHAIN_FRAMES": "3", "MSLAM_HIP_LEVEL_CHAIN_WAVES": "8"}, True)]


@pytest.mark.parametrize("form", _FORMS, ids=[f[0] for f in _FORMS])
def test_geometry_sizes_kernel_forms(pkg, orc, monkeypatch, form):
    """the six sizes below 128 px (and the widths below 64 that are multiples of 4: the only ones the fused kernels, the
    tiled blurred slab and the level chain take) under every form of the level kernels — all read at context creation
    (csrc/api.hip: create_impl), so they are set before it: planes and detections of a single call and of a 10-frame
    batch.  A level narrower than 64 px is one partial tile column with pitch 64."""
    _, env, chain = form
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for W, H, n, frame in F.small_geometry_cases():
        p = F.P(n_levels=n, **F.GEOMETRY_P)
        ref = _ref(orc, frame, p)
        c = _ctx(pkg, W, H, p, max_batch=10, **_capacities(W, H))
        try:
            what = (form[0], W, H)
            # the form this context took (DBG_FORMS): the fused kernels want dword columns, so only the widths that are
            # multiples of 4 reach them, and only a context whose levels are all fused keeps the blurred slab in tiles
            fused, tiled_slab = c.debug_forms()
            want_fused = n if W % 4 == 0 and env.get("MSLAM_HIP_FUSED_LEVELS") != "0" else 0
            want_tiled = 1 if want_fused == n and env.get("MSLAM_HIP_TILED_BLUR") != "0" else 0
            assert (fused, tiled_slab) == (want_fused, want_tiled), (what, "form", fused, tiled_slab)
            got = c.detect(frame, max_out=32768)
            _assert_planes(pkg, orc, c, frame, p, 0, what)
            _assert_same(got, ref, what, c, 0, frame, p, orc)
            c.set_profiling(2)
            dev = _run_batch(c, [frame] * 10)     # (the chain takes batches from 8 frames on; 10 = 3 + 3 + 3 + 1)
            stages = {nm for nm, _ in c.stage_times()}
            c.set_profiling(0)
            assert ("levels" in stages) == bool(chain and want_tiled), (what, "level chain", sorted(stages))
            assert ("blur" in stages) == (want_fused < n), (what, "stand-alone blur", sorted(stages))
            batch = _read_batch(pkg, c, 10)
            for t in (0, 5, 9):
                _assert_planes(pkg, orc, c, frame, p, t, what + (t,))
                _assert_same(batch[t], ref, what + (t,), c, t, frame, p, orc)
            del dev
        finally:
            c.close()


def test_rejected_geometries(pkg, orc):
    """each limit of build_geometry from the outside: creation fails with E_INVALID (before any device work), and a valid
    context created afterwards in the same process detects correctly"""
    for W, H, n, why in F.rejected_geometries():
        with pytest.raises(pkg.MslamHipError) as e:
            _ctx(pkg, W, H, F.P(n_levels=n, **F.GEOMETRY_P))
        assert e.value.code == pkg.E_INVALID, (W, H, n, why)
    assert pkg.DBG_SELECTED == F.DBG_SELECTED
    W, H, n, frame = F.geometry_cases()[1]
    p = F.P(n_levels=n, **F.GEOMETRY_P)
    c = _ctx(pkg, W, H, p, **_capacities(W, H))
    try:
        _assert_same(c.detect(frame), _ref(orc, frame, p), "after the rejections", c, 0, frame, p, orc)
    finally:
        c.close()


@pytest.fixture(scope="module")
def sparse(orc):
    """the sparse 640 x 480 frames, two ordinary synthetic views, and the oracle's detections (default parameters)"""
    import synth
    frames = dict(F.sparse_frames())
    tex = synth.make_stream(2, 640, 480, seed=1234)
    frames["texture0"], frames["texture1"] = tex[0], tex[1]
    return frames, {k: _ref(orc, f, F.P()) for k, f in frames.items()}


@pytest.mark.parametrize("mirror", ["1", "0"])
def test_sparse_single_frames(pkg, orc, sparse, monkeypatch, mirror):
    """frames with 0, 1, 2, 3, 4, 5 and 7 keypoints, an empty first level, empty middle levels, and totals on both sides
    of 64 and of 2048 (one full sweep of k_describe's base loop) through the synchronous call, both result paths
    (k_describe's mirror into the mapped block, and the packing kernel), on ONE context in an order that alternates
    large and tiny counts: rows of the call before must not show"""
    monkeypatch.setenv("MSLAM_HIP_MIRROR_RESULTS", mirror)
    frames, refs = sparse
    order = ["above_2048", "flat", "below_2048", "kp1", "texture0", "kp2", "above_64", "empty_middle", "below_64", "kp3",
             "above_2048", "one_square", "kp5", "flat", "kp4", "below_2048", "kp1"]
    assert set(order) >= set(F.sparse_frames())
    p = F.P()
    c = _ctx(pkg, 640, 480, p, max_keypoints=4096)
    try:
        for i, name in enumerate(order):
            got = c.detect(frames[name])
            _assert_same(got, refs[name], (mirror, i, name), c, 0, frames[name], p, orc)
            assert c.debug_counts(pkg.DBG_SELECTED, 1)[0].tolist() == F.level_counts(refs[name], 8), (mirror, i, name)
    finally:
        c.close()
    p2 = F.P(n_levels=2)
    c = _ctx(pkg, 640, 480, p2, max_keypoints=4096)
    try:
        ref = _ref(orc, frames["one_square"], p2)
        assert len(ref["xy"]) == 1
        _assert_same(c.detect(frames["texture0"]), _ref(orc, frames["texture0"], p2), "two levels, texture", c, 0, frames["texture0"], p2, orc)
        _assert_same(c.detect(frames["one_square"]), ref, "two levels, one keypoint", c, 0, frames["one_square"], p2, orc)
    finally:
        c.close()


def _expected_matches(orc, cur, prev):
    """the repository's convention: fewer than 2 `from` rows, or an empty `to`, gives no matches"""
    if prev is None or len(cur["desc"]) < 2 or len(prev["desc"]) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    return orc.match(cur["desc"], prev["desc"], 0.7)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 17])
def test_ragged_batches(pkg, orc, sparse, n):
    """batches that mix ordinary frames with frames of 0, 1, 3, 5 and 7 keypoints, empty levels and totals on both sides of
    2048 and 64, below and from 8 frames on (k_describe maps frames spread / XCD-grouped; 17 frames are two chunks): the
    0-keypoint frame sits at position 0, at the end, and at positions 7 and 8.  Every frame against the oracle, then the
    matcher chained over two batches (the second one is the first rotated by one frame: its first frame has the empty
    frame that ended the first batch as predecessor), then the packer: offsets are the cumulative counts, empty records
    included."""
    import torch
    frames, refs = sparse
    fill = ["kp1", "texture0", "empty_middle", "below_2048", "above_2048", "texture1", "one_square", "kp3", "below_64", "kp5",
            "above_64", "kp2", "texture0", "kp4"]
    seq, k = [], 0
    for t in range(n):
        if t in (0, n - 1, 7, 8):
            seq.append("flat")
        else:
            seq.append(fill[k % len(fill)])
            k += 1
    if n >= 7:
        assert {"kp1", "empty_middle", "below_2048", "above_2048"} <= set(seq)
    second = seq[1:] + seq[:1] if n > 1 else ["kp1"]
    p, K = F.P(), 4096
    c = _ctx(pkg, 640, 480, p, max_batch=n, max_keypoints=K)
    try:
        prev = None
        for rep, names in enumerate((seq, second)):
            dev = _run_batch(c, [frames[x] for x in names])
            got = _read_batch(pkg, c, n)
            counts = c.debug_counts(pkg.DBG_SELECTED, n)
            for t, name in enumerate(names):
                _assert_same(got[t], refs[name], (n, rep, t, name), c, t, frames[name], p, orc)
                assert counts[t].tolist() == F.level_counts(refs[name], 8), (n, rep, t, name)
            c.match_batch_dev(0.7, True)
            c.sync()
            v = c.batch_view()
            mc = pkg.read_device(c, v.match_count, (n,), np.int32)
            mf = pkg.read_device(c, v.match_from, (n, K), np.int32)
            mt = pkg.read_device(c, v.match_to, (n, K), np.int32)
            for t, name in enumerate(names):
                before = refs[names[t - 1]] if t else prev
                rf, rt = _expected_matches(orc, refs[name], before)
                assert mc[t] == len(rf), (n, rep, t, name, "match count", int(mc[t]), len(rf))
                assert np.array_equal(mf[t, :mc[t]], rf) and np.array_equal(mt[t, :mc[t]], rt), (n, rep, t, name, "matches")
            if rep == 1:
                assert names[0] != "flat" and len(prev["xy"]) == 0 and mc[0] == 0      # an empty `to` set: no matches
            cap = c.packed_capacity(n, False)
            buf = torch.zeros(cap, dtype=torch.uint8, device="cuda")
            c.pack_batch_dev(buf.data_ptr(), cap, False)
            c.sync()
            pk = pkg.unpack_batch(buf.cpu().numpy())
            cnt = np.array([len(refs[x]["xy"]) for x in names])
            assert pk["n_frames"] == n
            assert np.array_equal(pk["kp_offset"], np.concatenate([[0], np.cumsum(cnt)])), (n, rep, "keypoint offsets")
            assert np.array_equal(pk["match_offset"], np.concatenate([[0], np.cumsum(mc)])), (n, rep, "match offsets")
            for t, name in enumerate(names):
                a, b = pk["kp_offset"][t], pk["kp_offset"][t + 1]
                for key in F.KEYS:
                    assert F.same_bits(np.array(pk[key][a:b]), refs[name][key]), (n, rep, t, name, "packed", key)
                a, b = pk["match_offset"][t], pk["match_offset"][t + 1]
                assert np.array_equal(pk["match_from"][a:b], mf[t, :mc[t]]) and np.array_equal(pk["match_to"][a:b], mt[t, :mc[t]])
            prev = refs[names[-1]]
            del dev, buf
    finally:
        c.close()


@pytest.mark.parametrize("tiled", ["1", "0"])
def test_symmetric_orientations(pkg, orc, monkeypatch, tiled):
    """keypoints whose intensity-centroid moments are exactly symmetric — m01 == 0, m10 == 0, |m10| == |m01| in every sign
    combination, and 0/0 — through fast_atan2_deg's ax >= ay, x < 0 and y < 0 arms and util_cos's quadrant folds at
    pi/2, pi and 3 pi/2: full equality of every frame as a single call and as member 3 of a 9-frame batch, under both
    layouts of the blurred slab, and the device's angle of every classified keypoint equals orc.fast_atan2 of its
    moments"""
    monkeypatch.setenv("MSLAM_HIP_TILED_BLUR", tiled)
    p = F.P(**F.SYM_P)
    frames = F.symmetric_frames()
    names = list(frames)
    refs = {k: _ref(orc, f, p) for k, f in frames.items()}
    seen = {}
    c = _ctx(pkg, F.SYM_SIZE, F.SYM_SIZE, p, max_batch=9, max_keypoints=1024)
    try:
        for i, name in enumerate(names):
            got = c.detect(frames[name])
            _assert_same(got, refs[name], (tiled, name), c, 0, frames[name], p, orc)
            for (l, x, y, m10, m01), ang in zip(F.keypoint_moments(orc, frames[name], p, refs[name]), got["angle"]):
                cls = F.moment_class(m10, m01)
                if cls is not None:
                    want = np.float32(orc.fast_atan2(float(m01), float(m10)))
                    assert ang.view(np.uint32) == want.view(np.uint32), (tiled, name, cls, (l, x, y), float(ang), float(want))
                    seen[cls] = seen.get(cls, 0) + 1
            members = [names[(i + t - 3) % len(names)] for t in range(9)]
            assert members[3] == name
            dev = _run_batch(c, [frames[m] for m in members])
            batch = _read_batch(pkg, c, 9)
            _assert_same(batch[3], refs[name], (tiled, name, "member 3 of 9"), c, 3, frames[name], p, orc)
            del dev
    finally:
        c.close()
    assert all(seen.get(k, 0) >= 3 for k in F.SYMMETRY_CLASSES) and seen.get("0/0", 0) >= 1, seen


@pytest.mark.parametrize("config", F.PERIODIC_CONFIGS, ids=["%d-levels-area-%d" % c for c in F.PERIODIC_CONFIGS])
def test_periodic_ties(pkg, orc, config):
    """checkerboards (the sharp 8-px one and three softened ones): up to thousands of keypoints on a lattice that
    coincides with node split lines, a handful of distinct responses — a tie goes to the first keypoint in list order, so DBG_SELECTED is compared level by level in
    order, then the detection.  The levels with at most 2048 candidates run the quadtree's LDS form (the large forms
    have test_gpu_parity.py::test_quadtree_storage_forms)."""
    n, area = config
    p = F.P(n_levels=n, min_node_area=area)
    lds_levels = 0
    c = _ctx(pkg, 320, 240, p, max_keypoints=8192, max_candidates=16384)
    try:
        for name, frame in F.periodic_frames().items():
            ref, cand, sel = _ref(orc, frame, p), F.level_candidates(orc, frame, p), F.level_selected(orc, frame, p)
            got = c.detect(frame)
            _assert_lists(pkg, c, cand, sel, 0, (name, config))
            _assert_same(got, ref, (name, config), c, 0, frame, p, orc)
            N = c.debug_counts(pkg.DBG_CANDIDATES, 1)[0]
            assert N.tolist() == [len(x) for x in cand]
            lds_levels += int(((N > 0) & (N <= 2048)).sum())
    finally:
        c.close()
    if n > 1:
        assert lds_levels >= 3, lds_levels         # the resized levels of every board
    else:
        assert lds_levels == 0                     # (level 0: nothing of the sharp board, 3512 / 4425 candidates of the others)
