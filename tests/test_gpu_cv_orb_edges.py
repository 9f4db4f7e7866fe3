"""GPU parity of the cv::ORB mode's selection (csrc/k_cvorb.hip: k_fast_tiles, k_cv_select, retain_best_std) where it
branches on the data: the two batched instances and their storage, the counts on both sides of 1024 and 4096, the
heap-select fallback of introselect, ties, and keypoints whose intensity-centroid moments are zero.  Every comparison is
bit-exact against the oracle, stage by stage (DBG_CANDIDATES, DBG_SELECTED) and end to end, in both keypoint orders.
tests/test_cv_orb_edges.py proves on the CPU that the inputs (tests/cv_orb_frames.py) reach those branches."""
import numpy as np
import pytest

import cv_orb_frames as F

pytestmark = pytest.mark.gpu


def _orders(pkg, orc):
    return ((pkg.CV_ORDER_LIBSTDCXX, orc.ORDER_LIBSTDCXX, "library order"), (pkg.CV_ORDER_RASTER, orc.ORDER_RASTER, "raster order"))


class Refs:
    """the oracle's answers for one parameter set, computed once per distinct frame and order and left unchanged"""

    def __init__(self, orc, **kw):
        self.orc, self.kw, self.memo = orc, kw, {}

    def params(self, order):
        return self.orc.cvorb_params(order=order, **self.kw)

    def _get(self, what, name, frame, order, fn):
        key = (what, name, order)
        if key not in self.memo:
            v = fn(self.orc, frame, self.params(order)) if what != "detect" else self.orc.cvorb_detect(frame, self.params(order))
            for a in (v.values() if isinstance(v, dict) else v):
                a.setflags(write=False)
            self.memo[key] = v
        return self.memo[key]

    def detect(self, name, frame, order):
        return self._get("detect", name, frame, order, None)

    def candidates(self, name, frame):
        return self._get("cand", name, frame, 0, F.level_candidates)       # (FAST's list does not depend on the order)

    def selected(self, name, frame, order):
        return self._get("sel", name, frame, order, F.level_selected)


def _assert_same(got, ref, what):
    assert len(got["xy"]) == len(ref["xy"]), (what, "count", len(got["xy"]), len(ref["xy"]))
    for k in F.KEYS:
        assert F.same_bits(got[k], ref[k]), (what, k)


def _assert_stages(pkg, c, refs, name, frame, order, slot, what):
    cand, sel = refs.candidates(name, frame), refs.selected(name, frame, order)
    for l in range(c.params.n_levels):
        got = c.debug_keypoints(pkg.DBG_CANDIDATES, slot, l)
        assert len(got) == len(cand[l]) and F.same_bits(got, cand[l]), (what, "FAST level %d" % l)
        got = c.debug_keypoints(pkg.DBG_SELECTED, slot, l)
        assert len(got) == len(sel[l]) and F.same_bits(got, sel[l]), (what, "selection level %d" % l)


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


def _run_batch(c, frames):
    import torch
    dev = torch.from_numpy(np.ascontiguousarray(np.stack(frames))).cuda()
    c.detect_batch_dev(dev.data_ptr(), len(frames))
    c.sync()
    return dev      # (kept alive by the caller until the results are read)


def test_batched_selection_instances(pkg, orc):
    """launch_cv_select below and from 8 frames on: 7 frames are one launch of the large instance (take_all); 8 frames are
    both instances over one group of k_fast_tiles; 9 frames add a group of 8 that holds one frame; 17 frames are two
    chunks on two streams, the second with frame0 = 8 (counter zeroing, candidate and selection slots at an offset).
    The noise frame puts one level on the global arrays, two in the large instance's LDS (one just above 1024) and one in
    the small instance; everything else is small.  Six kinds of frame in a cycle of six: neighbours differ and every
    kind meets the level rotation (blockIdx.x + blockIdx.y) % 4 at two residues."""
    kw = dict(n_features=500, n_levels=4, fast_threshold=20)
    refs = Refs(orc, **kw)
    tex = F.texture_stream(2)            # two consecutive views of one scene: a pair the matcher has something to say about
    kinds = [("texture 0", tex[0]), ("texture 1", tex[1]), ("noise", F.noise_frame()), ("killer", F.killer_frame(240)),
             ("one-height", F.one_height_frame()), ("flat", F.flat_frame())]
    K = 2048
    c = pkg.Context(width=320, height=240, max_batch=17, detector=pkg.DETECTOR_CV_ORB, n_features=500, n_levels=4,
                    ini_fast_thr=20, max_candidates=8192, max_keypoints=K)
    try:
        seen_split, seen_all, residues = set(), set(), {}
        # (where the cycle starts: the noise frame is frame 0 of the batches of 7 and 8, the lone frame of the second group
        # of the batch of 9, and frame 8 — the first of the second chunk — of the batch of 17)
        for n, start in ((7, 2), (8, 2), (9, 0), (17, 0)):
            seq = [kinds[(start + i) % 6] for i in range(n)]
            assert all(seq[i][0] != seq[i + 1][0] for i in range(n - 1))
            n_chunks = 1 if n < 16 else 2
            chunks = [(n * k // n_chunks, n * (k + 1) // n_chunks) for k in range(n_chunks)]
            assert n != 17 or chunks == [(0, 8), (8, 17)]
            for porder, oorder, oname in _orders(pkg, orc):
                c.set_cv_keypoint_order(porder)
                dev = _run_batch(c, [f for _, f in seq])
                got = _read_batch(pkg, c, n)
                counts = c.debug_counts(pkg.DBG_CANDIDATES, n)
                for t, (name, frame) in enumerate(seq):
                    what = (n, oname, t, name)
                    _assert_same(got[t], refs.detect(name, frame, oorder), what)
                    assert counts[t].tolist() == [len(x) for x in refs.candidates(name, frame)], what
                    f0, f1 = [ch for ch in chunks if ch[0] <= t < ch[1]][0]
                    for l in range(4):
                        (seen_split if f1 - f0 >= 8 else seen_all).add(F.regime(int(counts[t, l])))
                    if n == 17:
                        residues.setdefault(name, set()).add(t % 4)
                    if t in (f0, f1 - 1):
                        _assert_stages(pkg, c, refs, name, frame, oorder, t, what)
                if n == 17:
                    c.match_batch_dev(0.9, False)
                    c.sync()
                    v = c.batch_view()
                    mc = pkg.read_device(c, v.match_count, (n,), np.int32)
                    mf = pkg.read_device(c, v.match_from, (n, K), np.int32)
                    mt = pkg.read_device(c, v.match_to, (n, K), np.int32)
                    for t in (7, 8):                       # the pair inside the first chunk and the pair across the boundary
                        rf, rt = orc.match(refs.detect(*seq[t], oorder)["desc"], refs.detect(*seq[t - 1], oorder)["desc"], 0.9)
                        assert len(rf) > 10 and mc[t] == len(rf), (oname, "matches", t)
                        assert np.array_equal(mf[t, :mc[t]], rf) and np.array_equal(mt[t, :mc[t]], rt), (oname, "matches", t)
                del dev
        assert seen_split >= {"small", "large-lds", "global"}, seen_split     # both instances, all three storages
        assert seen_all >= {"small", "global"}, seen_all                      # <= 1024 and > 4096 in the large instance
        assert all(len(r) > 1 for r in residues.values()) and len(residues) == 6, residues
    finally:
        c.close()


def test_selection_storage_bounds(pkg, orc):
    """exactly 1024 / 1025 / 4096 / 4097 FAST keypoints on one level: full LDS arrays of either instance (np2 == KP) and
    the first count beyond — as single calls (the large instance takes all four) and in a batch of 8 (1024 goes to the
    small instance).  max_candidates compares with the same count: 4096 fits a capacity of 4096, 4097 does not."""
    kw = dict(n_features=300, n_levels=1, fast_threshold=5)
    refs = Refs(orc, **kw)
    frames = {n: F.boundary_frame(n) for n in (1024, 1025, 4096, 4097)}
    for n, f in frames.items():
        assert len(refs.candidates(n, f)[0]) == n
    ckw = dict(width=640, height=480, detector=pkg.DETECTOR_CV_ORB, n_features=300, n_levels=1, ini_fast_thr=5, min_fast_thr=5, max_keypoints=1024)
    c = pkg.Context(max_batch=8, max_candidates=8192, **ckw)
    try:
        for porder, oorder, oname in _orders(pkg, orc):
            c.set_cv_keypoint_order(porder)
            for n, f in frames.items():
                _assert_same(c.detect(f), refs.detect(n, f, oorder), (oname, "single", n))
                _assert_stages(pkg, c, refs, n, f, oorder, 0, (oname, "single", n))
            seq = [1024, 1025, 4096, 4097, 1025, 4097, 1024, 4096]
            dev = _run_batch(c, [frames[n] for n in seq])
            got = _read_batch(pkg, c, 8)
            assert c.debug_counts(pkg.DBG_CANDIDATES, 8)[:, 0].tolist() == seq
            for t, n in enumerate(seq):
                _assert_same(got[t], refs.detect(n, frames[n], oorder), (oname, "batch", t, n))
                _assert_stages(pkg, c, refs, n, frames[n], oorder, t, (oname, "batch", t, n))
            del dev
    finally:
        c.close()
    c = pkg.Context(max_candidates=4096, **ckw)
    try:
        for porder, oorder, oname in _orders(pkg, orc):
            c.set_cv_keypoint_order(porder)
            _assert_same(c.detect(frames[4096]), refs.detect(4096, frames[4096], oorder), (oname, "capacity 4096", 4096))
            with pytest.raises(pkg.MslamHipError) as e:
                c.detect(frames[4097])
            assert e.value.code == pkg.E_CAPACITY and "candidates" in str(e.value)
            _assert_same(c.detect(frames[1025]), refs.detect(1025, frames[1025], oorder), (oname, "after the overflow", 1025))
    finally:
        c.close()


@pytest.mark.parametrize("n", [64, 240])
def test_depth_limit_branch(pkg, orc, n):
    """retain_best_std's single-thread heap select (introselect at depth 0), reached from an image: FAST responses in the
    median-of-3 killer order and its mirror, n_features = n / 8.  A single call runs it in the large instance, a batch of
    8 in the 1024-entry one (both keep 16-bit stopper ranks in LDS)."""
    kw = dict(n_features=n // 8, n_levels=1, fast_threshold=5)
    refs = Refs(orc, **kw)
    frames = {"killer": F.killer_frame(n), "mirror": F.killer_frame(n, True), "one-height": F.one_height_frame(),
              "two-height": F.two_height_frame()}
    for name in ("killer", "mirror"):
        # the claim "the branch ran" travels with this test: the oracle's library-order run enters heap select, once
        before = F.heap_select_calls(orc)
        refs.detect(name, frames[name], orc.ORDER_LIBSTDCXX)
        assert F.heap_select_calls(orc) == before + 1, name
        refs.detect(name, frames[name], orc.ORDER_RASTER)
        assert F.heap_select_calls(orc) == before + 1, name
        assert len(refs.candidates(name, frames[name])[0]) == n
    c = pkg.Context(width=320, height=240, max_batch=8, detector=pkg.DETECTOR_CV_ORB, n_features=n // 8, n_levels=1,
                    ini_fast_thr=5, min_fast_thr=5, max_keypoints=1024)
    try:
        for porder, oorder, oname in _orders(pkg, orc):
            c.set_cv_keypoint_order(porder)
            for name in ("killer", "mirror"):
                _assert_same(c.detect(frames[name]), refs.detect(name, frames[name], oorder), (oname, "single", name))
                _assert_stages(pkg, c, refs, name, frames[name], oorder, 0, (oname, "single", name))
            seq = ["killer", "mirror", "one-height", "killer", "mirror", "two-height", "mirror", "killer"]
            dev = _run_batch(c, [frames[k] for k in seq])
            got = _read_batch(pkg, c, 8)
            for t, name in enumerate(seq):
                _assert_same(got[t], refs.detect(name, frames[name], oorder), (oname, "batch", t, name))
                _assert_stages(pkg, c, refs, name, frames[name], oorder, t, (oname, "batch", t, name))
            del dev
    finally:
        c.close()


def test_retain_best_keeps_ties(pkg, orc):
    """retainBest keeps every response equal to the n-th largest: 300 equal FAST scores and Harris responses come back
    as 300 keypoints for n_features = 50 (and 100 of the two-height frame) — the output is larger than n_features, and
    max_keypoints, not n_features, is what it must fit"""
    kw = dict(n_features=50, n_levels=1, fast_threshold=5)
    refs = Refs(orc, **kw)
    frames = {"one-height": (F.one_height_frame(), 300), "two-height": (F.two_height_frame(), 100)}
    ckw = dict(width=320, height=240, detector=pkg.DETECTOR_CV_ORB, n_features=50, n_levels=1, ini_fast_thr=5, min_fast_thr=5)
    c = pkg.Context(max_keypoints=1024, **ckw)
    try:
        for porder, oorder, oname in _orders(pkg, orc):
            c.set_cv_keypoint_order(porder)
            for name, (f, n_out) in frames.items():
                ref = refs.detect(name, f, oorder)
                assert len(ref["xy"]) == n_out > 50 and len(np.unique(ref["response"])) == 1
                _assert_same(c.detect(f), ref, (oname, name))
                _assert_stages(pkg, c, refs, name, f, oorder, 0, (oname, name))
    finally:
        c.close()
    c = pkg.Context(max_keypoints=200, **ckw)
    try:
        tex = F.texture_frame(seed=5)
        for porder, oorder, oname in _orders(pkg, orc):
            c.set_cv_keypoint_order(porder)
            with pytest.raises(pkg.MslamHipError) as e:
                c.detect(frames["one-height"][0])
            assert e.value.code == pkg.E_CAPACITY and "keypoints" in str(e.value)
            ref = refs.detect("texture5", tex, oorder)
            assert 50 <= len(ref["xy"]) <= 200
            _assert_same(c.detect(tex), ref, (oname, "clean call after the overflow"))
    finally:
        c.close()


@pytest.mark.parametrize("view", ["as is", "transposed", "mirrored"])
def test_zero_moment_orientation(pkg, orc, view):
    """k_describe's orientation at atan2(0, 0) and on the axes, both detector modes: the interior dots of the one-height
    frame have both intensity-centroid moments exactly zero, the rim dots one of them — angles exactly 0, 90, 180 and
    270.  Transposed and mirrored, the axis cases change sign."""
    f = F.one_height_frame()
    f = {"as is": f, "transposed": np.ascontiguousarray(f.transpose(1, 0, 2)), "mirrored": np.ascontiguousarray(f[:, ::-1])}[view]
    H, W = f.shape[:2]
    c = pkg.Context(width=W, height=H, detector=pkg.DETECTOR_CV_ORB, n_features=50, n_levels=1, ini_fast_thr=5, min_fast_thr=5, max_keypoints=1024)
    try:
        for porder, oorder, oname in _orders(pkg, orc):
            c.set_cv_keypoint_order(porder)
            ref = orc.cvorb_detect(f, orc.cvorb_params(n_features=50, n_levels=1, fast_threshold=5, order=oorder))
            assert len(ref["xy"]) == 300 and {0.0, 90.0, 180.0} <= set(ref["angle"].tolist())
            _assert_same(c.detect(f), ref, ("cv::ORB", oname, view))
    finally:
        c.close()
    c = pkg.Context(width=W, height=H, n_levels=1, min_node_area=50, max_keypoints=1024)
    try:
        ref = orc.detect(f, orc.params(n_levels=1, min_size=50))
        assert len(ref["xy"]) == 300 and {0.0, 90.0, 180.0, 270.0} <= set(ref["angle"].tolist())
        _assert_same(c.detect(f), ref, ("in-tree", view))
    finally:
        c.close()
