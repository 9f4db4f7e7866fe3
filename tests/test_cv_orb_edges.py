"""The inputs of tests/test_gpu_cv_orb_edges.py do what that suite relies on — checked on the oracle alone, so that an
input which stops reaching its branch of k_cv_select fails here, loudly, instead of passing there for nothing."""
import numpy as np
import pytest

import cv_orb_frames as F


def _params(orc, order=None, **kw):
    return orc.cvorb_params(order=orc.ORDER_LIBSTDCXX if order is None else order, **kw)


@pytest.mark.parametrize("n", [1024, 1025, 4096, 4097])
def test_boundary_frames_hold_exactly_n_keypoints(orc, n):
    """one level with exactly 1024 / 1025 / 4096 / 4097 FAST keypoints inside the border: full LDS arrays of either
    instance (a bitonic network with np2 == KP) and the first count on the other side"""
    f = F.boundary_frame(n)
    p = _params(orc, n_features=300, n_levels=1, fast_threshold=5)
    cand = F.level_candidates(orc, f, p)[0]
    assert len(cand) == n
    key = cand[:, 1].astype(np.int64) * 4096 + cand[:, 0].astype(np.int64)
    assert (np.diff(key) > 0).all()                                        # raster order, one keypoint per dot
    assert cand[:, 2].min() >= 5 and len(np.unique(cand[:, 2])) > 100      # many scores, many ties: a real selection
    for order in (orc.ORDER_LIBSTDCXX, orc.ORDER_RASTER):
        d = orc.cvorb_detect(f, _params(orc, order, n_features=300, n_levels=1, fast_threshold=5))
        assert 300 <= len(d["xy"]) < 600


@pytest.mark.parametrize("n", [64, 128, 200, 240])
@pytest.mark.parametrize("mirror", [False, True])
def test_killer_frames_reach_heap_select(orc, n, mirror):
    """FAST responses in the median-of-3 killer order send the FIRST retainBest of the library-order reference into
    introselect's depth limit; the raster-order reference does not run introselect at all"""
    f = F.killer_frame(n, mirror)
    kw = dict(n_features=n // 8, n_levels=1, fast_threshold=5)
    a = F.median_of_3_killer(n)
    assert sorted(a.tolist()) == list(range(1, n + 1))
    cand = F.level_candidates(orc, f, _params(orc, **kw))[0]
    assert len(cand) == n
    assert (np.diff(cand[np.argsort(n + 1 - a if mirror else a), 2]) >= 0).all()    # the score rises with the height
    before = F.heap_select_calls(orc)
    lib = orc.cvorb_detect(f, _params(orc, orc.ORDER_LIBSTDCXX, **kw))
    assert F.heap_select_calls(orc) == before + 1
    ras = orc.cvorb_detect(f, _params(orc, orc.ORDER_RASTER, **kw))
    assert F.heap_select_calls(orc) == before + 1
    assert len(lib["xy"]) == len(ras["xy"]) >= n // 8
    assert sorted(map(tuple, lib["xy"].tolist())) == sorted(map(tuple, ras["xy"].tolist()))
    assert not np.array_equal(lib["xy"], ras["xy"])


@pytest.mark.parametrize("order", [0, 1])
def test_tie_frames_keep_every_tie(orc, order):
    """retainBest keeps ties: 300 dots of one height are 300 equal FAST scores AND 300 equal Harris responses, so a quota
    of 50 returns all of them; with two heights the first call keeps the 100 higher dots"""
    p = _params(orc, order, n_features=50, n_levels=1, fast_threshold=5)
    one = orc.cvorb_detect(F.one_height_frame(), p)
    assert F.level_counts(orc, F.one_height_frame(), p) == [300]
    assert len(one["xy"]) == 300 > p.n_features and len(np.unique(one["response"])) == 1
    assert {0.0, 90.0, 180.0} <= set(one["angle"].tolist())
    two = orc.cvorb_detect(F.two_height_frame(), p)
    assert len(two["xy"]) == 100 > p.n_features and len(np.unique(two["response"])) == 1


def test_zero_moment_angles_of_both_detectors(orc):
    """a dot whose neighbourhood is symmetric has intensity-centroid moments (0, 0); dots on the grid's rim have one
    moment exactly zero: the axis angles, and atan2(0, 0) = 0, all in one frame — also transposed and mirrored"""
    f = F.one_height_frame()
    for frame in (f, np.ascontiguousarray(f.transpose(1, 0, 2)), np.ascontiguousarray(f[:, ::-1])):
        cv = orc.cvorb_detect(frame, _params(orc, n_features=50, n_levels=1, fast_threshold=5))
        tree = orc.detect(frame, orc.params(n_levels=1, min_size=50))
        assert len(cv["xy"]) == len(tree["xy"]) == 300
        for d in (cv, tree):
            assert {0.0, 90.0, 180.0, 270.0} <= set(d["angle"].tolist())
            assert not (d["angle"].view(np.uint32) == 0x80000000).any()     # never -0.0
            assert (d["angle"] == 0.0).sum() > 150                           # the interior: both moments zero


def test_noise_frame_levels_fall_into_the_three_regimes(orc):
    p = _params(orc, n_features=500, n_levels=4, fast_threshold=20)
    n = F.level_counts(orc, F.noise_frame(), p)
    assert n[0] > F.SEL_LDS and F.SEL_LDS_SMALL < n[1] <= F.SEL_LDS and F.SEL_LDS_SMALL < n[2] <= F.SEL_LDS
    assert n[2] < F.SEL_LDS_SMALL + 64 and 0 < n[3] <= F.SEL_LDS_SMALL
    assert [F.regime(k) for k in n] == ["global", "large-lds", "large-lds", "small"]
    for frame in (*F.texture_stream(2), F.killer_frame(240), F.one_height_frame()):
        k = F.level_counts(orc, frame, p)
        assert max(k) <= F.SEL_LDS_SMALL and k[0] > 100
    assert F.level_counts(orc, F.flat_frame(), p) == [0, 0, 0, 0]
