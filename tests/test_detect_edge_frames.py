"""The inputs of tests/test_gpu_detect_edges.py do what that suite relies on — checked on the oracle alone, so that an
input which stops reaching its regime fails here, loudly, instead of passing there for nothing."""
import numpy as np
import pytest

import detect_edge_frames as F


def _detect(orc, frame, p):
    return orc.detect(frame, F.oparams(orc, p))


@pytest.fixture(scope="module")
def geometry(orc):
    """per geometry case: the oracle's per-level selections (border-relative coordinates)"""
    out = {}
    for W, H, n, frame in F.geometry_cases():
        p = F.P(n_levels=n, **F.GEOMETRY_P)
        out[(W, H, n)] = (frame, p, F.level_selected(orc, frame, p))
    return out


def test_level_sizes_and_cells_restate_the_oracle(orc, geometry):
    """level_sizes() equals the oracle's geometry, and FAST run cell by cell over reference_cells() reproduces the
    oracle's candidate list of every level (order included), so the cell table the GPU test compares DBG_CELLS with
    covers the same pixels in the same order as the oracle's.  What this cannot show is the `<=` of the drop test: a
    cell kept 6 px wide yields no candidate, the lists are the same with `<` (see reference_cells).  Every level's
    candidates fit the oracle's own list capacity (W H / 4 + 16)."""
    for (W, H, n), (frame, p, _) in geometry.items():
        op = F.oparams(orc, p)
        w, h, _ = orc.level_geometry(W, H, op)
        assert F.level_sizes(W, H, p) == list(zip(w, h)), (W, H, n)
        cand = F.level_candidates(orc, frame, p)
        for l, img in enumerate(orc.pyramid(orc.gray(frame), op)):
            rows = []
            for x0, y0, cw, ch, ox, oy in F.reference_cells(w[l], h[l]):
                sub = img[y0:y0 + ch, x0:x0 + cw]
                c = orc.fast(sub, p["ini_fast_thr"])
                if len(c) == 0:
                    c = orc.fast(sub, p["min_fast_thr"])
                rows += [(k["x"] + ox, k["y"] + oy, k["response"]) for k in c]
            assert F.same_bits(np.array(rows, np.float32).reshape(-1, 3), cand[l]), (W, H, l)
            assert len(cand[l]) <= W * H // 4 + 16, (W, H, l)


def test_remainder_classes_show_in_the_selected_coordinates(orc, geometry):
    """7-px column present, 7-px row present, dropped column present, dropped row present — each read off the selected
    coordinates of a single-level frame.  A 7-px last cell starts at 64 j and FAST tests its pixel 3 only, so keypoints
    at border-relative 64 j + 3 exist (the cell before ends its tests at 64 j + 2) and none beyond; where the last cell
    is dropped the selection ends at side - 38 - 4, reached from the cell before.  109 x 45 (both sides' cells 7 px in
    one direction) has keypoints on row y = 22 only, x up to 86."""
    seen = {"7px column": 0, "7px row": 0, "dropped column": 0, "dropped row": 0}
    for (W, H) in F.SINGLE_LEVEL_SIZES:
        sel = geometry[(W, H, 1)][2][0]
        assert len(sel) > 0, (W, H)
        for axis, side, name in ((0, W, "column"), (1, H, "row")):
            b, cls = side - 2 * F.BORDER, F.remainder_class(side)
            v = sel[:, axis]
            assert v.min() == 3 and v.max() == b - 4, (W, H, name, v.min(), v.max())      # noise: the whole testable span
            if cls == "7px":
                assert b - 4 == 64 * (b // 64) + 3 and (v == b - 4).sum() >= 1
                seen["7px " + name] += 1
            elif cls == "dropped":
                assert b - 6 <= 64 * (b // 64) and (v == b - 4).sum() >= 1
                seen["dropped " + name] += 1
    assert all(n >= 2 for n in seen.values()), seen
    sel = geometry[(109, 45, 1)][2][0]
    assert set(sel[:, 1].tolist()) == {3.0} and sel[:, 0].max() == 86 - F.BORDER
    det = _detect(orc, *geometry[(109, 45, 1)][:2])
    assert set(det["xy"][:, 1].tolist()) == {22.0} and det["xy"][:, 0].max() == 86.0
    assert len(geometry[(45, 45, 1)][2][0]) == 1              # one testable pixel, and this seed makes it a corner


def test_remainder_classes_cover_every_listed_side(orc):
    sides = {45, 46, 101, 102, 103, 107, 108, 109, 110, 172, 173}
    assert {W for W, _ in F.SINGLE_LEVEL_SIZES} == sides and {H for _, H in F.SINGLE_LEVEL_SIZES} == sides
    assert sorted(s - 38 for s in sides) == [7, 8, 63, 64, 65, 69, 70, 71, 72, 134, 135]
    assert {s for s in sides if F.remainder_class(s) == "7px"} == {45, 109, 173}
    assert {s for s in sides if F.remainder_class(s) == "dropped"} == {102, 103, 107, 108, 172}    # 108 and 172: b - 6 == 64 j exactly
    assert all(W < 128 and H < 128 for W, H in F.SMALL_SIZES) and len(F.SMALL_SIZES) == 6
    assert all(W < 64 and W % 4 == 0 for W, _, _ in F.NARROW_FUSED_SIZES)


def test_limit_sizes_sit_on_the_limits(orc, geometry):
    """level 1 of 54 x 54 is 45 px and holds keypoints (53 x 53: 44 px); 1702 x 64 and 64 x 1702 have exactly 64 initial
    quadtree nodes and 1715 x 64 would have 65; the 4114-px frames select coordinates above 4000 (the 12-bit kp_x / kp_y
    pack goes up to 4095)"""
    assert F.level_sizes(54, 54, F.P(n_levels=2)) == [(54, 54), (45, 45)]
    assert F.level_sizes(53, 53, F.P(n_levels=2)) == [(53, 53), (44, 44)]
    for W, H in ((1702, 64), (64, 1702)):
        long_side, short = max(W, H) - 38, min(W, H) - 38
        assert round(long_side / short) == 64 and int(np.floor((1715 - 38) / short + 0.5)) == 65
        sel = geometry[(W, H, 1)][2][0]
        assert sel[:, 0 if W > H else 1].max() == long_side - 4 and len(sel) > 1000
    for W, H in ((4114, 102), (102, 4114)):
        sel = geometry[(W, H, 1)][2][0]
        assert sel[:, 0 if W > H else 1].max() == 4114 - 38 - 4 == 4072
        det = _detect(orc, *geometry[(W, H, 1)][:2])
        assert det["xy"][:, 0 if W > H else 1].max() == 4091.0 > 4000 and len(det["xy"]) < 32768
    for W, H, n, _ in F.rejected_geometries():
        sizes = F.level_sizes(W, H, F.P(n_levels=n))
        w, h = sizes[-1]
        cells = len(F.reference_cells(*sizes[0])) if min(sizes[0]) > 44 else 0
        ratio = max(w - 38, 1) / max(h - 38, 1)
        nodes = int(np.floor(max(ratio, 1 / ratio) + 0.5))
        assert min(w, h) <= 44 or max(W, H) > 4114 or nodes > 64 or cells > 2048, (W, H, n)
    assert len(F.reference_cells(2925, 2861)) == 2070


def test_sparse_frames_have_the_stated_counts(orc):
    """flat: 0; one_square: [0 1 1 1 1 1 1 1] (level 0 empty) and exactly 1 keypoint with 2 levels; kp1 .. kp5: exactly
    1 .. 5; empty_middle: levels 4 and 5 empty between level 3 and level 6; the trimmed textured frames inside
    [1985, 2047] / [2049, 2112] and on either side of 64"""
    fr = F.sparse_frames()
    p = F.P()
    assert len(_detect(orc, fr["flat"], p)["xy"]) == 0
    for name, (_, counts) in F.SPARSE_SQUARES.items():
        assert F.level_counts(_detect(orc, fr[name], p), 8) == counts, name
    assert [sum(F.SPARSE_SQUARES["kp%d" % k][1]) for k in range(1, 6)] == [1, 2, 3, 4, 5]
    assert F.level_counts(_detect(orc, fr["one_square"], F.P(n_levels=2)), 2) == F.ONE_SQUARE_TWO_LEVELS
    c = F.SPARSE_SQUARES["empty_middle"][1]
    assert c[3] > 0 and c[4] == 0 and c[5] == 0 and c[6] > 0
    for name, (lo, hi) in F.TRIM_RANGES.items():
        n = len(_detect(orc, fr[name], p)["xy"])
        assert lo <= n <= hi, (name, n)
        assert name.endswith("64") or min(F.level_counts(_detect(orc, fr[name], p), 8)) > 0      # every level populated


def test_symmetric_frames_fill_every_moment_class(orc):
    """moments m10, m01 of every keypoint of symmetric_frames(), in numpy from orc.umax() on the oracle's pyramid: each
    of m01 == 0 (m10 > 0, m10 < 0), m10 == 0 (m01 > 0, m01 < 0) and |m10| == |m01| (four sign combinations) holds at
    least 3 keypoints, the 0/0 class (the softened dot) at least one per polarity — and the oracle's angle of every
    classified keypoint is fast_atan2 of its moments"""
    count = {k: 0 for k in F.SYMMETRY_CLASSES + ["0/0"]}
    saturated = 0
    for name, frame in F.symmetric_frames().items():
        p = F.P(**F.SYM_P)
        det = _detect(orc, frame, p)
        for (l, x, y, m10, m01), ang in zip(F.keypoint_moments(orc, frame, p, det), det["angle"]):
            cls = F.moment_class(m10, m01)
            if cls is not None:
                count[cls] += 1
                assert np.float32(orc.fast_atan2(float(m01), float(m10))).view(np.uint32) == ang.view(np.uint32)
                saturated += name.endswith(("0_255", "255_0"))
    assert all(count[k] >= 3 for k in F.SYMMETRY_CLASSES), count
    assert count["0/0"] >= 4 and saturated >= 8, (count, saturated)


@pytest.mark.parametrize("name", ["sharp8", "period8", "period7", "period8_phase"])
def test_checkerboards_are_full_of_ties(orc, name):
    """at least half of the selected keypoints share their response with another keypoint of the same level, in each of
    the three configurations, and there are as many as PERIODIC_MIN_KEYPOINTS states (thousands, where the stop area lets
    the tree grow); the sharp board has an empty level 0; period8_phase has selected keypoints on x = 19 + 3 and on the
    last testable column"""
    frame = F.periodic_frames()[name]
    for n, area in F.PERIODIC_CONFIGS:
        p = F.P(n_levels=n, min_node_area=area)
        sel = F.level_selected(orc, frame, p)
        total = sum(len(s) for s in sel)
        shared = 0
        for s in sel:
            _, c = np.unique(s[:, 2], return_counts=True)
            shared += int(c[c > 1].sum())
        assert total >= F.PERIODIC_MIN_KEYPOINTS[name][(n, area)] and 2 * shared >= total, (n, area, total, shared)
        if name == "sharp8":
            assert len(sel[0]) == 0 and (n == 1 or min(len(s) for s in sel[1:]) >= 16)
        else:
            assert min(len(s) for s in sel) >= 16
        if name == "period8_phase" and area < 4000:
            assert (sel[0][:, 0] == 3).any() and (sel[0][:, 0] == 320 - 38 - 4).any()
    assert set(F.PERIODIC_MIN_KEYPOINTS) == set(F.periodic_frames())


# ---- explain(), the attribution helper of the GPU file, on an oracle-backed stub context ----------------------------------
class _StubContext:
    """debug_keypoints(DBG_SELECTED) answered from the oracle's own selection (optionally with one entry altered)"""

    def __init__(self, sel):
        self.sel = sel

    def debug_keypoints(self, what, frame, level):
        assert what == F.DBG_SELECTED and frame == 5
        return self.sel[level].copy()


@pytest.fixture(scope="module")
def explained(orc):
    import functools
    import test_gpu_detect_edges as G
    frame, p = F.sparse_frames()["below_64"], F.P()
    ref = orc.detect(frame, F.oparams(orc, p))
    sel = F.level_selected(orc, frame, p)
    return functools.partial(G.explain, orc=orc), frame, p, ref, sel


def test_explain_names_the_keypoint_and_the_stage(orc, explained):
    """every branch of explain(): an unaltered detection agrees; a selection entry, an octave, an xy pair, a response, an
    angle (one ulp), one descriptor byte and the count, each altered alone at a keypoint of level 2 (or at the end),
    are named with the keypoint's index, level and coordinates and with the stage that is wrong, and nothing else"""
    explain, frame, p, ref, sel = explained
    n0, n1, n2 = len(sel[0]), len(sel[1]), len(sel[2])
    assert n0 > 0 and n1 > 0 and n2 > 2
    j = 2                                   # entry of level 2
    k = n0 + n1 + j                         # its index in the detection
    px, py = int(sel[2][j][0]) + F.BORDER, int(sel[2][j][1]) + F.BORDER
    where = "keypoint %d, level 2, (%d, %d)" % (k, px, py)
    copy = lambda: {key: a.copy() for key, a in ref.items()}
    ctx = _StubContext(sel)
    assert explain(ctx, 5, frame, p, copy()).startswith("stages agree")

    moved = [s.copy() for s in sel]
    moved[2][j, 0] += 1
    msg = explain(_StubContext(moved), 5, frame, p, copy())
    assert msg.startswith("selection: level 2 has %d keypoints, the oracle %d; first difference at entry %d " % (n2, n2, j)), msg
    short = [s.copy() for s in sel]
    short[1] = short[1][:-1]
    msg = explain(_StubContext(short), 5, frame, p, copy())
    assert msg.startswith("selection: level 1 has %d keypoints, the oracle %d; first difference at entry %d " % (n1 - 1, n1, n1 - 1)), msg

    got = copy()
    got["octave"][k] = 3
    assert explain(ctx, 5, frame, p, got) == where + ": octave 3"
    got = copy()
    got["xy"][k, 1] += 0.5
    assert explain(ctx, 5, frame, p, got).startswith(where + ": xy scaling ")
    got = copy()
    got["response"][k] += 1
    assert explain(ctx, 5, frame, p, got).startswith(where + ": response ")
    got = copy()
    got["angle"][k] = np.nextafter(got["angle"][k], np.float32(400))
    assert explain(ctx, 5, frame, p, got).startswith(where + ": angle ")
    got = copy()
    got["desc"][k, 9] ^= 4
    got["desc"][k, 15] ^= 128
    assert explain(ctx, 5, frame, p, got) == where + ": angle ok, descriptor bytes [9, 15] differ"
    # two faults: the first keypoint in list order is the one named
    got["angle"][k - 1] = np.nextafter(got["angle"][k - 1], np.float32(400))
    assert explain(ctx, 5, frame, p, got).startswith("keypoint %d, level 2, " % (k - 1)) and ": angle " in explain(ctx, 5, frame, p, got)

    total = len(ref["xy"])
    got = {key: a[:-1].copy() for key, a in ref.items()}
    assert explain(ctx, 5, frame, p, got).startswith("count: %d keypoints returned, keypoint %d, level " % (total - 1, total - 1))
    got = {key: np.concatenate([a, a[-1:]]) for key, a in ref.items()}
    assert explain(ctx, 5, frame, p, got) == "count: %d keypoints returned, %d selected" % (total + 1, total)
