"""Inputs of the native detector's edge tests (test_detect_edge_frames.py on the CPU, test_gpu_detect_edges.py on the
GPU): frames and sizes that steer build_geometry (csrc/api.hip), the level kernels, k_fast, k_quadtree and k_describe
into regimes the natural frames of test_gpu_parity.py never reach, and the oracle-side helpers both suites share.
Every generator is deterministic and states the property it claims; test_detect_edge_frames.py proves each claim on
the oracle alone.

Detector parameters travel as one dict P with the product's names (n_levels, scale_factor, ini_fast_thr,
min_fast_thr, min_node_area): ctx_kwargs(P) are Context arguments, oparams(orc, P) the oracle's."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KEYS = ("xy", "desc", "octave", "angle", "response")
BORDER, CELL, OVERLAP = 19, 64, 6
DBG_SELECTED = 3        # the package's debug item (test_rejected_geometries checks that the two agree)
DEFAULTS = dict(n_levels=8, scale_factor=1.2, ini_fast_thr=20, min_fast_thr=7, min_node_area=1000)


def P(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def oparams(orc, p):
    return orc.params(n_levels=p["n_levels"], scale_factor=p["scale_factor"], ini_fast_thr=p["ini_fast_thr"],
                      min_fast_thr=p["min_fast_thr"], min_size=p["min_node_area"])


def same_bits(a, b):
    """bit-for-bit: floats compared as uint32 views (so -0.0 != 0.0 and NaN payloads count)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    return bool(np.array_equal(a, b))


def bgr(gray):
    return np.ascontiguousarray(np.repeat(np.asarray(gray, np.uint8)[:, :, None], 3, axis=2))


def noise(W, H, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def soften(gray):
    """3 x 3 binomial filter in integers, (sum + 8) >> 4, replicated border.  The kernel is symmetric and the sums are
    order-free, so every mirror and diagonal symmetry of the input survives exactly — and FAST scores become graded: a
    two-valued drawing has equal scores on neighbouring corner pixels, which the strict non-maximum suppression removes
    together (a sharp square or bar end yields NO keypoint on level 0)."""
    a = np.pad(np.asarray(gray).astype(np.int32), 1, mode="edge")
    s = (a[:-2, :-2] + 2 * a[:-2, 1:-1] + a[:-2, 2:] + 2 * a[1:-1, :-2] + 4 * a[1:-1, 1:-1] + 2 * a[1:-1, 2:] +
         a[2:, :-2] + 2 * a[2:, 1:-1] + a[2:, 2:] + 8) >> 4
    return s.astype(np.uint8)


# ---- level and cell geometry, restated from the reference's loops (the oracle keeps them inside mso_fast_level) ----
def level_sizes(W, H, p):
    s, out = 1.0, []
    for l in range(p["n_levels"]):
        if l:
            s = float(np.float32(np.float32(p["scale_factor"]) * np.float32(s)))
        out.append((W, H) if l == 0 else (int(np.floor(W / s + 0.5)), int(np.floor(H / s + 0.5))))
    return out


def reference_cells(w, h):
    """the FAST cells of a w x h level, rows (x0, y0, cw, ch, ox, oy) in the reference's loop order: 64-px cells with a
    6-px overlap on the bordered rectangle [19, w - 19) x [19, h - 19); a cell that would start within 6 px of the end
    is dropped, the last one is cut at the end.  A transcription of the reference's loop (DCF:866-905), as the product's
    build_geometry and the oracle's mso_fast_level are.  The oracle pins it through its candidate lists EXCEPT for the
    inequality of the drop test: a cell kept exactly 6 px wide has no testable pixel and yields no candidate, so `<` and
    `<=` give the oracle the same lists — on that point the DBG_CELLS comparison is transcription against transcription."""
    bx, by = w - 2 * BORDER, h - 2 * BORDER
    out = []
    for i in range(by // CELL + 1):
        if by - OVERLAP <= CELL * i:
            continue
        for j in range(bx // CELL + 1):
            if bx - OVERLAP <= CELL * j:
                continue
            out.append((BORDER + CELL * j, BORDER + CELL * i, min(CELL + OVERLAP, bx - CELL * j),
                        min(CELL + OVERLAP, by - CELL * i), CELL * j, CELL * i))
    return np.array(out, np.int32).reshape(-1, 6)


def remainder_class(side):
    """what the cell loop does with the end of a side of `side` px: '7px' (a last cell 7 px wide: FAST tests 1 px of it),
    'dropped' (the last cell would start within 6 px of the end), or 'plain'"""
    b = side - 2 * BORDER
    j = b // CELL
    if b - OVERLAP <= CELL * j:
        return "dropped" if j > 0 else "plain"
    return "7px" if b - CELL * j == 7 else "plain"


# ---- 1. geometry ---------------------------------------------------------------------------------------------------
GEOMETRY_P = dict(ini_fast_thr=3, min_fast_thr=1, min_node_area=20)     # noise: nearly every testable pixel is a candidate

# single-level sizes, both sides from {45, 46, 101, 102, 103, 107, 108, 109, 110, 172, 173}: bordered sides
# b = side - 38 in {7, 8, 63, 64, 65, 69, 70, 71, 72, 134, 135}.  The first six are below 128 px (test_geometry_sizes_kernel_forms).
SINGLE_LEVEL_SIZES = [(45, 45), (109, 45), (45, 109), (108, 102), (109, 110), (46, 101),
                      (173, 46), (173, 173), (107, 172), (172, 107), (101, 173), (110, 103), (102, 172), (103, 173),
                      (172, 108)]
SMALL_SIZES = SINGLE_LEVEL_SIZES[:6]
# the first seed whose selection touches both ends of the testable span on both axes (45 x 45 has ONE testable pixel,
# 109 x 45 one row whose last pixel is all there is of the 7-px column); every size not listed does so with seed 0
NOISE_SEEDS = {(45, 45): 4, (109, 45): 1, (45, 109): 12, (46, 101): 4, (173, 46): 2}
# widths below one 64-px tile that are multiples of 4 (the fused level kernels want dword columns; 45 and 46 never reach
# them) and the full-tile width 64 of the limit cases below: one partial tile column, pitch 64
NARROW_FUSED_SIZES = [(52, 46, 1), (60, 109, 1), (56, 60, 2)]
# (W, H, n_levels): level 1 of 54 x 54 is 45 px (accepted; 53 x 53 gives 44: rejected); 64 initial quadtree nodes in both
# orientations (1664 / 26 = 64; the portrait one takes the reference's `max_x - min_y` branch); the largest side
LIMIT_SIZES = [(54, 54, 2), (1702, 64, 1), (64, 1702, 1), (4114, 102, 1), (102, 4114, 1)]


def geometry_cases():
    """(W, H, n_levels, frame): noise frames for contexts with GEOMETRY_P"""
    sizes = [(W, H, 1) for W, H in SINGLE_LEVEL_SIZES] + NARROW_FUSED_SIZES + LIMIT_SIZES
    return [(W, H, n, noise(W, H, NOISE_SEEDS.get((W, H), 0))) for W, H, n in sizes]


def small_geometry_cases():
    return [c for c in geometry_cases() if (c[0], c[1]) in SMALL_SIZES + [s[:2] for s in NARROW_FUSED_SIZES]]


def rejected_geometries():
    """(W, H, n_levels, why): creation must fail with E_INVALID before anything is detected"""
    return [(44, 109, 1, "a level must exceed 44 px"), (109, 44, 1, "a level must exceed 44 px"),
            (53, 53, 2, "level 1 is 44 px"), (4115, 102, 1, "beyond 4095 + 19 px"), (102, 4115, 1, "beyond 4095 + 19 px"),
            (1715, 64, 1, "1677 / 26 = 64.5: 65 initial nodes"), (64, 1715, 1, "65 initial nodes, portrait"),
            (2925, 2861, 1, "46 x 45 = 2070 cells on level 0")]


# ---- 2. sparse 640 x 480 frames (default parameters) --------------------------------------------------------------
def square_frame(bg, fg, x, y, s, W=640, H=480):
    f = np.full((H, W, 3), bg, np.uint8)
    f[y:y + s, x:x + s] = fg
    return f


# name -> (background, foreground, x, y, side) and the per-level counts the oracle gives; found by a search over contrast
# and size on the CPU (a sharp square has no level-0 keypoint; faint small ones lose levels one by one)
SPARSE_SQUARES = {
    "one_square": ((60, 200, 300, 200, 12), [0, 1, 1, 1, 1, 1, 1, 1]),
    "kp1": ((100, 108, 100, 100, 3), [0, 1, 0, 0, 0, 0, 0, 0]),
    "kp2": ((100, 108, 300, 200, 3), [0, 0, 1, 1, 0, 0, 0, 0]),
    "kp3": ((100, 108, 301, 203, 7), [0, 1, 1, 1, 0, 0, 0, 0]),
    "kp4": ((100, 114, 301, 203, 5), [0, 0, 0, 1, 1, 1, 1, 0]),
    "kp5": ((100, 120, 300, 200, 5), [0, 0, 0, 1, 1, 1, 1, 1]),
    "empty_middle": ((100, 109, 300, 200, 10), [0, 1, 1, 1, 0, 0, 1, 1]),      # levels 4 and 5 empty between 3 and 6
}
ONE_SQUARE_TWO_LEVELS = [0, 1]          # one_square on a 2-level context: exactly one keypoint
TRIM_ROWS = {"below_2048": 428, "above_2048": 432, "below_64": 36, "above_64": 40}
TRIM_RANGES = {"below_2048": (1985, 2047), "above_2048": (2049, 2112), "below_64": (33, 63), "above_64": (65, 96)}


def textured_frame():
    """a synthetic view with +-16 noise: 2081 keypoints at the default parameters"""
    import synth
    base = synth.make_stream(1, 640, 480, seed=1234)[0]
    rng = np.random.default_rng(7)
    return np.clip(base.astype(np.int16) + rng.integers(-16, 17, base.shape), 0, 255).astype(np.uint8)


def sparse_frames():
    """name -> 640 x 480 frame for the default parameters: `flat` (0 keypoints), the squares of SPARSE_SQUARES, and the
    textured frame with the rows from TRIM_ROWS[name] on flattened (totals inside TRIM_RANGES[name]: both sides of one
    full sweep of k_describe's base loop, 2048 positions in either launch shape, and both sides of 64)"""
    out = {"flat": np.full((480, 640, 3), 128, np.uint8)}
    for name, (sq, _) in SPARSE_SQUARES.items():
        out[name] = square_frame(*sq)
    tex = textured_frame()
    for name, r in TRIM_ROWS.items():
        f = tex.copy()
        f[r:] = 90
        out[name] = f
    return out


# ---- 3. exact symmetries of the intensity centroid -------------------------------------------------------------------
SYM_SIZE = 176
SYM_LEVELS = 2
SYM_P = dict(n_levels=SYM_LEVELS, min_node_area=100)
POLARITIES = {"bright": (60, 200), "dark": (200, 60), "bright_0_255": (0, 255), "dark_255_0": (255, 0)}


def _hbars(bg, fg):
    g = np.full((SYM_SIZE, SYM_SIZE), bg, np.uint8)
    for y, t, x0, x1 in ((50, 1, 56, 121), (88, 3, 56, 121), (126, 3, 50, 127)):
        g[y - t // 2:y + t // 2 + 1, x0:x1] = fg
    return g


def _squares(bg, fg):
    g = np.full((SYM_SIZE, SYM_SIZE), bg, np.uint8)
    g[40:73, 40:73] = fg
    g[104:137, 104:137] = fg
    return g


def _diagonal(bg, fg):
    """a diamond (vertices on the axes through its centre), a diagonal and an anti-diagonal bar (each symmetric about
    its own direction, so |m10| == |m01| at the ends), and a single dot (both moments zero)"""
    g = np.full((SYM_SIZE, SYM_SIZE), bg, np.uint8)
    y, x = np.mgrid[0:SYM_SIZE, 0:SYM_SIZE]
    g[np.abs(x - 60) + np.abs(y - 60) <= 20] = fg
    k = np.arange(0, 36)
    for d in (-1, 0, 1):                       # 3-px wide in the perpendicular direction
        g[100 + k + d, 100 + k - d] = fg       # diagonal bar
        g[40 + k + d, 135 - k + d] = fg        # anti-diagonal bar
    g[135, 45] = fg
    return g


def symmetric_frames():
    """name -> (176 x 176 frame, SYM_P): flat background with horizontal bars of odd thickness ending left and right
    (m01 == 0), their transpose (m10 == 0), axis-aligned squares (|m10| == |m01| at the corners, all four signs), and
    45-degree shapes; each bright-on-dark, dark-on-bright and at 0 / 255 (the -128 bias of the sdot4 moments), softened
    by the symmetric 3 x 3 filter so that FAST keeps one maximum on the axis of symmetry"""
    out = {}
    for pol, (bg, fg) in POLARITIES.items():
        out["hbars_" + pol] = bgr(soften(_hbars(bg, fg)))
        out["vbars_" + pol] = bgr(soften(_hbars(bg, fg).T))
        out["squares_" + pol] = bgr(soften(_squares(bg, fg)))
        out["diagonal_" + pol] = bgr(soften(_diagonal(bg, fg)))
    return out


def disc_moments(img, x, y, umax):
    """(m10, m01) of the radius-15 disc around (x, y) as the reference's ic_angle sums them"""
    m10 = m01 = 0
    for v in range(-15, 16):
        d = umax[abs(v)]
        row = img[y + v, x - d:x + d + 1].astype(np.int64)
        m10 += int((np.arange(-d, d + 1) * row).sum())
        m01 += int(v * row.sum())
    return m10, m01


def moment_class(m10, m01):
    """one of the symmetry classes (defined on the moments, not on angles), or None"""
    sg = lambda v: "+" if v > 0 else "-"
    if m10 == 0 and m01 == 0:
        return "0/0"
    if m01 == 0:
        return "m01=0,m10" + sg(m10)
    if m10 == 0:
        return "m10=0,m01" + sg(m01)
    if abs(m10) == abs(m01):
        return "|m10|=|m01|," + sg(m10) + sg(m01)
    return None


SYMMETRY_CLASSES = ["m01=0,m10+", "m01=0,m10-", "m10=0,m01+", "m10=0,m01-", "|m10|=|m01|,++", "|m10|=|m01|,+-",
                    "|m10|=|m01|,-+", "|m10|=|m01|,--"]


def keypoint_moments(orc, frame, p, det):
    """per detected keypoint (level, x, y, m10, m01) on the oracle's pyramid; level coordinates from DBG_SELECTED's twin,
    the oracle's own selection"""
    op = oparams(orc, p)
    pyr = orc.pyramid(orc.gray(frame), op)
    sel = level_selected(orc, frame, p)
    umax = orc.umax()
    out = []
    for l in range(p["n_levels"]):
        for x, y, _ in sel[l]:
            out.append((l, int(x) + BORDER, int(y) + BORDER) + disc_moments(pyr[l], int(x) + BORDER, int(y) + BORDER, umax))
    assert len(out) == len(det["xy"])
    return out


# ---- 4. ties in the quadtree -------------------------------------------------------------------------------------
PERIODIC_CONFIGS = [(4, 50), (1, 20), (4, 4000)]        # (n_levels, min_node_area)


def checkerboard(W, H, period, ox=0, oy=0, lo=40, hi=220, sharp=False):
    y, x = np.mgrid[0:H, 0:W]
    g = np.where((((x + ox) // period) + ((y + oy) // period)) % 2 == 0, lo, hi).astype(np.uint8)
    return bgr(g if sharp else soften(g))


def periodic_frames():
    """name -> 320 x 240 checkerboard: keypoints on a lattice that coincides with node split lines, a handful of distinct
    responses.  `sharp8` is the plain 0 / 255 board of 8-px squares: its level 0 is EMPTY (equal scores on neighbouring
    pixels: the strict non-maximum suppression removes them all), the resized levels hold 1670 keypoints with 103 distinct
    responses at (4 levels, stop area 50).  The others are softened, so level 0 is populated as well (up to 6659 keypoints,
    61 responses).  `period8_phase` has selected keypoints on x = 19 + 3 and on the last testable column
    x = 320 - 19 - 4 of level 0."""
    return {"sharp8": checkerboard(320, 240, 8, lo=0, hi=255, sharp=True), "period8": checkerboard(320, 240, 8),
            "period7": checkerboard(320, 240, 7), "period8_phase": checkerboard(320, 240, 8, 4, 3)}


# the fewest selected keypoints of a frame per (n_levels, min_node_area) of PERIODIC_CONFIGS: (4, 4000) stops the tree at
# its 16 first-generation nodes per populated level; sharp8 has nothing on level 0, hence nothing at all with one level
PERIODIC_MIN_KEYPOINTS = {"sharp8": {(4, 50): 1500, (1, 20): 0, (4, 4000): 48},
                          "period8": {(4, 50): 6000, (1, 20): 2500, (4, 4000): 64},
                          "period7": {(4, 50): 6000, (1, 20): 2500, (4, 4000): 64},
                          "period8_phase": {(4, 50): 6000, (1, 20): 2500, (4, 4000): 64}}


# ---- oracle stages ---------------------------------------------------------------------------------------------------
def level_candidates(orc, frame, p):
    """per level the FAST candidates, rows (x, y, response) as debug_keypoints(DBG_CANDIDATES) returns them"""
    op = oparams(orc, p)
    out = []
    for img in orc.pyramid(orc.gray(frame), op):
        h, w = img.shape
        c = orc.fast_level(img, op, cap=w * h + 16)
        out.append(np.stack([c["x"], c["y"], c["response"]], 1).reshape(-1, 3))
    return out


def level_selected(orc, frame, p):
    """per level the quadtree's selection in node-list order, rows (x, y, response) as DBG_SELECTED"""
    op = oparams(orc, p)
    H, W = frame.shape[:2]
    w, h, s = orc.level_geometry(W, H, op)
    out = []
    for l, img in enumerate(orc.pyramid(orc.gray(frame), op)):
        c = orc.fast_level(img, op, cap=w[l] * h[l] + 16)
        sel = orc.quadtree(c, w[l], h[l], s[l], p["min_node_area"]) if len(c) else c
        out.append(np.stack([sel["x"], sel["y"], sel["response"]], 1).reshape(-1, 3))
    return out


def level_counts(det, n_levels):
    return np.bincount(det["octave"], minlength=n_levels).tolist()
