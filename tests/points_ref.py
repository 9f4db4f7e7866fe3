"""Independent numpy reference of the RGB-D back-projection, and the coordinate edge list its tests share (test
infrastructure like match_ref.py: not a conftest.py, not under oracle/).

The documented contract (include/mslam_hip.h at mslam_hip_backproject, the header of modular-slam_amd/csrc/k_points.hip):

    pixel = the f32 coordinates widened to f64, truncated toward zero        (-0.5 is pixel 0, -1.0 is outside)
    a coordinate that is not finite, or whose pixel is outside [0, w) x [0, h), has no depth: valid = 0
    depth = f32(data[w * iy + ix]) * f32(factor)                             one float multiply
    valid = depth > FLT_EPSILON                                              (false for NaN)
    X = (x - cx) * z * (1 / fx),  Y = (y - cy) * z * (1 / fy),  Z = z        f64, left to right, z = f64(depth)
    an invalid point is (0, 0, 0)

Written from that description as array expressions; it shares no code with oracle/mslam_oracle.c, which
tests/test_points_ref.py compares it with bit for bit.
"""
import numpy as np

FLT_EPSILON = np.float32(2.0 ** -23)

# intrinsics that are not TUM's (525, 525, 319.5, 239.5): unequal focal lengths, a principal point off the half-pixel grid
FOCAL = (517.3, 516.5)
PRINCIPAL = (318.6, 255.3)
SIZES = ((1, 1), (37, 23), (333, 207), (640, 480))          # (w, h)
FACTORS = (1.0 / 5000.0, float(FLT_EPSILON), 1.0, 0.001)
# factor edges on the 1 x 4 depth row [0, 1, 2, 65535]: depth 1 exactly at the threshold (invalid: the test is >), just above
# it, a negative factor, NaN, +inf (0 * inf = NaN: invalid; the others z = inf), a denormal (every product <= FLT_EPSILON)
FACTOR_EDGE_DEPTH = np.array([[0, 1, 2, 65535]], np.uint16)
FACTOR_EDGES = (float(FLT_EPSILON), float(np.nextafter(FLT_EPSILON, np.float32(1))), -1.0, float("nan"), float("inf"), 1e-45)
FACTOR_EDGES_VALID = ([False, False, True, True], [False, True, True, True], [False] * 4, [False] * 4,
                      [False, True, True, True], [False] * 4)


def backproject(depth, xy, factor=1.0 / 5000.0, focal=(525.0, 525.0), principal=(319.5, 239.5)):
    """depth [h][w] u16, xy [n][2] -> (xyz [n][3] f64, valid [n] bool)"""
    depth = np.asarray(depth, np.uint16)
    h, w = depth.shape
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    x, y = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
    finite = np.isfinite(x) & np.isfinite(y)
    px, py = np.trunc(np.where(finite, x, -1.0)), np.trunc(np.where(finite, y, -1.0))
    inside = finite & (px >= 0) & (px < w) & (py >= 0) & (py < h)
    ix, iy = np.where(inside, px, 0).astype(np.int64), np.where(inside, py, 0).astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        d = depth[iy, ix].astype(np.float32) * np.float32(factor)            # f32 * f32 -> f32: one rounding
        d = np.where(inside, d, np.float32(0))
        valid = d > FLT_EPSILON
        z = d.astype(np.float64)
        X = (x - np.float64(principal[0])) * z * (np.float64(1.0) / np.float64(focal[0]))
        Y = (y - np.float64(principal[1])) * z * (np.float64(1.0) / np.float64(focal[1]))
    xyz = np.where(valid[:, None], np.stack([X, Y, z], 1), 0.0)
    return np.ascontiguousarray(xyz), valid


def has_no_depth(xy, w, h):
    """the coordinates the contract gives no depth at all: not finite, or outside the image after truncation toward zero.
    Stated a second way (without trunc): a finite c lies in pixel range [0, n) exactly when -1 < c < n."""
    xy = np.asarray(xy, np.float32).reshape(-1, 2).astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = (xy[:, 0] > -1.0) & (xy[:, 0] < w) & (xy[:, 1] > -1.0) & (xy[:, 1] < h)
    return ~(ok & np.isfinite(xy).all(1))


def edge_coordinates(w, h):
    """the explicit list: NaN in either or both coordinates, the truncation boundary at 0, the far border, and values the
    int conversion cannot represent"""
    nan, inf = np.nan, np.inf
    return np.array([(nan, 1), (1, nan), (nan, nan),
                     (-0.5, -0.99), (-1, 0), (0, -1),
                     (w - 0.01, h - 0.01), (w, 0), (0, h),
                     (inf, 0), (-inf, 0), (0, inf), (0, -inf), (1e10, 0), (-3e9, 0), (2147483648.0, 0),
                     (0, 1e10), (0, -3e9), (0, 2147483648.0), (4294967296.0, 0), (0, 4294967297.0)], np.float32)


def make_depth(w, h, seed):
    """random u16 depth with about 30 % zeros; row 0 and column 0 are nonzero, so a coordinate wrongly sent to pixel
    row / column 0 (what a NaN becomes in a saturating float -> int conversion) comes back valid"""
    rng = np.random.default_rng(seed)
    d = rng.integers(1, 65536, (h, w), dtype=np.uint16)
    d[rng.random((h, w)) < 0.3] = 0
    d[0, :] = rng.integers(1000, 65536, w, dtype=np.uint16)
    d[:, 0] = rng.integers(1000, 65536, h, dtype=np.uint16)
    return d


def make_coordinates(w, h, n, seed):
    """n random points reaching 3 px outside each border, then the edge list"""
    rng = np.random.default_rng(seed)
    xy = np.stack([rng.uniform(-3, w + 3, n), rng.uniform(-3, h + 3, n)], 1).astype(np.float32)
    return np.concatenate([xy, edge_coordinates(w, h)])
