"""Inputs of the cv::ORB edge tests (test_cv_orb_edges.py on the CPU, test_gpu_cv_orb_edges.py on the GPU): frames that
steer k_cv_select (csrc/k_cvorb.hip) into a chosen branch, and the oracle-side helpers both suites share.

A DOT FRAME is a gray background (three equal channels) with single pixels raised above it on a regular grid that
starts at (40, 40).  FAST makes every dot exactly one keypoint, in raster order, with a score that rises with the dot's
height — so the list of heights IS the list of responses the first retainBest sees, which is what decides the
instance, the storage and the path through libstdc++'s introselect."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# the two comparisons of k_cv_select: n_raw <= 1024 picks the instance, n <= KP the storage (4096 for the large one)
SEL_LDS_SMALL, SEL_LDS = 1024, 4096
EDGE = 31
KEYS = ("xy", "desc", "octave", "angle", "response")


def regime(n):
    """where k_cv_select<KP, SMALL> keeps a (level, frame) pair with n FAST keypoints once the batch is split"""
    return "small" if n <= SEL_LDS_SMALL else "large-lds" if n <= SEL_LDS else "global"


def dot_frame(W, H, pitch, heights, background=0):
    """len(heights) dots in raster order on the grid (40 + i * pitch, 40 + j * pitch), rows as long as fit left of W - 40"""
    heights = np.asarray(heights).astype(np.int64)
    xs, ys = np.arange(40, W - 40, pitch), np.arange(40, H - 40, pitch)
    assert len(heights) <= len(xs) * len(ys), "the grid holds %d dots" % (len(xs) * len(ys))
    assert heights.min() > 0 and background + heights.max() <= 255
    g = np.full((H, W), background, np.uint8)
    k = np.arange(len(heights))
    g[ys[k // len(xs)], xs[k % len(xs)]] = background + heights
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))


def median_of_3_killer(n):
    """the input that drives median-of-3 quickselect into its depth limit (restated from test_oracle_std_order.py, which
    pins the oracle's introselect against the real library on it): a permutation of 1 .. n for even n"""
    a = np.zeros(n, np.float32)
    k = n // 2
    for i in range(1, k + 1):
        if i % 2 == 1:
            a[i - 1] = i
            a[i] = k + i
        a[k + i - 1] = 2 * i
    return a


def boundary_frame(n):
    """640x480, pitch 7, n dots of random height above the threshold 5: a level of exactly n FAST keypoints"""
    return dot_frame(640, 480, 7, np.random.default_rng(n).integers(6, 200, n))


def killer_frame(n, mirror=False):
    """320x240, pitch 8: FAST responses that form the killer sequence (or its mirror n + 1 - a)"""
    a = median_of_3_killer(n).astype(np.int64)
    return dot_frame(320, 240, 8, (n + 1 - a if mirror else a) + 5)


def one_height_frame():
    return dot_frame(320, 240, 8, np.full(300, 60))


def two_height_frame():
    return dot_frame(320, 240, 8, np.where(np.arange(300) % 3 == 0, 90, 40))


def noise_frame(W=320, H=240, seed=8):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def texture_frame(W=320, H=240, seed=5):
    import synth
    return synth.make_stream(1, W, H, seed=seed)[0]


def texture_stream(n, W=320, H=240, seed=5):
    """n consecutive views of one synthetic scene (frame 0 is texture_frame(seed=seed))"""
    import synth
    return synth.make_stream(n, W, H, seed=seed)


def flat_frame(W=320, H=240, value=77):
    return np.full((H, W, 3), value, np.uint8)


def level_candidates(orc, frame, p):
    """per level the FAST keypoints inside runByImageBorder(edge), raster order: oracle pyramid -> orc.fast -> border filter
    (as test_gpu_cv_orb.py::test_cv_orb_stages); rows (x, y, response) as debug_keypoints(DBG_CANDIDATES) returns them"""
    H, W = frame.shape[:2]
    w, h, _, _ = orc.cvorb_geometry(W, H, p)
    e = p.edge_threshold
    out = []
    for l, img in enumerate(orc.cvorb_pyramid(orc.gray(frame), p)):
        kp = orc.fast(img, p.fast_threshold, cap=img.size // 4 + 16)
        kp = kp[(kp["x"] >= e) & (kp["x"] < w[l] - e) & (kp["y"] >= e) & (kp["y"] < h[l] - e)]
        out.append(np.stack([kp["x"], kp["y"], kp["response"]], 1))
    return out


def level_counts(orc, frame, p):
    return [len(c) for c in level_candidates(orc, frame, p)]


def level_selected(orc, frame, p):
    """per level what both retainBest calls leave, in p's order; rows (x, y, Harris response) as DBG_SELECTED"""
    H, W = frame.shape[:2]
    q = orc.cvorb_geometry(W, H, p)[3]
    out = []
    for l, img in enumerate(orc.cvorb_pyramid(orc.gray(frame), p)):
        s = orc.cvorb_level_keypoints(img, p, q[l], 1)
        out.append(np.stack([s["x"], s["y"], s["response"]], 1))
    return out


def heap_select_calls(orc):
    return int(orc.lib().mso_std_heap_select_calls())


def same_bits(a, b):
    """bit-for-bit: floats compared as uint32 views (so -0.0 != 0.0 and NaN payloads count)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    return bool(np.array_equal(a, b))
