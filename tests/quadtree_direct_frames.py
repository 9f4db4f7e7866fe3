"""Inputs of tests/test_gpu_quadtree_direct.py: the smallest frames at which the direct form of the quadtree selection
(k_quadtree_direct) can go wrong, and the per-level eligibility the kernels' host side must report.
tests/test_quadtree_direct_ref.py proves on the CPU that they reach the regimes they are named after."""
import os
import sys

import numpy as np

import quadtree_direct_ref as Q

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

DIRECT_MAX_CANDIDATES = 1024        # k_quadtree_direct's instance: candidates of a (level, frame) pair ...
DIRECT_MAX_SLOTS = 1365             # ... and slots of the level's tree table
DEFAULTS = dict(n_levels=8, scale_factor=1.2, ini_fast_thr=20, min_fast_thr=7, min_node_area=1000)


def P(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def dots(points, W=160, H=120, bg=60, fg=200):
    """single bright pixels on a flat field: each is a FAST corner of level 0, all with the same score"""
    f = np.full((H, W, 3), bg, np.uint8)
    for x, y in points:
        f[y, x] = fg
    return f


def textured(W, H, seed, n=1):
    import synth
    return list(synth.make_stream(n, W, H, seed=seed))


def noise(W, H, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


# name -> (frame, parameters): single-frame calls
def single_cases():
    return {
        # one candidate: the init node keeps at once
        "one_dot": (dots([(50, 40)]), P(n_levels=2, min_node_area=20)),
        # two candidates 4 px apart deep inside one quadrant: every dividing node has ONE child, the first pass leaves the
        # list as long as it was and the loop stops with a non-keep leaf
        "two_dots_one_quadrant": (dots([(40, 36), (44, 36)]), P(n_levels=2, min_node_area=20)),
        # five equal dots inside one leaf (and one far away, so that the tree divides): the first maximum wins
        "equal_dots_one_leaf": (dots([(30, 30), (36, 30), (30, 36), (36, 36), (33, 42), (120, 90)]),
                                P(n_levels=2, min_node_area=1000)),
        # several init nodes in a row / in a column (the reference's `delta_x = max_x - min_y`)
        "wide": (textured(400, 100, 11)[0], P(n_levels=2, min_node_area=100)),
        "tall": (textured(80, 300, 12)[0], P(n_levels=2, min_node_area=100)),
    }


# parameters the direct form does not take: every level runs the list passes
def fallback_cases():
    return {
        "area50": (textured(320, 240, 21)[0], P(n_levels=2, min_node_area=50)),         # depth 6: 5461 slots
        "area7": (textured(320, 240, 22)[0], P(n_levels=4, min_node_area=7)),           # depth 7 and more
        "area7_unbounded": (textured(320, 240, 23)[0], P(n_levels=8, min_node_area=7)),  # levels 6, 7: no depth bound
    }


BATCH_W, BATCH_H = 320, 240
BATCH_FLAT, BATCH_NOISE = 2, 5      # positions of the flat and of the noise frame


def batch_frames():
    """9 frames (the batched path: three instances by candidate count): textured ones, one flat (no candidates) and one
    of noise (level 0 beyond the direct instance's candidates: quad_run's instance takes that pair in the same launch)"""
    frames = textured(BATCH_W, BATCH_H, 31, n=9)
    frames[BATCH_FLAT] = np.full((BATCH_H, BATCH_W, 3), 128, np.uint8)
    frames[BATCH_NOISE] = noise(BATCH_W, BATCH_H, 32)
    return frames


BATCH_P = P(n_levels=3)
# level 0 too deep for the table, levels 1 and 2 direct: the direct kernel and all three of quad_run's instances in one call
BATCH_MIXED_P = P(n_levels=3, min_node_area=66)


def level_sizes(W, H, p):
    s, out = np.float32(1.0), []
    for l in range(p["n_levels"]):
        if l:
            s = np.float32(np.float32(p["scale_factor"]) * s)
        out.append((W, H, s) if l == 0 else (int(np.floor(W / float(s) + 0.5)), int(np.floor(H / float(s) + 0.5)), s))
    return out


def eligible_levels(W, H, p):
    """per level: does the direct form take it (bounded depth, table within the instance)"""
    out = []
    for w, h, s in level_sizes(W, H, p):
        d = Q.depth_bound(w, h, float(s), p["min_node_area"])
        nxg, nyg, _, _ = Q.init_grid(w, h)
        out.append(d is not None and d <= 10 and Q.table_slots(nxg * nyg, d) <= DIRECT_MAX_SLOTS)
    return out


def oparams(orc, p):
    return orc.params(n_levels=p["n_levels"], scale_factor=p["scale_factor"], ini_fast_thr=p["ini_fast_thr"],
                      min_fast_thr=p["min_fast_thr"], min_size=p["min_node_area"])


def rows(c):
    """an oracle keypoint list as debug_keypoints returns it: rows (x, y, response)"""
    return np.stack([c["x"], c["y"], c["response"]], 1).reshape(-1, 3)


def level_lists(orc, frame, p):
    """per level (w, h, scale, FAST candidates) of the oracle"""
    op = oparams(orc, p)
    H, W = frame.shape[:2]
    w, h, s = orc.level_geometry(W, H, op)
    out = []
    for l, img in enumerate(orc.pyramid(orc.gray(frame), op)):
        out.append((w[l], h[l], s[l], rows(orc.fast_level(img, op, cap=w[l] * h[l] + 16))))
    return out


def oracle_select(orc, cand, w, h, s, min_size):
    """orc.quadtree on rows (x, y, response)"""
    if not len(cand):
        return np.zeros((0, 3), np.float32)
    c = np.zeros(len(cand), orc.CAND_DT)
    c["x"], c["y"], c["response"] = cand[:, 0], cand[:, 1], cand[:, 2]
    return rows(orc.quadtree(c, w, h, s, min_size))
