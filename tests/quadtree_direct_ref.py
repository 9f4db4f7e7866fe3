"""The quadtree selection in closed form: a plain restatement of what k_quadtree_direct computes, checked
against the oracle's list simulation by test_quadtree_direct_ref.py.

The reference (distribute_keypoints_via_tree) walks a std::list pass by pass.  Three facts make its result a function of
the candidates that needs no passes:

1. keep-or-divide is static: a node keeps when it holds one candidate or `(float)area * sf * sf <= min_size`; a child's
   rectangle depends only on its parent's, a candidate's child on two centre compares.  So a candidate's whole path
   (init node i0, children c1, c2, ...) is geometry, and a node divides in the pass after the one that made it, or never.
2. the list order is a sort key: after the last pass the nodes stand grouped by depth, deepest group first; inside the
   depth-d group the order is lexicographic in (i0, c1), c2, ..., cd with digit j descending when d - j is even (i0 goes
   with c1); the depth-0 group ascends.
3. the stop rule is a function of per-depth totals: with K[d] / M[d] the real keep / non-keep nodes of depth d (real: not
   empty, every proper ancestor non-keep), the list after pass p has n_p = K[0] + ... + K[p] + M[p] nodes, the last pass
   P is the first p >= 1 with n_p == n_(p-1), and the leaves are the real keep nodes of depth <= P plus the real
   non-keep nodes of depth P.
"""
import functools
import math

import numpy as np

BORDER = 19
MAX_DEPTH = 12      # a tree deeper than this counts as unbounded (its table would not fit anything)


def init_grid(w, h):
    """(nxg, nyg, delta_x, delta_y) of initialize_nodes on the bordered rectangle [19, w - 19) x [19, h - 19)"""
    min_x, max_x, min_y, max_y = BORDER, w - BORDER, BORDER, h - BORDER
    ratio = (max_x - min_x) / (max_y - min_y)
    if ratio > 1:
        nxg = int(math.floor(ratio + 0.5))
        return nxg, 1, (max_x - min_x) / nxg, float(max_y - min_y)
    nyg = int(math.floor(1 / ratio + 0.5))
    return 1, nyg, float(max_x - min_y), (max_y - min_y) / nyg      # sic: max_x - min_y


@functools.lru_cache(maxsize=None)
def area_keep(dx, dy, sf, min_size):
    """the reference's float32 rule on the unsigned area"""
    area = np.float32((dx * dy) & 0xFFFFFFFF)
    return bool(np.float32(np.float32(area * np.float32(sf)) * np.float32(sf)) <= np.float32(min_size))


def init_rect(i, nxg, delta_x, delta_y):
    ix, iy = i % nxg, i // nxg
    return int(delta_x * ix), int(delta_y * iy), int(delta_x * (ix + 1)), int(delta_y * (iy + 1))


def depth_bound(w, h, sf, min_size):
    """the depth at which every node keeps by area, from the largest init rectangle halved with ceil; None: unbounded"""
    nxg, nyg, delta_x, delta_y = init_grid(w, h)
    rects = [init_rect(i, nxg, delta_x, delta_y) for i in range(nxg * nyg)]
    dx = max(r[2] - r[0] for r in rects)
    dy = max(r[3] - r[1] for r in rects)
    d = 0
    while not area_keep(dx, dy, sf, min_size):
        if d == MAX_DEPTH or (dx <= 1 and dy <= 1):
            return None
        dx, dy, d = (dx + 1) >> 1, (dy + 1) >> 1, d + 1
    return d


def table_slots(n_init, depth):
    return n_init * (4 ** (depth + 1) - 1) // 3


def select(cand, w, h, sf, min_size):
    """cand: rows (x, y, response).  Returns (indices of the selected candidates in list order, info) or (None, info) when
    the depth is unbounded.  info: P, depth, n_init, dropped, cut (non-keep leaves left by the early stop)."""
    nxg, nyg, delta_x, delta_y = init_grid(w, h)
    n_init = nxg * nyg
    D = depth_bound(w, h, sf, min_size)
    info = dict(depth=D, n_init=n_init, dropped=0, cut=0, P=0)
    if D is None:
        return None, info
    cnt, akeep = {}, set()       # the node table, keyed (depth, i0 * 4^depth + digits); the kernel keeps it dense

    # 1. descent and counting: every candidate on its own
    paths = []
    for x, y, _ in cand:
        x, y = float(np.float32(x)), float(np.float32(y))
        idx = (int(x / delta_x) & 0xFFFFFFFF) + (int(y / delta_y) & 0xFFFFFFFF) * nxg
        if idx >= n_init:
            info["dropped"] += 1
            paths.append(None)
            continue
        bx, by, ex, ey = init_rect(idx, nxg, delta_x, delta_y)
        q, d = idx, 0
        while True:
            cnt[d, q] = cnt.get((d, q), 0) + 1
            if area_keep(ex - bx, ey - by, sf, min_size) or d == D:
                akeep.add((d, q))
                break
            cx, cy = bx + ((ex - bx + 1) >> 1), by + ((ey - by + 1) >> 1)
            c = (1 if cx <= x else 0) + (2 if cy <= y else 0)
            bx, ex = (cx, ex) if c & 1 else (bx, cx)
            by, ey = (cy, ey) if c & 2 else (by, cy)
            q, d = q * 4 + c, d + 1
        paths.append((q, d))

    # 2. node classes and the last pass
    K, M = [0] * (D + 2), [0] * (D + 2)
    keep_leaf, open_node = set(), set()
    for (d, q), n in cnt.items():
        if d and cnt[d - 1, q >> 2] < 2:
            continue                                    # not real: an ancestor kept
        if n == 1 or (d, q) in akeep:
            keep_leaf.add((d, q))
            K[d] += 1
        else:
            open_node.add((d, q))
            M[d] += 1
    P = 1
    while K[P] + M[P] != M[P - 1]:
        P += 1
    info["P"] = P
    top = min(P, D)
    info["cut"] = M[P]

    # 3. rank in list order: depth blocks from the deepest down, descending digits complemented
    def entry(node):
        d, q = node
        i0, low = q >> (2 * d), q & ((1 << (2 * d)) - 1)
        if d & 1:
            i0 = n_init - 1 - i0
        return -d, (i0 << (2 * d)) | (low ^ (0x33333333 & ((1 << (2 * d)) - 1)))

    leaves = [s for s in keep_leaf if s[0] <= top] + [s for s in open_node if s[0] == P]
    rank = {s: r for r, s in enumerate(sorted(leaves, key=entry))}

    # 4. winners: the first maximum of every leaf
    best = [None] * len(rank)
    for k, (path, row) in enumerate(zip(paths, cand)):
        if path is None:
            continue
        q, dk = path
        for d in range(min(dk, top) + 1):
            s = (d, q >> (2 * (dk - d)))
            if s in keep_leaf or d == top:
                break
        r = rank[s]
        if best[r] is None or float(row[2]) > float(cand[best[r]][2]):
            best[r] = k
    return best, info
