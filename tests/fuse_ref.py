"""Reference restatement of landmark fusion (not a test): the semantics include/mslam_hip.h states at
mslam_hip_kf_fuse_search, in numpy — the search (projection, eligibility, 3-D gate, knn-2, acceptance), the one-to-one
resolution and the store-wide replacement — built on tests/guided_match_ref.py's projection and window functions so the two
agree bit for bit; HipBackend.fuse's bookkeeping; and the tracker's fusion step on top of tests/local_map_ref.py and
tests/reloc_ref.py.  Shares no code with the product.

An entry is (desc [n, 32] u8, world [n, 3] f64, landmark ids [n] i64).  Also here: the case table tests/test_fuse.py proves
and tests/test_gpu_fuse.py runs, the cases away from the default frame (other extents and radii, a real pose and camera)
that tests/test_lm_table_edges.py proves and tests/test_gpu_fuse_edges.py runs, and the scene file `mslam_harness --fuse`
reads."""
import struct

import numpy as np

import guided_match_ref as gm
import local_map_ref as lm
import reloc_ref as rr

CAM = gm.CAM
FUSE_KEEP_ID, FUSE_DROP_ID = 0x7ffffffe, 0x7ffffffd


def entry(desc, world, lids):
    return (np.asarray(desc, np.uint8).reshape(-1, 32), np.asarray(world, np.float64).reshape(-1, 3),
            np.asarray(lids, np.int64).reshape(-1))


def eligible(keep_lids, drop_lids):
    """-> (keep [nk] bool, drop [nd] bool): a landmark whose id occurs anywhere in the other entry is out"""
    return ~np.isin(keep_lids, drop_lids), ~np.isin(drop_lids, keep_lids)


def drop_keypoints(world, R, t, cam, width, height):
    """the drop entry's landmarks as keypoints -> (xy [n, 2] f32, in frame [n] bool)"""
    u, v, c2 = gm.project(world, R, t, cam)
    with np.errstate(all="ignore"):
        xy = np.stack([u, v], 1).astype(np.float32)
        return xy, (c2 > 0) & gm.in_frame(xy, width, height)


def gate(keep_point, drop_world, max_world_distance):
    """((dx dx + dy dy) + dz dz) <= max_world_distance^2, a NaN giving False"""
    with np.errstate(all="ignore"):
        d = drop_world - keep_point
        return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) <= np.float64(max_world_distance) * np.float64(max_world_distance)


def accepted(keep, drop, R, t, radius, max_distance=50, ratio=0.7, max_world_distance=np.inf, cam=CAM, width=640, height=480):
    """per keep landmark the accepted (drop position, d0), or None"""
    kd, kw, kl = entry(*keep)
    dd, dw, dl = entry(*drop)
    k_ok, d_ok = eligible(kl, dl)
    xy, d_in = drop_keypoints(dw, R, t, cam, width, height)
    u, v, c2 = gm.project(kw, R, t, cam)
    out = [None] * len(kd)
    for j in np.flatnonzero(k_ok):
        cand = gm.candidates(xy, u[j], v[j], c2[j], width, height, radius) & d_ok & d_in & gate(kw[j], dw, max_world_distance)
        cand = np.flatnonzero(cand)
        if len(cand) == 0:
            continue
        d = gm.hamming(dd[cand], kd[j])
        order = np.lexsort((cand, d))[:2]                       # by distance, then by drop position
        d0 = np.int32(d[order[0]])
        d1 = np.int32(d[order[1]]) if len(order) > 1 else gm.ABSENT
        if gm.accept(d0, d1, max_distance, ratio):
            out[j] = (int(cand[order[0]]), int(d0))
    return out


def search(keep, drop, R, t, radius, **kw):
    """-> dict(keep_pos, drop_pos, keep_lid, drop_lid, dist), ordered by keep position: of several keep landmarks that
    accept one drop position the one with the least (d0, keep position) keeps the pair, the others get none"""
    acc = accepted(keep, drop, R, t, radius, **kw)
    best = {}
    for j, a in enumerate(acc):
        if a is not None and (a[0] not in best or (a[1], j) < best[a[0]]):
            best[a[0]] = (a[1], j)
    rows = sorted((j, i, d) for i, (d, j) in best.items())
    kl, dl = entry(*keep)[2], entry(*drop)[2]
    return dict(keep_pos=np.array([r[0] for r in rows], np.int32), drop_pos=np.array([r[1] for r in rows], np.int32),
                keep_lid=np.array([kl[r[0]] for r in rows], np.int64), drop_lid=np.array([dl[r[1]] for r in rows], np.int64),
                dist=np.array([r[2] for r in rows], np.int32))


def replace_ids(store, from_ids, to_ids, world_xyz=None):
    """store = {id: entry}.  -> (new store, number of landmarks whose id matched); simultaneous, the later of a repeated
    `from` wins"""
    src = {int(f): p for p, f in enumerate(np.asarray(from_ids, np.int64).reshape(-1).tolist())}
    to = np.asarray(to_ids, np.int64).reshape(-1)
    xyz = None if world_xyz is None else np.asarray(world_xyz, np.float64).reshape(-1, 3)
    out, n = {}, 0
    for id, e in store.items():
        d, w, l = entry(*e)
        w, l = w.copy(), l.copy()
        for i, old in enumerate(l.tolist()):
            if old in src:
                n += 1
                l[i] = to[src[old]]
                if xyz is not None:
                    w[i] = xyz[src[old]]
        out[id] = (d.copy(), w, l)
    return out, n


def fuse(store, keep_id, drop_id, R, t, radius, **kw):
    """search, then drop_lid -> keep_lid with the keep landmark's world point -> (pairs, new store, n_rewritten)"""
    pairs = search(store[keep_id], store[drop_id], R, t, radius, **kw)
    new, n = replace_ids(store, pairs["drop_lid"], pairs["keep_lid"], entry(*store[keep_id])[1][pairs["keep_pos"]])
    return pairs, new, n


def backend_fuse(obs, landmarks, anchor, keep_lids, drop_lids):
    """HipBackend.fuse on plain dicts (obs: id -> (landmark ids, camera points)) -> the three, renamed"""
    to = dict(zip(np.asarray(drop_lids).tolist(), np.asarray(keep_lids).tolist()))
    obs = {k: (np.array([to.get(l, l) for l in ids.tolist()], np.int64).reshape(-1), cam) for k, (ids, cam) in obs.items()}
    gone = {d for d, k in to.items() if d != k}
    return obs, {l: p for l, p in landmarks.items() if l not in gone}, {l: a for l, a in anchor.items() if l not in gone}


# ---- the tracker's fusion step --------------------------------------------------------------------------------------------

class FusionTracker(lm.LocalMapTracker):
    """local_map_ref.LocalMapTracker with the loop detection of tests/test_gpu_pose_graph.py's _expected_loop (every keyframe
    at least min_gap older that is not in the new keyframe's neighbourhood is verified by reloc_ref.relocalize; none while
    the last closure is fewer than min_gap keyframes back) and, with fusion, HipKeyframeTracker._fuse_loop restated.  There
    is no pose graph and no bundle adjustment here: the walk has no noise but the depth quantisation, so the tracked pose of
    the new keyframe stands for its corrected pose."""

    def __init__(self, fusion=False, min_gap=5, min_inliers=60, radius=8.0, max_distance=50, world_distance=0.1, width=640,
                 height=480, **kw):
        super().__init__(**kw)
        self.fusion, self.min_gap, self.min_inliers = fusion, min_gap, min_inliers
        self.radius, self.max_distance, self.world_distance, self.extent = radius, max_distance, world_distance, (width, height)
        self.loops, self.last_closure = [], None

    def process(self, desc, xy, depth):
        f = self.frame
        out = super().process(desc, xy, depth)
        k = out["keyframe"]
        out["loop"] = None
        if k <= 0 or self.depth is None:
            return out
        if self.last_closure is not None and k - self.last_closure < self.min_gap:
            return out
        near = lm.neighbours(self.graph, k, self.depth)
        cands = [j for j in self.ids if k - j >= self.min_gap and j not in near]
        if not cands:
            return out
        best = rr.relocalize(desc, xy, self.store, cands, self.cam, seed=f, min_inliers=self.min_inliers)["best"]
        if best < 0:
            return out
        loop = cands[best]
        event = dict(keyframe=k, loop=loop, frame=f)
        self.last_closure = k
        self._map_of = None
        if self.fusion:
            event["fusion"] = self.fuse_loop(k, loop)
        self.loops.append(event)
        out["loop"] = (k, loop)
        return out

    def fuse_loop(self, new_id, loop_id):
        old = sorted(lm.neighbours(self.graph, loop_id, self.depth))[-64:]
        new = sorted(lm.neighbours(self.graph, new_id, self.depth))[-64:]
        self.serial += 2                                        # the two unions
        store = {k: (self.store[k][0], self.store[k][1], self.lids[k]) for k in self.store}
        if self.map is not None:
            store[lm.LOCAL_MAP_ID] = self.map                   # the union the frame was tracked on is a live entry too
        store[FUSE_KEEP_ID] = lm.union(self.store, self.lids, old)
        store[FUSE_DROP_ID] = lm.union(self.store, self.lids, new)
        pairs, store, n = fuse(store, FUSE_KEEP_ID, FUSE_DROP_ID, self.R, self.t, self.radius, max_distance=self.max_distance,
                               ratio=self.ratio, max_world_distance=self.world_distance, cam=self.cam, width=self.extent[0],
                               height=self.extent[1])
        for k in self.store:
            self.store[k], self.lids[k] = store[k][:2], store[k][2]
        edges = []
        for k in new:
            for other, c in zip(old, lm.covisible(self.lids, k, old)):
                if c > 0 and other != k and other not in self.graph[k]:
                    self.graph[k].add(other)
                    self.graph[other].add(k)
                    edges.append((k, other))
        return dict(n_pairs=len(pairs["keep_lid"]), n_rewritten=n, edges=edges, pairs=pairs)


def run_ring(seq, fusion, **kw):
    """the ring walk of tests/loop_walk.py with tests/test_gpu_pose_graph.py's parameters -> (rows, tracker)"""
    trk = FusionTracker(fusion=fusion, depth=2, cam=seq["cam"], new_keyframe_min_landmarks=200, width=seq["width"],
                        height=seq["height"], **kw)
    return [trk.process(fr["desc"], fr["xy"], fr["depth"]) for fr in seq["frames"]], trk


# ---- cases ------------------------------------------------------------------------------------------------------------------

IDENTITY = dict(R=np.eye(3), t=np.zeros(3), cam=gm.IDENTITY_CAM, width=640, height=480)   # with Z = 1: u = X, v = Y exactly


def near(rng, desc, bits):
    return rr._flip_bits(rng, np.asarray(desc, np.uint8).reshape(-1, 32), bits)


def random_case(seed, nk, nd, shared=0, width=640, height=480, spread=1.5, twin_spread=1.0, deeper=0.001):
    """nk keep landmarks at Z = 1 uniform over the frame and a little beyond; of the nd drop landmarks up to two thirds (at most
    4/3 of nk: one per keep landmark, a third of those a second copy) sit within `spread` px of a keep landmark, 0.0 .. `deeper`
    (0.001) deeper, and carry its descriptor with a few flipped bits; a quarter of the keep landmarks are look-alikes of another keep landmark within a pixel of it, so two
    keep landmarks claim one drop landmark (`twin_spread`: how far, in px, a look-alike sits from its model); `shared` ids
    occur on both sides.
    -> dict(keep, drop, radius, kw)"""
    rng = np.random.default_rng(seed)
    kw_ = np.stack([rng.uniform(-10, width + 10, nk), rng.uniform(-10, height + 10, nk), np.ones(nk)], 1)
    kd = rng.integers(0, 256, (nk, 32), dtype=np.uint8)
    dw = np.stack([rng.uniform(-10, width + 10, nd), rng.uniform(-10, height + 10, nd), np.ones(nd)], 1)
    dd = rng.integers(0, 256, (nd, 32), dtype=np.uint8)
    if nk and nd:
        twin = rng.choice(nk, nk // 4, replace=False)          # keep landmarks that are look-alikes of another one, next to it:
        of = rng.integers(0, nk, len(twin))                    # both claim that one's duplicate
        kw_[twin, :2] = kw_[of, :2] + rng.uniform(-twin_spread, twin_spread, (len(twin), 2))
        kd[twin] = near(rng, kd[of], 3)
        dup = rng.choice(nd, min((2 * nd + 2) // 3, nk + nk // 3), replace=False)
        src = np.concatenate([rng.permutation(nk), rng.integers(0, nk, nk // 3)])[:len(dup)]   # a third of them a second copy
        dw[dup, :2] = kw_[src, :2] + rng.uniform(-spread, spread, (len(dup), 2))
        dw[dup, 2] = 1.0 + rng.uniform(0.0, deeper, len(dup))
        for i, k in zip(dup, src):                             # 1 .. 15 flipped bits: where several drop landmarks copy one
            dd[i] = near(rng, kd[k], int(rng.integers(1, 16)))[0]   # keep landmark the ratio test passes some and fails others
    kl = 1000 + np.arange(nk, dtype=np.int64)
    dl = 500000 + np.arange(nd, dtype=np.int64)
    for s in range(min(shared, nk, nd)):
        dl[(7 * s) % nd] = kl[(3 * s) % nk]
    return dict(keep=(kd, kw_, kl), drop=(dd, dw, dl), radius=4.0,
                kw=dict(IDENTITY, width=width, height=height, max_distance=50, ratio=0.7, max_world_distance=2.0))


CHUNK = 1024                                   # keep landmarks per pass of the one-workgroup resolution
CHUNK_SIZES = [(1024, 1024), (1025, 1100), (2100, 2100)]   # exactly one pass; one landmark in the second; three passes
SIZES = [(0, 5), (5, 0), (1, 1), (2, 2), (7, 40), (8, 40), (9, 40), (31, 20), (32, 20), (33, 20), (255, 257), (256, 256),
         (257, 255), (4500, 3), (3, 3000)] + CHUNK_SIZES   # (keep, drop): the search's 8 / 32 landmarks per workgroup (the
                                               # latter above 4096 keep landmarks), the other kernels' 256, either side large,
                                               # and many pairs in every pass of the resolution


def plant_chunks(case, seed, tail=60):
    """Into a random_case, in place: the last `tail` keep landmarks each get a place of their own in the frame and a
    duplicate among the last `tail` drop landmarks, so the last pass of the resolution compacts (nearly) a pair per landmark;
    and per pass after the first, up to three drop landmarks claimed by a keep landmark of that pass AND by one of the first
    pass: the later one at distance 2 against 4 (it takes the pair), at 6 against 4 (it gets none) and at 4 against 4 (the lower
    keep position takes it).  -> the planted (first-pass keep, later keep, drop position, winner) rows"""
    rng = np.random.default_rng(seed)
    (kd, kw_, kl), (dd, dw, dl) = case["keep"], case["drop"]
    nk, nd, w, h = len(kd), len(dd), case["kw"]["width"], case["kw"]["height"]

    def place(j, i, bits):                                      # keep j somewhere new, drop i its duplicate
        kw_[j] = (rng.uniform(20, w - 20), rng.uniform(20, h - 20), 1.0)
        kd[j] = rng.integers(0, 256, 32, dtype=np.uint8)
        dw[i] = (kw_[j, 0] + rng.uniform(-1, 1), kw_[j, 1] + rng.uniform(-1, 1), 1.0 + rng.uniform(0.0, 0.001))
        dd[i] = near(rng, kd[j], bits)[0]

    tail = min(tail, nk, nd)
    for m in range(tail):
        place(nk - tail + m, nd - tail + m, int(rng.integers(1, 4)))
    rows = []
    for c in range(1, (nk + CHUNK - 1) // CHUNK):
        for m, bits in enumerate((2, 6, 4)):
            b, i = 100 + 40 * c + 7 * m, 200 + 40 * c + 11 * m          # clear of the shared ids' positions
            a = c * CHUNK + 5 + 300 * m
            if a >= nk or (a >= nk - tail and bits >= 4):                # (one of the tail gives its pair up only for another)
                continue
            place(b, i, 4)
            kw_[a] = kw_[b] + (0.25, -0.25, 0.0)
            kd[a] = near(rng, dd[i], bits)[0]
            rows.append((b, a, i, a if bits < 4 else b))
    return rows


def sized_case(nk, nd):
    """the case of one entry of SIZES"""
    case = random_case(100 + nk + nd, nk, nd, shared=3 if min(nk, nd) > 30 else 1 if min(nk, nd) > 3 else 0)
    case["planted"] = plant_chunks(case, nk + nd) if (nk, nd) in CHUNK_SIZES else []
    return case


# ---- away from the default frame -------------------------------------------------------------------------------------------

FRAMES = [(100, 80), (20, 20), (4114, 102), (8192, 8192)]
FRAME_SIZES = [(65, 64), (513, 700)]


def frame_radii(width, height):
    """half a pixel, two radii of tests/test_gpu_guided_match.py and one beyond the frame (brute force: every eligible drop
    landmark in the frame is a candidate of every keep landmark)"""
    return [0.5, 15.0, 47.5, float(max(width, height) + 10)]


def frame_case(nk, nd, width, height):
    """random_case in a width x height frame with every duplicate inside the smallest radius: 0.2 px beside its keep
    landmark and so little deeper that u = X / Z moves by 0.2 px at most, a look-alike 0.05 px from its model"""
    return random_case(7 * width + height + nk, nk, nd, shared=3, width=width, height=height, spread=0.2, twin_spread=0.05,
                       deeper=0.2 / (max(width, height) + 10))


POSE_R = rr.po.rodrigues([0.3, -0.2, 0.1])
POSE_T = np.array([0.4, -0.3, 0.6])
POSED_SIZES = [(300, 280), (1025, 1100)]


def posed_case(seed, nk, nd, shared=0, width=640, height=480, spread=1.5):
    """random_case's scene in the frame of a camera at a real pose: pixels uniform over the frame and a little beyond, depths
    uniform in 0.5 .. 4 m, camera point ((u - cx) / fx Z, (v - cy) / fy Z, Z) with guided_match_ref.CAM, and
    world = R^T (c - t).  A duplicate is 0 .. 1 mm deeper than its keep landmark; half of the other drop landmarks are further
    copies 0.1 .. 0.5 m behind a keep landmark: inside its window but beyond the gate of 0.05 m, which alone keeps them from
    taking the pair or spoiling the ratio test.
    -> dict(keep, drop, radius, kw)"""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = CAM

    def world(px, z):
        c = np.stack([(px[:, 0] - cx) / fx * z, (px[:, 1] - cy) / fy * z, z], 1)
        return (c - POSE_T) @ POSE_R                                          # rows of R^T (c - t)

    kpx = np.stack([rng.uniform(-10, width + 10, nk), rng.uniform(-10, height + 10, nk)], 1)
    kz = rng.uniform(0.5, 4.0, nk)
    kd = rng.integers(0, 256, (nk, 32), dtype=np.uint8)
    dpx = np.stack([rng.uniform(-10, width + 10, nd), rng.uniform(-10, height + 10, nd)], 1)
    dz = rng.uniform(0.5, 4.0, nd)
    dd = rng.integers(0, 256, (nd, 32), dtype=np.uint8)
    twin = rng.choice(nk, nk // 4, replace=False)
    of = rng.integers(0, nk, len(twin))
    kpx[twin] = kpx[of] + rng.uniform(-1.0, 1.0, (len(twin), 2))
    kz[twin] = kz[of] + rng.uniform(0.0, 0.001, len(twin))
    kd[twin] = near(rng, kd[of], 3)
    dup = rng.choice(nd, min((2 * nd + 2) // 3, nk + nk // 3), replace=False)
    src = np.concatenate([rng.permutation(nk), rng.integers(0, nk, nk // 3)])[:len(dup)]
    dpx[dup] = kpx[src] + rng.uniform(-spread, spread, (len(dup), 2))
    dz[dup] = kz[src] + rng.uniform(0.0, 0.001, len(dup))
    rest = np.setdiff1d(np.arange(nd), dup)
    far = rest[:len(rest) // 2]                                               # further copies, behind their keep landmark
    far_src = src[rng.integers(0, len(src), len(far))]
    dpx[far] = kpx[far_src] + rng.uniform(-spread, spread, (len(far), 2))
    dz[far] = kz[far_src] + rng.uniform(0.1, 0.5, len(far))
    for i, k in zip(np.concatenate([dup, far]), np.concatenate([src, far_src])):
        dd[i] = near(rng, kd[k], int(rng.integers(1, 16)))[0]
    kl = 1000 + np.arange(nk, dtype=np.int64)
    dl = 500000 + np.arange(nd, dtype=np.int64)
    for s in range(min(shared, nk, nd)):
        dl[(7 * s) % nd] = kl[(3 * s) % nk]
    return dict(keep=(kd, world(kpx, kz), kl), drop=(dd, world(dpx, dz), dl), radius=4.0,
                kw=dict(R=POSE_R, t=POSE_T, cam=CAM, width=width, height=height, max_distance=50, ratio=0.7, max_world_distance=0.05))


def gate_alone(case):
    """the (keep, drop) position pairs that pass every test of the search but the 3-D gate"""
    kw = case["kw"]
    (kd, kw_, kl), (dd, dw, dl) = entry(*case["keep"]), entry(*case["drop"])
    k_ok, d_ok = eligible(kl, dl)
    xy, d_in = drop_keypoints(dw, kw["R"], kw["t"], kw["cam"], kw["width"], kw["height"])
    u, v, c2 = gm.project(kw_, kw["R"], kw["t"], kw["cam"])
    out = []
    for j in np.flatnonzero(k_ok):
        cand = gm.candidates(xy, u[j], v[j], c2[j], kw["width"], kw["height"], case["radius"]) & d_ok & d_in
        out += [(int(j), int(i)) for i in np.flatnonzero(cand & ~gate(kw_[j], dw, kw["max_world_distance"]))]
    return out


def hand_case(name):
    """small planted scenes, one per rule -> dict(keep, drop, radius, kw, expect = [(keep_pos, drop_pos, dist)])"""
    rng = np.random.default_rng(11)
    D = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    f32 = np.float32

    def flip(row, bits):
        r = np.unpackbits(row)
        r[:bits] ^= 1
        return np.packbits(r)

    kw = dict(IDENTITY, max_distance=50, ratio=0.7, max_world_distance=np.inf)
    radius = 4.0
    if name == "window_edge":          # exactly at the radius is in, the next f32 beyond is out
        keep = ([D[0], D[1]], [(100, 100, 1), (200, 100, 1)], [1, 2])
        drop = ([D[0], D[1]], [(104, 100, 1), (np.nextafter(f32(204), f32(np.inf)), 100, 1)], [11, 12])
        expect = [(0, 0, 0)]
    elif name == "frame_border":       # a drop landmark at x = 0 is in frame; at x = width it is not; nor at y < 0
        keep = ([D[0], D[1], D[2]], [(1, 50, 1), (639, 50, 1), (50, 1, 1)], [1, 2, 3])
        drop = ([D[0], D[1], D[2], D[1]], [(0, 50, 1), (640, 50, 1), (50, -0.5, 1), (np.nextafter(f32(640), f32(0)), 50, 1)], [11, 12, 13, 14])
        expect = [(0, 0, 0), (1, 3, 0)]
    elif name == "behind":             # c2 <= 0 on either side
        keep = ([D[0], D[1], D[2]], [(100, 100, 0), (200, 100, -1), (300, 100, 1)], [1, 2, 3])
        drop = ([D[0], D[1], D[2], D[2]], [(100, 100, 0), (200, 100, 1), (300, 100, -1), (301, 100, 1)], [11, 12, 13, 14])
        expect = [(2, 3, 0)]
    elif name == "nan_point":          # a NaN world point on either side is no searcher and no candidate
        keep = ([D[0], D[1]], [(np.nan, 100, 1), (200, 100, 1)], [1, 2])
        drop = ([D[0], D[1], D[1]], [(100, 100, 1), (200, np.nan, 1), (201, 100, 1)], [11, 12, 13])
        expect = [(1, 2, 0)]
    elif name in ("gate_at", "gate_beyond", "gate_inf"):   # dx = 0.25 exactly (0.0625 is exact in f64), and dx = 3
        keep = ([D[0], D[1]], [(100, 100, 1), (300, 100, 1)], [1, 2])
        drop = ([D[0], D[1]], [(100.25, 100, 1), (303, 100, 1)], [11, 12])
        kw["max_world_distance"] = {"gate_at": 0.25, "gate_beyond": np.nextafter(0.25, 0.0), "gate_inf": np.inf}[name]
        expect = {"gate_at": [(0, 0, 0)], "gate_beyond": [], "gate_inf": [(0, 0, 0), (1, 1, 0)]}[name]
    elif name == "gate_before_ratio":  # a look-alike inside the window but beyond the gate does not spoil the ratio test
        keep = ([D[0]], [(100, 100, 1)], [1])
        drop = ([flip(D[0], 3), flip(D[0], 4)], [(101, 100, 1), (100, 103, 1)], [11, 12])
        kw["max_world_distance"] = 2.0
        expect = [(0, 0, 3)]
    elif name == "ratio_rejects":      # the same two with the gate off: 3 < 0.7 * 4 fails
        keep = ([D[0]], [(100, 100, 1)], [1])
        drop = ([flip(D[0], 3), flip(D[0], 4)], [(101, 100, 1), (100, 103, 1)], [11, 12])
        expect = []
    elif name == "equal_distance":     # equal distances: the lower drop position is the first neighbour (3 < 1.01 * 3 accepts it)
        keep = ([D[0], D[1]], [(100, 100, 1), (300, 100, 1)], [1, 2])
        drop = ([flip(D[0], 3), flip(D[0], 3), flip(D[1], 30), flip(D[1], 10), flip(D[1], 10)],
                [(101, 100, 1), (100, 101, 1), (300, 101, 1), (301, 100, 1), (299, 100, 1)], [11, 12, 13, 14, 15])
        kw["ratio"] = 1.01
        expect = [(0, 0, 3), (1, 3, 10)]
    elif name == "equal_distance_rejected":   # ... and with the usual ratio d0 == d1 is rejected
        keep = ([D[0]], [(100, 100, 1)], [1])
        drop = ([flip(D[0], 3), flip(D[0], 3)], [(101, 100, 1), (100, 101, 1)], [11, 12])
        expect = []
    elif name == "lone_and_max_distance":   # a lone candidate is accepted up to max_distance
        keep = ([D[0], D[1]], [(100, 100, 1), (300, 100, 1)], [1, 2])
        drop = ([flip(D[0], 50), flip(D[1], 51)], [(100, 100, 1), (300, 100, 1)], [11, 12])
        expect = [(0, 0, 50)]
    elif name == "two_claim_one":      # keep 0 and 2 both accept drop 0 at distance 4, keep 1 at distance 3: the least (d0, position)
        keep = ([flip(D[0], 4), flip(D[0], 3), flip(D[0], 4)], [(100, 100, 1), (101, 100, 1), (100, 101, 1)], [1, 2, 3])
        drop = ([D[0], D[5]], [(100.5, 100.5, 1), (400, 400, 1)], [11, 12])
        expect = [(1, 0, 3)]
    elif name == "two_claim_one_tie":  # equal distances: the lower keep position keeps the pair, the other gets none
        keep = ([D[6], flip(D[0], 4), flip(D[0], 4)], [(400, 100, 1), (101, 100, 1), (100, 101, 1)], [1, 2, 3])
        drop = ([D[0], flip(D[0], 200)], [(100.5, 100.5, 1), (100, 100, 1)], [11, 12])
        expect = [(1, 0, 4)]
    elif name == "shared_ids":         # id 2 is on both sides: keep 1 does not search, drop 0 is no candidate (keep 0 would take it)
        keep = ([D[0], D[1]], [(100, 100, 1), (300, 100, 1)], [1, 2])
        drop = ([D[0], D[1], D[0]], [(100, 100, 1), (300, 100, 1), (102, 100, 1)], [2, 12, 13])
        expect = [(0, 2, 0)]
    elif name == "repeated_id":        # an id repeated inside the drop entry: both are landmarks of their own to the search
        keep = ([D[0], D[1]], [(100, 100, 1), (300, 100, 1)], [1, 2])
        drop = ([D[0], D[1]], [(100, 100, 1), (300, 100, 1)], [11, 11])
        expect = [(0, 0, 0), (1, 1, 0)]
    else:
        raise KeyError(name)
    return dict(keep=entry(*keep), drop=entry(*drop), radius=radius, kw=kw, expect=expect)


HAND_CASES = ["window_edge", "frame_border", "behind", "nan_point", "gate_at", "gate_beyond", "gate_inf", "gate_before_ratio",
              "ratio_rejects", "equal_distance", "equal_distance_rejected", "lone_and_max_distance", "two_claim_one", "two_claim_one_tie", "shared_ids",
              "repeated_id"]


# ---- the scene file of `mslam_harness <plugin> --fuse <scene>` ---------------------------------------------------------------

def write_scene(path, keep, drop, R, t, radius, cam=CAM, width=640, height=480, max_distance=50, ratio=0.7, max_world_distance=np.inf,
                others=()):
    """little-endian: magic "MSFU", i32 version 1, i32 width, height, max_distance, f64 fx fy cx cy radius ratio
    max_world_distance, R (9 f64), t (3 f64), i32 number of entries; then per entry (keep, drop, then `others`, which the
    replacement must reach as well): i32 n, descriptors n x 32, world points n x 3 f64, landmark ids n x i64"""
    with open(path, "wb") as f:
        f.write(b"MSFU" + struct.pack("<4i", 1, width, height, max_distance))
        f.write(struct.pack("<7d", cam[0], cam[1], cam[2], cam[3], radius, ratio, max_world_distance))
        f.write(np.asarray(R, "<f8").reshape(9).tobytes() + np.asarray(t, "<f8").reshape(3).tobytes())
        entries = [keep, drop] + list(others)
        f.write(struct.pack("<i", len(entries)))
        for e in entries:
            d, w, l = entry(*e)
            f.write(struct.pack("<i", len(d)) + d.tobytes() + w.astype("<f8").tobytes() + l.astype("<i8").tobytes())
