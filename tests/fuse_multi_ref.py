"""Reference restatement of landmark fusion into many target entries (not a test): the semantics include/mslam_hip.h
states at mslam_hip_kf_fuse_search_multi, in numpy — per target the search of tests/fuse_ref.py (its projection, in-frame
test, 3-D gate, knn-2 and acceptance, on tests/guided_match_ref.py's functions) with eligibility taken over all listed
entries, the per-target resolution, the two cross-target steps on landmark ids, and the store-wide replacement — and the
tracker's fusion step with every keyframe of the new side as a target, on top of fuse_ref.FusionTracker.  Shares no code
with the product.

An entry is (desc [n, 32] u8, world [n, 3] f64, landmark ids [n] i64).  Also here: the hand cases and random cases that
tests/test_fuse_multi.py proves and tests/test_gpu_fuse_multi.py runs, and the scene file `mslam_harness --fuse-multi`
reads."""
import struct

import numpy as np

import fuse_ref as fr
import guided_match_ref as gm
import local_map_ref as lm
import reloc_ref as rr

CAM = gm.CAM
KEYS = ("target", "keep_pos", "drop_pos", "keep_lid", "drop_lid", "dist")


def eligible(keep_lids, drop_lids_per_target):
    """-> (keep [nk] bool, [drop [nd_m] bool per target]): a keep landmark whose id occurs in ANY listed drop entry is out in
    every target, and so is a drop landmark whose id occurs in the keep entry"""
    every = np.concatenate([np.asarray(l, np.int64).reshape(-1) for l in drop_lids_per_target] + [np.zeros(0, np.int64)])
    return ~np.isin(keep_lids, every), [~np.isin(l, keep_lids) for l in drop_lids_per_target]


def accepted(keep, drop, k_ok, d_ok, R, t, radius, max_distance, ratio, max_world_distance, cam, width, height):
    """fuse_ref.accepted for one target with the eligibility given: per keep landmark the accepted (drop position, d0), or
    None.  The window and the gate are evaluated for all (keep, drop) pairs at once, with the expressions of
    guided_match_ref.candidates and fuse_ref.gate (tests/test_fuse_multi.py holds the result to fuse_ref.accepted)."""
    kd, kw, kl = fr.entry(*keep)
    dd, dw, dl = fr.entry(*drop)
    out = [None] * len(kd)
    if len(kd) == 0 or len(dd) == 0:
        return out
    xy, d_in = fr.drop_keypoints(dw, R, t, cam, width, height)
    u, v, c2 = gm.project(kw, R, t, cam)
    x, y = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        window = (np.abs(x[None, :] - u[:, None]) <= np.float64(radius)) & (np.abs(y[None, :] - v[:, None]) <= np.float64(radius))
        d = dw[None, :, :] - kw[:, None, :]
        gate = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) <= np.float64(max_world_distance) * np.float64(max_world_distance)
        cand_of = window & gate & (d_ok & d_in)[None, :] & (k_ok & (c2 > 0))[:, None]
    for j in np.flatnonzero(cand_of.any(1)):
        cand = np.flatnonzero(cand_of[j])
        dist = gm.hamming(dd[cand], kd[j])
        order = np.lexsort((cand, dist))[:2]                    # by distance, then by drop position
        d0 = np.int32(dist[order[0]])
        d1 = np.int32(dist[order[1]]) if len(order) > 1 else gm.ABSENT
        if gm.accept(d0, d1, max_distance, ratio):
            out[j] = (int(cand[order[0]]), int(d0))
    return out


def search_multi(keep, drops, Rs, ts, radius, max_distance=50, ratio=0.7, max_world_distance=np.inf, cam=CAM, width=640, height=480,
                 stages=None):
    """-> dict(target, keep_pos, drop_pos, keep_lid, drop_lid, dist), ordered by (target, keep position).  `stages`, a dict,
    receives the rows (target, keep_pos, drop_pos, dist) left by the per-target resolution ("rows"), dropped by step A
    ("dropped_a") and dropped by step B ("dropped_b")."""
    kl = fr.entry(*keep)[2]
    dls = [fr.entry(*d)[2] for d in drops]
    Rs = np.asarray(Rs, np.float64).reshape(-1, 3, 3)
    ts = np.asarray(ts, np.float64).reshape(-1, 3)
    assert len(Rs) == len(ts) == len(drops)
    k_ok, d_oks = eligible(kl, dls)
    rows = []                                                   # (dist, target, keep_pos, drop_pos)
    for m, drop in enumerate(drops):
        acc = accepted(keep, drop, k_ok, d_oks[m], Rs[m], ts[m], radius, max_distance, ratio, max_world_distance, cam, width, height)
        best = {}                                               # per-target: the least (d0, keep position) per drop position
        for j, a in enumerate(acc):
            if a is not None and (a[0] not in best or (a[1], j) < best[a[0]]):
                best[a[0]] = (a[1], j)
        rows += [(d, m, j, i) for i, (d, j) in best.items()]
    by_drop = {}                                                # step A: per drop id the least (dist, target, keep_pos)
    for r in rows:
        l = int(dls[r[1]][r[3]])
        if l not in by_drop or r[:3] < by_drop[l][:3]:
            by_drop[l] = r
    after_a = sorted(by_drop.values())
    by_keep = {}                                                # step B: per keep id the least (dist, target, drop_pos)
    for r in after_a:
        l = int(kl[r[2]])
        if l not in by_keep or (r[0], r[1], r[3]) < (by_keep[l][0], by_keep[l][1], by_keep[l][3]):
            by_keep[l] = r
    final = sorted(by_keep.values(), key=lambda r: (r[1], r[2]))
    if stages is not None:
        fmt = lambda rs: sorted((r[1], r[2], r[3], r[0]) for r in rs)
        stages.update(rows=fmt(rows), dropped_a=fmt(set(rows) - set(after_a)), dropped_b=fmt(set(after_a) - set(final)))
    return dict(target=np.array([r[1] for r in final], np.int32), keep_pos=np.array([r[2] for r in final], np.int32),
                drop_pos=np.array([r[3] for r in final], np.int32), keep_lid=np.array([kl[r[2]] for r in final], np.int64),
                drop_lid=np.array([dls[r[1]][r[3]] for r in final], np.int64), dist=np.array([r[0] for r in final], np.int32))


def fuse_multi(store, keep_id, drop_ids, Rs, ts, radius, **kw):
    """search_multi, then drop_lid -> keep_lid with the winning keep position's world point -> (pairs, new store, n_rewritten)"""
    pairs = search_multi(store[keep_id], [store[d] for d in drop_ids], Rs, ts, radius, **kw)
    new, n = fr.replace_ids(store, pairs["drop_lid"], pairs["keep_lid"], fr.entry(*store[keep_id])[1][pairs["keep_pos"]])
    return pairs, new, n


def rows_of(p):
    return list(zip(p["target"].tolist(), p["keep_pos"].tolist(), p["drop_pos"].tolist(), p["dist"].tolist()))


# ---- the tracker's fusion step -----------------------------------------------------------------------------------------------

class MultiFusionTracker(fr.FusionTracker):
    """fuse_ref.FusionTracker with HipKeyframeTracker(loop_fusion_keyframes=True)'s fusion step restated: one union (the old
    side, keep) and every keyframe of the new side a target under its own pose.  There is no pose graph and no bundle
    adjustment here, so the pose a keyframe was tracked with stands for its corrected pose."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.kf_pose = {}

    def process(self, desc, xy, depth):
        out = super().process(desc, xy, depth)
        if out["keyframe"] >= 0:
            self.kf_pose.setdefault(out["keyframe"], (out["R"], out["t"]))
        return out

    def fuse_loop(self, new_id, loop_id):
        self.kf_pose[new_id] = (self.R.copy(), self.t.copy())   # (the keyframe was made inside this very step)
        old = sorted(lm.neighbours(self.graph, loop_id, self.depth))[-64:]
        new = sorted(lm.neighbours(self.graph, new_id, self.depth))[-64:]
        self.serial += 1                                        # the one union
        store = {k: (self.store[k][0], self.store[k][1], self.lids[k]) for k in self.store}
        if self.map is not None:
            store[lm.LOCAL_MAP_ID] = self.map                   # the union the frame was tracked on is a live entry too
        store[fr.FUSE_KEEP_ID] = lm.union(self.store, self.lids, old)
        pairs, store, n = fuse_multi(store, fr.FUSE_KEEP_ID, new, [self.kf_pose[k][0] for k in new], [self.kf_pose[k][1] for k in new],
                                     self.radius, max_distance=self.max_distance, ratio=self.ratio,
                                     max_world_distance=self.world_distance, cam=self.cam, width=self.extent[0], height=self.extent[1])
        for k in self.store:
            self.store[k], self.lids[k] = store[k][:2], store[k][2]
        edges = []
        for k in new:
            for other, c in zip(old, lm.covisible(self.lids, k, old)):
                if c > 0 and other != k and other not in self.graph[k]:
                    self.graph[k].add(other)
                    self.graph[other].add(k)
                    edges.append((k, other))
        return dict(n_pairs=len(pairs["keep_lid"]), n_rewritten=n, edges=edges, pairs=pairs, targets=new)


def run_ring(seq, **kw):
    """fuse_ref.run_ring with the multi-target fusion step -> (rows, tracker)"""
    trk = MultiFusionTracker(fusion=True, depth=2, cam=seq["cam"], new_keyframe_min_landmarks=200, width=seq["width"],
                             height=seq["height"], **kw)
    return [trk.process(f["desc"], f["xy"], f["depth"]) for f in seq["frames"]], trk


# ---- hand cases ---------------------------------------------------------------------------------------------------------------

HAND_CASES = ["single_target", "keep_id_in_another_target", "drop_id_two_keep_ids", "drop_id_two_keep_ids_tie",
              "two_drop_ids_one_keep_id", "a_before_b", "same_pair_two_targets", "id_twice_in_one_entry", "empty_and_behind"]


def hand_case(name):
    """small planted scenes under fuse_ref.IDENTITY (u = X, v = Y at Z = 1), one per rule
    -> dict(keep, drops, Rs, ts, radius, kw, expect = [(target, keep_pos, drop_pos, dist)])"""
    rng = np.random.default_rng(12)
    D = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    eye, zero = np.eye(3), np.zeros(3)

    def flip(row, bits):
        r = np.unpackbits(row)
        r[:bits] ^= 1
        return np.packbits(r)

    kw = dict(cam=gm.IDENTITY_CAM, width=640, height=480, max_distance=50, ratio=0.7, max_world_distance=np.inf)
    poses = None
    A, B, C_, E = (100, 100, 1), (300, 100, 1), (100, 300, 1), (300, 300, 1)
    if name == "single_target":                 # (a) fuse_ref's "equal_distance" scene: one target, no cross ids
        c = fr.hand_case("equal_distance")
        kw = {k: v for k, v in c["kw"].items() if k not in ("R", "t")}
        keep, drops = c["keep"], [c["drop"]]
        expect = [(0, j, i, d) for j, i, d in c["expect"]]
    elif name == "keep_id_in_another_target":   # (b) keep id 1 occurs in target 1: keep 0 pairs in no target, not even with its twin in target 0
        keep = ([D[0], D[1]], [A, B], [1, 2])
        drops = [([D[0], D[1]], [A, B], [11, 12]), ([D[5]], [(500, 400, 1)], [1])]
        expect = [(0, 1, 1, 0)]
    elif name == "drop_id_two_keep_ids":        # (c) drop id 11 pairs with keep id 1 in target 0 (4) and keep id 2 in target 1 (3)
        keep = ([D[0], D[1]], [A, B], [1, 2])
        drops = [([flip(D[0], 4)], [A], [11]), ([flip(D[1], 3)], [B], [11])]
        expect = [(1, 1, 0, 3)]                 # the losing keep landmark gets no row
    elif name == "drop_id_two_keep_ids_tie":    # ... at equal distances the lower target wins
        keep = ([D[0], D[1]], [A, B], [1, 2])
        drops = [([flip(D[0], 4)], [A], [11]), ([flip(D[1], 4)], [B], [11])]
        expect = [(0, 0, 0, 4)]
    elif name == "two_drop_ids_one_keep_id":    # (d) drop ids 11 (target 0, 5) and 12 (target 1, 2) claim keep id 1
        keep = ([D[0]], [A], [1])
        drops = [([flip(D[0], 5)], [A], [11]), ([flip(D[0], 2)], [(101, 100, 1)], [12])]
        expect = [(1, 0, 0, 2)]
    elif name == "a_before_b":                  # keep id 1's better row (5) loses drop id 11 in step A, so its row with 12 (7) stays
        keep = ([D[0], D[1]], [A, B], [1, 2])
        drops = [([flip(D[0], 5)], [A], [11]), ([flip(D[1], 1), flip(D[0], 7)], [B, (100, 101, 1)], [11, 12])]
        expect = [(1, 0, 1, 7), (1, 1, 0, 1)]
    elif name == "same_pair_two_targets":       # (e) one row, the lower target
        keep = ([D[0]], [A], [1])
        drops = [([flip(D[0], 3)], [A], [11]), ([flip(D[0], 3)], [A], [11])]
        expect = [(0, 0, 0, 3)]
    elif name == "id_twice_in_one_entry":       # (f) drop id 11 at two positions (step A), keep id 3 at two positions (step B)
        keep = ([D[0], D[1], D[2], D[3]], [A, B, C_, E], [1, 2, 3, 3])
        drops = [([D[0], flip(D[1], 2), flip(D[2], 2), flip(D[3], 1)], [A, B, C_, E], [11, 11, 12, 13])]
        expect = [(0, 0, 0, 0), (0, 3, 3, 1)]
    elif name == "empty_and_behind":            # (g) an empty target and one whose pose puts everything behind the camera
        keep = ([D[0], D[1]], [A, B], [1, 2])
        drops = [(D[:0], np.zeros((0, 3)), []), ([D[0]], [A], [11]), ([D[0]], [A], [12]), ([D[1]], [B], [13])]
        poses = [(eye, zero), (eye, np.array([0.0, 0.0, -5.0])), (eye, zero), (eye, zero)]
        expect = [(2, 0, 0, 0), (3, 1, 0, 0)]
    else:
        raise KeyError(name)
    if poses is None:
        poses = [(eye, zero)] * len(drops)
    return dict(keep=fr.entry(*keep), drops=[fr.entry(*d) for d in drops], Rs=np.stack([p[0] for p in poses]),
                ts=np.stack([p[1] for p in poses]), radius=4.0, kw=kw, expect=expect)


# ---- a planted two-pose scene --------------------------------------------------------------------------------------------------

def _world(px, z, R, t, cam=CAM):
    """the world points that project to pixels px at depths z under the world -> camera pose (R, t)"""
    fx, fy, cx, cy = cam
    c = np.stack([(px[:, 0] - cx) / fx * z, (px[:, 1] - cy) / fy * z, z], 1)
    return (c - t) @ R                                           # rows of R^T (c - t)


def two_pose_scene(seed=1, n=30, width=640, height=480):
    """Two cameras half a radian of yaw apart.  Keep: n landmarks seen by camera 0, then n seen by camera 1 (uniform over
    each frame, 1 .. 3 m deep).  Target 0 holds duplicates of the first n, target 1 of the second n: up to 1 mm away, a few
    flipped bits, ids of their own.  Many of target 1's lie outside camera 0's frame.
    -> dict(keep, drops, Rs, ts, radius, kw)"""
    rng = np.random.default_rng(seed)
    Rs = np.stack([np.eye(3), rr.po.rodrigues([0.0, 0.5, 0.0])])
    ts = np.stack([np.zeros(3), np.array([0.1, 0.0, 0.05])])
    world, desc = [], rng.integers(0, 256, (2 * n, 32), dtype=np.uint8)
    for m in range(2):
        px = np.stack([rng.uniform(10, width - 10, n), rng.uniform(10, height - 10, n)], 1)
        world.append(_world(px, rng.uniform(1.0, 3.0, n), Rs[m], ts[m]))
    world = np.concatenate(world)
    drops = []
    for m in range(2):
        src = np.arange(m * n, (m + 1) * n)
        dd = np.stack([fr.near(rng, desc[k], int(rng.integers(1, 8)))[0] for k in src])
        drops.append(fr.entry(dd, world[src] + rng.uniform(-0.001, 0.001, (n, 3)), 5000 + 1000 * m + np.arange(n)))
    return dict(keep=fr.entry(desc, world, 100 + np.arange(2 * n)), drops=drops, Rs=Rs, ts=ts, radius=4.0,
                kw=dict(cam=CAM, width=width, height=height, max_distance=50, ratio=0.7, max_world_distance=0.05))


# ---- posed random cases with planted cross-target conflicts ------------------------------------------------------------------

TARGET_SIZES = (0, 1, 9, 257)
RANDOM_CASES = [(1, 1024), (2, 1025), (3, 1), (3, 1024), (64, 1025)]     # (n_drop, keep landmarks): either side of the
                                                                         # 1024-landmark chunk of the compaction; one keep
                                                                         # landmark needs three targets for both conflicts


def random_case(n_drop, nk, seed=None, width=640, height=480):
    """nk keep landmarks, each uniform over the frame of one of n_drop cameras (poses a few degrees and centimetres apart)
    and 0.5 .. 4 m deep; target m holds sizes[m] landmarks (257, 9, 1 for the first three, the rest drawn from
    TARGET_SIZES), most of them duplicates of a keep landmark (up to 0.5 mm away, 1 .. 15 flipped bits), ids of their own; a
    few ids are shared between the sides.  Planted on top, on landmarks moved to places of their own:
      step A  one drop id paired with two keep ids (in targets 0 and 1; at two positions of target 0 when n_drop == 1);
      step B  two drop ids claiming one keep id (from targets 0 and 1; with n_drop == 1 the keep id sits at two keep positions).
    With one keep landmark the three rows are those of targets 0, 1 (one drop id) and 2 (another).
    -> dict(keep, drops, Rs, ts, radius, kw)"""
    rng = np.random.default_rng(1000 * n_drop + nk if seed is None else seed)
    sizes = [257, 9, 1][:n_drop] + [int(s) for s in rng.choice(TARGET_SIZES, max(n_drop - 3, 0))]
    Rs = np.stack([rr.po.rodrigues(rng.uniform(-0.04, 0.04, 3)) for _ in range(n_drop)])
    ts = rng.uniform(-0.05, 0.05, (n_drop, 3))
    cam_of = rng.integers(0, n_drop, nk)
    px = np.stack([rng.uniform(40, width - 40, nk), rng.uniform(40, height - 40, nk)], 1)
    z = rng.uniform(0.5, 4.0, nk)
    kw_ = np.concatenate([_world(px[j:j + 1], z[j:j + 1], Rs[cam_of[j]], ts[cam_of[j]]) for j in range(nk)])
    kd = rng.integers(0, 256, (nk, 32), dtype=np.uint8)
    kl = 1000 + np.arange(nk, dtype=np.int64)
    drops, next_lid = [], 500000
    for m, n in enumerate(sizes):
        dd = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        dw = np.stack([rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.uniform(0.5, 4, n)], 1)
        dup = np.flatnonzero(rng.uniform(size=n) < 0.8)
        src = rng.integers(0, nk, len(dup))
        dw[dup] = kw_[src] + rng.uniform(-0.0005, 0.0005, (len(dup), 3))
        for i, k in zip(dup, src):
            dd[i] = fr.near(rng, kd[k], int(rng.integers(1, 16)))[0]
        dl = next_lid + np.arange(n, dtype=np.int64)
        next_lid += n
        if nk > 16 and n > 16:                                   # shared ids, away from the planted positions
            dl[8:11] = kl[8:11]
        drops.append([dd, dw, dl])

    def place(j, bits_and_targets):
        """keep j to a place of its own; per (target, position, bits, lid) a duplicate of it"""
        kw_[j] = _world(np.array([[rng.uniform(40, width - 40), rng.uniform(40, height - 40)]]), np.array([rng.uniform(4.5, 5.0)]), Rs[0], ts[0])[0]
        kd[j] = rng.integers(0, 256, 32, dtype=np.uint8)
        for m, i, bits, lid in bits_and_targets:
            drops[m][0][i] = fr.near(rng, kd[j], bits)[0]
            drops[m][1][i] = kw_[j] + rng.uniform(-0.0005, 0.0005, 3)
            drops[m][2][i] = lid

    L, M1, M2 = 900001, 900002, 900003
    if nk == 1:
        assert n_drop >= 3
        place(0, [(0, 0, 4, L), (1, 0, 2, L), (2, 0, 6, M1)])    # A drops target 0's row, B drops target 2's
    elif n_drop == 1:
        place(nk - 1, [(0, 0, 2, L)])
        place(nk - 2, [(0, 1, 5, L)])                            # A drops this one
        place(nk - 3, [(0, 2, 3, M1)])
        place(nk - 4, [(0, 3, 6, M2)])                           # B drops this one:
        kl[nk - 4] = kl[nk - 3]                                  # one keep id at two positions
    else:
        place(nk - 1, [(0, 0, 2, L)])
        place(nk - 2, [(1, 0, 5, L)])                            # A drops this one
        place(nk - 3, [(0, 1, 3, M1), (1, 1, 6, M2)])            # B drops the second
    return dict(keep=fr.entry(kd, kw_, kl), drops=[fr.entry(*d) for d in drops], Rs=Rs, ts=ts, radius=4.0,
                kw=dict(cam=CAM, width=width, height=height, max_distance=50, ratio=0.7, max_world_distance=0.05))


# ---- the scene file of `mslam_harness <plugin> --fuse-multi <scene>` ---------------------------------------------------------

def write_scene(path, keep, drops, Rs, ts, radius, cam=CAM, width=640, height=480, max_distance=50, ratio=0.7,
                max_world_distance=np.inf, others=()):
    """little-endian: magic "MSFM", i32 version 1, i32 width, height, max_distance, number of targets, f64 fx fy cx cy radius
    ratio max_world_distance, per target R (9 f64) and t (3 f64), i32 number of entries; then per entry (keep, the targets in
    order, then `others`, which the replacement must reach as well): i32 n, descriptors n x 32, world points n x 3 f64,
    landmark ids n x i64"""
    Rs = np.asarray(Rs, "<f8").reshape(-1, 9)
    ts = np.asarray(ts, "<f8").reshape(-1, 3)
    with open(path, "wb") as f:
        f.write(b"MSFM" + struct.pack("<5i", 1, width, height, max_distance, len(drops)))
        f.write(struct.pack("<7d", cam[0], cam[1], cam[2], cam[3], radius, ratio, max_world_distance))
        for R, t in zip(Rs, ts):
            f.write(R.tobytes() + t.tobytes())
        entries = [keep] + list(drops) + list(others)
        f.write(struct.pack("<i", len(entries)))
        for e in entries:
            d, w, l = fr.entry(*e)
            f.write(struct.pack("<i", len(d)) + d.tobytes() + w.astype("<f8").tobytes() + l.astype("<i8").tobytes())
