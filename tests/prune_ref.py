"""Removing observations from the keyframe store and from the backend, restated in numpy: the reference the CPU, GPU and
host tests of mslam_hip_kf_remove_observations, HipBackend.remove_observations and the pruned bundle adjustment compare
with.  It is the body RgbdFeatureFrontend::removeObservation leaves commented out (rgbd_feature_frontend.cpp:469-487),
which update(const BackendOutputType&) calls for every outlier observation (:224-230).

A store is a dict: entry id -> (descriptors [n, 32] u8, world points [n, 3] f64, landmark ids [n] i64)."""
import numpy as np

import ba_ref

T = 256   # the kernel's chunk: positions a workgroup compacts between two barriers (kPruneChunk in csrc/k_prune.hip)


def entry(desc, world, lids):
    return (np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), np.ascontiguousarray(world, np.float64).reshape(-1, 3),
            np.ascontiguousarray(lids, np.int64).reshape(-1))


def remove_observations(store, kf_ids, lids):
    """row p removes landmark lids[p] from entry kf_ids[p], every position that holds it; survivors keep their order and
    move bit for bit; entries no row names are the same objects -> (new store, removed [n] i32 = the positions row p's
    landmark held before the call, n_removed = the positions removed, each counted once)"""
    kf_ids = [int(k) for k in np.asarray(kf_ids).reshape(-1)]
    lids = [int(l) for l in np.asarray(lids).reshape(-1)]
    assert len(kf_ids) == len(lids)
    for k, l in zip(kf_ids, lids):
        if k not in store:
            raise KeyError(k)
        if l < 0:
            raise ValueError(l)
    new, removed, n_removed = dict(store), np.zeros(len(kf_ids), np.int32), 0
    for k in sorted(set(kf_ids)):
        d, w, i = entry(*store[k])
        gone = {l for kk, l in zip(kf_ids, lids) if kk == k}
        hit = np.array([x in gone for x in i.tolist()], bool).reshape(-1)
        new[k] = (d[~hit].copy(), w[~hit].copy(), i[~hit].copy())
        n_removed += int(hit.sum())
    for p, (k, l) in enumerate(zip(kf_ids, lids)):
        removed[p] = int(np.count_nonzero(entry(*store[k])[2] == l))
    return new, removed, n_removed


def backend_remove(obs, landmarks, anchor, pairs):
    """HipBackend.remove_observations on copies: obs = id -> (landmark ids, camera points), landmarks = id -> point,
    anchor = id -> keyframe.  The named observations go (every position); a landmark whose anchor no longer observes it
    moves to the smallest keyframe id that does; a landmark nobody observes leaves both maps.  Pairs the backend does not
    hold are ignored -> (obs, landmarks, anchor, number of observations dropped)"""
    obs = {k: (np.array(v[0], np.int64), np.array(v[1], np.float64)) for k, v in obs.items()}
    landmarks, anchor = dict(landmarks), dict(anchor)
    pairs = {(int(k), int(l)) for k, l in pairs}
    n, touched = 0, set()
    for k in sorted(obs):
        lids, cam = obs[k]
        hit = np.array([(k, l) in pairs for l in lids.tolist()], bool).reshape(-1)
        n += int(hit.sum())
        touched |= set(lids[hit].tolist())
        obs[k] = (lids[~hit], cam[~hit])
    for l in sorted(touched):
        who = sorted(k for k in obs if l in set(obs[k][0].tolist()))
        if not who:
            landmarks.pop(l, None)
            anchor.pop(l, None)
        elif anchor.get(l) not in who:
            anchor[l] = who[0]
    return obs, landmarks, anchor, n


def write_scene(path, store, kf_ids, lids):
    """the scene file `mslam_harness --prune` reads: "MSPR", i32 version 1, i32 entries, i32 rows; per entry i32 id, i32 n,
    n x 32 descriptor bytes, n x 3 f64 world points, n x i64 landmark ids; then rows x i32 entry id, rows x i64 landmark id"""
    kf_ids, lids = np.asarray(kf_ids, "<i4").reshape(-1), np.asarray(lids, "<i8").reshape(-1)
    with open(path, "wb") as f:
        f.write(b"MSPR" + np.array([1, len(store), len(kf_ids)], "<i4").tobytes())
        for k in store:
            d, w, i = entry(*store[k])
            f.write(np.array([k, len(i)], "<i4").tobytes() + d.tobytes() + w.astype("<f8").tobytes() + i.astype("<i8").tobytes())
        f.write(kf_ids.tobytes() + lids.tobytes())


# ---- cases ------------------------------------------------------------------------------------------------------------
def random_entry(rng, n, first_lid):
    """n landmarks with distinct ids first_lid, first_lid + 1, ..."""
    return entry(rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.normal(size=(n, 3)), first_lid + np.arange(n, dtype=np.int64))


PATTERNS = ("nothing", "everything", "first", "last", "every_other", "one_chunk", "straddle")


def pattern_positions(name, n):
    """the positions of an n-landmark entry a removal pattern names (those that exist)"""
    pos = {"nothing": [], "everything": range(n), "first": [0], "last": [n - 1], "every_other": range(0, n, 2),
           "one_chunk": range(T, 2 * T) if n >= 2 * T else range(0, min(T, n)),
           "straddle": range(T - 3, T + 4)}[name]
    return np.array([p for p in pos if 0 <= p < n], np.int64)


def random_case(seed, sizes, fraction=0.3, first_id=100):
    """a store of len(sizes) entries (ids first_id, first_id + 1, ...) that share some landmark ids, and a shuffled row list
    naming `fraction` of every entry's landmarks, some rows twice, some ids the entry does not hold"""
    rng = np.random.default_rng(seed)
    store, kf, lid = {}, [], []
    for e, n in enumerate(sizes):
        d, w, i = random_entry(rng, n, 1000 * (e // 2))          # pairs of entries share their ids
        store[first_id + e] = (d, w, i)
        take = rng.choice(n, size=int(round(fraction * n)), replace=False) if n else np.zeros(0, np.int64)
        kf += [first_id + e] * len(take)
        lid += i[take].tolist()
        kf += [first_id + e] * 2
        lid += [5_000_000 + e, (1 << 62) + e]                    # absent ids, one of them in the fresh range
        if len(take):
            kf.append(first_id + e)
            lid.append(int(i[take[0]]))                          # a duplicate row
    order = rng.permutation(len(kf))
    return store, np.array(kf, np.int32)[order], np.array(lid, np.int64)[order]


def hand_case(name):
    """small stores with one rule each -> (store, kf_ids, lids)"""
    rng = np.random.default_rng(7)
    d = lambda n: rng.integers(0, 256, (n, 32), dtype=np.uint8)
    w = lambda n: rng.normal(size=(n, 3))
    if name == "order":
        return {1: entry(d(6), w(6), [10, 11, 12, 13, 14, 15]), 2: entry(d(3), w(3), [10, 11, 12])}, [1, 1], [13, 10]
    if name == "repeat_inside":          # id 11 twice in entry 1: one landmark, both positions go; and a duplicate row
        return {1: entry(d(5), w(5), [10, 11, 12, 11, 13]), 2: entry(d(2), w(2), [11, 12])}, [1, 1, 1], [11, 12, 11]
    if name == "absent":
        return {1: entry(d(4), w(4), [10, 11, 12, 13])}, [1, 1], [99, 12]
    if name == "emptied":
        return {1: entry(d(2), w(2), [10, 11]), 2: entry(d(2), w(2), [10, 11])}, [1, 1], [11, 10]
    raise KeyError(name)


# ---- the pruned bundle adjustment ---------------------------------------------------------------------------------------
BA_SCENES = ((6, 60, 4, 6, 0.5, 1), (8, 80, 3, 10, 0.3, 2), (5, 40, 5, 4, 1.0, 3))   # (K, L, views, nbad, off, seed)


def planted_scene(K, L, views, nbad, off, seed):
    """ba_ref.make_scene(K, L, seed, noise=0.002, views) with one observation of each of nbad distinct landmarks displaced by
    `off` metres in a random direction (rng = default_rng(100 + seed)) -> (scene, the planted observation indices)"""
    sc = ba_ref.make_scene(K, L, seed, noise=0.002, views=views)
    rng = np.random.default_rng(100 + seed)
    planted = [int(rng.choice(np.flatnonzero(sc["obs_lm"] == l))) for l in rng.choice(L, size=nbad, replace=False)]
    for m, v in zip(planted, rng.normal(size=(nbad, 3))):
        sc["obs_cam"][m] += off * v / np.linalg.norm(v)
    return sc, np.array(planted)


def max_position_error(poses, truth):
    return float(np.max(np.linalg.norm(np.asarray(poses)[:, 4:] - truth[:, 4:], axis=1)))


_PRUNED = {}


def pruned_reference(which, linear_solver="qr"):
    """solve, drop the flagged observations, solve again from the first result, all with ba_ref -> dict(scene, planted,
    first, mask (the first solve's flags), second, mask2 (the second solve's flags on what was kept), keep, r2 (the first
    solve's squared residual norms)); computed once per scene and solver"""
    key = (which, linear_solver)
    if key not in _PRUNED:
        sc, planted = planted_scene(*BA_SCENES[which])
        okf, olm, cam = sc["obs_kf"], sc["obs_lm"], sc["obs_cam"]
        first = ba_ref.solve_scene(sc, linear_solver=linear_solver)
        r = ba_ref.residuals(first["poses"], first["landmarks"], okf, olm, cam)
        r2 = np.sum(r * r, 1)
        mask = r2 > 0.15 * 0.15
        keep = ~mask
        second = ba_ref.bundle_adjust(first["poses"], first["landmarks"], okf[keep], olm[keep], cam[keep], sc["fixed"],
                                      linear_solver=linear_solver)
        mask2 = ba_ref.outliers(second["poses"], second["landmarks"], okf[keep], olm[keep], cam[keep])
        _PRUNED[key] = dict(scene=sc, planted=planted, first=first, mask=mask, second=second, mask2=mask2, keep=keep, r2=r2)
    return _PRUNED[key]


def backend_of(pkg, ctx, sc, **kw):
    """a HipBackend holding the scene: keyframe ids 0 .. K-1 (0 is constant), landmark ids = the scene's indices, the
    scene's start state"""
    b = pkg.HipBackend(ctx, **kw)
    for k in range(len(sc["poses"])):
        sel = sc["obs_kf"] == k
        b.add_keyframe(k, sc["poses"][k], sc["obs_lm"][sel].astype(np.int64), sc["obs_cam"][sel])
    for l in range(len(sc["landmarks"])):
        if l in b.landmarks:
            b.landmarks[l] = sc["landmarks"][l].copy()
    return b
