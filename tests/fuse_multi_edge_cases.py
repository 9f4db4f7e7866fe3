"""Edge cases of landmark fusion into many target entries (not a test): the builders tests/test_fuse_multi_edges.py proves
on the CPU and tests/test_gpu_fuse_multi_edges.py runs against k_fuse_multi.hip.  Every case is a dict(keep, drops, Rs, ts,
radius, kw) as tests/fuse_multi_ref.py's cases are, so that fuse_multi_ref.search_multi / fuse_multi is its expectation.

  lifted         a case of tests/fuse_ref.py (hand cases, SIZES, frames and radii, the real pose) as target m of n_drop
  dealt          one drop entry of fuse_ref dealt out to M targets, with both cross-target conflicts planted in every pass
  posed_targets  fuse_multi_ref.random_case with the targets' sizes and the planted pairs given: wide_64, big_targets
  crowded        three keep landmarks with a thousand candidates each in one target
  key_extremes   hand-built scenes that decide each claim key at a margin of one
  relabelled     a case with every landmark id replaced by ids on one wrapping probe chain
  union_sides    keep and one target built by the store's union, whose capacity exceeds its count
  tight          every keep landmark (or every drop landmark) is a pair"""
import numpy as np

import fuse_multi_ref as fm
import fuse_ref as fr
import guided_match_ref as gm
import lm_table_ref as lt
import reloc_ref as rr

DECOY_LID = 70000000                            # ids no case of fuse_ref or fuse_multi_ref uses
TOP = (1 << 63) - 1
LIFTS = [(0, 1), (1, 3), (63, 64)]              # (m, n_drop)
FRAMES = fr.FRAMES + [(2000, 1100), (1056, 1000)]
BIN_THREADS, MAX_CELLS, CHUNK = 1024, 4096, 1024


def grid_of(width, height):
    """guided_grid of csrc/common.hpp restated -> (shift, nx, ny)"""
    s = 5
    while (((width - 1) >> s) + 1) * (((height - 1) >> s) + 1) > MAX_CELLS:
        s += 1
    return s, ((width - 1) >> s) + 1, ((height - 1) >> s) + 1


def cells_per_thread(width, height):
    """k_fusem_bin's `per` and the number of threads whose cell range is not empty"""
    _, nx, ny = grid_of(width, height)
    per = (nx * ny + BIN_THREADS - 1) // BIN_THREADS
    return per, sum(min(t * per, nx * ny) < min(t * per + per, nx * ny) for t in range(BIN_THREADS))


def search_shape(nk):
    """k_fusem_search's launch restated -> (threads of a workgroup, workgroups per target, keep landmarks of the last one)"""
    block = 256 if nk > 4096 else 64
    per = block // 8
    return block, (nk + per - 1) // per, nk - (nk - 1) // per * per


def _kw(case):
    return {k: v for k, v in case["kw"].items() if k not in ("R", "t")}


def _case(keep, drops, Rs, ts, radius, kw, **more):
    return dict(keep=fr.entry(*keep), drops=[fr.entry(*d) for d in drops], Rs=np.asarray(Rs, np.float64).reshape(-1, 3, 3),
                ts=np.asarray(ts, np.float64).reshape(-1, 3), radius=radius, kw=kw, **more)


def reference(case, stages=None, **over):
    return fm.search_multi(case["keep"], case["drops"], case["Rs"], case["ts"], case["radius"], stages=stages, **dict(case["kw"], **over))


# ---- 1. the single-target library as one target of many ----------------------------------------------------------------------

def lifted(case, m, n_drop):
    """the fuse_ref case (keep, drop, one pose) as target m of n_drop.  The other targets are decoys with ids of their own
    and 0, 1, 9, 0, ... landmarks: every second one (the odd ones) under the case's rotation with t_z = -100, which puts both
    sides behind its camera, the even ones under the case's own pose with random descriptors and world points in the frame"""
    kw = _kw(case)
    R, t = np.asarray(case["kw"]["R"], np.float64), np.asarray(case["kw"]["t"], np.float64)
    rng = np.random.default_rng(1000 * n_drop + m)
    drops, Rs, ts, lid = [], [], [], DECOY_LID
    for o in range(n_drop):
        Rs.append(R)
        if o == m:
            drops.append(case["drop"])
            ts.append(t)
            continue
        k = len(drops) - (o > m)                                 # the decoy's number
        n = (0, 1, 9)[k % 3]
        px = np.stack([rng.uniform(0, kw["width"], n), rng.uniform(0, kw["height"], n)], 1)
        drops.append((rng.integers(0, 256, (n, 32), dtype=np.uint8), fm._world(px, rng.uniform(1.0, 2.0, n), R, t, kw["cam"]),
                      lid + np.arange(n)))
        lid += n
        ts.append(np.array([t[0], t[1], -100.0]) if k % 2 else t)
    return _case(case["keep"], drops, Rs, ts, case["radius"], kw, m=m)


def no_repeats(case):
    """no id occurs twice inside the keep entry or inside the drop entry"""
    return all(len(np.unique(fr.entry(*case[s])[2])) == len(fr.entry(*case[s])[2]) for s in ("keep", "drop"))


# ---- 2. one drop entry dealt out to several targets --------------------------------------------------------------------------

DEALT = [("sized", 2100, 2100, 5), ("sized", 1025, 1100, 3), ("posed", 1025, 1100, 4)]


def dealt_source(kind, nk, nd):
    return fr.sized_case(nk, nd) if kind == "sized" else fr.posed_case(40 + nk, nk, nd, shared=5)


def dealt(case, M):
    """target m holds the drop positions m::M of the fuse_ref case, every target under the case's pose.  Planted on keep
    landmarks moved to places of their own, as fuse_multi_ref.random_case plants: in every 1024-landmark pass of the
    compaction one keep landmark with rows in targets 0 and 1 that carry one drop id (step A drops target 0's, distance 4
    against 2) and a row in target 2 with another drop id (step B drops it, 6 against 2); in the first pass two more drop ids
    carried by rows of two keep landmarks in targets 0 and 1 (step A drops the second, 5 against 2)"""
    kw = _kw(case)
    R, t = np.asarray(case["kw"]["R"], np.float64), np.asarray(case["kw"]["t"], np.float64)
    kd, kw_, kl = (a.copy() for a in fr.entry(*case["keep"]))
    dd, dw, dl = fr.entry(*case["drop"])
    drops = [[dd[m::M].copy(), dw[m::M].copy(), dl[m::M].copy()] for m in range(M)]
    nk = len(kd)
    rng = np.random.default_rng(nk + M)
    flat = kw["cam"] == gm.IDENTITY_CAM                           # fuse_ref's scenes at Z = 1, gate 2: a place of its own is a pixel

    def place(j, plants):
        px = np.array([[rng.uniform(40, kw["width"] - 40), rng.uniform(40, kw["height"] - 40)]])
        kw_[j] = fm._world(px, np.array([1.0 if flat else rng.uniform(4.5, 5.0)]), R, t, kw["cam"])[0]
        kd[j] = rng.integers(0, 256, 32, dtype=np.uint8)
        for m, i, bits, lid in plants:
            drops[m][0][i] = fr.near(rng, kd[j], bits)[0]
            drops[m][1][i] = kw_[j] + rng.uniform(-0.0005, 0.0005, 3)
            drops[m][2][i] = lid

    planted = []
    for c in range((nk + CHUNK - 1) // CHUNK):
        j, i, lid = min(c * CHUNK + 17, nk - 1), 10 + 3 * c, 900001 + 10 * c
        place(j, [(0, i, 4, lid), (1, i, 2, lid), (2, i, 6, lid + 1)])
        planted.append(j)
    for e in range(2):
        place(31 + 2 * e, [(0, 40 + e, 2, 900501 + e)])
        place(32 + 2 * e, [(1, 40 + e, 5, 900501 + e)])
    return _case((kd, kw_, kl), drops, [R] * M, [t] * M, case["radius"], kw, planted=planted)


# ---- 3. shapes only the multi kernels have -----------------------------------------------------------------------------------

def posed_targets(sizes, nk, seed, plants=(), width=640, height=480):
    """fuse_multi_ref.random_case with the targets' sizes given and without its conflicts: nk keep landmarks, each uniform
    over the frame of one of the cameras (poses a few degrees and centimetres apart), 0.5 .. 4 m deep; four fifths of a
    target's landmarks are duplicates of a keep landmark (up to 0.5 mm away, 1 .. 15 flipped bits); ids of their own but for
    three shared ones per larger target.  plants = [(keep position, [(target, position, bits, id)])]: that keep landmark goes
    to a place of its own, 4.5 .. 5 m deep, and each listed target landmark becomes a duplicate of it under that id."""
    rng = np.random.default_rng(seed)
    M = len(sizes)
    Rs = np.stack([rr.po.rodrigues(rng.uniform(-0.04, 0.04, 3)) for _ in range(M)])
    ts = rng.uniform(-0.05, 0.05, (M, 3))
    cam_of = rng.integers(0, M, nk)
    px = np.stack([rng.uniform(40, width - 40, nk), rng.uniform(40, height - 40, nk)], 1)
    z = rng.uniform(0.5, 4.0, nk)
    kw_ = np.concatenate([fm._world(px[j:j + 1], z[j:j + 1], Rs[cam_of[j]], ts[cam_of[j]]) for j in range(nk)] + [np.zeros((0, 3))])
    kd = rng.integers(0, 256, (nk, 32), dtype=np.uint8)
    kl = 1000 + np.arange(nk, dtype=np.int64)
    drops, lid = [], 500000
    for n in sizes:
        dd = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        dw = np.stack([rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.uniform(0.5, 4, n)], 1)
        dup = np.flatnonzero(rng.uniform(size=n) < 0.8)
        src = rng.integers(0, nk, len(dup))
        dw[dup] = kw_[src] + rng.uniform(-0.0005, 0.0005, (len(dup), 3))
        for i, k in zip(dup, src):
            dd[i] = fr.near(rng, kd[k], int(rng.integers(1, 16)))[0]
        dl = lid + np.arange(n, dtype=np.int64)
        lid += n
        if nk > 16 and n > 16:
            dl[8:11] = kl[8:11]
        drops.append([dd, dw, dl])
    for j, dups in plants:
        kw_[j] = fm._world(np.array([[rng.uniform(40, width - 40), rng.uniform(40, height - 40)]]), np.array([rng.uniform(4.5, 5.0)]), Rs[0], ts[0])[0]
        kd[j] = rng.integers(0, 256, 32, dtype=np.uint8)
        for m, i, bits, l in dups:
            drops[m][0][i] = fr.near(rng, kd[j], bits)[0]
            drops[m][1][i] = kw_[j] + rng.uniform(-0.0005, 0.0005, 3)
            drops[m][2][i] = l
    return _case((kd, kw_, kl), drops, Rs, ts, 4.0,
                 dict(cam=fm.CAM, width=width, height=height, max_distance=50, ratio=0.7, max_world_distance=0.05))


def _conflicts(j, lid=900001):
    """random_case's two conflicts on the keep landmarks j, j - 1, j - 2 and positions 0 and 1 of targets 0 and 1"""
    return [(j, [(0, 0, 2, lid)]), (j - 1, [(1, 0, 5, lid)]), (j - 2, [(0, 1, 3, lid + 1), (1, 1, 6, lid + 2)])]


WIDE_NK = 4127
WIDE_PASSES = [100, 1100, 2100, 3100, 4100]     # keep positions, one per pass of the compaction, that pair in target 60


def wide_64():
    """64 targets, 4127 keep landmarks: above 4096 (the 256-thread search), no multiple of 32 or 256.  Targets 60 .. 63 hold
    9, 257, 1 and 9 landmarks; target 60 has a pair in each of the five passes of the compaction, targets 61, 62 and 63 one
    each, two of them at keep positions above 4096; the two conflicts sit on keep landmarks 4115 .. 4117."""
    rng = np.random.default_rng(64)
    sizes = [257, 9, 1] + [int(s) for s in rng.choice(fm.TARGET_SIZES, 57)] + [9, 257, 1, 9]
    plants = [(j, [(60, p, 2 + p, 910000 + p)]) for p, j in enumerate(WIDE_PASSES)]
    plants += [(4120, [(61, 200, 3, 910061)]), (2000, [(62, 0, 4, 910062)]), (WIDE_NK - 1, [(63, 8, 5, 910063)])]
    return posed_targets(sizes, WIDE_NK, 6464, plants + _conflicts(4117))


BIG_SIZES = [1024, 1025, 2100, 0, 1]
BIG_PLANTS = [(20, 2, 1030), (21, 2, 2090), (22, 4, 0), (23, 1, 1024), (24, 0, 1023)]     # (keep position, target, position)


def big_targets():
    """300 keep landmarks; targets of 1024, 1025, 2100, 0 and 1 landmarks: a large slice followed by tiny ones.  Pairs are
    planted at the last position of target 0, at position 1024 of target 1, at 1030 and 2090 of target 2 and on target 4's
    one landmark."""
    plants = [(j, [(m, i, 2, 920000 + j)]) for j, m, i in BIG_PLANTS]
    return posed_targets(BIG_SIZES, 300, 77, plants + _conflicts(299))


CROWD = 1000                                    # candidates per keep landmark


def crowded(d1=8):
    """Under fuse_ref.IDENTITY: three keep landmarks at the centres of three cells, 64 px apart; target 1 of 3 holds 3000
    landmarks, a thousand inside each one's window of radius 16 (so each of the 8 lanes of a landmark walks 125 of them).
      keep 0  16 near-copies at distances 2, 3, 3, 4, 4, ... at random places among the others
      keep 1  two at the least distance 5 (ratio 1.01 accepts the lower drop position, the usual ratio rejects)
      keep 2  d0 = 4 and d1 = `d1`: ratio 0.5 rejects 4 < 0.5 * 8 and accepts 4 < 0.5 * 9
    Target 0 holds 9 strangers; target 2 one further copy of keep 0 at distance 5 under an id of its own: step B drops it."""
    rng = np.random.default_rng(5)
    centres = np.array([(240.0, 240.0), (336.0, 240.0), (432.0, 240.0)])
    kd = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    keep = (kd, np.concatenate([centres, np.ones((3, 1))], 1), [1, 2, 3])
    n = 3 * CROWD
    at = np.repeat(np.arange(3), CROWD)[rng.permutation(n)]
    dw = np.stack([centres[at, 0] + rng.uniform(-15.5, 15.5, n), centres[at, 1] + rng.uniform(-15.5, 15.5, n), np.ones(n)], 1)
    dd = rng.integers(0, 256, (n, 32), dtype=np.uint8)

    def plant(k, bits):
        own = rng.permutation(np.flatnonzero(at == k))[:len(bits)]
        for i, b in zip(np.sort(own), bits):
            dd[i] = _flip(kd[k], b, rng)
        return np.sort(own)

    plant(0, [2] + [3 + e // 2 for e in range(15)])
    plant(1, [5, 5] + [20] * 4)
    plant(2, [4, d1] + [30] * 4)
    px = np.stack([rng.uniform(0, 640, 9), rng.uniform(300, 480, 9)], 1)
    t0 = (rng.integers(0, 256, (9, 32), dtype=np.uint8), np.concatenate([px, np.ones((9, 1))], 1), 600 + np.arange(9))
    t2 = ([_flip(kd[0], 5, rng)], [(241.0, 239.0, 1.0)], [700])
    eye = dict(fr.IDENTITY)
    kw = dict(cam=eye["cam"], width=640, height=480, max_distance=50, ratio=0.7, max_world_distance=np.inf)
    return _case(keep, [t0, (dd, dw, 10000 + np.arange(n)), t2], [np.eye(3)] * 3, [np.zeros(3)] * 3, 16.0, kw)


def _flip(row, bits, rng=None):
    """`row` with `bits` bits flipped: the first ones, or random ones with an rng"""
    r = np.unpackbits(np.asarray(row, np.uint8))
    r[np.arange(bits) if rng is None else rng.choice(256, bits, replace=False)] ^= 1
    return np.packbits(r)


KEY_EXTREMES = ["d256", "d255", "d0", "a_distance", "a_target", "b_distance", "b_target", "positions"]
PAD = 1280                                      # entries padded to max_keypoints of the small context


def key_extremes(name):
    """64 targets under fuse_ref.IDENTITY; the targets in between are empty or hold one stranger.  `hi` pads an entry with
    landmarks behind the camera so that the landmark of interest sits at position 1279.
      d256 / d255   complementary descriptors at keep 1279 and position 1279 of target 63: a lone pair at max_distance 256
                    (the largest claim key: 256 << 22 | 63 << 16 | 1279), none at 255
      d0            max_distance 0 pairs identical descriptors only
      a_distance    drop id 11: distance 3 in target 63 against 4 in target 0;  a_target: 4 against 4, the lower target,
                    whose row has the higher keep position
      b_distance    keep id 1: drop id 12 at distance 3 in target 63 against drop id 11 at 4 in target 0;  b_target: 4 against
                    4, the lower target, whose row has the higher drop position
      positions     equal distance and target, keep and drop positions crossed: drop id 11 twice in target 0 (step A: the lower
                    keep position, which holds the higher drop position), keep id 3 at keep positions 2 and 3 (step B: the
                    lower drop position, which the higher keep position holds)
    -> the case with expect = [(target, keep_pos, drop_pos, dist)]"""
    rng = np.random.default_rng(13)
    D = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    A, B, C_, E = (100, 100, 1), (300, 100, 1), (100, 300, 1), (300, 300, 1)
    kw = dict(cam=gm.IDENTITY_CAM, width=640, height=480, max_distance=50, ratio=0.7, max_world_distance=np.inf)

    def hi(desc, world, lids, first):
        n = PAD - len(lids)
        return (np.concatenate([rng.integers(0, 256, (n, 32), dtype=np.uint8), np.asarray(desc, np.uint8).reshape(-1, 32)]),
                np.concatenate([np.tile((50.0, 50.0, -1.0), (n, 1)), np.asarray(world, np.float64).reshape(-1, 3)]),
                np.concatenate([first + np.arange(n), lids]))

    first, last = None, None
    if name in ("d256", "d255"):
        keep, last = hi([D[0]], [A], [1], 2000), hi([~D[0]], [A], [11], 4000)
        kw["max_distance"] = int(name[1:])
        expect = [(63, PAD - 1, PAD - 1, 256)] if name == "d256" else []
    elif name == "d0":
        keep = ([D[0], D[1]], [A, B], [1, 2])
        last = ([D[0], _flip(D[1], 1)], [A, B], [11, 12])
        kw["max_distance"] = 0
        expect = [(63, 0, 0, 0)]
    elif name in ("a_distance", "a_target"):
        keep = ([D[0], D[1]], [A, B], [1, 2])
        first = ([_flip(D[1], 4)], [B], [11])                      # the lower target holds the HIGHER keep position
        last = hi([_flip(D[0], 3 if name == "a_distance" else 4)], [A], [11], 4000)
        expect = [(63, 0, PAD - 1, 3)] if name == "a_distance" else [(0, 1, 0, 4)]
    elif name in ("b_distance", "b_target"):
        keep = hi([D[0]], [A], [1], 2000)
        first = hi([_flip(D[0], 4)], [A], [11], 4000)              # ... and the higher drop position
        last = ([_flip(D[0], 3 if name == "b_distance" else 4)], [(101, 100, 1)], [12])
        expect = [(63, PAD - 1, 0, 3)] if name == "b_distance" else [(0, PAD - 1, PAD - 1, 4)]
    elif name == "positions":
        keep = ([D[0], D[1], D[2], D[3]], [A, B, C_, E], [1, 2, 3, 3])
        first = ([_flip(D[1], 4), _flip(D[0], 4), _flip(D[3], 2), _flip(D[2], 2)], [B, A, E, C_], [11, 11, 12, 13])
        expect = [(0, 0, 1, 4), (0, 3, 2, 2)]
    else:
        raise KeyError(name)
    drops, lid = [], DECOY_LID
    for m in range(64):
        if m == 0 and first is not None:
            drops.append(first)
        elif m == 63 and last is not None:
            drops.append(last)
        elif m % 2:
            drops.append((rng.integers(0, 256, (1, 32), dtype=np.uint8), [(rng.uniform(0, 640), rng.uniform(350, 480), 1.0)], [lid + m]))
        else:
            drops.append((D[:0], np.zeros((0, 3)), []))
    return _case(keep, drops, [np.eye(3)] * 64, [np.zeros(3)] * 64, 4.0, kw, expect=expect)


PLACEHOLDER = 123456789                         # stands in the store for the id 2^63 - 1, which only a replacement can give


def relabelled(case, seed):
    """the case with every landmark id replaced through a bijection onto ids of one probe chain: half of them have the last
    bucket of every table as their home, half a bucket 0 .. 63, which the chain has wrapped over (lm_table_cases.chain_pair's
    `displaced`); two of the ids are 0 and 2^63 - 1"""
    keep, drops = case["keep"], case["drops"]
    old = np.unique(np.concatenate([keep[2]] + [d[2] for d in drops]))
    pool = lt.colliding(len(old), seed=seed)
    pool[1::2] = lt.ids_with_hash_low(np.arange(len(pool[1::2])) % 64, seed=seed + 1)
    pool[2], pool[3] = 0, TOP
    assert len(np.unique(pool)) == len(pool) and PLACEHOLDER not in pool.tolist()
    new = pool[np.random.default_rng(seed).permutation(len(pool))]
    swap = lambda l: new[np.searchsorted(old, l)]
    return dict(case, keep=(keep[0], keep[1], swap(keep[2])), drops=[(d[0], d[1], swap(d[2])) for d in drops])


def longest_probes(case):
    """the longest probe (steps from home) in the keep table and in the drop table of a call on the case, whose entries
    were added from the host, so that the tables are sized by the entries' counts"""
    kl = case["keep"][2]
    dl = np.concatenate([d[2] for d in case["drops"]])
    return (int(lt.occupied(kl, lt.lm_bucket_count(len(kl)))[1].max()), int(lt.occupied(dl, lt.lm_bucket_count(len(dl)))[1].max()))


UNION_KEEP, UNION_TARGET = 1, 10                # store ids of the two unions; their sources are 101.., 201..


def union_sides(big=False):
    """-> dict(store, keep_sources, target_sources, drop_ids, Rs, ts, radius, kw): the keep entry is the union of three
    overlapping slices of a posed_targets keep entry (listed out of order), target 0 the union of three overlapping slices of
    its first target; targets 1 and 2 are ordinary entries behind it in the list, so their place in the drop arrays depends
    on the union's capacity, the sum of its sources.  big: the keep sources sum to 1500 > 1280 landmarks, 600 distinct."""
    nk, cut = (600, [(0, 500), (50, 550), (100, 600)]) if big else (300, [(0, 150), (100, 250), (200, 300)])
    c = posed_targets([200, 257, 9], nk, 31 + big, _conflicts(nk - 1))
    store = {}
    for k, (a, b) in enumerate(cut):
        store[101 + k] = tuple(x[a:b] for x in c["keep"])
    for k, (a, b) in enumerate([(0, 100), (60, 160), (120, 200)]):
        store[201 + k] = tuple(x[a:b] for x in c["drops"][0])
    store[11], store[12] = c["drops"][1], c["drops"][2]
    return dict(store=store, keep_sources=[102, 103, 101], target_sources=[201, 203, 202], drop_ids=[UNION_TARGET, 11, 12],
                Rs=c["Rs"], ts=c["ts"], radius=c["radius"], kw=c["kw"])


def union_reference(u):
    """the store with the two unions in it, as local_map_ref.union builds them, and the case search_multi takes"""
    import local_map_ref as lm
    s = u["store"]
    two, lids = {k: e[:2] for k, e in s.items()}, {k: e[2] for k, e in s.items()}
    store = dict(s)
    store[UNION_KEEP] = lm.union(two, lids, u["keep_sources"])
    store[UNION_TARGET] = lm.union(two, lids, u["target_sources"])
    case = _case(store[UNION_KEEP], [store[k] for k in u["drop_ids"]], u["Rs"], u["ts"], u["radius"], u["kw"])
    return store, case


def union_stale(u, case, K=1280):
    """What the two union ids hold BEFORE the unions are built, K landmarks each under ids of their own, so that the slots'
    places from the unions' counts up to their capacities hold landmarks that would pair if a kernel took them in: under the
    target union's id exact copies of the keep union's landmarks, under the keep union's id exact copies of target 1's.
    -> ({id: entry}, the case a call would see if counts were capacities)"""
    def copies(e, first):
        at = np.arange(K) % len(e[0])
        return (e[0][at], e[1][at], first + np.arange(K, dtype=np.int64))

    stale = {UNION_KEEP: copies(case["drops"][1], 81000000), UNION_TARGET: copies(case["keep"], 80000000)}
    caps = [min(sum(len(u["store"][s][2]) for s in src), K) for src in (u["keep_sources"], u["target_sources"])]

    def padded(e, old, cap):
        return tuple(np.concatenate([x, o[len(x):cap]]) for x, o in zip(e, old))

    seen = dict(case, keep=padded(case["keep"], stale[UNION_KEEP], caps[0]),
                drops=[padded(case["drops"][0], stale[UNION_TARGET], caps[1])] + case["drops"][1:])
    return stale, seen


TIGHT = [(1280, [640, 0, 639, 1]), (300, [100, 99, 1])]


def tight(nk, sizes):
    """nk keep landmarks on a 40-column grid of 16 x 15 px, far more than a radius apart; the targets' landmarks, in list
    order, are duplicates of distinct keep landmarks, each seen at its grid point by its target's camera: every keep landmark
    pairs (or, with fewer target landmarks, every one of those), so the number of pairs is min(nk, all targets' landmarks)"""
    rng = np.random.default_rng(nk)
    M, nd = len(sizes), sum(sizes)
    assert nk <= 1280
    Rs = np.stack([rr.po.rodrigues(rng.uniform(-0.04, 0.04, 3)) for _ in range(M)])
    ts = rng.uniform(-0.05, 0.05, (M, 3))
    order = rng.permutation(nk)
    cam_of = np.zeros(nk, np.int64)
    cam_of[order[:nd]] = np.repeat(np.arange(M), sizes)[:nk]
    j = np.arange(nk)
    px = np.stack([8.0 + 16 * (j % 40), 8.0 + 15 * (j // 40)], 1)
    z = rng.uniform(0.5, 4.0, nk)
    kw_ = np.concatenate([fm._world(px[k:k + 1], z[k:k + 1], Rs[cam_of[k]], ts[cam_of[k]]) for k in range(nk)])
    kd = rng.integers(0, 256, (nk, 32), dtype=np.uint8)
    drops, at = [], 0
    for n in sizes:
        src = order[at:at + n][:max(nk - at, 0)]
        dd = np.stack([fr.near(rng, kd[k], int(rng.integers(1, 16)))[0] for k in src] + [np.zeros(32, np.uint8)])[:len(src)]
        drops.append((dd, kw_[src] + rng.uniform(-0.0005, 0.0005, (len(src), 3)), 500000 + at + np.arange(len(src))))
        at += n
    return _case((kd, kw_, 1000 + j), drops, Rs, ts, 4.0,
                 dict(cam=fm.CAM, width=640, height=480, max_distance=50, ratio=0.7, max_world_distance=0.05))
