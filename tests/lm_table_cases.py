"""The cases of tests/test_gpu_lm_table_edges.py (not a test): stores whose landmark ids are made with tests/lm_table_ref.py
to sit on one probe chain of the id table, and unions of enough blocks for a second and third pass of the block scan.
tests/test_lm_table_edges.py proves on the CPU, from the references alone, that every case reaches the path it is named
after; the GPU tests then compare the library with the references on exactly these cases.

A store is local_map_ref's pair of dicts: {id: (desc [n, 32] u8, world [n, 3] f64)} and {id: landmark ids [n] i64}."""
import numpy as np

import fuse_ref as fr
import lm_table_ref as lt

K = 320
TOP = (1 << 63) - 1


def entry(rng, lids):
    lids = np.asarray(lids, np.int64).reshape(-1)
    return (rng.integers(0, 256, (len(lids), 32), dtype=np.uint8), rng.normal(size=(len(lids), 3)) * 3.0), lids


def build(rng, lids):
    store = {}
    for i in lids:
        store[i], lids[i] = entry(rng, lids[i])
    return store, lids


def table_of(keys, count=None):
    """the table a call makes for `count` keys (default: as many as listed) -> (buckets, bucket, probe length)"""
    buckets = lt.lm_bucket_count(len(keys) if count is None else count)
    return (buckets,) + lt.occupied(keys, buckets)


# ---- one chain -------------------------------------------------------------------------------------------------------------

SHARES = (0, 80, 160)


def chain_pair(share, displaced=False):
    """entries 1 and 2 of 160 landmarks with `share` ids in common; all 320 - share ids have the last bucket as their home.
    displaced: every other id is one whose home is bucket 0 .. 63 instead, buckets the chain has wrapped over.  The
    positions inside an entry are shuffled."""
    rng = np.random.default_rng(20 + share + displaced)
    pool = lt.colliding(320 - share, seed=30 + share)
    if displaced:
        pool[1::2] = lt.ids_with_hash_low(np.arange(len(pool[1::2])) % 64, seed=40 + share)
    return build(rng, {1: rng.permutation(pool[:160]), 2: rng.permutation(pool[160 - share:])})


def contended():
    """64 entries (ids 100, 103, ..., added in a shuffled order) that each hold the same 5 colliding ids, rotated: in the
    union's insert 64 threads of different list positions walk one chain for every id -> (store, lids, three list orders)"""
    rng = np.random.default_rng(50)
    five = lt.colliding(5, seed=51)
    ids = [100 + 3 * int(k) for k in rng.permutation(64)]
    store, lids = build(rng, {i: np.roll(five, n) for n, i in enumerate(ids)})
    return store, lids, [sorted(ids), sorted(ids)[::-1], ids]


def repeats():
    """two entries on one chain with ids repeated inside them, one of the repeated ids shared"""
    rng = np.random.default_rng(60)
    pool = lt.colliding(55, seed=61)
    a = pool[:40].copy()
    a[39], a[20] = a[0], a[25]
    b = np.concatenate([pool[:15], pool[40:]])
    b[29], b[7] = b[2], b[0]
    return build(rng, {1: a, 2: b})


# ---- lists longer than the store --------------------------------------------------------------------------------------------

def update_world_case():
    """a store of K = 320 whose entries hold 300 listed ids (some twice) and 100 ids the list does not hold, and a list of
    1050 places: the 300, 700 strangers and 50 of the 300 a second time, shuffled.  Two of the 300 are 0 and 2^62 - 1, the ends
    of the range a caller may give; every other id is on one chain
    -> (store, lids, list ids, list points)"""
    rng = np.random.default_rng(70)
    pool = lt.colliding(1100, seed=71)
    ends = np.array([0, (1 << 62) - 1], np.int64)                          # the least and the largest id a caller may give
    held, strangers, unlisted = np.concatenate([pool[:298], ends]), pool[300:1000], pool[1000:]
    store, lids = build(rng, {3: rng.permutation(held), 4: np.concatenate([held[100:], unlisted, held[7:8], held[7:8]]),
                              9: np.concatenate([np.arange(1000, 1020), unlisted[:50], held[:5]])})
    ids = rng.permutation(np.concatenate([held, strangers, held[:50]]))
    return store, lids, ids, rng.normal(size=(len(ids), 3))


def replace_case():
    """a store of K = 320 on one chain and two lists of 600: the first (ids alone) swaps two held ids, sends held ids to 2^62,
    2^63 - 1, 0 and to 200 colliding ids of [2^62, 2^63), lists 50 `from` ids twice, and names 2^63 - 1 and 344 colliding
    strangers the store does not hold; the second (with points) rewrites what the first one wrote: its `from` ids are those
    of the top range, 2^63 - 1 and 0 included -> (store as {id: entry of fuse_ref}, [(from, to, points or None)])"""
    rng = np.random.default_rng(80)
    pool = lt.colliding(320 + 50 + 344 + 250, seed=81)
    h, o, s, back = pool[:320], pool[320:370], pool[370:714], pool[714:]
    top = lt.colliding(200, seed=82, below=1 << 63, at_least=1 << 62)
    (store, lids) = build(rng, {5: rng.permutation(h), 6: np.concatenate([h[:150], o])})
    store = {i: (store[i][0], store[i][1], lids[i]) for i in store}
    f1 = np.concatenate([h[:2], h[2:5], [TOP], h[5:205], h[5:55], s])
    t1 = np.concatenate([h[:2][::-1], [1 << 62, TOP, 0], [12345], rng.permutation(top), top[:50][::-1], np.arange(344)])
    f2 = np.concatenate([top, [TOP, 1 << 62, 0], h[:2], back[:145], s[:250]])
    t2 = np.concatenate([back[:200][::-1], [7, TOP, h[2]], h[:2][::-1], top[:145], np.arange(250) + 5000])
    assert len(f1) == len(t1) == len(f2) == len(t2) == 600
    p1, p2 = rng.permutation(600), rng.permutation(600)        # (of a `from` listed twice the later place wins, wherever)
    return store, [(f1[p1].astype(np.int64), t1[p1].astype(np.int64), None),
                   (f2[p2].astype(np.int64), t2[p2].astype(np.int64), rng.normal(size=(600, 3)))]


def fusion_case():
    """fuse_ref.random_case(31, 300, 280, shared=40) with every landmark id, the shared ones included, replaced by a
    colliding id, and a third entry that holds drop ids and colliding strangers -> (case, store {10: keep, 20: drop, 30:})"""
    case = fr.random_case(31, 300, 280, shared=40)
    rng = np.random.default_rng(90)
    kl, dl = case["keep"][2], case["drop"][2]
    old = np.unique(np.concatenate([kl, dl]))
    new = lt.colliding(len(old) + 60, seed=91)
    kl[:], dl[:] = new[np.searchsorted(old, kl)], new[np.searchsorted(old, dl)]
    third = np.concatenate([dl[::2], new[len(old):], dl[:25]])
    return case, {10: case["keep"], 20: case["drop"],
                  30: (rng.integers(0, 256, (len(third), 32), dtype=np.uint8), rng.normal(size=(len(third), 3)), third)}


# ---- unions of more than 256 blocks ------------------------------------------------------------------------------------------

BLOCKS = {256: (1024, 64, 1000), 258: (1536, 43, 1500), 576: (2304, 64, 2280)}   # nb: (max_keypoints, entries, the large one)
LARGE = 500


def union_blocks(nb):
    """n - 1 entries of 0 .. 40 landmarks (ids 10 ..; the first of them empty) and the large entry LARGE, whose id lies in
    the middle of theirs: the small entries draw from its landmark ids and 20 more, so those above it take their landmarks
    from it and the union fits.  Two list orders: the large entry last, and at the place where its blocks straddle block 256
    (with exactly 256 blocks, where the first order has that already: in the middle)
    -> (max_keypoints, store, lids, orders, blocks per entry)"""
    k_max, n, n_large = BLOCKS[nb]
    rng = np.random.default_rng(nb)
    pool = 10000 + rng.permutation(n_large + 20)
    lids = {LARGE: pool[:n_large].copy()}
    small = [10 + 20 * k for k in range(n - 1)]                            # ids 10 .. on both sides of LARGE
    for k, i in enumerate(small):
        lids[i] = rng.permutation(pool)[:0 if k == 0 else int(rng.integers(1, 41))]
    store, lids = build(rng, lids)
    bx = (n_large + 255) // 256
    assert bx * n == nb and max(small) > LARGE > min(small)
    at = 255 // bx if 255 // bx < n - 1 else n // 2                        # list position whose blocks hold block 255
    return k_max, store, lids, [small + [LARGE], small[:at] + [LARGE] + small[at:]], bx


def winner_blocks(lids, order, bx):
    """local_map_ref.union's rule restated for where the winners sit: the block index (list position x bx + landmark
    position / 256) of every landmark the union takes, ascending"""
    best = {}
    for k, kf in enumerate(order):
        for i, l in enumerate(np.asarray(lids[kf]).tolist()):
            if l not in best or (kf, i) > best[l][:2]:
                best[l] = (kf, i, k)
    return np.array(sorted(k * bx + i // 256 for _, i, k in best.values()), np.int64)


def growth():
    """on the context of 2304: a union of 2 blocks, of 576, the 2 again, then 258 (42 of the small entries and an entry of
    1400 landmarks, id 501) -> (max_keypoints, store, lids, [(list, nb)])"""
    k_max, store, lids, orders, bx = union_blocks(576)
    rng = np.random.default_rng(7)
    store[501], lids[501] = entry(rng, rng.permutation(lids[LARGE])[:1400])
    small = [i for i in orders[0] if i != LARGE]
    two = [small[5], small[40]]
    return k_max, store, lids, [(two, 2), (orders[0], 576), (two, 2), (small[:42] + [501], 258)]
