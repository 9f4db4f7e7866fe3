"""The stores of tests/test_gpu_distinct_union.py (not a test).  tests/test_distinct_union.py proves on the CPU, from the
references alone, that each case is what it is named after; the GPU tests then compare the library with
tests/distinct_ref.py on exactly these cases.

A store is local_map_ref's pair of dicts: {id: (desc [n, 32] u8, world [n, 3] f64)} and {id: landmark ids [n] i64}.
Every case has at most 64 entries of at most 320 landmarks and fits a context of K = 512 unless it is made not to."""
import numpy as np

import lm_table_ref as lt

K = 512
ZERO, ONES = np.zeros(32, np.uint8), np.full(32, 0xFF, np.uint8)


def flipped(rng, base, n_flips):
    """`base` with n_flips distinct bits inverted"""
    bits = np.unpackbits(np.asarray(base, np.uint8))
    at = rng.permutation(256)[:n_flips]
    bits[at] ^= 1
    return np.packbits(bits)


def _points(rng, n):
    return rng.normal(size=(n, 3)) * 3.0


def observed(rng, held, max_flips=40, shuffle=True):
    """held: {entry id: landmark ids}.  Every landmark id gets a base descriptor, every observation of it the base with
    0 .. max_flips bits inverted; positions inside an entry are shuffled -> (store, lids)"""
    every = np.unique(np.concatenate([np.asarray(v, np.int64).reshape(-1) for v in held.values()] + [np.zeros(0, np.int64)]))
    base = {int(l): rng.integers(0, 256, 32, dtype=np.uint8) for l in every}
    store, lids = {}, {}
    for i, l in held.items():
        l = np.asarray(l, np.int64).reshape(-1)
        if shuffle:
            l = rng.permutation(l)
        desc = np.array([flipped(rng, base[int(x)], int(rng.integers(0, max_flips + 1))) for x in l], np.uint8).reshape(-1, 32)
        store[i], lids[i] = (desc, _points(rng, len(l))), l
    return store, lids


# ---- the N ladder ------------------------------------------------------------------------------------------------------------

def ladder(copies=3):
    """64 entries (ids 200, 205, ...); landmark j = 1 .. 64 of each copy is held by the j entries with the smallest ids, so
    every N from 1 to 64 occurs `copies` times and the entry of the smallest id holds 64 * copies landmarks
    -> (store, lids, a shuffled list order)"""
    rng = np.random.default_rng(100)
    ids = [200 + 5 * r for r in range(64)]
    held = {i: np.array([1000 * c + j for c in range(copies) for j in range(r + 1, 65)], np.int64) for r, i in enumerate(ids)}
    store, lids = observed(rng, held)
    return store, lids, [int(i) for i in rng.permutation(ids)]


# ---- ties and extremes ------------------------------------------------------------------------------------------------------

SAME, AABB, AAABB, EXTREME = 1, 2, 3, 4     # the landmark ids of ties()


def ties():
    """entries 10 < 20 < 30 < 40 < 50, listed out of order, that hold (among 20 ordinary landmarks)
        SAME     in all five, one descriptor;
        AABB     in 20 .. 50: A, A, B, B — every median is 0, the most recent (a B) is chosen;
        AAABB    in all five: A, A, A, B, B — an A has median 0, a B has d(A, B): the most recent A (entry 30);
        EXTREME  in 30, 40, 50: all-ones, all-ones, all-zeros — all-zeros has median 256, all-ones has 0: entry 40.  A
                 median kept in eight bits would make 256 a 0 and the most recent observation (all-zeros) the choice
    -> (store, lids, list order, {landmark id: the entry whose observation is chosen})"""
    rng = np.random.default_rng(110)
    ids = [10, 20, 30, 40, 50]
    held = {i: np.concatenate([100 + rng.permutation(30)[:20], [SAME, AAABB]]) for i in ids}
    for i in ids[1:]:
        held[i] = np.concatenate([held[i], [AABB]])
    for i in ids[2:]:
        held[i] = np.concatenate([held[i], [EXTREME]])
    store, lids = observed(rng, held)
    A, B = rng.integers(0, 256, 32, dtype=np.uint8), rng.integers(0, 256, 32, dtype=np.uint8)

    def put(i, l, d):
        store[i][0][np.flatnonzero(lids[i] == l)[0]] = d
    for i in ids:
        put(i, SAME, A)
    for i, d in zip(ids[1:], (A, A, B, B)):
        put(i, AABB, d)
    for i, d in zip(ids, (A, A, A, B, B)):
        put(i, AAABB, d)
    for i, d in zip(ids[2:], (ONES, ONES, ZERO)):
        put(i, EXTREME, d)
    return store, lids, [30, 50, 10, 40, 20], {SAME: 50, AABB: 50, AAABB: 30, EXTREME: 40}


# ---- repeats inside an entry ---------------------------------------------------------------------------------------------------

REPEATED = 7


def repeats():
    """entries 1, 2, 3 of 40 landmarks and entry 4 of 320.  Landmark REPEATED sits in entry 4 at positions 3, 200 and 300:
    the lower two carry the ideal descriptor I itself, position 300 carries I with 100 bits inverted; entries 1 .. 3 carry I
    with 10 bits inverted each.  Only position 300 is entry 4's observation, and it loses; an implementation that counted
    position 3 or 200 would choose I -> (store, lids, list order, I)"""
    rng = np.random.default_rng(120)
    small = {i: np.concatenate([[REPEATED], 500 + rng.permutation(60)[:39]]) for i in (1, 2, 3)}
    store, lids = observed(rng, small)
    big = np.concatenate([500 + np.arange(60), 2000 + np.arange(260)])
    big[[3, 200, 300]] = REPEATED
    s4, l4 = observed(rng, {4: big}, shuffle=False)
    store[4], lids[4] = s4[4], l4[4]
    ideal = rng.integers(0, 256, 32, dtype=np.uint8)
    for i in (1, 2, 3):
        store[i][0][np.flatnonzero(lids[i] == REPEATED)[0]] = flipped(rng, ideal, 10)
    store[4][0][3] = store[4][0][200] = ideal
    store[4][0][300] = flipped(rng, ideal, 100)
    return store, lids, [2, 4, 1, 3], ideal


# ---- sizes ------------------------------------------------------------------------------------------------------------------

SIZES = (0, 1, 256, 257, 300)


def sizes():
    """entries 10 .. 14 of 0, 1, 256, 257 and 300 landmarks drawn from one pool of 400, so the three large ones overlap
    heavily and every union fits K -> (store, lids, the list orders: the empty entry in the middle, first and last)"""
    rng = np.random.default_rng(130)
    held = {10 + k: 3000 + rng.permutation(400)[:n] for k, n in enumerate(SIZES)}
    store, lids = observed(rng, held)
    return store, lids, [[12, 14, 10, 13, 11], [10, 11, 12, 13, 14], [14, 13, 12, 11, 10], [13, 12, 14]]


# ---- probe chains -------------------------------------------------------------------------------------------------------------

def chains():
    """five entries of 120 landmarks drawn from 160 ids whose hashes all end in 0xFFFF: in a table of any size up to 65536
    buckets they share the last bucket as their home, so every lookup of the new kernels walks one chain that wraps
    -> (store, lids, list order)"""
    rng = np.random.default_rng(140)
    pool = lt.colliding(160, seed=141)
    held = {i: pool[rng.permutation(160)[:120]] for i in (3, 4, 5, 6, 7)}
    store, lids = observed(rng, held)
    return store, lids, [5, 3, 7, 4, 6]


# ---- capacity -----------------------------------------------------------------------------------------------------------------

def capacity():
    """entries 1 .. 4 of 200 landmarks: 1, 2 and 3 draw on a pool of 250, entry 2 holds 100 of its own as well and entry 4
    only ids of its own: 1 + 2 + 3 hold 350 distinct ids (fits K = 512), all four 550
    -> (store, lids, a list that does not fit, its distinct count, a list that fits)"""
    rng = np.random.default_rng(150)
    held = {1: np.arange(200), 2: np.concatenate([np.arange(150, 250), 6000 + np.arange(100)]), 3: 50 + np.arange(200),
            4: 5000 + np.arange(200)}
    store, lids = observed(rng, held)
    too_many = [1, 2, 4, 3]
    needed = len(np.unique(np.concatenate([lids[i] for i in too_many])))
    return store, lids, too_many, needed, [3, 1, 2]
