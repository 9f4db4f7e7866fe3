"""Independent numpy reference of the brute-force 256-bit Hamming knn-2 matcher + ratio test, and generators of planted
edge cases for it (test infrastructure like mse_pnp_ref.py: not a conftest.py, not under oracle/).

The documented behaviour (reference orb_feature.cpp:84-117, as restated in modular-slam_amd/csrc/k_match.hip's header):
BFMatcher(NORM_HAMMING).knnMatch(query = to, train = from, k = 2); a query's neighbours are ranked by distance, on
equal distance the lower train index ranks first; then the ratio test distance0 < ratio * distance1 on the float
distances, evaluated in double; output pairs (fromIndex = train index, toIndex = query index) in query order.  Fewer
than two train rows: no matches (the reference reads match[1] out of bounds there).  A missing neighbour is reported as
index -1 / distance INT_MAX.

Written from that description with a popcount over the xor; it shares no code with oracle/mslam_oracle.c, which
tests/test_match_ref.py compares it with.

The generators return lists of `Case`s: one train set (`from_desc`), its queries (`to_desc`) and `claims`, what the
case says it plants.  Every claim is checked against the reference's OUTPUT in tests/test_match_ref.py (on the CPU), so a
GPU test that runs a case cannot pass vacuously.  All generators are deterministic.

The "weights" construction used for the distance extremes: relative to a base vector z and a fixed permutation of the
256 bit positions, P(k) is the vector with the first k permuted bits set; hamming(z ^ P(a), z ^ P(b)) = |a - b|.  A train
set of rows z ^ P(w_j) and queries z ^ P(c) therefore has exactly known distances |c - w_j|, up to 256 (the
complement), in every byte and dword of the descriptor.
"""
import collections

import numpy as np

INT_MAX = 2 ** 31 - 1
TILE = 32                 # train rows per tile of the matrix-core kernel
MM_MAX_TRAIN = 32736      # its train limit (32 * 1023)
RATIOS = (0.0, 1.0 / 3.0, 0.5, 0.7, 0.75, 0.8, 1.0, 1.5)

Case = collections.namedtuple("Case", "name from_desc to_desc claims")


# ---- the reference --------------------------------------------------------------------------------------------------
def _popcount64(x):
    """population count of every uint64 of x (SWAR; no table, no numpy-version dependence)"""
    x = x - ((x >> np.uint64(1)) & np.uint64(0x5555555555555555))
    x = (x & np.uint64(0x3333333333333333)) + ((x >> np.uint64(2)) & np.uint64(0x3333333333333333))
    x = (x + (x >> np.uint64(4))) & np.uint64(0x0F0F0F0F0F0F0F0F)
    return (x * np.uint64(0x0101010101010101)) >> np.uint64(56)


def _rows(d):
    return np.ascontiguousarray(d, np.uint8).reshape(-1, 32)


def distances(from_desc, to_desc):
    """[n_to, n_from] Hamming distances (small inputs only: the whole matrix is materialised)"""
    f, t = _rows(from_desc).view(np.uint64), _rows(to_desc).view(np.uint64)
    return _popcount64(t[:, None, :] ^ f[None, :, :]).sum(-1).astype(np.int32)


def knn2(from_desc, to_desc, max_pairs=1 << 22):
    """-> (idx0, idx1, dist0, dist1), int32 [n_to]: nearest and second nearest train row (`from`) of every query (`to`).
    Queries are processed in chunks of at most max_pairs (query, train) pairs: 4 M pairs are 128 MB of xor words."""
    f, t = _rows(from_desc).view(np.uint64), _rows(to_desc).view(np.uint64)
    n_from, n_to = len(f), len(t)
    i0 = np.full(n_to, -1, np.int32)
    i1 = np.full(n_to, -1, np.int32)
    d0 = np.full(n_to, INT_MAX, np.int32)
    d1 = np.full(n_to, INT_MAX, np.int32)
    if n_from == 0 or n_to == 0:
        return i0, i1, d0, d1
    step = max(1, max_pairs // n_from)
    for q in range(0, n_to, step):
        d = _popcount64(t[q:q + step, None, :] ^ f[None, :, :]).sum(-1).astype(np.int32)
        rows = np.arange(len(d))
        a = d.argmin(1)                    # first occurrence of the minimum: the lower train index wins a tie
        i0[q:q + step], d0[q:q + step] = a, d[rows, a]
        if n_from >= 2:
            d[rows, a] = 1 << 20           # the runner-up: the same rule over the remaining rows
            b = d.argmin(1)
            i1[q:q + step], d1[q:q + step] = b, d[rows, b]
    return i0, i1, d0, d1


def ratio_filter(knn, n_from, ratio):
    """ratio test + ordered compaction of a knn2 result -> (from_idx, to_idx), int32"""
    i0, _, d0, d1 = knn
    if n_from < 2 or len(i0) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    ok = d0.astype(np.float32).astype(np.float64) < np.float64(ratio) * d1.astype(np.float32).astype(np.float64)
    to = np.nonzero(ok)[0].astype(np.int32)
    return i0[to].astype(np.int32), to


def match(from_desc, to_desc, ratio=0.7):
    return ratio_filter(knn2(from_desc, to_desc), len(_rows(from_desc)), ratio)


# ---- building blocks of the generators ----------------------------------------------------------------------------
def _pack(bits):
    return np.packbits(np.asarray(bits, bool).reshape(-1, 256), axis=1, bitorder="little")


class _Weights:
    """the weights construction of the module docstring"""

    def __init__(self, seed):
        rng = np.random.default_rng(seed)
        self.z = rng.integers(0, 256, 32, dtype=np.uint8)
        self.perm = rng.permutation(256)

    def rows(self, weights):
        w = np.asarray(weights, np.int64).reshape(-1)
        bits = np.zeros((len(w), 256), bool)
        bits[:, self.perm] = np.arange(256)[None, :] < w[:, None]
        return _pack(bits) ^ self.z[None, :]


def flip(row, k, rng):
    """`row` with k distinct random bits flipped"""
    bits = np.zeros(256, bool)
    bits[rng.permutation(256)[:k]] = True
    return row ^ _pack(bits)[0]


def n_tiles(n_from):
    return (n_from + TILE - 1) // TILE


def slice_boundaries(n_from):
    """train rows at which a slice of the sliced matrix-core kernel begins: tile n_tiles * s / n_slices for the single
    call's n_slices = min(8, (n_from + 255) / 256) and for the captured form's fixed 8 (0 and n_from themselves excluded)"""
    T, out = n_tiles(n_from), set()
    for ns in (max(1, min(8, (n_from + 255) // 256)), 8):
        for s in range(1, ns):
            r = (T * s // ns) * TILE
            if 0 < r < n_from:
                out.add(r)
    return sorted(out)


# ---- generators -------------------------------------------------------------------------------------------------------
def distance_extremes(n_from, seed=11):
    """Distances at both ends of the range, at any train size.  Three train sets in the weights construction, queries of
    every weight c = 0..256:
      all_equal      every row the complement of the base (weight 256): every row ties at 256 - c, the answer is rows 0
                     and 1 — (v, v) for every v, with (0, 0) and (256, 256);
      one_at_255     one row of weight 255 at the middle of the last tile, the rest 256: (255 - c, 256 - c) — every
                     (v, v + 1), with (255, 256); the winner sits late, the runner-up is the first far row;
      one_at_0       one row of weight 0 (the last real row), the rest 256: (c, 256 - c) up to c = 128, with (0, 256) at
                     c = 0; beyond it the far rows 0 and 1 are the two nearest.
    claims: pairs = the (d0, d1) the case is built to produce."""
    w = _Weights(seed)
    c = np.arange(257)
    to = w.rows(c)
    cases = []
    weights = np.full(n_from, 256)
    pairs = {(int(256 - x), int(256 - x) if n_from >= 2 else INT_MAX) for x in c}
    cases.append(Case("all_equal", w.rows(weights), to, dict(pairs=pairs, rows01=True)))
    if n_from >= 3:
        p = min(n_from - 1, (n_tiles(n_from) - 1) * TILE + 15)
        weights = np.full(n_from, 256)
        weights[p] = 255
        pairs = {(255 - int(x), 256 - int(x)) for x in c[:256]} | {(0, 0)}
        cases.append(Case("one_at_255", w.rows(weights), to, dict(pairs=pairs, planted=p)))
        weights = np.full(n_from, 256)
        weights[n_from - 1] = 0
        pairs = {(int(x), 256 - int(x)) if x <= 128 else (256 - int(x), 256 - int(x)) for x in c}
        cases.append(Case("one_at_0", w.rows(weights), to, dict(pairs=pairs, planted=n_from - 1)))
    return cases


def _position_plan(n_from):
    """(winner row, runner-up row, tie) triples over distinct train rows.  Rows are handed out at most once (a planted row
    is near one query only); a triple whose rows are taken or out of range is dropped."""
    T = n_tiles(n_from)
    last = n_from - 1
    mid = (T // 2) * TILE
    used, plan = set(), []

    def add(wr, rr, tie):
        if tie and wr > rr:
            wr, rr = rr, wr        # equal distances: the lower row is the winner
        if wr == rr or not (0 <= wr < n_from and 0 <= rr < n_from) or wr in used or rr in used:
            return False
        used.update((wr, rr))
        plan.append((wr, rr, tie))
        return True

    # first and last tile, both in the (partial) last tile
    add(0, last, False), add(last - 1, 1, False), add(2, last - 2, True), add((T - 1) * TILE, last - 3, False)
    if n_from - (T - 1) * TILE >= 6:
        add(last - 4, (T - 1) * TILE + 1, False)
    # each side of every slice boundary, in both orders, once with equal distances
    for b in slice_boundaries(n_from):
        add(b - 1, b, True), add(b + 1, b - 2, False), add(b - 3, b + 2, False), add(b + 3, b - 4, False)
    # same tile (other / same half-wave lane), adjacent tiles
    add(mid + 10, mid + 6, False), add(mid + 7, mid + 11, True), add(mid + 9, mid + 8, False)
    add(mid + 16, mid + 48, False), add(mid + 49, mid + 17, True)
    # every residue as a winner and as a runner-up (both half-wave lanes, all 16 accumulator registers), in the first
    # tiles from a residue-dependent start on that still have both rows free
    for rho in range(TILE):
        other = (rho * 7 + 3) % TILE
        for role in (0, 1):
            for k in range(T):
                ta, tb = (rho * 5 + 2 * role + k) % T, (rho * 11 + 1 + 3 * role + k) % T
                wr, rr = (ta * TILE + rho, tb * TILE + other) if role == 0 else (ta * TILE + other, tb * TILE + rho)
                if add(wr, rr, rho % 4 == role):
                    break
    return plan


def position_extremes(n_from, seed=12):
    """Winner and runner-up at planted ROWS.  Random train rows (far from everything: ~128 +- 8) with, for query i, two
    rows replaced by copies of the query with a few bits flipped (distances 0..12, some pairs equal).
    claims: planted = [(winner row, runner-up row)] per query, boundaries = the slice boundaries of this size."""
    rng = np.random.default_rng(seed + n_from)
    plan = _position_plan(n_from)
    f = rng.integers(0, 256, (n_from, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (max(len(plan), 1), 32), dtype=np.uint8)
    for i, (wr, rr, tie) in enumerate(plan):
        k0 = int(rng.integers(0, 7))
        k1 = k0 if tie else k0 + 1 + int(rng.integers(0, 6))
        f[wr] = flip(t[i], k0, rng)
        f[rr] = flip(t[i], k1, rng)
    return [Case("positions", f, t[:len(plan)], dict(planted=[(a, b) for a, b, _ in plan], ties=[x for _, _, x in plan],
                                                      boundaries=slice_boundaries(n_from)))]


def masked_tail(n_from, seed=13):
    """n_from % 32 in {1, 2, 31}: the best match of every query is the LAST real row (distance 0..8), every other row is
    far.  The rows the partial last tile re-reads are copies of that best row: unmasked, one of them takes the runner-up
    slot at the winner's distance.  claims: winner = n_from - 1; the runner-up is a real row, or none for n_from = 1."""
    assert n_from % TILE in (1, 2, 31)
    rng = np.random.default_rng(seed + n_from)
    f = rng.integers(0, 256, (n_from, 32), dtype=np.uint8)
    q = f[n_from - 1].copy()
    t = np.stack([flip(q, k, rng) for k in range(9)])
    return [Case("masked_tail", f, t, dict(winner=n_from - 1))]


def max_age(n_from, seed=14):
    """n_from in {16384, 16385, 32735, 32736}: winners in the first tile (rows 0 and 31: the oldest keys; from 16385 rows
    on their age is >= 2^14, the bit the age shares with the distance field) against a competitor in the last tile.
    Weights construction, every other row at weight 256; queries of weight c in {0, 254, 255} see the planted rows at
    distance w - c: 255, 1 and 0 from a row of weight 255.  Train sets:
      same_R      row R and the late row both at weight 255: equal distances, row R must win (R = 0, 31);
      minus1_R    row R at 255, the late row at 254: the late row must win, row R is the runner-up (for c = 255 row R is
                  at 0 and the late row at 1 like every far row: row R wins, the first far row is the runner-up —
                  distance 0 has no "minus one");
      far_same    every row at 256: distance 256, rows 0 and 1;
      far_minus1  every row at 256 but the late row at 255: the late row wins at 255 over row 0 at 256.
    (Row 31 cannot WIN at distance 256: rows 0..30 would have to be farther.)
    claims: expect = {c: (idx0, idx1, d0, d1)}."""
    assert n_from in (16384, 16385, 32735, 32736)
    w = _Weights(seed)
    late = (n_tiles(n_from) - 1) * TILE + min(5, n_from - 1 - (n_tiles(n_from) - 1) * TILE)
    cs = (0, 254, 255)
    to = w.rows(cs)
    cases = []
    for R in (0, 31):
        weights = np.full(n_from, 256)
        weights[R] = weights[late] = 255
        exp = {c: (R, late, 255 - c, 255 - c) for c in cs}
        cases.append(Case("same_%d" % R, w.rows(weights), to, dict(expect=exp, rows=(R, late))))
        weights = weights.copy()
        weights[late] = 254
        exp = {0: (late, R, 254, 255), 254: (late, R, 0, 1), 255: (R, 1 if R == 0 else 0, 0, 1)}
        cases.append(Case("minus1_%d" % R, w.rows(weights), to, dict(expect=exp, rows=(R, late))))
    weights = np.full(n_from, 256)
    exp = {c: (0, 1, 256 - c, 256 - c) for c in cs}
    cases.append(Case("far_same", w.rows(weights), to, dict(expect=exp, rows=(0, 1))))
    weights = weights.copy()
    weights[late] = 255
    exp = {0: (late, 0, 255, 256), 254: (late, 0, 1, 2), 255: (late, 0, 0, 1)}
    cases.append(Case("far_minus1", w.rows(weights), to, dict(expect=exp, rows=(0, late))))
    return cases


def ratio_grid(m):
    """train = [all-zero row, row with its first m bits set]; query d0 has d0 bits set beyond bit m, d0 = 0..256 - m:
    distances (d0, d0 + m).  Over m = 0..256 every pair 0 <= d0 <= d1 <= 256 exactly once (33 153 queries); m = 0 is the
    exact tie (row 0 wins).  claims: pairs = [(d0, d1)] in query order."""
    assert 0 <= m <= 256
    bits = np.arange(256)
    f = _pack(np.stack([bits < 0, bits < m]))
    d0 = np.arange(257 - m)
    t = _pack((bits[None, :] >= m) & (bits[None, :] < m + d0[:, None]))
    return [Case("ratio_grid_%d" % m, f, t, dict(pairs=[(int(x), int(x) + m) for x in d0]))]


def mixed(n_from, n_to, seed=15):
    """the shape sweeps' data: random train rows with some exact duplicates (ties); a third of the queries are random,
    the rest train rows with 0..20 bits flipped — close neighbours at every position, equal distances between duplicates"""
    rng = np.random.default_rng([seed, n_from, n_to])
    f = rng.integers(0, 256, (n_from, 32), dtype=np.uint8)
    if n_from >= 4:
        dup = rng.integers(0, n_from, max(1, n_from // 8))
        f[dup] = f[rng.integers(0, n_from, len(dup))]
    t = rng.integers(0, 256, (n_to, 32), dtype=np.uint8)
    if n_from:
        for q in range(0, n_to, 3):
            t[q] = flip(f[int(rng.integers(0, n_from))], int(rng.integers(0, 21)), rng)
        for q in range(1, n_to, 3):
            t[q] = flip(f[n_from - 1 - int(rng.integers(0, min(n_from, 40)))], int(rng.integers(0, 21)), rng)
    return [Case("mixed", f, t, {})]
