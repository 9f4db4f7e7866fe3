"""tests/match_ref.py on the CPU: the numpy reference equals the oracle's matcher, and every generator plants what it claims.

The coverage assertions below are computed from the REFERENCE's output only (never from a claim alone): they are what
keeps tests/test_gpu_match_edges.py, which runs the same cases on the GPU, from passing vacuously."""
import numpy as np
import pytest

import match_ref as mr

POSITION_SIZES = (2, 3, 33, 65, 257, 300, 513, 2049, 2060, 4097, 32736)
TAIL_SIZES = (1, 2, 31, 33, 34, 63, 257, 258, 287, 4097, 32705, 32735)
AGE_SIZES = (16384, 16385, 32735, 32736)


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _check_case(orc, case):
    ref = mr.knn2(case.from_desc, case.to_desc)
    assert _same(ref, orc.match_knn2_raw(case.from_desc, case.to_desc)), case.name
    for ratio in mr.RATIOS:
        assert _same(mr.ratio_filter(ref, len(case.from_desc), ratio), orc.match(case.from_desc, case.to_desc, ratio)), (case.name, ratio)
    return ref


def test_reference_equals_oracle_on_random_and_tie_shapes(orc):
    """the shapes of test_gpu_parity.py's matcher tests (random descriptors; few distinct descriptors: many ties)"""
    rng = np.random.default_rng(1)
    for n_from, n_to in [(2000, 2000), (513, 257), (1, 5), (2, 3), (300, 1), (32, 64), (33, 600), (17000, 130), (33000, 70),
                         (0, 4), (4, 0)]:
        f = rng.integers(0, 256, (n_from, 32), dtype=np.uint8)
        t = rng.integers(0, 256, (n_to, 32), dtype=np.uint8)
        _check_case(orc, mr.Case("random", f, t, {}))
    rng = np.random.default_rng(2)
    base = rng.integers(0, 256, (7, 32), dtype=np.uint8)
    f = base[rng.integers(0, 7, 700)]
    t = base[rng.integers(0, 7, 300)].copy()
    t[::3, 0] ^= 1
    ref = _check_case(orc, mr.Case("ties", f, t, {}))
    assert (ref[2] == ref[3]).mean() > 0.9
    for n_from, n_to in [(0, 3), (1, 31), (2, 33), (3, 2), (65, 129), (2049, 257), (32737, 33)]:
        _check_case(orc, mr.mixed(n_from, n_to)[0])


def test_tie_rule_is_observable():
    """two equal train rows: the lower index first, the other second — flipping the rule changes this result"""
    f = np.zeros((3, 32), np.uint8)
    f[0, 0] = 1
    i0, i1, d0, d1 = mr.knn2(f, np.zeros((1, 32), np.uint8))
    assert (i0[0], i1[0], d0[0], d1[0]) == (1, 2, 0, 0)
    assert [x[0] for x in mr.knn2(f[:1], f[:1])] == [0, -1, 0, mr.INT_MAX]
    assert [len(x) for x in mr.match(f[:1], f, 1.5)] == [0, 0]          # n_from < 2: no matches
    assert [len(x) for x in mr.match(f, f[:0], 1.5)] == [0, 0]


@pytest.mark.parametrize("n_from", [1, 2, 3, 31, 33, 257, 2049, 32736, 32737, 65535])
def test_distance_extremes(orc, n_from):
    d0s, d1s, pairs = set(), set(), set()
    for case in mr.distance_extremes(n_from):
        ref = _check_case(orc, case) if n_from <= 2049 else mr.knn2(case.from_desc, case.to_desc)
        got = set(zip(ref[2].tolist(), ref[3].tolist()))
        assert got == case.claims["pairs"], case.name
        if case.claims.get("rows01"):
            assert (ref[0] == 0).all() and (ref[1] == (1 if n_from >= 2 else -1)).all()
        if "planted" in case.claims:   # the planted row is the winner wherever it is strictly nearest
            d = mr.distances(case.from_desc[[case.claims["planted"], 0]], case.to_desc)
            assert ((ref[0] == case.claims["planted"]) == (d[:, 0] < d[:, 1])).all()
        pairs |= got
        d0s |= set(ref[2].tolist())
        d1s |= set(ref[3].tolist())
    if n_from >= 3:
        assert d0s == set(range(257)) and d1s == set(range(257))
        assert {(0, 0), (0, 256), (255, 256), (256, 256)} <= pairs
    else:
        assert d0s == set(range(257))


def _roles(planted, boundaries):
    """the boundaries that have a (winner, runner-up) pair within 4 rows of them, winner below / above the boundary"""
    w_before = {b for b in boundaries for w, r in planted if b - 4 <= w < b <= r <= b + 3}
    w_after = {b for b in boundaries for w, r in planted if b - 4 <= r < b <= w <= b + 3}
    return w_before, w_after


@pytest.mark.parametrize("n_from", POSITION_SIZES)
def test_position_extremes(orc, n_from):
    (case,) = mr.position_extremes(n_from)
    ref = _check_case(orc, case) if n_from <= 4097 else mr.knn2(case.from_desc, case.to_desc)
    planted = list(zip(ref[0].tolist(), ref[1].tolist()))
    assert planted == case.claims["planted"] and len(planted) >= 1
    ties = (ref[2] == ref[3])
    assert ties.tolist() == case.claims["ties"] and (ref[3] <= 12).all()
    T, last = mr.n_tiles(n_from), n_from - 1
    tile = lambda r: r // mr.TILE   # noqa: E731
    assert (0, last) in planted or n_from < 3
    if n_from >= 257:
        assert ties.any()
        assert any(tile(w) == tile(r) for w, r in planted)                                  # same tile
        assert any(tile(w) == tile(r) and (w % 32 // 4) % 2 != (r % 32 // 4) % 2 for w, r in planted)   # ... other half-wave lane
        assert any(abs(tile(w) - tile(r)) == 1 for w, r in planted)                         # adjacent tiles
        assert any(tile(w) == 0 and tile(r) == T - 1 for w, r in planted)                   # first and last tile
        if n_from - (T - 1) * 32 >= 4:   # (a last tile of one row holds one planted row)
            assert any(tile(w) == T - 1 and tile(r) == 0 for w, r in planted)
            assert any(tile(w) == T - 1 and tile(r) == T - 1 for w, r in planted)           # both in the (partial) last tile
        # each side of every slice boundary, in both orders
        w_before, w_after = _roles(planted, case.claims["boundaries"])
        assert case.claims["boundaries"] == mr.slice_boundaries(n_from) and len(case.claims["boundaries"]) >= 7
        assert w_before == set(case.claims["boundaries"]) and w_after == set(case.claims["boundaries"])
    if n_from >= 2049:
        # every row of a tile as a winner and as a runner-up: both half-wave lanes, all 16 accumulator registers
        assert {w % 32 for w, _ in planted} == set(range(32)) and {r % 32 for _, r in planted} == set(range(32))


def test_slice_boundaries_restate_the_kernel_rule():
    assert mr.slice_boundaries(256) == [32, 64, 96, 128, 160, 192, 224]       # one slice in the single call, 8 captured
    assert mr.slice_boundaries(257) == [32, 64, 96, 128, 160, 192, 224]       # 9 tiles: 2 slices begin at tile 4 (= 8ths' tile 4)
    assert 128 in mr.slice_boundaries(257)
    assert mr.slice_boundaries(32) == [] and mr.slice_boundaries(33) == [32]
    assert mr.slice_boundaries(32736) == [(1023 * s // 8) * 32 for s in range(1, 8)]


@pytest.mark.parametrize("n_from", TAIL_SIZES)
def test_masked_tail(orc, n_from):
    (case,) = mr.masked_tail(n_from)
    ref = _check_case(orc, case)
    assert n_from % 32 in (1, 2, 31)
    assert (ref[0] == n_from - 1).all() and ref[2].tolist() == list(range(9))
    if n_from == 1:
        assert (ref[1] == -1).all() and (ref[3] == mr.INT_MAX).all()
    else:
        assert ((0 <= ref[1]) & (ref[1] < n_from - 1)).all() and (ref[3] > (60 if n_from > 2 else -1)).all()
    # the rows a partial last tile re-reads are copies of the WINNER: were they real, the runner-up would sit at the
    # winner's distance — the reference's runner-up is far from it
    assert (ref[3] - ref[2] > 50).all() or n_from <= 2


@pytest.mark.parametrize("n_from", AGE_SIZES)
def test_max_age(orc, n_from):
    seen = set()
    for case in mr.max_age(n_from):
        ref = mr.knn2(case.from_desc, case.to_desc)
        assert _same(ref, orc.match_knn2_raw(case.from_desc, case.to_desc)), case.name
        for k, c in enumerate((0, 254, 255)):
            got = tuple(int(x[k]) for x in ref)
            assert got == case.claims["expect"][c], (case.name, c)
            seen.add((got[0], got[2]))
    late = [r for r, _ in seen if r >= (mr.n_tiles(n_from) - 1) * 32]
    assert late and all(r < n_from for r in late)
    # winners in rows 0 and 31 (age of row 0: 32 * (tiles - 1) + 31) and in the last tile, at distances 0, 1, 255, 256
    assert {(0, d) for d in (0, 1, 255, 256)} <= seen and {(31, d) for d in (0, 1, 255)} <= seen
    assert {d for r, d in seen if r in late} >= {0, 1, 254, 255}
    age0 = 32 * (mr.n_tiles(n_from) - 1) + 31
    assert (age0 >= 1 << 14) == (n_from > 16384) and age0 < 1 << 15


def test_ratio_grid(orc):
    """every pair 0 <= d0 <= d1 <= 256 exactly once over m = 0..256, and the ratio test of all of them at eight ratios"""
    pairs = []
    for m in range(257):
        (case,) = mr.ratio_grid(m)
        assert len(case.from_desc) == 2
        ref = mr.knn2(case.from_desc, case.to_desc)
        assert _same(ref, orc.match_knn2_raw(case.from_desc, case.to_desc)), m
        got = list(zip(ref[2].tolist(), ref[3].tolist()))
        assert got == case.claims["pairs"] and (ref[0] == 0).all() and (ref[1] == 1).all()
        pairs += got
        for ratio in mr.RATIOS:
            assert _same(mr.ratio_filter(ref, 2, ratio), orc.match(case.from_desc, case.to_desc, ratio)), (m, ratio)
    assert len(pairs) == 33153 == len(set(pairs))
    assert set(pairs) == {(a, b) for b in range(257) for a in range(b + 1)}
