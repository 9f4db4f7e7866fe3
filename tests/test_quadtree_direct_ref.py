"""The closed form of the quadtree selection (tests/quadtree_direct_ref.py, what k_quadtree_direct computes) against the
oracle's list simulation, element for element, on seeded random candidate lists: landscape, portrait and square levels,
scales 1.2^0 .. 1.2^7, min_size 7 .. 4000, 1 .. 1000 candidates, uniform, clustered, one tight cluster, and partly out
of range.  Draws whose geometric depth is unbounded (min_size / sf^2 below one pixel: the reference ends through its stop
rule alone) are the old kernels' and are skipped here, at most 10 % of the draws."""
import numpy as np
import pytest

import quadtree_direct_frames as F
import quadtree_direct_ref as Q

N_DRAWS = 500
SHAPES = [(640, 480), (480, 640), (320, 320), (400, 100), (80, 300), (1280, 720), (160, 120), (213, 777)]
MIN_SIZES = [7, 20, 50, 100, 400, 1000, 2500, 4000]


def _draw(rng):
    W, H = SHAPES[rng.integers(len(SHAPES))]
    lvl = int(rng.integers(8))
    sf = np.float32(1.0)
    for _ in range(lvl):
        sf = np.float32(sf * np.float32(1.2))
    w, h = max(45, int(round(W / float(sf)))), max(45, int(round(H / float(sf))))
    bw, bh = w - 2 * Q.BORDER, h - 2 * Q.BORDER
    min_size = int(MIN_SIZES[rng.integers(len(MIN_SIZES))])
    n = int(np.exp(rng.uniform(0, np.log(1000))))
    kind = ("uniform", "clustered", "tight", "out_of_range")[rng.integers(4)]
    if kind == "uniform":
        x, y = rng.integers(0, bw, n), rng.integers(0, bh, n)
    elif kind == "clustered":
        k = int(rng.integers(1, 6))
        cx, cy = rng.integers(0, bw, k), rng.integers(0, bh, k)
        which = rng.integers(0, k, n)
        x = np.clip(cx[which] + rng.normal(0, 6, n).astype(int), 0, bw - 1)
        y = np.clip(cy[which] + rng.normal(0, 6, n).astype(int), 0, bh - 1)
    elif kind == "tight":
        cx, cy = rng.integers(0, bw), rng.integers(0, bh)
        x = np.clip(cx + rng.integers(-3, 4, n), 0, bw - 1)
        y = np.clip(cy + rng.integers(-3, 4, n), 0, bh - 1)
    else:
        x, y = rng.integers(0, bw + bw // 3 + 2, n), rng.integers(0, bh + bh // 3 + 2, n)
    resp = rng.integers(1, 256 if rng.integers(2) else 4, n)      # few distinct responses: ties, the first maximum wins
    cand = np.stack([x, y, resp], 1).astype(np.float32)
    return kind, w, h, sf, min_size, cand


@pytest.fixture(scope="module")
def draws(orc):
    rng = np.random.default_rng(20240611)
    out = []
    for _ in range(N_DRAWS):
        kind, w, h, sf, min_size, cand = _draw(rng)
        c = np.zeros(len(cand), orc.CAND_DT)
        c["x"], c["y"], c["response"] = cand[:, 0], cand[:, 1], cand[:, 2]
        ref = orc.quadtree(c, w, h, sf, min_size)
        got, info = Q.select(cand, w, h, float(sf), min_size)
        out.append((kind, (w, h, float(sf), min_size), cand, ref, got, info))
    return out


def test_equals_the_oracle_element_for_element(draws):
    for kind, geom, cand, ref, got, info in draws:
        if got is None:
            continue
        want = np.stack([ref["x"], ref["y"], ref["response"]], 1).reshape(-1, 3)
        assert len(got) == len(want), (kind, geom, len(cand), info, len(got), len(want))
        assert np.array_equal(cand[got].reshape(-1, 3), want), (kind, geom, len(cand), info)


def test_at_most_a_tenth_of_the_draws_is_unbounded(draws):
    skipped = sum(1 for d in draws if d[4] is None)
    print("unbounded draws: %d of %d" % (skipped, len(draws)))
    assert skipped * 10 <= len(draws), skipped


def test_the_draw_reaches_the_regimes(draws):
    done = [d for d in draws if d[4] is not None]
    cut = sum(1 for d in done if d[5]["cut"] > 0)
    multi = sum(1 for d in done if d[5]["n_init"] > 1)
    dropped = sum(1 for d in done if d[5]["dropped"] > 0)
    idle = sum(1 for d in done if d[5]["P"] == d[5]["depth"] + 1)
    print("early stop left non-keep leaves: %d, several init nodes: %d, dropped candidates: %d, last pass idle at the "
          "depth bound: %d" % (cut, multi, dropped, idle))
    assert cut >= 20 and multi >= 20 and dropped >= 20
    assert {d[0] for d in done} == {"uniform", "clustered", "tight", "out_of_range"}


def test_depth_bound_of_the_shapes_the_project_runs():
    sf = [np.float32(1.0)]
    for _ in range(7):
        sf.append(np.float32(sf[-1] * np.float32(1.2)))
    sizes = [(640, 480)] + [(int(round(640 / float(s))), int(round(480 / float(s)))) for s in sf[1:]]
    depths = [Q.depth_bound(w, h, float(s), 1000) for (w, h), s in zip(sizes, sf)]
    assert depths == [5, 5, 5, 4, 4, 4, 4, 4]
    assert Q.table_slots(1, 5) == 1365 and Q.table_slots(1, 4) == 341
    assert Q.depth_bound(320, 240, 1.0, 50) == 6 and Q.table_slots(1, 6) == 5461


# ---- the frames of tests/test_gpu_quadtree_direct.py reach the regimes they are named after ------------------------------
def _infos(orc, frame, p):
    out = []
    for w, h, s, cand in F.level_lists(orc, frame, p):
        got, info = Q.select(cand, w, h, float(s), p["min_node_area"])
        if got is not None:
            assert np.array_equal(cand[got].reshape(-1, 3), F.oracle_select(orc, cand, w, h, s, p["min_node_area"]))
        out.append((cand, got, info))
    return out


def test_gpu_single_frames_reach_their_regimes(orc):
    cases = F.single_cases()
    for name, (frame, p) in cases.items():
        assert all(F.eligible_levels(frame.shape[1], frame.shape[0], p)), name
    info = {name: _infos(orc, *cases[name]) for name in cases}
    cand, got, i = info["one_dot"][0]
    assert len(cand) == 1 and got == [0] and tuple(cand[0][:2]) == (50 - 19, 40 - 19)
    cand, got, i = info["two_dots_one_quadrant"][0]
    assert len(cand) == 2 and len(got) == 1 and i["P"] == 1 and i["cut"] == 1 and i["depth"] == 5     # a non-keep leaf
    cand, got, i = info["equal_dots_one_leaf"][0]
    assert len(cand) == 6 and len(set(cand[:, 2])) == 1 and got == [4, 0, 5]     # candidate 0 wins the leaf of 0 .. 3
    for name in ("wide", "tall"):
        for cand, got, i in info[name]:
            assert i["n_init"] >= 6 and len(got) > 10 and i["P"] > 2, (name, i)


def test_gpu_fallback_cases_are_not_eligible(orc):
    for name, (frame, p) in F.fallback_cases().items():
        assert not any(F.eligible_levels(320, 240, p)), name
    p = F.fallback_cases()["area7_unbounded"][1]
    depths = [Q.depth_bound(w, h, float(s), 7) for w, h, s in F.level_sizes(320, 240, p)]
    assert depths[0] == 7 and depths[6] is None and depths[7] is None, depths
    assert Q.depth_bound(320, 240, 1.0, 50) == 6


def test_gpu_batch_frames_reach_their_regimes(orc):
    assert F.eligible_levels(F.BATCH_W, F.BATCH_H, F.BATCH_P) == [True, True, True]
    assert F.eligible_levels(F.BATCH_W, F.BATCH_H, F.BATCH_MIXED_P) == [True, False, True]
    frames = F.batch_frames()
    n = [[len(c) for _, _, _, c in F.level_lists(orc, f, F.BATCH_P)] for f in frames]
    assert n[F.BATCH_FLAT] == [0, 0, 0]
    assert n[F.BATCH_NOISE][0] > 2048 and n[F.BATCH_NOISE][2] > F.DIRECT_MAX_CANDIDATES
    for t, row in enumerate(n):
        if t not in (F.BATCH_FLAT, F.BATCH_NOISE):
            assert all(64 < x <= 512 for x in row), (t, row)
