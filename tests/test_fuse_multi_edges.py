"""The edge cases of tests/fuse_multi_edge_cases.py without a GPU: tests/fuse_multi_ref.py's restatement, and arithmetic of
k_fuse_multi.hip restated here, prove that every case reaches the path it is named for — a lifted single-target case gives
fuse_ref.search's result in its target and nothing in the decoys; a dealt case drops rows in both cross-target steps; the
frame extents give every number of cells per thread of the binning; wide_64 makes the prefix loop of the compaction take a
second trip over a non-zero count; and so on, one assertion per path.  tests/test_gpu_fuse_multi_edges.py then holds the
kernels to the restatement on the same cases."""
import functools

import numpy as np
import pytest

import fuse_multi_edge_cases as ec
import fuse_multi_ref as fm
import fuse_ref as fr

FR_KEYS = ("keep_pos", "drop_pos", "keep_lid", "drop_lid", "dist")


def _is_lift_of(case, single, what):
    """the lifted case's result is fuse_ref.search's of the single-target case with a target column of m, and no decoy
    leaves a row even before the cross-target steps -> the number of pairs"""
    st = {}
    got = ec.reference(case, st)
    ref = fr.search(single["keep"], single["drop"], radius=case["radius"], **dict(single["kw"], **{k: case["kw"][k] for k in ("max_world_distance",)}))
    for k in FR_KEYS:
        assert got[k].dtype == ref[k].dtype and got[k].tobytes() == ref[k].tobytes(), (what, k)
    assert got["target"].tolist() == [case["m"]] * len(ref["dist"]), what
    assert all(r[0] == case["m"] for r in st["rows"]), what
    return len(ref["dist"])


@pytest.mark.parametrize("name", fr.HAND_CASES)
def test_lifted_hand_cases(name):
    single = fr.hand_case(name)
    for m, n_drop in ec.LIFTS:
        case = ec.lifted(single, m, n_drop)
        assert len(case["drops"]) == n_drop and [len(d[0]) for o, d in enumerate(case["drops"]) if o != m] == [(0, 1, 9)[k % 3] for k in range(n_drop - 1)]
        got = ec.reference(case)
        if name == "repeated_id":                                  # both positions of the repeated drop id are rows of the
            assert not ec.no_repeats(single) and len(got["dist"]) == 1   # single call; step A leaves one here
            continue
        assert ec.no_repeats(single)
        _is_lift_of(case, single, (name, m, n_drop))
        assert fm.rows_of(got) == [(m, j, i, d) for j, i, d in single["expect"]]


def test_lifted_decoys_are_in_front_or_behind_as_stated():
    case = ec.lifted(fr.hand_case("equal_distance"), 63, 64)
    kw = case["kw"]
    seen = {(False, 1): 0, (False, 9): 0, (True, 1): 0, (True, 9): 0}
    for k, (d, R, t) in enumerate(zip(case["drops"][:63], case["Rs"], case["ts"])):
        _, inside = fr.drop_keypoints(d[1], R, t, kw["cam"], kw["width"], kw["height"])
        _, keep_in = fr.drop_keypoints(case["keep"][1], R, t, kw["cam"], kw["width"], kw["height"])
        assert (t[2] == -100.0) == bool(k % 2) and (not inside.any() and not keep_in.any() if k % 2 else inside.all())
        if len(d[0]):
            seen[(bool(k % 2), len(d[0]))] += 1
    assert min(seen.values()) > 0


@pytest.mark.parametrize("nk,nd", fr.SIZES)
def test_lifted_sizes(nk, nd):
    single = fr.sized_case(nk, nd)
    assert ec.no_repeats(single)
    n = _is_lift_of(ec.lifted(single, 2, 4), single, (nk, nd))
    assert min(nk, nd) == 0 or n > 0


def test_frame_extents_give_every_number_of_cells_per_thread():
    """k_fusem_bin: per = ceil(cells / 1024) takes 1, 2, 3 and 4 over the extents, with idle threads at 2 and 3"""
    per = {e: ec.cells_per_thread(*e) for e in ec.FRAMES}
    assert {p for p, _ in per.values()} == {1, 2, 3, 4}
    assert ec.grid_of(8192, 8192) == (7, 64, 64) and per[(8192, 8192)] == (4, 1024)
    assert ec.grid_of(2000, 1100) == (5, 63, 35) and per[(2000, 1100)] == (3, 735) and 1024 - 735 == 289
    assert ec.grid_of(1056, 1000) == (5, 33, 32) and per[(1056, 1000)] == (2, 528)
    assert per[(100, 80)] == (1, 12) and per[(20, 20)] == (1, 1)
    for w, h in ec.FRAMES:
        s, nx, ny = ec.grid_of(w, h)
        assert nx * ny <= ec.MAX_CELLS and (s == 5 or (((w - 1) >> (s - 1)) + 1) * (((h - 1) >> (s - 1)) + 1) > ec.MAX_CELLS)


@pytest.mark.parametrize("width,height", ec.FRAMES)
def test_lifted_frames_and_radii(width, height):
    for nk, nd in fr.FRAME_SIZES:
        single = fr.frame_case(nk, nd, width, height)
        assert ec.no_repeats(single)
        case = ec.lifted(single, 1, 3)
        total = 0
        for radius in fr.frame_radii(width, height):
            total += _is_lift_of(dict(case, radius=radius), single, (width, height, nk, nd, radius))
        assert total > 0


@pytest.mark.parametrize("nk,nd", fr.POSED_SIZES)
def test_lifted_real_pose(nk, nd):
    single = fr.posed_case(40 + nk, nk, nd, shared=5)
    case = ec.lifted(single, 1, 3)
    n = _is_lift_of(case, single, "gate")
    open_ = dict(case, kw=dict(case["kw"], max_world_distance=np.inf))
    assert n >= 30 and _is_lift_of(open_, single, "no gate") != n                # the gate decides some pairs


@functools.lru_cache(None)
def _dealt(kind, nk, nd, M):
    case = ec.dealt(ec.dealt_source(kind, nk, nd), M)
    st = {}
    return case, ec.reference(case, st), st


@pytest.mark.parametrize("kind,nk,nd,M", ec.DEALT)
def test_dealt_cases_drop_rows_in_both_steps_in_every_pass(kind, nk, nd, M):
    case, ref, st = _dealt(kind, nk, nd, M)
    print("%s %d / %d dealt to %d: %d rows, A drops %d, B drops %d -> %d pairs" % (
        kind, nk, nd, M, len(st["rows"]), len(st["dropped_a"]), len(st["dropped_b"]), len(ref["dist"])))
    assert [len(d[0]) for d in case["drops"]] == [len(range(m, nd, M)) for m in range(M)]
    assert len(st["dropped_a"]) >= 3 and len(st["dropped_b"]) >= 3 and len(ref["dist"]) > 0
    assert len(case["planted"]) == (nk + ec.CHUNK - 1) // ec.CHUNK
    for c, j in enumerate(case["planted"]):                          # per pass: A drops target 0's row, B target 2's
        i = 10 + 3 * c
        assert j // ec.CHUNK == c and (0, j, i, 4) in st["dropped_a"] and (2, j, i, 6) in st["dropped_b"]
        assert (1, j, i, 2) in fm.rows_of(ref)
    assert len(set(ref["keep_lid"].tolist())) == len(set(ref["drop_lid"].tolist())) == len(ref["dist"])
    assert all((ref["target"] == m).any() for m in range(M))


@functools.lru_cache(None)
def _wide():
    case = ec.wide_64()
    st = {}
    return case, ec.reference(case, st), st


def test_wide_64_reaches_the_second_trip_of_the_prefix_loop():
    case, ref, st = _wide()
    nk = len(case["keep"][0])
    sizes = [len(d[0]) for d in case["drops"]]
    print("wide_64: %d rows, A drops %d, B drops %d -> %d pairs" % (len(st["rows"]), len(st["dropped_a"]), len(st["dropped_b"]), len(ref["dist"])))
    assert nk == 4127 > 4096 and nk % 32 and nk % 256 and len(sizes) == 64 and sizes[60:] == [9, 257, 1, 9]
    blocks = (nk + 255) // 256
    assert blocks == 17 and 63 * blocks == 1071 > 1024 and 60 * blocks + 4 == 1024      # k_fusem_compact's `before`, its 1025th count
    t, kp = ref["target"], ref["keep_pos"]
    counts = np.zeros((64, blocks), np.int64)
    np.add.at(counts, (t, kp // 256), 1)
    assert counts.reshape(-1)[1024] > 0 and counts.reshape(-1)[1024:].sum() >= 4          # what the second trip adds up
    assert all((t == m).any() for m in (60, 61, 62, 63)) and (kp >= 4096).sum() >= 2
    assert sorted(set((kp[t == 60] // ec.CHUNK).tolist())) == [0, 1, 2, 3, 4]               # all five passes of a target m > 0
    assert set(ec.WIDE_PASSES) <= set(kp[t == 60].tolist())
    assert len(st["dropped_a"]) > 0 and len(st["dropped_b"]) > 0


@pytest.mark.parametrize("nk", [4096, 4097])
def test_search_form_boundaries_have_pairs(nk):
    case = fm.random_case(3, nk)
    st = {}
    ref = ec.reference(case, st)
    assert len(case["keep"][0]) == nk and len(ref["dist"]) > 50 and len(st["dropped_a"]) > 0 and len(st["dropped_b"]) > 0
    # the last shape of the 64-thread form, the first of the 256-thread form (one landmark in its last workgroup); wide_64's
    # last workgroup holds 31 of 32
    assert ec.search_shape(nk) == {4096: (64, 512, 8), 4097: (256, 129, 1)}[nk] and ec.search_shape(ec.WIDE_NK) == (256, 129, 31)
    assert ref["keep_pos"].max() == nk - 1                           # a pair in that last workgroup


def test_big_targets_pair_beyond_the_strides():
    case = ec.big_targets()
    ref = ec.reference(case)
    rows = fm.rows_of(ref)
    assert [len(d[0]) for d in case["drops"]] == [1024, 1025, 2100, 0, 1] and len(case["keep"][0]) == 300
    assert all((ref["target"] == m).any() for m in (0, 1, 2, 4)) and not (ref["target"] == 3).any()
    for j, m, i in ec.BIG_PLANTS:
        assert (m, j, i, 2) in rows
    two = ref["drop_pos"][ref["target"] == 2]
    assert (two >= 1024).any() and (two >= 2048).any()
    assert rows[-1][0] == 4 and rows[-1][2] == 0                      # target 4's one landmark


def _candidates(case, m):
    """per keep landmark the number of in-frame landmarks of target m inside its window"""
    kw = case["kw"]
    xy, inside = fr.drop_keypoints(case["drops"][m][1], case["Rs"][m], case["ts"][m], kw["cam"], kw["width"], kw["height"])
    u, v, c2 = fm.gm.project(case["keep"][1], case["Rs"][m], case["ts"][m], kw["cam"])
    return [int((fm.gm.candidates(xy, u[j], v[j], c2[j], kw["width"], kw["height"], case["radius"]) & inside).sum()) for j in range(len(u))]


def test_crowded_windows_and_the_strict_ratio():
    case = ec.crowded()
    assert [len(d[0]) for d in case["drops"]] == [9, 3000, 1]
    assert _candidates(case, 1) == [ec.CROWD] * 3 and min(_candidates(case, 1)) >= 20
    st = {}
    rows = fm.rows_of(ec.reference(case, st))
    assert [r[:2] + r[3:] for r in rows] == [(1, 0, 2), (1, 2, 4)] and st["dropped_b"] == [(2, 0, 0, 5)]
    loose = fm.rows_of(ec.reference(case, ratio=1.01))
    assert [r[:2] + r[3:] for r in loose] == [(1, 0, 2), (1, 1, 5), (1, 2, 4)]
    dd, kd = case["drops"][1][0], case["keep"][0]
    for j in range(3):                                              # best and second best by (distance, position)
        d = fm.gm.hamming(dd, kd[j])
        order = np.lexsort((np.arange(len(d)), d))
        assert loose[j][2] == order[0] and [int(d[order[0]]), int(d[order[1]])] == [[2, 3], [5, 5], [4, 8]][j]
    assert fm.rows_of(ec.reference(case, ratio=0.5)) == [(2, 0, 0, 5)]                     # 4 < 0.5 * 8 is false
    nine = ec.crowded(d1=9)
    assert [r[:2] + r[3:] for r in fm.rows_of(ec.reference(nine, ratio=0.5))] == [(1, 2, 4), (2, 0, 5)]


@pytest.mark.parametrize("name", ec.KEY_EXTREMES)
def test_key_extremes(name):
    case = ec.key_extremes(name)
    assert len(case["drops"]) == 64 and fm.rows_of(ec.reference(case)) == case["expect"]
    if name == "d256":
        assert fm.gm.hamming(case["drops"][63][0][-1:], case["keep"][0][-1])[0] == 256
        assert (256 << 22 | 63 << 16 | (ec.PAD - 1)) < 1 << 31
    if name in ("d256", "d0", "positions"):
        return
    st = {}
    ec.reference(case, st)
    lost = st["dropped_a"] + st["dropped_b"]
    assert len(lost) == (0 if name == "d255" else 1) and (not lost or abs(lost[0][3] - case["expect"][0][3]) <= 1)


@functools.lru_cache(None)
def _chained(which):
    base = fm.random_case(3, 4097) if which == "boundary" else _dealt(*ec.DEALT[1])[0]
    return base, ec.relabelled(base, 300 + len(which))


@pytest.mark.parametrize("which", ["boundary", "dealt"])
def test_chained_ids_give_long_probes_and_the_same_positions(which):
    base, case = _chained(which)
    ids = np.concatenate([case["keep"][2]] + [d[2] for d in case["drops"]])
    assert 0 in ids and ec.TOP in ids
    k, d = ec.longest_probes(case)
    print("%s: longest probe %d in the keep table, %d in the drop table" % (which, k, d))
    assert k > 100 and d > 100
    a, b = ec.reference(base), ec.reference(case)
    assert fm.rows_of(a) == fm.rows_of(b) and len(a["dist"]) > 50
    assert b["keep_lid"].tolist() == case["keep"][2][b["keep_pos"]].tolist() != a["keep_lid"].tolist()


@pytest.mark.parametrize("big", [False, True])
def test_union_sides_have_capacity_above_their_count(big):
    u = ec.union_sides(big)
    store, case = ec.union_reference(u)
    for dst, src in ((ec.UNION_KEEP, u["keep_sources"]), (ec.UNION_TARGET, u["target_sources"])):
        assert len(store[dst][2]) < sum(len(u["store"][s][2]) for s in src)
    total = sum(len(u["store"][s][2]) for s in u["keep_sources"])
    assert (total > 1280 >= len(store[ec.UNION_KEEP][2])) == big
    st = {}
    ref = ec.reference(case, st)
    assert all((ref["target"] == m).any() for m in range(3)) and len(st["dropped_a"]) > 0 and len(st["dropped_b"]) > 0
    # what the slots hold between count and capacity would pair: on either side alone, a kernel that took the capacity for
    # the count gives another result
    stale, seen = ec.union_stale(u, case)
    assert all(len(e[0]) == 1280 for e in stale.values())
    for side in (dict(case, keep=seen["keep"]), dict(case, drops=seen["drops"])):
        assert len(side["keep"][0]) + len(side["drops"][0][0]) > len(case["keep"][0]) + len(case["drops"][0][0])
        assert fm.rows_of(ec.reference(side)) != fm.rows_of(ref)


@pytest.mark.parametrize("nk,sizes", ec.TIGHT)
def test_tight_cases_pair_every_landmark(nk, sizes):
    case = ec.tight(nk, sizes)
    ref = ec.reference(case)
    nd = sum(len(d[0]) for d in case["drops"])
    assert [len(d[0]) for d in case["drops"]] == sizes and len(ref["dist"]) == min(nk, nd)
    assert (nk == 1280 and nd == nk) or nd < nk
    if nd < nk:
        assert sorted(zip(ref["target"].tolist(), ref["drop_pos"].tolist())) == [(m, i) for m, n in enumerate(sizes) for i in range(n)]
    else:
        assert ref["keep_pos"].tolist() != sorted(ref["keep_pos"].tolist()) and sorted(ref["keep_pos"].tolist()) == list(range(nk))
