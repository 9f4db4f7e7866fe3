"""The landmark-id table of csrc/lm_table.hpp on the MI355X, driven where small consecutive ids never take it: probe chains of
hundreds of keys that wrap from the last bucket to bucket 0, keys found behind foreign keys, 64 list positions racing on one
chain, lists longer than the store, ids at the top of the allowed range; and unions of 256, 258 and 576 blocks, where the
block scan takes a second and third pass and the block buffer grows.  Every case comes from tests/lm_table_cases.py, and
tests/test_lm_table_edges.py proves on the CPU that it reaches the path it is named after.  Everything is compared exactly
with tests/local_map_ref.py, tests/fuse_ref.py and the update_world restatement of tests/test_gpu_ba.py: these calls are
pure functions of ids, positions and integer distances."""
import numpy as np
import pytest

import fuse_ref as fr
import lm_table_cases as lc
import local_map_ref as lm
from test_gpu_ba import _update_ref
from test_gpu_fuse import _args, _same_pairs, _same_store
from test_gpu_local_map import _check_union, _fill, _read, _same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(width=0, height=0, max_keypoints=lc.K)
    yield c
    c.close()


def _refill(c, store, lids):
    c.kf_clear()
    _fill(c, store, lids)


def _covisible(c, lids, ids):
    for own in ids:
        assert np.array_equal(c.kf_covisible(own, ids), lm.covisible(lids, own, ids)), own
        assert np.array_equal(c.kf_covisible(own, ids[::-1]), lm.covisible(lids, own, ids[::-1])), own


# ---- one chain -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("displaced", [False, True], ids=["chain", "displaced"])
@pytest.mark.parametrize("share", lc.SHARES)
def test_union_and_covisible_on_one_wrapping_chain(ctx, share, displaced):
    store, lids = lc.chain_pair(share, displaced)
    _refill(ctx, store, lids)
    for order in ([1, 2], [2, 1]):
        ref = _check_union(ctx, store, lids, order, what=(share, displaced, order))
        assert len(ref[2]) == 320 - share
    _covisible(ctx, lids, [1, 2])
    assert ctx.kf_covisible(1, [1, 2]).tolist() == [160, share]
    for i in (1, 2):                                                   # the sources are untouched
        _same(_read(ctx, i), (store[i][0], store[i][1], lids[i]), i)


def test_sixty_four_list_positions_race_on_one_chain(ctx):
    store, lids, orders = lc.contended()
    _refill(ctx, store, lids)
    top = max(lids)
    for order in orders:
        ref = _check_union(ctx, store, lids, order, what="contended")
        assert np.array_equal(ref[0], store[top][0]) and np.array_equal(ref[2], lids[top])
        got = _read(ctx, 900)
        assert got[1].tobytes() == store[top][1].tobytes()             # every id takes the largest entry's observation
    for own in (orders[2][0], top):
        assert np.array_equal(ctx.kf_covisible(own, orders[2]), lm.covisible(lids, own, orders[2]))
        assert ctx.kf_covisible(own, orders[2]).tolist() == [5] * 64


def test_repeats_inside_entries_on_a_chain(ctx):
    store, lids = lc.repeats()
    _refill(ctx, store, lids)
    for order in ([1, 2], [2, 1], [1], [2]):
        _check_union(ctx, store, lids, order, what=order)
    _covisible(ctx, lids, [1, 2])
    assert ctx.kf_covisible(1, [1, 2, 1]).tolist() == [38, 14, 38]


# ---- lists longer than the store --------------------------------------------------------------------------------------------

def test_update_world_with_a_colliding_list_longer_than_the_store(ctx):
    store, lids, ids, xyz = lc.update_world_case()
    _refill(ctx, store, lids)
    ref, n = _update_ref({k: (lids[k], store[k][1]) for k in store}, ids, xyz)
    assert ctx.kf_update_world(ids, xyz) == n == 300 + 200 + 2 + 5
    for k, (l, w) in ref.items():
        got = _read(ctx, k)
        assert np.array_equal(got[2], l) and np.array_equal(got[0], store[k][0]), k
        assert got[1].tobytes() == w.tobytes(), k
    assert ref[4][1].tobytes() != store[4][1].tobytes()


def test_replace_ids_with_colliding_lists_and_the_top_of_the_range(ctx):
    store, calls = lc.replace_case()
    ctx.kf_clear()
    for i, (d, w, l) in store.items():
        ctx.kf_add(i, d, w, l)
    for step, (f, t, xyz) in enumerate(calls):
        store, n = fr.replace_ids(store, f, t, xyz)
        assert ctx.kf_replace_ids(f, t, xyz) == n > 200, step
        _same_store(ctx, store, step)
    # and 2^63 - 1 as `from` and `to` of one short list: both entries hold each of the two ids once
    f, t = np.array([lc.TOP, 7], np.int64), np.array([3, lc.TOP], np.int64)
    store, n = fr.replace_ids(store, f, t)
    assert ctx.kf_replace_ids(f, t) == n == 4
    _same_store(ctx, store, "top")


def test_fusion_eligibility_on_colliding_ids(ctx):
    case, store = lc.fusion_case()
    ref = fr.search(case["keep"], case["drop"], radius=case["radius"], **case["kw"])
    ctx.kf_clear()
    for i, e in store.items():
        ctx.kf_add(i, *fr.entry(*e))
    _same_pairs(ctx.kf_fuse_search(10, 20, **_args(case)), ref, "search")
    _same_store(ctx, store, "search changes nothing")
    assert ctx.kf_covisible(10, [20, 30]).tolist() == [40, int(lm.covisible({k: e[2] for k, e in store.items()}, 10, [30])[0])]
    pairs, new, n = fr.fuse(store, 10, 20, radius=case["radius"], **case["kw"])
    got = ctx.kf_fuse(10, 20, **_args(case))
    _same_pairs(got, ref, "fuse")
    assert got["n_rewritten"] == n > len(ref["keep_pos"]) > 50
    _same_store(ctx, new, "fuse")
    assert ctx.kf_covisible(10, [20]).tolist() == [40 + len(ref["keep_pos"])]


# ---- unions of more than 256 blocks ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nb", sorted(lc.BLOCKS))
def test_union_block_counts(pkg, nb):
    k_max, store, lids, orders, bx = lc.union_blocks(nb)
    c = pkg.Context(width=0, height=0, max_keypoints=k_max)
    _fill(c, store, lids)
    for order in orders:
        ref = _check_union(c, store, lids, order, what=(nb, order.index(lc.LARGE)))
        assert len(ref[2]) == len(lc.winner_blocks(lids, order, bx))
    c.kf_union(901, orders[0], sync=False)                             # the _dev form takes the same passes
    c.sync()
    _same(_read(c, 901), lm.union(store, lids, orders[0]), "dev")
    c.close()


def test_block_buffer_grows_and_is_laid_out_again(pkg):
    k_max, store, lids, calls = lc.growth()
    c = pkg.Context(width=0, height=0, max_keypoints=k_max)
    _fill(c, store, lids)
    seen = []
    for order, nb in calls:
        _check_union(c, store, lids, order, what=nb)
        seen.append(_read(c, 900))
    for a, b in zip(seen[0], seen[2]):                                 # the small union after the large one is the one before it
        assert a.tobytes() == b.tobytes()
    c.close()
