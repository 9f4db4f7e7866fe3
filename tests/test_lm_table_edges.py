"""The landmark-id table's edges without a GPU: tests/lm_table_ref.py's numpy hash and bucket count against the functions of
csrc/lm_table.hpp themselves, compiled into a small host program; and, from the references alone, that every case of
tests/lm_table_cases.py and every new case of tests/fuse_ref.py reaches the path tests/test_gpu_lm_table_edges.py and
tests/test_gpu_fuse_edges.py name it after — chain lengths, the wrap from the last bucket to bucket 0, keys behind foreign
keys, block counts, winners beyond a pass of the block scan, pairs beyond a pass of the resolution.  A restatement that were
silently wrong would leave those GPU tests ordinary random-id tests that pass."""
import os
import subprocess

import numpy as np
import pytest

import fuse_ref as fr
import lm_table_cases as lc
import lm_table_ref as lt
import local_map_ref as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modular-slam_amd", "csrc")

PROGRAM = r"""
#include "lm_table.hpp"
#include <cstdio>
int main(int argc, char** argv)
{
    FILE* f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if(!f)
        return 2;
    unsigned long long x;
    while(fread(&x, 8, 1, f) == 1)
        printf("h %016llx\n", mslam::lm_hash(x));
    fclose(f);
    for(int a = 2; a < argc; ++a)
    {
        const size_t keys = (size_t)strtoull(argv[a], nullptr, 10);
        printf("b %zu %zu\n", keys, mslam::lm_bucket_count(keys));
    }
    return 0;
}
"""


# ---- the restatement against the header ------------------------------------------------------------------------------------

def test_numpy_hash_and_bucket_count_equal_the_compiled_header(tmp_path):
    rng = np.random.default_rng(0)
    crafted = np.concatenate([lt.colliding(2000, seed=1), lt.ids_with_hash_low(np.arange(64), seed=2),
                              lt.colliding(200, seed=3, below=1 << 63, at_least=1 << 62),
                              lt.ids_with_hash_low(rng.integers(0, 1 << 16, 500), seed=4)])
    ids = np.concatenate([crafted, rng.integers(0, 1 << 63, 1000, dtype=np.int64), [0, (1 << 63) - 1, 1, 1 << 62, (1 << 62) - 1]])
    keys = [0, 1, 5, 31, 32, 33, 64, 160, 255, 256, 257, 320, 512, 513, 600, 1050, 2304, 4500, 32768, 32769, 65535, 1 << 24]
    src, exe, data = tmp_path / "lm_hash_host.cpp", tmp_path / "lm_hash_host", tmp_path / "ids.bin"
    src.write_text(PROGRAM)
    ids.astype("<u8").tofile(str(data))
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-O2", "-x", "hip", "--offload-host-only",
                           "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe), str(data)] + [str(k) for k in keys], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split("\n")
    got = np.array([int(l.split()[1], 16) for l in lines if l.startswith("h ")], np.uint64)
    assert len(got) == len(ids) and np.array_equal(got, lt.lm_hash(ids))
    assert [tuple(int(x) for x in l.split()[1:]) for l in lines if l.startswith("b ")] == [(k, lt.lm_bucket_count(k)) for k in keys]
    # and the crafted ids are what they are made to be, by the header's own hash
    n = 2000
    assert np.all(got[:n] & np.uint64(0xFFFF) == 0xFFFF) and np.array_equal(got[n:n + 64] & np.uint64(0xFFFF), np.arange(64, dtype=np.uint64))
    assert np.all(got[n + 64:n + 264] & np.uint64(0xFFFF) == 0xFFFF) and crafted[n + 64:n + 264].min() >= 1 << 62
    assert crafted[:n + 64].max() < 1 << 62 and len(np.unique(crafted[:n])) == n


def test_inverse_and_sequential_insert():
    rng = np.random.default_rng(1)
    x = rng.integers(0, 1 << 63, 1000, dtype=np.int64).astype(np.uint64)
    assert np.array_equal(lt.lm_unhash(lt.lm_hash(x)), x) and np.array_equal(lt.lm_hash(lt.lm_unhash(x)), x)
    assert lt.lm_hash([1]).tolist() != [1] and len(np.unique(lt.lm_hash(np.arange(1000)))) == 1000
    # three keys of home 63 in a table of 64, one of home 0: buckets 63, 0, 1 and the displaced key behind them
    ids = np.concatenate([lt.ids_with_hash_low([63, 63, 63], seed=5), lt.ids_with_hash_low([0], seed=6), ])
    bucket, steps = lt.occupied(np.concatenate([ids, ids[:1]]), 64)
    assert bucket.tolist() == [63, 0, 1, 2, 63] and steps.tolist() == [0, 1, 2, 2, 0]
    b2, _ = lt.occupied(ids[::-1], 64)
    assert sorted(b2.tolist()) == sorted(bucket[:4].tolist())          # the occupied set does not depend on the order


# ---- one chain ---------------------------------------------------------------------------------------------------------------

def _run_from_last(bucket, buckets):
    """the occupied buckets are one run that starts at the last bucket and wraps -> its length"""
    occ = set(bucket.tolist())
    assert occ == {(buckets - 1 + s) % buckets for s in range(len(occ))}, sorted(occ)[:5]
    return len(occ)


@pytest.mark.parametrize("share", lc.SHARES)
def test_chain_pair_is_one_wrapping_chain_in_both_calls_tables(share):
    store, lids = lc.chain_pair(share)
    assert len(lids[1]) == len(lids[2]) == 160 and lm.covisible(lids, 1, [2])[0] == share
    # the union's table: sized by the sum of the entries' counts, whatever they share
    buckets, bucket, steps = lc.table_of(np.concatenate([lids[1], lids[2]]), 320)
    assert buckets == 1024 and _run_from_last(bucket, buckets) == 320 - share
    assert steps.max() == 320 - share - 1 and {buckets - 1, 0} <= set(bucket.tolist())
    assert share != 0 or steps.max() >= 300
    # covisible's table holds entry `id` alone
    for own in (1, 2):
        buckets, bucket, steps = lc.table_of(lids[own])
        assert buckets == 512 and _run_from_last(bucket, buckets) == 160 and steps.max() == 159


@pytest.mark.parametrize("share", lc.SHARES)
def test_displaced_keys_have_their_homes_inside_the_chain(share):
    store, lids = lc.chain_pair(share, displaced=True)
    every = np.unique(np.concatenate([lids[1], lids[2]]))
    assert len(every) == 320 - share and lm.covisible(lids, 1, [2])[0] == share
    for keys, count, buckets in ((np.concatenate([lids[1], lids[2]]), 320, 1024), (lids[1], 160, 512), (lids[2], 160, 512)):
        home = lt.home(keys, buckets)
        chain, plain = np.unique(keys[home == buckets - 1]), np.unique(keys[home != buckets - 1])
        assert len(chain) >= 70 and len(plain) >= 70 and set(home[home != buckets - 1].tolist()) <= set(range(64))
        # the chain's keys alone cover buckets 0 .. 63, the homes of all the others: whichever thread comes first, a key of
        # the one kind sits behind keys of the other, and the table is one run from the last bucket on
        assert len(chain) - 1 >= 64
        b, bucket, steps = lc.table_of(keys, count)
        assert b == buckets and _run_from_last(bucket, buckets) == len(chain) + len(plain)
        first = lt.occupied(np.concatenate([chain, plain]), buckets)[1]    # the chain's threads first: every other key is behind
        assert first[len(chain):].min() > 0 and first[len(chain):].max() >= len(chain)
        last = lt.occupied(np.concatenate([plain, chain]), buckets)[1]     # the others first: the chain runs through them
        assert (last[len(plain):] > 0).sum() >= len(chain) - 1 and last[len(plain):].max() >= len(chain) + 63
        assert steps.max() >= 100 and (steps[home != buckets - 1] > 0).sum() > 10   # in list order: some of each


def test_contended_entries_race_on_one_chain():
    store, lids, orders = lc.contended()
    assert len(lids) == 64 and len(orders) == 3 and all(sorted(o) == orders[0] for o in orders) and orders[2] != orders[0]
    five = set(lids[orders[0][0]].tolist())
    assert len(five) == 5 and all(set(l.tolist()) == five and len(l) == 5 for l in lids.values())
    assert len({tuple(l.tolist()) for l in lids.values()}) == 5        # the positions differ from entry to entry
    buckets, bucket, steps = lc.table_of(np.concatenate([lids[i] for i in orders[0]]))
    assert buckets == 1024 and _run_from_last(bucket, buckets) == 5 and steps.max() == 4
    top = max(lids)
    for o in orders:
        d, w, l = lm.union(store, lids, o)
        assert np.array_equal(l, lids[top]) and np.array_equal(d, store[top][0])
    assert orders[2].index(top) not in (0, 63)


def test_repeats_sit_on_a_chain():
    store, lids = lc.repeats()
    a, b = lids[1], lids[2]
    assert a[39] == a[0] and a[25] == a[20] not in b and b[29] == b[2] and b[7] == b[0] == a[0]
    buckets, bucket, steps = lc.table_of(np.concatenate([a, b]))
    assert _run_from_last(bucket, buckets) == len(np.unique(np.concatenate([a, b]))) == 52 and steps.max() == 51
    l12, l21 = lm.union(store, lids, [1, 2])[2], lm.union(store, lids, [2, 1])[2]
    assert len(l12) == len(l21) == 52
    assert lm.covisible(lids, 1, [1, 2]).tolist() == [38, 14] and lm.covisible(lids, 2, [1, 2]).tolist() == [14, 28]
    # the higher position of a repeat wins: entry 2's id b[0] is taken at position 7, entry 1's own a[20] at position 25
    d = lm.union(store, lids, [1, 2])[0]
    assert np.array_equal(d[np.flatnonzero(l12 == b[0])[0]], store[2][0][7])
    assert np.array_equal(d[np.flatnonzero(l12 == a[20])[0]], store[1][0][25])


# ---- lists longer than the store ---------------------------------------------------------------------------------------------

def test_update_world_list_is_one_chain_longer_than_the_store():
    store, lids, ids, xyz = lc.update_world_case()
    assert len(ids) == 1050 > 256 and len(ids) > lc.K and len(np.unique(ids)) == 1000
    held = set(np.concatenate(list(lids.values())).tolist()) & set(ids.tolist())
    assert len(held) == 300 and len(ids) - len(np.unique(ids)) == 50
    buckets, bucket, steps = lc.table_of(ids)
    assert buckets == 4096 and len(set(bucket.tolist())) == 1000 and steps.max() >= 997 and {4095, 0, 996} <= set(bucket.tolist())
    assert {0, (1 << 62) - 1} <= held and lt.home([0], buckets)[0] == 0      # id 0 hashes to 0: its home is inside the chain
    # store ids the list does not hold walk the whole chain to its empty end
    missing = set(np.concatenate(list(lids.values())).tolist()) - set(ids.tolist())
    on_chain = [m for m in missing if lt.home([m], buckets)[0] == buckets - 1]
    assert len(on_chain) == 100 and len(missing) == 120 and all(len(l) <= lc.K for l in lids.values())


def test_replace_lists_reach_the_top_of_the_id_range():
    store, calls = lc.replace_case()
    (f1, t1, x1), (f2, t2, x2) = calls
    assert x1 is None and x2.shape == (600, 3) and len(f1) == len(f2) == 600 > lc.K
    assert all(len(e[2]) <= lc.K and e[2].max() < 1 << 62 for e in store.values())
    buckets, bucket, steps = lc.table_of(f1)
    assert buckets == 2048 and len(np.unique(f1)) == 550 and steps.max() >= 540 and {2047, 0} <= set(bucket.tolist())
    assert {1 << 62, lc.TOP, 0} <= set(t1.tolist()) and lc.TOP in f1.tolist()
    h = store[5][2]
    swap = [(int(a), int(b)) for a, b in zip(f1, t1) if (int(b), int(a)) in set(zip(f1.tolist(), t1.tolist()))]
    assert len(swap) == 2 and all(a in h.tolist() for a, _ in swap)
    mid, n1 = fr.replace_ids(store, f1, t1)
    after = np.concatenate([e[2] for e in mid.values()])
    assert n1 > 300 and {1 << 62, lc.TOP, 0} <= set(after.tolist()) and (after >= 1 << 62).sum() > 200
    # the second list's `from` ids are what the first one wrote: top-range ids on a chain, 2^63 - 1, 2^62 and 0
    _, b2, s2 = lc.table_of(f2)
    assert s2.max() >= 590 and len(np.unique(f2)) == 600
    end, n2 = fr.replace_ids(mid, f2, t2, x2)
    assert n2 > 200 and {lc.TOP, 1 << 62, 0} <= set(f2.tolist())
    last = np.concatenate([e[2] for e in end.values()])
    assert 0 not in last.tolist() and 7 in last.tolist() and lc.TOP in last.tolist()      # 2^63 - 1 -> 7 and 2^62 -> 2^63 - 1 at once


def test_fusion_case_collides_on_every_table():
    case, store = lc.fusion_case()
    kl, dl = case["keep"][2], case["drop"][2]
    assert len(kl) == 300 and len(dl) == 280 and len(set(kl.tolist()) & set(dl.tolist())) == 40
    for keys in (kl, dl):
        buckets, bucket, steps = lc.table_of(keys)
        assert buckets == 1024 and _run_from_last(bucket, buckets) == len(keys) and steps.max() == len(keys) - 1
    k_ok, d_ok = fr.eligible(kl, dl)
    assert (~k_ok).sum() == 40 and (~d_ok).sum() == 40
    pairs, new, n = fr.fuse(store, 10, 20, radius=case["radius"], **case["kw"])
    assert len(pairs["keep_pos"]) > 50 and n > len(pairs["keep_pos"])
    _, bucket, steps = lc.table_of(pairs["drop_lid"], min(300, 280))                       # kf_fuse's replacement table
    assert steps.max() == len(pairs["drop_lid"]) - 1
    assert new[30][1].tobytes() != fr.entry(*store[30])[1].tobytes()                       # the third entry is rewritten


# ---- unions of more than 256 blocks ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nb", sorted(lc.BLOCKS))
def test_union_block_counts_and_winners_beyond_a_pass(nb):
    k_max, store, lids, orders, bx = lc.union_blocks(nb)
    n, n_large = len(orders[0]), len(lids[lc.LARGE])
    assert n * bx == nb and (n, k_max) == {256: (64, 1024), 258: (43, 1536), 576: (64, 2304)}[nb]
    assert (bx - 1) * 256 < n_large <= bx * 256 <= k_max and max(len(lids[i]) for i in orders[0] if i != lc.LARGE) <= 40
    assert min(len(l) for l in lids.values()) == 0 and orders[0][-1] == lc.LARGE and orders[1] != orders[0]
    for o in orders:
        blocks = lc.winner_blocks(lids, o, bx)
        ref = lm.union(store, lids, o)
        assert len(blocks) == len(ref[2]) <= k_max and len(ref[2]) > n_large
        at = o.index(lc.LARGE)
        large = blocks[(blocks >= at * bx) & (blocks < (at + 1) * bx)]
        assert len(set(large.tolist())) == bx and 256 < len(large) < n_large      # it wins in all its blocks, and loses some
        empty = set(range(nb)) - set(blocks.tolist())
        if o is orders[0] and nb > 256:                                           # the large entry last: beyond block 256
            assert at * bx < 256 <= (at + 1) * bx - 1 or at * bx >= 512
            assert (blocks >= 256).sum() > 100 and min(empty) < 256               # counts of 0 before them
        if o is orders[0] and nb > 512:
            assert (blocks >= 512).sum() > 100 and ((blocks >= 256) & (blocks < 512)).sum() > 10 and any(256 <= e < 512 for e in empty)
        if o is orders[1] and nb > 512:                                           # its blocks straddle the first pass's end
            assert at * bx < 256 <= (at + 1) * bx - 1 and (blocks >= 256).sum() > 100 and (blocks >= 512).sum() > 10


def test_growth_sequence_block_counts():
    k_max, store, lids, calls = lc.growth()
    assert [nb for _, nb in calls] == [2, 576, 2, 258] and calls[0][0] == calls[2][0] and k_max == 2304
    for o, nb in calls:
        bx = max((max(len(lids[i]) for i in o) + 255) // 256, 1)
        assert bx * len(o) == nb and len(lm.union(store, lids, o)[2]) <= k_max
    assert len(lm.union(store, lids, calls[0][0])[2]) > 2
    o, nb = calls[3]
    assert (lc.winner_blocks(lids, o, 6) >= 256).sum() > 100


# ---- fusion: passes of the resolution, frames, a real pose ---------------------------------------------------------------------

def test_old_sizes_are_what_they_were():
    for nk, nd in ((7, 40), (257, 255), (3, 3000)):
        a = fr.sized_case(nk, nd)
        b = fr.random_case(100 + nk + nd, nk, nd, shared=3 if min(nk, nd) > 30 else 1 if min(nk, nd) > 3 else 0)
        assert all(x.tobytes() == y.tobytes() for s in ("keep", "drop") for x, y in zip(a[s], b[s])) and a["planted"] == []


@pytest.mark.parametrize("nk,nd", fr.CHUNK_SIZES)
def test_resolution_passes_hold_many_pairs(nk, nd):
    case = fr.sized_case(nk, nd)
    assert set(fr.CHUNK_SIZES) <= set(fr.SIZES) and fr.CHUNK == 1024
    got = fr.search(case["keep"], case["drop"], radius=case["radius"], **case["kw"])
    kp = got["keep_pos"]
    print("%d x %d: %d pairs, %d from 1024 on, %d from 2048 on" % (nk, nd, len(kp), (kp >= 1024).sum(), (kp >= 2048).sum()))
    assert (kp < 1024).sum() >= 500
    # every keep position beyond the first pass that the size has, up to 50, holds a pair
    assert (kp >= 1024).sum() >= min(50, nk - 1024)
    assert (kp >= 2048).sum() >= min(50, max(nk - 2048, 0))
    if nk == 1024:
        assert (kp >= 960).sum() >= 50                                   # the first pass's last wave is full of them
    if nk == 1025:
        assert kp[-1] == 1024                                            # one pair, placed behind the first pass's hundreds
    if nk > 2048:
        # drop positions claimed from two passes, with both outcomes: what each keep landmark accepts on its own, and who keeps it
        acc = fr.accepted(case["keep"], case["drop"], radius=case["radius"], **case["kw"])
        rows = dict(zip(got["drop_pos"].tolist(), kp.tolist()))
        assert len(case["planted"]) == 4
        for b, a, i, winner in case["planted"]:
            assert b < 1024 <= a and acc[b] is not None and acc[a] is not None and acc[b][0] == acc[a][0] == i and rows[i] == winner
            assert (min((acc[b][1], b), (acc[a][1], a))[1]) == winner
        assert {a // 1024 for _, a, _, w in case["planted"] if w == a} == {1, 2} and any(w == b for b, _, _, w in case["planted"])


@pytest.mark.parametrize("width,height", fr.FRAMES)
def test_frames_and_radii_have_pairs(width, height):
    radii = fr.frame_radii(width, height)
    assert radii[:3] == [0.5, 15.0, 47.5] and radii[3] == max(width, height) + 10
    for nk, nd in fr.FRAME_SIZES:
        case = fr.frame_case(nk, nd, width, height)
        n = [len(fr.search(case["keep"], case["drop"], radius=r, **case["kw"])["keep_pos"]) for r in radii]
        print("%d x %d, %d / %d: pairs per radius %s" % (width, height, nk, nd, n))
        assert sum(n) >= 1 and n[0] >= 1                                 # the duplicates lie inside the smallest radius
        # brute force: every eligible drop landmark in the frame is inside the window of every keep landmark in front
        kw = case["kw"]
        xy, d_in = fr.drop_keypoints(case["drop"][1], kw["R"], kw["t"], kw["cam"], width, height)
        u, v, c2 = fr.gm.project(case["keep"][1], kw["R"], kw["t"], kw["cam"])
        j = int(np.argmax(u))
        assert np.array_equal(fr.gm.candidates(xy, u[j], v[j], c2[j], width, height, radii[3]), d_in) and 0 < d_in.sum() <= nd


@pytest.mark.parametrize("nk,nd", fr.POSED_SIZES)
def test_posed_case_has_pairs_and_a_gate_that_bites(nk, nd):
    case = fr.posed_case(40 + nk, nk, nd, shared=5)
    kw = case["kw"]
    assert kw["cam"] == fr.gm.CAM and kw["max_world_distance"] == 0.05
    assert np.abs(kw["R"] - np.eye(3)).max() > 0.1 and np.allclose(kw["R"] @ kw["R"].T, np.eye(3), atol=1e-12) and np.abs(kw["t"]).min() > 0.1
    z = fr.gm.project(case["keep"][1], kw["R"], kw["t"], kw["cam"])[2]
    assert 0.49 < z.min() < 0.7 and 3.5 < z.max() < 4.01                 # depths of 0.5 .. 4 m, not Z = 1
    got = fr.search(case["keep"], case["drop"], radius=case["radius"], **kw)
    open_ = fr.search(case["keep"], case["drop"], radius=case["radius"], **dict(kw, max_world_distance=np.inf))
    alone = fr.gate_alone(case)
    print("posed %d / %d: %d pairs, %d without the gate, %d candidates rejected by the gate alone" % (
        nk, nd, len(got["keep_pos"]), len(open_["keep_pos"]), len(alone)))
    assert len(got["keep_pos"]) >= 30 and len(alone) >= 1
    assert list(zip(got["keep_pos"].tolist(), got["drop_pos"].tolist())) != list(zip(open_["keep_pos"].tolist(), open_["drop_pos"].tolist()))
    assert nk <= 1024 or got["keep_pos"][-1] >= 1024 or (got["keep_pos"] >= 960).sum() > 5
