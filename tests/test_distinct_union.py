"""The union's DISTINCTIVE descriptor mode without a GPU: the ABI and the Python surface; the properties of
tests/distinct_ref.py's restatement; the per-lane pieces of csrc/distinct.hpp, compiled into a small host program, against
that restatement; and, from the references alone, that every case of tests/distinct_cases.py is what
tests/test_gpu_distinct_union.py names it after."""
import os
import re
import subprocess

import numpy as np
import pytest

import distinct_cases as dc
import distinct_ref as dr
import local_map_ref as lm
import lm_table_ref as lt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modular-slam_amd", "csrc")


# ---- the surface ---------------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_exported_and_the_version_stays(pkg):
    hdr = open(os.path.join(ROOT, "include", "mslam_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("mslam_hip_set_union_descriptor", "mslam_hip_get_union_descriptor"):
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in pkg.ABI_SYMBOLS and hasattr(pkg.lib(), name), name
    assert re.search(r"#define MSLAM_HIP_UNION_DESC_RECENT 0\b", code) and re.search(r"#define MSLAM_HIP_UNION_DESC_DISTINCTIVE 1\b", code)
    assert re.search(r"#define MSLAM_HIP_ABI_VERSION 5\b", code) and pkg.lib().mslam_hip_abi_version() == 5
    assert (pkg.UNION_DESC_RECENT, pkg.UNION_DESC_DISTINCTIVE) == (0, 1)
    # the header says what deviates from ORB-SLAM
    text = hdr[hdr.index("Which descriptor a union row carries"):hdr.index("int mslam_hip_set_union_descriptor")]
    assert text.count("DEVIATES") >= 3 and "UpdateNormalAndDepth" in text and "ComputeDistinctiveDescriptors" in text


class _FakeContext:
    def __init__(self):
        self.modes = []

    def set_union_descriptor(self, mode):
        self.modes.append(mode)


def test_tracker_option_validates_its_arguments(pkg):
    with pytest.raises(pkg.MslamHipError) as e:
        pkg.HipKeyframeTracker(_FakeContext(), union_descriptor="distinctive")              # no local map to apply it to
    assert e.value.code == pkg.E_INVALID
    for bad in ("median", 2, ""):
        c = _FakeContext()
        with pytest.raises(pkg.MslamHipError) as e:
            pkg.HipKeyframeTracker(c, local_map_depth=2, union_descriptor=bad)
        assert e.value.code == pkg.E_INVALID and c.modes == []
    for mode in ("distinctive", "recent"):
        c = _FakeContext()
        pkg.HipKeyframeTracker(c, local_map_depth=2, union_descriptor=mode)
        assert c.modes == [mode]
    c = _FakeContext()
    pkg.HipKeyframeTracker(c, local_map_depth=2)                                            # None: the context's mode is left alone
    pkg.HipKeyframeTracker(c)
    assert c.modes == []
    doc = " ".join(pkg.HipKeyframeTracker.__doc__.split())
    assert "NOT MEASURED" in doc.split("union_descriptor =")[1].split("lm_cull = True")[0]
    assert "the descriptors of a pair are not merged" not in doc and "follow the context's union descriptor mode" in doc


# ---- the reference's properties -------------------------------------------------------------------------------------------------

def _random_store(seed, n_entries=9, pool=120, per_entry=60):
    rng = np.random.default_rng(seed)
    held = {int(i): 100 + rng.permutation(pool)[:per_entry] for i in rng.permutation(50)[:n_entries]}
    return dc.observed(rng, held) + (rng,)


def test_rows_of_one_or_two_observations_equal_the_recent_union():
    store, lids, rng = _random_store(1)
    ids = sorted(store)
    for order in (ids[:1], ids[:2], ids[1::-1], ids[3:5]):
        got, ref = dr.union(store, lids, order), lm.union(store, lids, order)
        assert all(np.array_equal(a, b) for a, b in zip(got, ref)), order
    got, ref = dr.union(store, lids, ids), lm.union(store, lids, ids)
    n = dr.counts(lids, ids, ref[2])
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
    assert np.array_equal(got[0][n <= 2], ref[0][n <= 2]) and (n <= 2).sum() > 0
    differ = (got[0] != ref[0]).any(axis=1)
    assert differ.sum() > 10 and n[differ].min() >= 3                     # and the mode is no restatement of the recent one


def test_choice_is_invariant_under_a_permutation_of_the_list():
    store, lids, rng = _random_store(2)
    ids = sorted(store)
    first = dr.choose(store, lids, ids)
    for _ in range(4):
        order = [int(i) for i in rng.permutation(ids)]
        assert dr.choose(store, lids, order) == first
        d, w, l = dr.union(store, lids, order)
        for r, x in enumerate(l.tolist()):
            kf, i, _ = first[x]
            assert np.array_equal(d[r], store[kf][0][i])


def test_ties_and_the_nine_bit_median():
    store, lids, order, winners = dc.ties()
    chosen = dr.choose(store, lids, order)
    assert {l: chosen[l][0] for l in winners} == winners
    assert [chosen[l][2] for l in (dc.SAME, dc.AABB, dc.AAABB, dc.EXTREME)] == [5, 4, 5, 3]
    # the extremes: all-zeros against two all-ones is 256 away from both, which eight bits cannot hold
    assert dr.hamming(dc.ZERO, dc.ONES) == 256 and dr.medians([dc.ONES, dc.ONES, dc.ZERO]) == [0, 0, 256]
    assert dr.key(256, 63) == 16384 > dr.key(255, 0) and dr.key(256 & 0xFF, 63) == 0
    d, _, l = dr.union(store, lids, order)
    assert np.array_equal(d[np.flatnonzero(l == dc.EXTREME)[0]], dc.ONES)
    assert np.array_equal(lm.union(store, lids, order)[0][np.flatnonzero(l == dc.EXTREME)[0]], dc.ZERO)
    # A, A, A, B, B: the most recent A although both B are more recent
    a = store[30][0][np.flatnonzero(lids[30] == dc.AAABB)[0]]
    assert np.array_equal(d[np.flatnonzero(l == dc.AAABB)[0]], a)
    assert not np.array_equal(lm.union(store, lids, order)[0][np.flatnonzero(l == dc.AAABB)[0]], a)


# ---- csrc/distinct.hpp against the restatement ---------------------------------------------------------------------------------

PROGRAM = r"""
#include "distinct.hpp"
#include <cstdio>
#include <cstring>
#include <vector>
// input: records of [u32 n | n x 32 descriptor bytes | n x u32 rank].  Per record, the kernel's steps on the header's
// pieces: column c of lane a = the distance to observation c (stored [c][lane], 64 lanes apart), each lane's median, the
// least key -> "c <n> <winner> <median of the winner> <key>", and every lane's median -> "m ..."
int main(int argc, char** argv)
{
    FILE* f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if(!f)
        return 2;
    uint32_t n;
    while(fread(&n, 4, 1, f) == 1)
    {
        if(n < 1 || n > 64)
            return 3;
        std::vector<uint32_t> desc(n * 8), rank(n);
        if(fread(desc.data(), 32, n, f) != n || fread(rank.data(), 4, n, f) != n)
            return 4;
        std::vector<uint16_t> dist(64 * 64, 0xFFFF);
        for(uint32_t a = 0; a < n; ++a)
            for(uint32_t c = 0; c < n; ++c)
                dist[c * 64 + a] = (uint16_t)mslam::distinct_distance(&desc[a * 8], &desc[c * 8]);
        uint32_t best = mslam::kDistinctAbsent, winner = 0, median = 0;
        printf("m");
        for(uint32_t a = 0; a < n; ++a)
        {
            const uint32_t m = mslam::distinct_mth_smallest(&dist[a], 64, (int)n, ((int)n - 1) / 2);
            const uint32_t key = mslam::distinct_key(m, (int)rank[a]);
            printf(" %u", m);
            if(key < best)
                best = key, winner = a, median = m;
        }
        printf("\nc %u %u %u %u\n", n, winner, median, best);
    }
    fclose(f);
    return 0;
}
"""


def _records():
    """every N from 1 to 64: noisy copies of a base (as real observations are), uniformly random descriptors, and rows made
    of all-zeros and all-ones only (distances 0 and 256); ranks are a permutation of 0 .. 63 cut to N"""
    rng = np.random.default_rng(7)
    out = []
    for n in range(1, 65):
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        noisy = np.array([dc.flipped(rng, base, int(rng.integers(0, 41))) for _ in range(n)], np.uint8)
        uniform = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        ends = np.where(rng.integers(0, 2, (n, 1)).astype(bool), dc.ONES[None], dc.ZERO[None]).astype(np.uint8)
        few = noisy.copy()
        few[rng.integers(0, 2, n).astype(bool)] = noisy[0]                # many equal medians: the rank decides
        for d in (noisy, uniform, ends, few):
            out.append((d.reshape(n, 32), rng.permutation(64)[:n].astype(np.uint32)))
    out.append((np.array([dc.ONES, dc.ONES, dc.ZERO]), np.array([0, 1, 2], np.uint32)))
    out.append((np.array([dc.ZERO, dc.ONES]), np.array([5, 9], np.uint32)))
    return out


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]], ids=["plain", "sanitized"])
def test_compiled_header_equals_the_restatement(tmp_path, flags):
    records = _records()
    src, exe, data = tmp_path / "distinct_host.cpp", tmp_path / "distinct_host", tmp_path / "records.bin"
    src.write_text(PROGRAM)
    with open(str(data), "wb") as f:
        for d, r in records:
            f.write(np.uint32(len(d)).tobytes() + np.ascontiguousarray(d, np.uint8).tobytes() + r.astype("<u4").tobytes())
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-O1", "-x", "hip", "--offload-host-only",
                           "-I", CSRC] + flags + [str(src), "-o", str(exe)])
    out = subprocess.run([str(exe), str(data)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", out.stderr
    lines = out.stdout.strip().split("\n")
    assert len(lines) == 2 * len(records)
    seen_256 = seen_tie = 0
    for (d, r), lm_, lc_ in zip(records, lines[0::2], lines[1::2]):
        med = dr.medians(list(d))
        assert [int(x) for x in lm_.split()[1:]] == med
        keys = [dr.key(m, k) for m, k in zip(med, r)]
        winner = int(np.argmin(keys))
        assert [int(x) for x in lc_.split()[1:]] == [len(d), winner, med[winner], keys[winner]]
        # the key's order is the rule's order: the least median, then the largest rank
        assert winner == min(range(len(d)), key=lambda a: (med[a], -int(r[a])))
        seen_256 += 256 in med
        seen_tie += med.count(min(med)) > 1
    assert seen_256 > 10 and seen_tie > 50
    assert lines[-3].split()[1:] == ["3", "1", "0", str(dr.key(0, 1))]       # the extremes: all-ones of rank 1, not all-zeros


# ---- the cases are what they are named after -----------------------------------------------------------------------------------

def test_ladder_has_every_n_and_both_median_parities():
    store, lids, order = dc.ladder()
    assert len(order) == 64 and sorted(order) != order and max(len(l) for l in lids.values()) == 192 <= dc.K
    l = lm.union(store, lids, order)[2]
    n = dr.counts(lids, order, l)
    assert sorted(n.tolist()) == sorted(list(range(1, 65)) * 3) and len(l) == 192
    ranks = {i: sorted(order).index(i) for i in order}
    assert any(ranks[i] != k for k, i in enumerate(order))                # rank != list position
    got, ref = dr.union(store, lids, order), lm.union(store, lids, order)
    differ = (got[0] != ref[0]).any(axis=1)
    assert differ.sum() > 100 and not differ[n <= 2].any()
    assert differ[n == 64].any() or differ[n == 63].any()


def test_repeats_count_the_highest_position_only():
    store, lids, order, ideal = dc.repeats()
    assert np.flatnonzero(lids[4] == dc.REPEATED).tolist() == [3, 200, 300] and len(lids[4]) == 320
    obs = dr.observations(lids, order)[dc.REPEATED]
    assert sorted(kf for kf, _ in obs) == [1, 2, 3, 4] and (4, 300) in obs
    kf, i, n = dr.choose(store, lids, order)[dc.REPEATED]
    assert n == 4 and kf in (1, 2, 3)
    d, _, l = dr.union(store, lids, order)
    row = int(np.flatnonzero(l == dc.REPEATED)[0])
    assert not np.array_equal(d[row], ideal) and np.array_equal(lm.union(store, lids, order)[0][row], store[4][0][300])
    # had position 3 or 200 counted for entry 4, the ideal descriptor would have been chosen
    wrong = dr.medians([store[k][0][int(np.flatnonzero(lids[k] == dc.REPEATED)[0])] for k in (1, 2, 3)] + [ideal])
    assert min(range(4), key=lambda a: (wrong[a], -a)) == 3                 # (no median is below the ideal's; entry 4 is the most recent)


def test_sizes_chains_and_capacity():
    store, lids, orders = dc.sizes()
    assert [len(lids[i]) for i in sorted(lids)] == list(dc.SIZES) and orders[0][2] == 10 and len(lids[10]) == 0
    for o in orders:
        ref = lm.union(store, lids, o)
        assert len(ref[2]) <= 400 < dc.K
        assert (dr.union(store, lids, o)[0] != ref[0]).any() and dr.counts(lids, o, ref[2]).max() == 3
    store, lids, order = dc.chains()
    every = np.unique(np.concatenate(list(lids.values())))
    assert np.all(lt.lm_hash(every) & np.uint64(0xFFFF) == 0xFFFF) and len(every) > 150
    buckets = lt.lm_bucket_count(sum(len(l) for l in lids.values()))
    bucket, steps = lt.occupied(np.concatenate([lids[i] for i in order]), buckets)
    assert buckets == 2048 and steps.max() >= 150 and {buckets - 1, 0} <= set(bucket.tolist())
    assert dr.counts(lids, order, every).max() == 5
    store, lids, too_many, needed, fits = dc.capacity()
    assert needed == 550 > dc.K and len(lm.union(store, lids, fits)[2]) == 350 and len(too_many) > 2 and len(fits) > 2
    assert (dr.union(store, lids, fits)[0] != lm.union(store, lids, fits)[0]).any()
