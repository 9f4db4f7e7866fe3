"""The matcher kernels (modular-slam_amd/csrc/k_match.hip) at their edges, bit for bit against tests/match_ref.py.

The matrix-core kernel packs distance and train index into one f32 sort key, (dot + 258) + age * 2^-14: the planted
cases of match_ref (distances 0 and 256, winners at maximal age, the partial last tile, every row of a tile, every slice
boundary, every (d0, d1) pair of the ratio table) go through every way a matcher kernel is launched:

  route A  match_knn2, one call: sliced k_match_knn2_fp4<2> + k_match_merge (n_slices = min(8, (n_from + 255) / 256)), the
           xor/popcount kernel above 32736 train rows or on request;
  route B  match, one call: the captured-graph form (fixed 8 slices + k_merge_ratio) and the plain form (profiling on, or a
           context created with MSLAM_HIP_MATCH_GRAPH=0, or staging buffers too large for the call);
  route C  the batched kernels under relocalize(): unsliced <2> up to 4 candidates; from 5 on the hand-scheduled loop
           <4, false, PIPE>, and with MSLAM_HIP_MATCH_PIPE=0 the compiler-scheduled <4> and, from
           MSLAM_HIP_MATCH_SKIP_FROM train rows on, <4, SKIP>;
  route D  sequences of calls on one context: capacity regrowth, graph re-capture and fall-back, stale `partial` keys.

Everything is compared with array_equal: these are exact-integer properties.  tests/test_match_ref.py shows on the CPU,
from the reference's output alone, that the cases contain what they claim.

Which of PIPE / SKIP / plain <4> ran cannot be told from outside: last_match_kernel() reports matrix or popcount only, so
the selection among the loop forms rests on launch_match_knn2's rules (pair count and the two environment knobs, read per
launch) as restated above; likewise `_Staging` below restates mslam_hip_match's choice between its two forms, and is used
only to assert that both are reached, never to decide a result.

No test retries or loops on a failure: the first mismatch ends the test.
"""
import functools

import numpy as np
import pytest

import match_ref as mr

pytestmark = pytest.mark.gpu

AUTO, POPCOUNT = 0, 1
KINDS = pytest.mark.parametrize("kind", [AUTO, POPCOUNT], ids=["auto", "popcount"])

N_FROM_SWEEP = (0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 513, 2047, 2048, 2049, 32735, 32736, 32737, 65535)
N_TO_SWEEP = (1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049)
GENERATOR_SIZES = {
    "distance_extremes": (1, 2, 3, 33, 257, 2049, 32736, 32737, 65535),
    "position_extremes": (2, 3, 33, 65, 257, 300, 513, 2049, 2060, 4097, 32736, 32737),
    "masked_tail": (1, 2, 31, 33, 34, 63, 257, 258, 287, 4097, 32705, 32735, 32737),
    "max_age": (16384, 16385, 32735, 32736),
}


def _kernel(kind, n_from):
    return "popcount" if kind == POPCOUNT or n_from > mr.MM_MAX_TRAIN else "matrix"


@functools.lru_cache(maxsize=None)
def _cases(gen, arg, arg2=None):
    """the cases of one generator with their reference knn-2 (computed once per session: the routes and both matcher
    kinds share it)"""
    cases = getattr(mr, gen)(arg) if arg2 is None else getattr(mr, gen)(arg, arg2)
    return [(c, mr.knn2(c.from_desc, c.to_desc)) for c in cases]


def _all_generator_cases():
    for gen, sizes in GENERATOR_SIZES.items():
        for n in sizes:
            for case, ref in _cases(gen, n):
                yield "%s(%d)/%s" % (gen, n, case.name), case, ref


def _assert_knn2(got, ref, tag):
    for name, g, r in zip(("idx0", "idx1", "dist0", "dist1"), got, ref):
        if not np.array_equal(g, r):
            bad = np.nonzero(g != r)[0]
            q = int(bad[0])
            raise AssertionError("%s: %s differs at %d queries, first %d: got %s, reference %s"
                                 % (tag, name, len(bad), q, [int(x[q]) for x in got], [int(x[q]) for x in ref]))


def _assert_pairs(got, ref, tag):
    assert len(got[0]) == len(ref[0]), (tag, len(got[0]), len(ref[0]))
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), tag


def _tiled(case, ref, n_to):
    """the case with its queries repeated to n_to rows (a query's result does not depend on the other queries)"""
    sel = np.arange(n_to) % len(case.to_desc)
    return case.to_desc[sel], tuple(x[sel] for x in ref)


class _Staging:
    """mslam_hip_match's choice between the captured and the plain form, restated from api.hip: the staging capacities
    start at 0, grow to max(needed, current, 2048) — both, when either is exceeded — and never shrink; the captured form is
    taken when graphs are enabled, profiling is off, the train capacity is within the matrix-core range and both
    capacities together are at most 2 * (n_from + n_to) + 2048 (its upload moves whole capacities)."""

    def __init__(self, graph=True):
        self.fc = self.tc = 0
        self.graph = graph
        self.profiling = False
        self.seen = {"graph": 0, "plain": 0}

    def _grow(self, nf, nt):
        if nf > self.fc or nt > self.tc:
            self.fc, self.tc = max(nf, self.fc, 2048), max(nt, self.tc, 2048)

    def knn2(self, nf, nt):
        if nt:
            self._grow(nf, nt)

    def match(self, nf, nt):
        """-> "graph" / "plain", or None when the call returns before any launch"""
        if nt == 0 or nf < 2:
            return None
        fits = lambda: self.fc <= mr.MM_MAX_TRAIN and self.fc + self.tc <= 2 * (nf + nt) + 2048   # noqa: E731
        g = self.graph and not self.profiling
        form = "graph" if g and self.fc >= nf and self.tc >= nt and fits() else None
        if form is None:
            self._grow(nf, nt)
            form = "graph" if g and fits() else "plain"
        self.seen[form] += 1
        return form

    def kernel(self, form, kind, nf):
        """the captured form decides on the train CAPACITY (within the matrix-core range whenever it is taken)"""
        return ("popcount" if kind == POPCOUNT else "matrix") if form == "graph" else _kernel(kind, nf)


def _matcher_ctx(pkg, kind):
    c = pkg.Context(width=0, height=0, max_keypoints=1024)
    c.set_matcher(kind)
    return c


# ---- route A: match_knn2 --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sweep_case(n_from, n_to):
    (case,) = mr.mixed(n_from, n_to)
    return case, mr.knn2(case.from_desc, case.to_desc)


@KINDS
def test_knn2_shape_sweep(pkg, kind):
    """every train size of the sweep (tile and slice edges, 32736 / 32737: the switch to the xor/popcount kernel, 65535: its
    last size) against every query count (the 256-query workgroup and 32-query tile edges); 65536 train rows are refused and
    the context works afterwards"""
    c = _matcher_ctx(pkg, kind)
    for n_from in N_FROM_SWEEP:
        for n_to in N_TO_SWEEP:
            if n_from >= 32735 and n_to > 512:
                continue
            case, ref = _sweep_case(n_from, n_to)
            _assert_knn2(c.match_knn2(case.from_desc, case.to_desc), ref, "knn2 %d x %d" % (n_from, n_to))
            assert c.last_match_kernel() == _kernel(kind, n_from), (n_from, n_to)
    with pytest.raises(pkg.MslamHipError) as e:
        c.match_knn2(np.zeros((65536, 32), np.uint8), np.zeros((3, 32), np.uint8))
    assert e.value.code == pkg.E_INVALID
    with pytest.raises(pkg.MslamHipError) as e:
        c.match(np.zeros((65536, 32), np.uint8), np.zeros((3, 32), np.uint8))
    assert e.value.code == pkg.E_INVALID
    case, ref = _sweep_case(65535, 33)
    _assert_knn2(c.match_knn2(case.from_desc, case.to_desc), ref, "after the refused call")
    assert c.last_match_kernel() == "popcount"
    case, ref = _sweep_case(257, 129)
    _assert_knn2(c.match_knn2(case.from_desc, case.to_desc), ref, "after the refused call")
    c.close()


@KINDS
def test_knn2_generators(pkg, kind):
    c = _matcher_ctx(pkg, kind)
    for tag, case, ref in _all_generator_cases():
        _assert_knn2(c.match_knn2(case.from_desc, case.to_desc), ref, tag)
        assert c.last_match_kernel() == _kernel(kind, len(case.from_desc)), tag
    for m in range(257):
        (case, ref), = _cases("ratio_grid", m)
        _assert_knn2(c.match_knn2(case.from_desc, case.to_desc), ref, case.name)
    c.close()


# ---- route B: match ---------------------------------------------------------------------------------------------------
def _form_ctx(pkg, monkeypatch, form, kind):
    """form: "graph" (the default), "profiling" (set_profiling(1): plain form), "env" (created with MSLAM_HIP_MATCH_GRAPH=0)"""
    if form == "env":
        monkeypatch.setenv("MSLAM_HIP_MATCH_GRAPH", "0")
    c = _matcher_ctx(pkg, kind)
    if form == "profiling":
        c.set_profiling(1)
    st = _Staging(graph=form == "graph")
    return c, st


def _match_and_check(c, st, kind, from_desc, to_desc, ref, ratio, tag):
    got = c.match(from_desc, to_desc, ratio)
    _assert_pairs(got, mr.ratio_filter(ref, len(from_desc), ratio), tag)
    form = st.match(len(from_desc), len(to_desc))
    if form:
        assert c.last_match_kernel() == st.kernel(form, kind, len(from_desc)), (tag, form)
    return form


FORMS = pytest.mark.parametrize("form", ["graph", "profiling", "env"])


@FORMS
@KINDS
def test_match_generators(pkg, monkeypatch, form, kind):
    """every planted case through match(): with its own few queries and with the queries repeated to 1100 rows (a fresh
    context takes the captured form from n_from + n_to = 1024 on), at ratios 0.7 and 1.0, in ascending train size on a
    context per generator so that the captured form is reached where it can be"""
    seen = {"graph": 0, "plain": 0}
    for gen, sizes in GENERATOR_SIZES.items():
        c, st = _form_ctx(pkg, monkeypatch, form, kind)
        for n in sizes:
            if n > mr.MM_MAX_TRAIN and form != "graph":
                continue       # (beyond the matrix-core range every form is the same plain popcount call: once is enough)
            for case, ref in _cases(gen, n):
                tag = "%s(%d)/%s" % (gen, n, case.name)
                for ratio in (0.7, 1.0):
                    _match_and_check(c, st, kind, case.from_desc, case.to_desc, ref, ratio, tag)
                    to, tref = _tiled(case, ref, 1100)
                    _match_and_check(c, st, kind, case.from_desc, to, tref, ratio, tag + " x1100")
        c.close()
        for k in seen:
            seen[k] += st.seen[k]
    assert seen["graph" if form == "graph" else "plain"] > 100
    assert form == "graph" or seen["graph"] == 0


@FORMS
@KINDS
def test_match_ratio_grid(pkg, monkeypatch, form, kind):
    """all 33 153 pairs 0 <= d0 <= d1 <= 256 against the 257-entry ratio table at eight ratios.  The captured form gets the
    queries repeated to 1100 rows (n_to above 1024: k_merge_ratio), the plain forms the 257 - m queries as they are
    (k_match_merge / k_ratio_compact)."""
    c, st = _form_ctx(pkg, monkeypatch, form, kind)
    for ratio in mr.RATIOS:
        for m in range(257):
            (case, ref), = _cases("ratio_grid", m)
            to, tref = _tiled(case, ref, 1100) if form == "graph" else (case.to_desc, ref)
            got = _match_and_check(c, st, kind, case.from_desc, to, tref, ratio, "%s ratio %r" % (case.name, ratio))
            assert got == ("graph" if form == "graph" else "plain")
    c.close()


# ---- route C: the batched kernels under relocalize() ----------------------------------------------------------------
RELOC_K = 600
RELOC_COUNTS = (0, 1, 2, 31, 32, 33, 127, 128, 129, 511, 512, 513, RELOC_K)
RELOC_TRAIN = (2, 31, 32, 33, 64, 65, 96, 97, 4097, 32736, 32737)
# (candidates, MSLAM_HIP_MATCH_PIPE, MSLAM_HIP_MATCH_SKIP_FROM): <= 4 candidates take the unsliced <2> kernel whatever the
# knobs; from 5 on PIPE, then with PIPE off <4> below 6000 train rows and SKIP from there on, and SKIP everywhere
RELOC_CONFIGS = [(1, None, None), (4, None, None), (5, "1", None), (5, "0", None), (5, "0", "0"), (64, "1", None),
                 (64, "0", None), (64, "0", "0")]


def _reloc_cases(n):
    """the planted cases that exist at train size n, and one of mixed descriptors"""
    out = list(_cases("distance_extremes", n)) + list(_cases("position_extremes", n)) + list(_cases("mixed", n, 200))
    if n % 32 in (1, 2, 31):
        out += _cases("masked_tail", n)
    if n == 32736:
        out += _cases("max_age", n)
    if n == 2:
        for m in (0, 1, 2, 127, 128, 129, 255, 256):
            out += _cases("ratio_grid", m)
    return out


@pytest.mark.parametrize("n_cand,pipe,skip_from", RELOC_CONFIGS)
@KINDS
def test_relocalize_pairs(pkg, monkeypatch, kind, n_cand, pipe, skip_from):
    """match(from = uploaded query, to = landmarks of candidate k): the uploaded frame is the TRAIN side of every pair, the
    stored keyframes are the query sides.  Candidate k holds rows (k + j) % n of the case's queries, j < count_k, with
    neighbouring counts from RELOC_COUNTS (empty workgroups, partial query tiles, the full capacity); its pairs must equal
    the reference's ratio test over the same rows.  No pose is asked for (iterations = 1; best = -1 is a result)."""
    if pipe is not None:
        monkeypatch.setenv("MSLAM_HIP_MATCH_PIPE", pipe)
    if skip_from is not None:
        monkeypatch.setenv("MSLAM_HIP_MATCH_SKIP_FROM", skip_from)
    c = pkg.Context(width=0, height=0, max_keypoints=RELOC_K)
    c.set_matcher(kind)
    c.kf_reserve(n_cand)
    counts = [RELOC_COUNTS[(7 * k + 9) % len(RELOC_COUNTS)] for k in range(n_cand)]
    assert n_cand < len(RELOC_COUNTS) or set(counts) == set(RELOC_COUNTS)
    rng = np.random.default_rng(3)
    world = rng.normal(size=(RELOC_K, 3)) + (0, 0, 4)
    ids = list(range(10, 10 + n_cand))
    for n in RELOC_TRAIN:
        for case, ref in _reloc_cases(n):
            tag = "train %d %s" % (n, case.name)
            sels = [(k + np.arange(cnt)) % len(case.to_desc) for k, cnt in enumerate(counts)]
            for cid, sel in zip(ids, sels):
                c.kf_add(cid, case.to_desc[sel], world[:len(sel)])
            for ratio in (0.7, 1.0):
                res = c.relocalize(case.from_desc, np.zeros((n, 2), np.float32), ids, ratio=ratio, iterations=1,
                                   with_pairs=True)
                assert c.last_match_kernel() == _kernel(kind, n), tag
                for k, sel in enumerate(sels):
                    want = mr.ratio_filter(tuple(x[sel] for x in ref), n, ratio)
                    assert res["candidates"][k]["n_matches"] == len(want[0]), (tag, k, ratio)
                    _assert_pairs(res["pairs"][k], want, (tag, k, ratio))
    c.close()


# ---- route D: call sequences on one context -------------------------------------------------------------------------
@pytest.mark.parametrize("graph_env", ["1", "0"])
def test_call_sequence_state(pkg, monkeypatch, graph_env):
    """40 seeded match / match_knn2 calls on ONE context, sizes jumping between tiny, mid and near the limits, the matcher
    kind alternating, profiling switched on for calls 13 to 20: staging buffers regrow, the captured graph is dropped,
    re-captured and bypassed, `partial` and the output arrays hold what larger calls left there — every result is checked"""
    monkeypatch.setenv("MSLAM_HIP_MATCH_GRAPH", graph_env)
    c = pkg.Context(width=0, height=0, max_keypoints=1024)
    st = _Staging(graph=graph_env == "1")
    rng = np.random.default_rng(40)
    tiny = [(2, 1), (3, 7), (5, 40), (33, 3), (40, 40), (1, 9), (0, 5)]
    mid = [(300, 257), (1000, 1100), (2049, 2100), (4097, 300), (700, 2049), (224, 2100)]
    big = [(32735, 33), (32736, 300), (32736, 2100), (32704, 40)]
    beyond = [(32737, 33), (65535, 40)]   # (from here on the staging buffers exceed the captured form's range for good)
    for i in range(40):
        groups = (tiny, mid) if i < 12 else (tiny, mid, big) if i < 32 else (tiny, mid, big, beyond)
        group = groups[int(rng.integers(0, len(groups)))]
        n_from, n_to = group[int(rng.integers(0, len(group)))]
        kind = i % 2 if i % 7 else (i // 7) % 2
        if i in (13, 21):
            c.set_profiling(1 if i == 13 else 0)
            st.profiling = i == 13
        c.set_matcher(kind)
        case, ref = _sweep_case(n_from, n_to)
        tag = "call %d: %d x %d kind %d" % (i, n_from, n_to, kind)
        if rng.integers(0, 3) == 0:
            _assert_knn2(c.match_knn2(case.from_desc, case.to_desc), ref, tag)
            st.knn2(n_from, n_to)
            assert c.last_match_kernel() == _kernel(kind, n_from), tag
        else:
            _match_and_check(c, st, kind, case.from_desc, case.to_desc, ref, (0.7, 0.8, 1.0)[i % 3], tag)
    assert st.seen["plain"] >= 5 and (st.seen["graph"] >= 5 or graph_env == "0"), st.seen
    c.close()


@KINDS
def test_fewer_tiles_than_slices_after_a_larger_call(pkg, kind):
    """the captured form always launches 8 slices: after a call that filled all of them (2048 train rows x 4096 queries),
    calls with 7, 2 and 1 train tiles at nearly as many queries stay in the captured form, where the slices without tiles must
    overwrite the keys the larger call left in `partial`"""
    c = _matcher_ctx(pkg, kind)
    st = _Staging()
    (big, big_ref), = _cases("position_extremes", 2048)
    to, tref = _tiled(big, big_ref, 4096)
    assert _match_and_check(c, st, kind, big.from_desc, to, tref, 1.0, "2048 x 4096") == "graph"
    for n_from in (224, 223, 40, 33, 32, 31, 3, 2):
        for case, ref in list(_cases("position_extremes", n_from)) + list(_cases("distance_extremes", n_from)):
            to, tref = _tiled(case, ref, 2100)
            tag = "%d x 2100 %s" % (n_from, case.name)
            assert _match_and_check(c, st, kind, case.from_desc, to, tref, 1.0, tag) == "graph", tag
            assert _match_and_check(c, st, kind, case.from_desc, to[:2075], tuple(x[:2075] for x in tref), 0.7, tag) == "graph", tag
    c.close()
