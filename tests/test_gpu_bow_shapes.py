"""GPU BoW on DBoW3-shaped and hand-shaped vocabularies (tools/vocab_shapes.py), bit-exact against the independent
reference of tools/bow_ref.py (f64 compared as uint64 bit patterns).  Unlike synth.make_vocabulary's complete
heap-numbered trees, these have BFS slots that differ from node ids, leaves at several depths, nodes with 1 to 40
children, ties between siblings, permuted word tables and zero-weight (stopped) words.  Each test first asserts on
the reference that its input reaches the case it is about."""
import functools

import numpy as np
import pytest

import bow_ref
import quicklz
import synth
import vocab_shapes

pytestmark = pytest.mark.gpu

K = 4096
SEEDS = {"mixed": 1, "wide": 2, "large": 4}


def u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _frames():
    return synth.make_stream(6, 640, 480, seed=1234)


@functools.lru_cache(maxsize=None)
def _docs():
    import __graft_entry__ as g
    orc = g.load_oracle()
    return tuple(orc.detect(f, orc.params())["desc"] for f in _frames())


@functools.lru_cache(maxsize=None)
def _blob(kind, weighting, compressed=0):
    if kind == "dbow3":
        return vocab_shapes.make_dbow3_vocabulary(list(_docs()), 10, 4, seed=1, weighting=weighting,
                                                  compressed=compressed > 0, level=max(compressed, 1))
    return vocab_shapes.make_irregular_vocabulary(kind, seed=SEEDS[kind], weighting=weighting, compressed=compressed > 0,
                                                  level=max(compressed, 1))


@functools.lru_cache(maxsize=None)
def _ref(kind, weighting):
    return bow_ref.RefVocabulary(_blob(kind, weighting))


def _queries(R, seed):
    """detected descriptors, random ones, and leaf descriptors with 0-3 bits flipped"""
    rng = np.random.default_rng(seed)
    near = R.desc[rng.choice(np.nonzero(R.is_leaf)[0], 900)].copy()
    for r in range(len(near)):
        for _ in range(int(rng.integers(0, 4))):
            b = int(rng.integers(0, 256))
            near[r, b >> 3] ^= np.uint8(1 << (b & 7))
    return [_docs()[0], rng.integers(0, 256, (1500, 32), dtype=np.uint8), near, _docs()[1][:1]]


def _assert_vec(got, exp):
    assert np.array_equal(got[0], exp[0]) and np.array_equal(u64(got[1]), u64(exp[1]))


CASES = [(kind, w) for kind in ("dbow3", "mixed", "wide") for w in (0, 1, 2, 3)]


@pytest.mark.parametrize("kind,weighting", CASES)
def test_words_vectors_scores(pkg, orc, kind, weighting):
    """bow_info, bow_words, bow_transform and bow_score against the reference (and the oracle)"""
    blob, R = _blob(kind, weighting), _ref(kind, weighting)
    V = orc.Vocabulary(blob)
    qs = _queries(R, 11)
    allq = np.concatenate(qs[:3])
    node, tie = R.descend(allq)
    d = R.depth[node]
    # preconditions: slots are not node ids; the two descriptors of a 16-lane group (2j, 2j+1) end at different
    # depths; ties are broken by stream order on the way down; stopped words are hit wherever the vocabulary has them
    assert (R.bfs != np.arange(R.n_nodes)).any()
    assert (d[0::2][:len(d) // 2] != d[1::2][:len(d) // 2]).sum() > 10
    assert tie.sum() > 10
    if (R.weight[R.is_leaf] == 0).any():
        assert (R.weight[node] == 0).sum() > 10
    c = pkg.Context(width=0, height=0, max_keypoints=K)
    c.bow_load(blob)
    info = c.bow_info()
    assert (info["k"], info["L"], info["n_nodes"], info["n_words"]) == (R.k, R.L, R.n_nodes, R.n_words)
    vecs = []
    for q in qs:
        gw, gwt = c.bow_words(q)
        rw, rwt = R.words(q)
        assert np.array_equal(gw, rw) and np.array_equal(u64(gwt), u64(rwt))
        gv, rv = c.bow_transform(q), R.bow_vector(q)
        _assert_vec(gv, rv)
        _assert_vec(gv, V.bow_vector(q))
        vecs.append(rv)
    for a in vecs:
        for b in vecs:
            s = c.bow_score(*a, *b)
            assert u64(s) == u64(bow_ref.score_l1(*a, *b)) and s == orc.bow_score_l1(*a, *b)
    c.close()


@pytest.mark.parametrize("kind,weighting", [("dbow3", 0), ("mixed", 2), ("wide", 1), ("dbow3", 3)])
def test_database_ties_and_removal(pkg, kind, weighting):
    """add / query / remove: duplicate entries score equal and come back in entry-id order"""
    blob, R = _blob(kind, weighting), _ref(kind, weighting)
    qs = _queries(R, 12)
    sets = [qs[0][:800], qs[2][:500], qs[0][:800], qs[1][:600], qs[2][200:700], qs[0][:800], qs[0][400:1200]]
    vecs = [R.bow_vector(s) for s in sets]
    assert all(len(v[0]) > 0 for v in vecs)
    c = pkg.Context(width=0, height=0, max_keypoints=K)
    c.bow_load(blob)
    assert [c.bow_db_add(s) for s in sets] == list(range(len(sets)))
    removed = set()

    def expect(q):
        qv = R.bow_vector(q)
        exp = [(bow_ref.score_l1(*qv, *vecs[e]), e) for e in range(len(sets)) if e not in removed]
        exp = sorted([x for x in exp if x[0] > 0], key=lambda x: (-x[0], x[1]))
        return [e for _, e in exp], [s for s, _ in exp]

    for q in (sets[0], sets[4], qs[0][100:900]):
        ids, sc = c.bow_db_query(q, len(sets))
        eids, esc = expect(q)
        assert list(ids) == eids and np.array_equal(u64(sc), u64(esc))
    eids, esc = expect(sets[0])
    assert eids[:3] == [0, 2, 5] and esc[0] == esc[1] == esc[2] > esc[3]     # three identical entries tie
    ids, _ = c.bow_db_query(sets[0], 3)
    assert list(ids) == [0, 2, 5]                            # ... and come back in entry-id order
    for e in (2, 4):
        c.bow_db_remove(e)
        removed.add(e)
    ids, sc = c.bow_db_query(sets[0], len(sets))
    eids, esc = expect(sets[0])
    assert list(ids) == eids and ids[0] == 0 and ids[1] == 5 and np.array_equal(u64(sc), u64(esc))
    c.close()


@functools.lru_cache(maxsize=None)
def _stopped_large(weighting):
    """the large irregular vocabulary with weight 0 on every leaf that frame 4's descriptors reach"""
    R0 = bow_ref.RefVocabulary(vocab_shapes.make_irregular_vocabulary("large", seed=SEEDS["large"], weighting=weighting))
    hit = np.unique(R0.descend(_docs()[4])[0])
    blob = vocab_shapes.make_irregular_vocabulary("large", seed=SEEDS["large"], weighting=weighting, zero_nodes=hit)
    return blob, bow_ref.RefVocabulary(blob)


@pytest.mark.parametrize("weighting", [0, 1, 2, 3])
def test_batch_with_a_stopped_frame(pkg, weighting):
    """detect -> bow_batch_dev over two batches of three; frame 4's every feature lands on a zero-weight word: its
    vector is empty and it has no best entry, while the other frames find theirs"""
    import torch
    blob, R = _stopped_large(weighting)
    fv = [R.bow_vector(d) for d in _docs()]
    assert len(fv[4][0]) == 0 and all(len(fv[t][0]) > 100 for t in (0, 1, 2, 3, 5))
    assert bow_ref.score_l1(*fv[5], *fv[3]) > 0                # frame 5 still finds an entry behind the empty one
    c = pkg.Context(width=640, height=480, max_batch=3, max_keypoints=K)
    c.bow_load(blob)
    dev = torch.from_numpy(_frames()).cuda()
    for b in range(2):
        c.detect_batch_dev(dev[3 * b:].data_ptr(), 3)
        c.bow_batch_dev(True)
        c.sync()
        v = c.bow_view()
        n = pkg.read_device(c, v.n_words, (3,), np.int32)
        words = pkg.read_device(c, v.words, (3, K), np.uint32)
        vals = pkg.read_device(c, v.values, (3, K), np.float64)
        be = pkg.read_device(c, v.best_entry, (3,), np.int32)
        bs = pkg.read_device(c, v.best_score, (3,), np.float64)
        for i in range(3):
            t = 3 * b + i
            assert n[i] == len(fv[t][0])
            _assert_vec((words[i, :n[i]], vals[i, :n[i]]), fv[t])
            exp = sorted([(bow_ref.score_l1(*fv[t], *fv[e]), e) for e in range(t)], key=lambda x: (-x[0], x[1]))
            exp = [x for x in exp if x[0] > 0]
            if t == 4:
                assert not exp
            if not exp:
                assert be[i] == -1 and bs[i] == 0.0
            else:
                assert be[i] == exp[0][1] and u64(bs[i]) == u64(exp[0][0])
    c.close()


@pytest.mark.parametrize("kind,weighting", [("mixed", 0), ("wide", 2), ("dbow3", 1), ("dbow3", 2)])
def test_flat_mode(pkg, kind, weighting):
    """flat assignment on word tables in permuted order (vocab_shapes) and in node-id order (dbow3): lowest word id
    on ties; vectors from the flat words; back to the descent"""
    blob, R = _blob(kind, weighting), _ref(kind, weighting)
    assert R.flat_ok
    qs = _queries(R, 13)
    leaf_desc = R.desc[R.node_of_word]
    u, cnt = np.unique(leaf_desc, axis=0, return_counts=True)
    twins = u[cnt > 1]                                       # descriptors of two or more words
    q = np.concatenate([twins, qs[2][:700], qs[1][:300]])
    dist = bow_ref.hamming(q[:len(twins) + 100, None, :], leaf_desc[None])
    assert ((dist == dist.min(1, keepdims=True)).sum(1) > 1).sum() > 5         # ties between words
    c = pkg.Context(width=0, height=0, max_keypoints=K)
    c.bow_load(blob)
    c.bow_set_assignment(pkg.BOW_ASSIGN_FLAT)
    gw, gwt = c.bow_words(q)
    rw, rwt = R.words_flat(q)
    assert np.array_equal(gw, rw) and np.array_equal(u64(gwt), u64(rwt))
    _assert_vec(c.bow_transform(q), R.bow_vector_from_words(rw, rwt))
    c.bow_set_assignment(pkg.BOW_ASSIGN_TREE)
    gw, _ = c.bow_words(q)
    assert np.array_equal(gw, R.words(q)[0]) and not np.array_equal(gw, rw)
    c.close()


def _retabled(blob, table):
    """the same stream with another word table"""
    R = bow_ref.RefVocabulary(blob)
    head = blob[:29 + (R.n_nodes - 1) * bow_ref.REC.itemsize]
    t = np.array(table, np.dtype([("wid", "<u4"), ("nid", "<u4")]))
    return head + np.uint32(len(t)).tobytes() + t.tobytes()


def _table_case(case):
    """the "mixed" vocabulary with another word table.  "extra": one word more, on an inner node (every leaf keeps its
    own word); "missing": the last word's leaf has no record, so it falls back to word 0 (Node::word_id's default), a
    second leaf's word; "shuffled": the one-to-one table in another row order."""
    blob, R = _blob("mixed", 0), _ref("mixed", 0)
    table = [(int(w), int(n)) for w, n in R.word_table]
    if case == "extra":
        table = table + [(len(table), int(np.nonzero(~R.is_leaf)[0][5]))]
    elif case == "missing":
        table = [(w, n) for w, n in table if w != len(table) - 1]
    else:
        table = [table[i] for i in np.random.default_rng(3).permutation(len(table))]
    bad = _retabled(blob, table)
    return bad, bow_ref.RefVocabulary(bad)


@pytest.mark.parametrize("case", ["extra", "missing"])
def test_flat_needs_one_word_per_leaf(pkg, orc, case):
    """flat mode needs a word table that maps one-to-one onto the leaves: setting FLAT fails, also after TREE was set
    (that used to re-enable it), and the descent keeps working"""
    blob, Rb = _table_case(case)
    leaves = np.nonzero(Rb.is_leaf)[0]
    assert not Rb.flat_ok
    assert Rb.n_words != len(leaves) or len(np.unique(Rb.word_of_node[leaves])) < len(leaves)
    q = _queries(_ref("mixed", 0), 14)[2]
    c = pkg.Context(width=0, height=0, max_keypoints=K)
    c.bow_load(blob)
    for first in (None, pkg.BOW_ASSIGN_TREE, pkg.BOW_ASSIGN_TREE):
        if first is not None:
            c.bow_set_assignment(first)
        with pytest.raises(pkg.MslamHipError) as e:
            c.bow_set_assignment(pkg.BOW_ASSIGN_FLAT)
        assert e.value.code == pkg.E_INVALID
        gw, gwt = c.bow_words(q)                              # still the descent
        rw, rwt = Rb.words(q)
        assert np.array_equal(gw, rw) and np.array_equal(u64(gwt), u64(rwt))
        assert np.array_equal(gw, orc.Vocabulary(blob).words(q)[0])
    c.close()


def test_flat_on_a_shuffled_table(pkg):
    blob, Rs = _table_case("shuffled")
    assert Rs.flat_ok and not np.array_equal(Rs.word_table["wid"], np.sort(Rs.word_table["wid"]))
    q = _queries(_ref("mixed", 0), 14)[2][:300]
    c = pkg.Context(width=0, height=0, max_keypoints=K)
    c.bow_load(blob)
    c.bow_set_assignment(pkg.BOW_ASSIGN_TREE)
    c.bow_set_assignment(pkg.BOW_ASSIGN_FLAT)
    gw, gwt = c.bow_words(q)
    rw, rwt = Rs.words_flat(q)
    assert np.array_equal(gw, rw) and np.array_equal(u64(gwt), u64(rwt))
    c.close()


def test_shared_word_sums_own_weights(pkg, orc):
    """two leaves with different weights share word 0 ("missing" table): BowVector::addWeight adds each hit's own
    weight, in feature order (the vector kernel used to add the first hit's weight once per hit)"""
    blob, Rb = _table_case("missing")
    q = np.concatenate([_queries(_ref("mixed", 0), 14)[2], Rb.reaching(np.nonzero(Rb.is_leaf & (Rb.word_of_node == 0))[0])])
    hit = np.unique(Rb.descend(q)[0])
    shared = hit[Rb.word_of_node[hit] == 0]
    assert len(shared) == 2 and Rb.weight[shared[0]] != Rb.weight[shared[1]] and (Rb.weight[shared] > 0).all()
    c = pkg.Context(width=0, height=0, max_keypoints=K)
    c.bow_load(blob)
    gv, rv = c.bow_transform(q), Rb.bow_vector(q)
    _assert_vec(gv, rv)
    _assert_vec(gv, orc.Vocabulary(blob).bow_vector(q))
    c.close()


@pytest.mark.parametrize("kind,weighting,level", [("dbow3", 0, 1), ("dbow3", 2, 3), ("mixed", 1, 1), ("wide", 3, 3)])
def test_compressed_stream(pkg, kind, weighting, level):
    """the QuickLZ-compressed stream (toStream compressed = true) gives identical words, vectors and scores"""
    plain, packed = _blob(kind, weighting), _blob(kind, weighting, level)
    assert packed[8] == 1 and len(packed) < len(plain)
    R = _ref(kind, weighting)
    qs = _queries(R, 15)
    out = []
    for blob in (plain, packed):
        c = pkg.Context(width=0, height=0, max_keypoints=K)
        c.bow_load(blob)
        info = c.bow_info()
        res = [(info["k"], info["L"], info["n_nodes"], info["n_words"])]
        for q in qs:
            w, wt = c.bow_words(q)
            v = c.bow_transform(q)
            res.append((w.tobytes(), u64(wt).tobytes(), v[0].tobytes(), u64(v[1]).tobytes()))
            _assert_vec(v, R.bow_vector(q))
        c.close()
        out.append(res)
    assert out[0] == out[1]


def test_large_irregular_tree_and_flat(pkg, orc):
    """>= 10^5 words at depths up to 7 under nodes of up to 36 children: tree mode against the reference, flat mode
    against the oracle's brute force (and the reference on a sample), batched flat path"""
    import torch
    blob, R = _blob("large", 0), _ref("large", 0)
    V = orc.Vocabulary(blob)
    assert R.n_words >= 100000 and R.depth.max() == 7 and R.flat_ok
    qs = _queries(R, 16)
    c = pkg.Context(width=640, height=480, max_batch=3, max_keypoints=K)
    c.bow_load(blob)
    for q in qs:
        gw, gwt = c.bow_words(q)
        rw, rwt = R.words(q)
        assert np.array_equal(gw, rw) and np.array_equal(u64(gwt), u64(rwt))
        _assert_vec(c.bow_transform(q), R.bow_vector(q))
    c.bow_set_assignment(pkg.BOW_ASSIGN_FLAT)
    q = np.concatenate([qs[2][:300], qs[1][:200]])
    gw, gwt = c.bow_words(q)
    fw, fwt = V.words_flat(q)
    assert np.array_equal(gw, fw) and np.array_equal(u64(gwt), u64(fwt))
    assert np.array_equal(gw[:24], R.words_flat(q[:24])[0])
    _assert_vec(c.bow_transform(q), R.bow_vector_from_words(fw, fwt))
    c.detect_batch_dev(torch.from_numpy(_frames()).cuda().data_ptr(), 3)
    c.bow_batch_dev(False)
    c.sync()
    v = c.bow_view()
    n = pkg.read_device(c, v.n_words, (3,), np.int32)
    words = pkg.read_device(c, v.words, (3, K), np.uint32)
    vals = pkg.read_device(c, v.values, (3, K), np.float64)
    for t in range(3):
        ev = R.bow_vector_from_words(*V.words_flat(_docs()[t]))
        _assert_vec((words[t, :n[t]], vals[t, :n[t]]), ev)
    c.close()
