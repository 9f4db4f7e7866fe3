"""CPU tests on DBoW3-shaped and hand-shaped vocabularies (tools/vocab_shapes.py): the generators really produce the
shapes the GPU tests rely on, and the oracle agrees with the independent reference of tools/bow_ref.py on them."""
import functools

import numpy as np
import pytest

import bow_ref
import quicklz
import synth
import vocab_shapes


@functools.lru_cache(maxsize=None)
def _docs():
    import __graft_entry__ as g
    orc = g.load_oracle()
    return tuple(orc.detect(f, orc.params())["desc"] for f in synth.make_stream(6, 640, 480, seed=1234))


@functools.lru_cache(maxsize=None)
def _blob(kind, weighting):
    if kind == "dbow3":
        return vocab_shapes.make_dbow3_vocabulary(list(_docs()), 10, 4, seed=1, weighting=weighting)
    return vocab_shapes.make_irregular_vocabulary(kind, seed={"mixed": 1, "wide": 2, "large": 4}[kind], weighting=weighting)


CASES = [(kind, w) for kind in ("dbow3", "mixed", "wide") for w in (0, 1, 2, 3)] + [("large", 0)]


def _queries(R, seed):
    """detected descriptors, random ones, and leaf descriptors with 0-3 bits flipped (these reach duplicate
    siblings and zero-weight leaves)"""
    rng = np.random.default_rng(seed)
    leaves = np.nonzero(R.is_leaf)[0]
    near = R.desc[rng.choice(leaves, 600)].copy()
    for r in range(len(near)):
        for _ in range(int(rng.integers(0, 4))):
            b = int(rng.integers(0, 256))
            near[r, b >> 3] ^= np.uint8(1 << (b & 7))
    return [_docs()[0], rng.integers(0, 256, (700, 32), dtype=np.uint8), near]


def test_dbow3_vocabulary_shape():
    """the properties of a tree Vocabulary::create writes (dbow3.patch:845-1360), which a complete heap-numbered tree
    does not have: every one of them is asserted, so a generator change cannot quietly make the GPU tests vacuous"""
    for w in (0, 1, 2, 3):
        R = bow_ref.RefVocabulary(_blob("dbow3", w))
        assert (R.k, R.L, R.weighting, R.scoring) == (10, 4, w, 0)
        fan = np.array([len(c) for c in R.children if c])
        leaf = np.nonzero(R.is_leaf)[0]
        assert fan.max() == 10 and fan.min() < 10 and (fan < 10).sum() > 20          # fewer than k children
        assert set(R.depth[leaf].tolist()) >= {3, 4} and R.depth.max() == 4          # leaves above depth L
        assert (R.bfs != np.arange(R.n_nodes)).sum() > R.n_nodes // 2                 # BFS slot != node id
        assert np.array_equal(R.word_table["wid"], np.arange(R.n_words))             # createWords: node-id order
        assert np.array_equal(R.node_of_word, leaf) and R.flat_ok
        dup = sum(len(c) - len(np.unique(R.desc[c], axis=0)) for c in R.children if len(c) > 1)
        assert dup > 0                                                                # identical siblings
        # toStream: the children of the node popped from the stack, all of them, in creation (= id) order
        assert all(c == sorted(c) for c in R.children)
        assert R.stream_ids[0] == 1 and R.children[0] == list(range(1, 11))
        zero = (R.weight[leaf] == 0).sum()
        assert (zero > 50) if w in (0, 2) else (zero == 0 and (R.weight[leaf] == 1).all())
        if w in (0, 2):                                                               # idf = ln(6 / Ni), Ni in 1..6
            assert set(np.round(np.exp(R.weight[leaf]) * 1e6).astype(int).tolist()) <= {
                round(6 / n * 1e6) for n in range(1, 7)}


@pytest.mark.parametrize("kind", ["mixed", "wide", "large"])
def test_irregular_vocabulary_shape(kind):
    R = bow_ref.RefVocabulary(_blob(kind, 0))
    leaf = np.nonzero(R.is_leaf)[0]
    fan = np.array([len(c) for c in R.children if c])
    depths = set(R.depth[leaf].tolist())
    assert (R.k, R.L) == (3, 2) and R.depth.max() == 7 and fan.max() > 3               # the header describes nothing
    assert all(c == sorted(c, reverse=True) for c in R.children)                      # siblings: decreasing ids
    assert not np.array_equal(R.word_of_node[leaf], np.arange(len(leaf)))              # permuted word table
    assert not np.array_equal(R.word_table["wid"], np.arange(R.n_words))
    assert R.flat_ok and (R.weight[leaf] == 0).sum() > 0.05 * len(leaf)
    assert (R.bfs != np.arange(R.n_nodes)).any()
    dup = sum(len(c) - len(np.unique(R.desc[c], axis=0)) for c in R.children if len(c) > 1)
    assert dup > 0
    if kind == "mixed":
        assert len(R.children[0]) == 1 and len(R.children[1]) == 1                      # root with one child, chain
        assert fan.max() == 40 and (fan > 32).any() and (fan == 1).sum() > 3
        big = R.children[int(np.argmax([len(c) for c in R.children]))]
        assert R.is_leaf[big].any() and not R.is_leaf[big].all()                        # leaf and inner siblings
        assert depths == {4, 5, 6, 7}
    elif kind == "wide":
        assert depths == set(range(1, 8)) and len(R.children[0]) == 37
    else:
        assert R.n_words >= 100000 and depths >= {3, 4, 5, 6, 7} and len(R.children[0]) > 1


@pytest.mark.parametrize("kind,weighting", CASES)
def test_oracle_against_reference(orc, kind, weighting):
    """words, weights, vectors (f64 bit patterns) and scores of the oracle against the reference"""
    blob = _blob(kind, weighting)
    R = bow_ref.RefVocabulary(blob)
    V = orc.Vocabulary(blob)
    assert (V.k, V.L, V.n_nodes, V.n_words, V.weighting) == (R.k, R.L, R.n_nodes, R.n_words, R.weighting)
    vecs = []
    for q in _queries(R, 5):
        w, wt = V.words(q)
        rw, rwt = R.words(q)
        assert np.array_equal(w, rw) and np.array_equal(wt.view(np.uint64), rwt.view(np.uint64))
        v, rv = V.bow_vector(q), R.bow_vector(q)
        assert np.array_equal(v[0], rv[0]) and np.array_equal(v[1].view(np.uint64), rv[1].view(np.uint64))
        vecs.append(rv)
    for a in vecs:
        for b in vecs:
            assert orc.bow_score_l1(*a, *b) == bow_ref.score_l1(*a, *b)
    q = _queries(R, 6)[2][:40]
    fw, fwt = V.words_flat(q)
    rfw, rfwt = R.words_flat(q)
    assert np.array_equal(fw, rfw) and np.array_equal(fwt, rfwt)


def test_reference_covers_the_edges():
    """the inputs of the GPU tests reach what they are meant to reach, judged by the reference alone"""
    R = bow_ref.RefVocabulary(_blob("mixed", 2))
    q = _queries(R, 5)
    node, tie = R.descend(np.concatenate(q))
    assert tie.sum() > 20                                                    # ties broken by stream order
    d = R.depth[node]
    assert (d[0::2][:len(d) // 2] != d[1::2][:len(d) // 2]).sum() > 50       # lane-group pairs end at different depths
    assert (R.weight[node] == 0).sum() > 20                                  # zero-weight words are hit
    w, wt = R.words(q[2])
    v = R.bow_vector_from_words(w, wt)
    assert len(v[0]) < len(np.unique(w))                                     # ... and skipped
    # an all-stopped descriptor set gives an empty vector
    stopped = q[2][R.weight[R.descend(q[2])[0]] == 0]
    assert len(stopped) > 0 and len(R.bow_vector(stopped)[0]) == 0


def test_compressed_reference_parse():
    blob = _blob("mixed", 1)
    for level in (1, 3):
        packed = quicklz.compress_vocabulary(blob, level)
        assert packed[8] == 1 and len(packed) < len(blob)
        R, P = bow_ref.RefVocabulary(blob), bow_ref.RefVocabulary(packed)
        q = _queries(R, 3)[1]
        assert np.array_equal(R.words(q)[0], P.words(q)[0])
    assert vocab_shapes.make_irregular_vocabulary("mixed", seed=1, weighting=1, compressed=True) == quicklz.compress_vocabulary(blob, 1)


def test_make_vocabulary_unchanged():
    """bench.py and the goldens use synth.make_vocabulary: its bytes stay what they were"""
    import hashlib
    assert hashlib.sha256(synth.make_vocabulary(10, 3)).hexdigest() == _SHA_10_3
    assert hashlib.sha256(synth.make_vocabulary(4, 3, seed=5, weighting=2)).hexdigest() == _SHA_4_3


_SHA_10_3 = "63223cd0b73ca537ad1588161617c01eec87d64615e682442a2e8e9317f8bc76"
_SHA_4_3 = "d2360afcb8d2ed9517958c014d01cb0e186918eeee197590ea7ab90953450529"


def test_shared_word_id_sums_own_weights(orc):
    """a leaf without a word record falls back to word 0 (Node::word_id's default), so two leaves with different
    weights share a word: BowVector::addWeight adds each hit's own weight, in feature order"""
    blob = _blob("mixed", 0)
    R = bow_ref.RefVocabulary(blob)
    head = blob[:29 + (R.n_nodes - 1) * bow_ref.REC.itemsize]
    t = R.word_table[R.word_table["wid"] != R.n_words - 1]
    bad = head + np.uint32(len(t)).tobytes() + t.tobytes()
    Rb, V = bow_ref.RefVocabulary(bad), orc.Vocabulary(bad)
    both = np.nonzero(Rb.is_leaf & (Rb.word_of_node == 0))[0]
    q = np.concatenate([_queries(R, 14)[2], Rb.reaching(both)])
    node = Rb.descend(q)[0]
    shared = np.unique(node[Rb.word_of_node[node] == 0])
    assert len(shared) == 2 and Rb.weight[shared[0]] != Rb.weight[shared[1]]
    w, wt = Rb.words(q)
    hits = wt[(w == 0) & (wt > 0)]
    own, first = 0.0, 0.0
    for x in hits:
        own += x
        first += hits[0]
    assert own != first                                      # summing the first hit's weight would differ
    bw, bv = V.bow_vector(q)
    rw, rv = Rb.bow_vector(q)
    assert bw[0] == rw[0] == 0 and np.array_equal(bw, rw) and np.array_equal(bv.view(np.uint64), rv.view(np.uint64))
