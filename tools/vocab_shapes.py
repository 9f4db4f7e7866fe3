"""Vocabularies shaped like the ones DBoW3 writes, not only complete heap-numbered trees (synth.make_vocabulary).

make_dbow3_vocabulary restates Vocabulary::create from the published algorithm (dbow3.patch, line numbers below):
fewer than k children where a node holds <= k descriptors (duplicates kept), leaves above depth L, node ids in
creation order (not BFS), word ids in node-id order, idf weights of 0 and the toStream DFS order.
make_irregular_vocabulary builds hand-shaped trees without k-means: single-child chains, leaves at depths 1 to 7,
nodes with more than 32 children, siblings written with decreasing ids, duplicate sibling descriptors, a permuted
word table, zero-weight leaves and header k / L that disagree with the stored tree.  numpy only."""
import math
import struct

import numpy as np

from bow_ref import MAGIC, REC, TF, BINARY, hamming


class Tree:
    """nodes in id order: parent, children (in the order they are written), descriptor, weight; the word table"""

    def __init__(self):
        self.parent, self.children, self.desc, self.weight = [0], [[]], [np.zeros(32, np.uint8)], [0.0]
        self.words = []                                      # (word id, node id) in table order

    def add(self, parent, desc, weight=0.0):
        nid = len(self.parent)
        self.parent.append(parent)
        self.children.append([])
        self.desc.append(np.asarray(desc, np.uint8))
        self.weight.append(float(weight))
        self.children[parent].append(nid)
        return nid

    def leaves(self):
        return [n for n in range(1, len(self.parent)) if not self.children[n]]

    def descend(self, desc):
        """Vocabulary::transform's greedy descent (strict `<`, the first written child wins ties) -> leaf node ids"""
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        D = np.stack(self.desc)
        maxc = max(len(c) for c in self.children)
        pad = np.full((len(self.children), maxc), -1, np.int64)
        for p, ch in enumerate(self.children):
            pad[p, :len(ch)] = ch
        leaf = np.array([not c for c in self.children])
        leaf[0] = False
        cur = np.zeros(len(d), np.int64)
        while True:
            act = np.nonzero(~leaf[cur])[0]
            if len(act) == 0:
                return cur
            ch = pad[cur[act]]
            dist = np.where(ch >= 0, hamming(d[act, None, :], D[np.maximum(ch, 0)]), 1 << 30)
            cur[act] = ch[np.arange(len(act)), dist.argmin(1)]

    def to_stream(self, k, L, weighting, scoring=0, compressed=False, level=1):
        """Vocabulary::toStream (dbow3.patch:2252-2355): header, then a stack of parents starting at the root; each
        popped parent writes all its children in order and pushes the inner ones.  Then the word table."""
        recs = []
        stack = [0]
        while stack:
            pid = stack.pop()
            for c in self.children[pid]:
                recs.append((c, pid, self.weight[c], 32, 1, 0, self.desc[c]))
                if self.children[c]:
                    stack.append(c)
        assert len(recs) == len(self.parent) - 1
        r = np.array(recs, REC)
        w = np.array(self.words, np.dtype([("wid", "<u4"), ("nid", "<u4")]))
        blob = b"".join([struct.pack("<QBI", MAGIC, 0, len(self.parent)), struct.pack("<iiii", k, L, scoring, weighting),
                         r.tobytes(), struct.pack("<I", len(w)), w.tobytes()])
        if compressed:
            import quicklz
            blob = quicklz.compress_vocabulary(blob, level)
        return blob


def _majority(X):
    """DescManip::meanValue for binary descriptors: a bit is set when at least ceil(n/2) of the descriptors set it"""
    bits = np.unpackbits(X, axis=1).sum(0)
    return np.packbits(bits >= len(X) // 2 + len(X) % 2)


def _kmeans(X, k, rng, max_iter=100):
    """HKmeansStep's k-means (dbow3.patch:845-1135) on > k descriptors, seeded by initiateClustersKMpp
    (:1180-1245): the first centre uniformly at random, then one descriptor drawn with probability proportional to
    its distance to the nearest centre so far, while that total is > 0 (so fewer than k centres when the descriptors
    hold fewer than k distinct values).  Association: the first centre with the least distance.  Centres: majority
    bits; a centre left without descriptors keeps its value.  Stops when no association changes (DBoW3 has no
    iteration limit; max_iter only guards against a cycle)."""
    centres = [X[rng.integers(len(X))]]
    mind = hamming(X, centres[0]).astype(np.float64)
    while len(centres) < k:
        d = hamming(X, centres[-1])
        mind = np.where((mind > 0) & (d < mind), d, mind)
        total = mind.sum()
        if not total > 0:
            break
        cut = 0.0
        while cut == 0.0:
            cut = rng.random() * total
        i = int(np.searchsorted(np.cumsum(mind), cut))     # the first running sum >= cut
        centres.append(X[min(i, len(X) - 1)])
    C = np.stack(centres)
    last = None
    for _ in range(max_iter):
        assoc = hamming(X[:, None, :], C[None]).argmin(1)
        if last is not None and np.array_equal(assoc, last):
            break
        last = assoc
        for c in range(len(C)):
            if (assoc == c).any():
                C[c] = _majority(X[assoc == c])
    return C, [np.nonzero(assoc == c)[0] for c in range(len(C))]


def make_dbow3_vocabulary(docs, k=10, L=4, seed=0, weighting=0, scoring=0, compressed=False, level=1, tree=False):
    """Vocabulary::create(training_features, k, L, weighting, scoring) (dbow3.patch:120-180) on `docs`, a list of
    (n_i, 32) uint8 descriptor arrays (one per training image).  Returns the toStream bytes (QuickLZ-compressed at
    `level` when `compressed`), or (bytes, Tree) with tree=True."""
    X = np.concatenate([np.asarray(d, np.uint8).reshape(-1, 32) for d in docs])
    rng = np.random.default_rng(seed)
    t = Tree()

    def step(parent, idx, cur_level):                       # HKmeansStep(parent_id, descriptors, current_level)
        if len(idx) == 0:
            return
        if len(idx) <= k:                                   # trivial case: one cluster per descriptor, duplicates kept
            centres, groups = X[idx], [np.array([i]) for i in range(len(idx))]
        else:
            centres, groups = _kmeans(X[idx], k, rng)
        ids = [t.add(parent, c) for c in centres]          # children numbered first ...
        if cur_level < L:
            for nid, g in zip(ids, groups):                 # ... then the recursion (:1120-1135); a one-feature
                if len(g) > 1:                              # cluster is never split: a leaf above depth L
                    step(nid, idx[g], cur_level + 1)

    step(0, np.arange(len(X)), 1)
    # createWords (:1271-1293): leaves in node-id order
    leaves = t.leaves()
    t.words = [(w, n) for w, n in enumerate(leaves)]
    # setNodeWeights (:1303-1360): 1 for TF / BINARY; ln(N / Ni) for IDF / TF_IDF, Ni = training images that reach
    # the word; a word no image reaches keeps 0
    if weighting in (TF, BINARY):
        for n in leaves:
            t.weight[n] = 1.0
    else:
        word_of = {n: w for w, n in t.words}
        Ni = np.zeros(len(leaves), np.int64)
        for d in docs:
            Ni[np.unique([word_of[n] for n in t.descend(d).tolist()])] += 1
        for w, n in t.words:
            if Ni[w] > 0:
                t.weight[n] = math.log(float(len(docs)) / float(Ni[w]))
    blob = t.to_stream(k, L, weighting, scoring, compressed, level)
    return (blob, t) if tree else blob


def make_irregular_vocabulary(shape="mixed", seed=0, weighting=0, header_k=3, header_L=2, zero_frac=0.15,
                              zero_nodes=(), compressed=False, level=1, tree=False):
    """A hand-shaped tree with random node descriptors.  Shapes:
    "mixed": the root has ONE child, which heads a single-child chain and then a node with 40 children (leaves and
      inner nodes mixed; three 16-lane rounds of k_bow_descend), whose subtrees hold leaves at depths 4 to 7,
      more single-child links and nodes of 17-36 children; one of the root-near inner nodes has 8 identical children.
    "wide": the root has 37 children, 12 of them leaves at depth 1; the inner ones carry random subtrees with leaves
      at depths 2 to 7, each inner node with 1-5 children (duplicate sibling descriptors included).
    "large": >= 10^5 words under several root children, leaves at depths 2 to 7 (fan-outs 4-36).
    Every shape writes siblings in decreasing id order, permutes the word table (word ids not in leaf order),
    gives weight 0 to a `zero_frac` share of the leaves and to the leaves in `zero_nodes`, and stores header
    k / L (`header_k`, `header_L`) that describe no part of the tree.  Weights: 1 for TF / BINARY, else idf-like."""
    rng = np.random.default_rng(seed)
    t = Tree()

    def rand_desc():
        return rng.integers(0, 256, 32, dtype=np.uint8)

    def subtree(parent, depth, max_depth, fan, p_inner=(0.75, 0.45)):
        n = int(rng.integers(fan[0], fan[1] + 1))
        made = [t.add(parent, rand_desc()) for _ in range(n)]
        if n > 1 and rng.random() < 0.3:                    # a duplicate sibling descriptor
            i, j = rng.choice(n, 2, replace=False)
            t.desc[made[j]] = t.desc[made[i]].copy()
        for nid in made:
            if depth + 1 <= max_depth and rng.random() < p_inner[depth >= 3]:
                subtree(nid, depth + 1, max_depth, fan, p_inner)

    if shape == "mixed":
        chain = t.add(0, rand_desc())                       # the root's only child
        for _ in range(2):
            chain = t.add(chain, rand_desc())               # a single-child chain, depths 1-3
        wide = [t.add(chain, rand_desc()) for _ in range(40)]
        for i, nid in enumerate(wide):
            if i % 3 == 0:
                continue                                    # leaves at depth 4 among inner siblings
            if i == 5:
                lone = t.add(nid, rand_desc())              # one more single-child link
                subtree(lone, 6, 7, (2, 5))
            elif i == 7:
                subtree(nid, 5, 6, (17, 36))                # more than 16 children again
            elif i == 8:
                d = rand_desc()
                for _ in range(8):
                    t.add(nid, d)                           # 8 identical siblings: ties by stream order
            else:
                subtree(nid, 5, 7, (1, 6))
    elif shape == "wide":
        for i in range(37):
            nid = t.add(0, rand_desc())
            if i % 3 != 1:
                subtree(nid, 2, 7, (1, 5), (0.6, 0.4))
    elif shape == "large":
        while len(t.leaves()) < 100000:
            nid = t.add(0, rand_desc())
            subtree(nid, 2, 7, (4, 36), (0.85, 0.12))
    else:
        raise ValueError(shape)
    leaves = t.leaves()
    perm = rng.permutation(len(leaves))
    t.words = [(int(perm[i]), n) for i, n in enumerate(leaves)]
    rng.shuffle(t.words)                                    # table rows in no particular order either
    if weighting in (TF, BINARY):
        w = np.ones(len(leaves))
    else:
        w = np.log(2000.0 / rng.integers(1, 1000, len(leaves)))
    w[rng.random(len(leaves)) < zero_frac] = 0.0
    zero = set(int(n) for n in zero_nodes)
    for i, n in enumerate(leaves):
        t.weight[n] = 0.0 if n in zero else float(w[i])
    t.children = [list(reversed(c)) for c in t.children]   # siblings written with decreasing ids
    blob = t.to_stream(header_k, header_L, weighting, 0, compressed, level)
    return (blob, t) if tree else blob
