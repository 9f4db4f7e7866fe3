"""An independent restatement of DBoW3's word assignment, BoW vectors and L1 score in plain Python / numpy.

It parses the vocabulary stream itself (compressed streams through tools/quicklz.py) and never calls the oracle, so
the oracle and the HIP library can both be checked against it.  What it restates:
  Vocabulary::fromStream            dbow3.patch:2544-2651  children in stream order (push_back, :2626)
  Vocabulary::transform(f, id, w)   dbow3.patch:1760-1860  greedy descent, strict `<`: the first child in stream
                                                           order wins a tie
  Vocabulary::transform(fs, v)      dbow3.patch:1432-1530  `if (w > 0)` skips stopped words; TF / TF_IDF use
                                                           BowVector::addWeight, IDF / BINARY addIfNotExist
  BowVector::normalize(L1)          sum of |v| in ascending word order (std::map order)
  L1Scoring::score                  -(sum over common words of |a-b| - |a| - |b|) / 2, ascending word order
and the exhaustive ("flat") assignment: the least distance over all words, the lower word id on ties."""
import struct

import numpy as np

MAGIC = 88877711233
REC = np.dtype([("id", "<u4"), ("pid", "<u4"), ("w", "<f8"), ("cols", "<i4"), ("rows", "<i4"), ("type", "<i4"),
                ("d", "u1", (32,))])
POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.uint8)
TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3


def hamming(a, b):
    """256-bit Hamming distance over the last axis of two broadcastable uint8 arrays"""
    return POPCOUNT[np.bitwise_xor(a, b)].sum(-1, dtype=np.int64)


class RefVocabulary:
    def __init__(self, blob):
        import quicklz
        blob = quicklz.decompress_vocabulary(bytes(blob))
        sig, _, n = struct.unpack_from("<QBI", blob, 0)
        assert sig == MAGIC and n > 0
        self.k, self.L, self.scoring, self.weighting = struct.unpack_from("<iiii", blob, 13)
        recs = np.frombuffer(blob, REC, n - 1, 29)
        assert (recs["cols"] == 32).all() and (recs["rows"] == 1).all() and (recs["type"] == 0).all()
        self.n_nodes = n
        self.stream_ids = recs["id"].astype(np.int64)
        self.parent = np.zeros(n, np.int64)
        self.weight = np.zeros(n, np.float64)
        self.desc = np.zeros((n, 32), np.uint8)
        self.parent[self.stream_ids] = recs["pid"]
        self.weight[self.stream_ids] = recs["w"]
        self.desc[self.stream_ids] = recs["d"]
        self.children = [[] for _ in range(n)]
        for nid, pid in zip(recs["id"].tolist(), recs["pid"].tolist()):
            self.children[pid].append(nid)
        pos = 29 + (n - 1) * REC.itemsize
        self.n_words, = struct.unpack_from("<I", blob, pos)
        table = np.frombuffer(blob, np.dtype([("wid", "<u4"), ("nid", "<u4")]), self.n_words, pos + 4)
        assert pos + 4 + table.nbytes == len(blob)
        self.word_table = table
        self.word_of_node = np.zeros(n, np.int64)          # Node::word_id defaults to 0
        self.node_of_word = np.zeros(self.n_words, np.int64)
        self.word_of_node[table["nid"]] = table["wid"]
        self.node_of_word[table["wid"]] = table["nid"]
        self.is_leaf = np.array([len(c) == 0 for c in self.children])
        self.is_leaf[0] = False
        self.depth = np.zeros(n, np.int64)
        order = [0]
        for p in order:                                      # BFS: a parent's depth is known before its children's
            for c in self.children[p]:
                self.depth[c] = self.depth[p] + 1
                order.append(c)
        self.bfs = np.array(order, np.int64)
        assert len(order) == n                               # connected
        maxc = max(len(c) for c in self.children)
        self.child_pad = np.full((n, maxc), -1, np.int64)
        for p, ch in enumerate(self.children):
            self.child_pad[p, :len(ch)] = ch
        leaves = np.nonzero(self.is_leaf)[0]
        nid = table["nid"].astype(np.int64)
        self.flat_ok = bool(self.n_words <= (1 << 20) and len(np.unique(table["wid"])) == self.n_words
                            and len(leaves) == self.n_words and self.is_leaf[nid].all() and len(np.unique(nid)) == self.n_words)

    def descend(self, desc):
        """the greedy descent for every descriptor -> (leaf node, tie_by_order): tie_by_order[i] is True when at some
        level of descriptor i's path two or more children shared the least distance (the first in stream order won)"""
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        cur = np.zeros(len(d), np.int64)
        tie = np.zeros(len(d), bool)
        while True:
            act = np.nonzero(~self.is_leaf[cur])[0]
            if len(act) == 0:
                return cur, tie
            ch = self.child_pad[cur[act]]
            dist = np.where(ch >= 0, hamming(d[act, None, :], self.desc[np.maximum(ch, 0)]), 1 << 30)
            best = dist.argmin(1)                            # the first minimum = the first child in stream order
            tie[act] |= (dist == dist.min(1, keepdims=True)).sum(1) > 1
            cur[act] = ch[np.arange(len(act)), best]

    def reaching(self, nodes, seed=0, per_node=2, tries=64):
        """random descriptors whose descent ends at each of `nodes` (per_node of each), for test inputs"""
        rng = np.random.default_rng(seed)
        out = {int(n): [] for n in nodes}
        for _ in range(tries):
            d = rng.integers(0, 256, (4096, 32), dtype=np.uint8)
            for i, n in enumerate(self.descend(d)[0].tolist()):
                if n in out and len(out[n]) < per_node:
                    out[n].append(d[i])
            if all(len(v) == per_node for v in out.values()):
                return np.stack([x for v in out.values() for x in v])
        raise ValueError("no descriptor reaches some of the nodes")

    def words(self, desc):
        node, _ = self.descend(desc)
        return self.word_of_node[node].astype(np.uint32), self.weight[node]

    def words_flat(self, desc):
        assert self.flat_ok
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        leaf_desc = self.desc[self.node_of_word]
        w = np.empty(len(d), np.int64)
        step = max(1, (1 << 21) // self.n_words)
        for s in range(0, len(d), step):
            w[s:s + step] = hamming(d[s:s + step, None, :], leaf_desc[None]).argmin(1)   # lowest word id on ties
        return w.astype(np.uint32), self.weight[self.node_of_word[w]]

    def bow_vector_from_words(self, word, weight):
        tf = self.weighting in (TF_IDF, TF)
        acc = {}
        for w, x in zip(word.tolist(), weight.tolist()):
            if not x > 0:                                    # stopped word
                continue
            if tf:
                acc[w] = acc[w] + x if w in acc else x       # addWeight
            elif w not in acc:
                acc[w] = x                                   # addIfNotExist
        keys = sorted(acc)
        assert self.scoring == 0                             # L1_NORM
        norm = 0.0
        for key in keys:
            norm += abs(acc[key])
        vals = [acc[key] / norm for key in keys] if norm > 0 else [acc[key] for key in keys]
        return np.array(keys, np.uint32), np.array(vals, np.float64)

    def bow_vector(self, desc):
        return self.bow_vector_from_words(*self.words(desc))


def score_l1(w1, v1, w2, v2):
    """L1Scoring::score on two normalised vectors with ascending word ids"""
    b = dict(zip(np.asarray(w2).tolist(), np.asarray(v2).tolist()))
    s = 0.0
    for w, a in zip(np.asarray(w1).tolist(), np.asarray(v1).tolist()):
        if w in b:
            s += abs(a - b[w]) - abs(a) - abs(b[w])
    return -s / 2.0
