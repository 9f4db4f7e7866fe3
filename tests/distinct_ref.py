"""Reference restatement of the union's DISTINCTIVE descriptor mode (not a test): among the observations of a landmark in
the listed entries — one per entry, its highest position there — the descriptor with the least median Hamming distance to
all of them (ORB-SLAM's MapPoint::ComputeDistinctiveDescriptors); rows, order, world points and ids are those of
tests/local_map_ref.py::union.  Plain numpy and dicts; shares no code with the product.

    distance   popcount of the xor over the 256 bits, 0 .. 256
    median     of observation a: the N distances from a to every observation (itself included: 0), sorted ascending,
               the entry at index (N - 1) // 2
    choice     the least median; of equal medians the observation of the largest keyframe id

Also the loop of local_map_ref.LocalMapTracker run on this union: DistinctLocalMapTracker substitutes that module's `union`
for the time of each of its own process() calls and puts it back."""
import numpy as np

import local_map_ref as lm
import track_ref as tr

_recent_union = lm.union    # the module's own function, whatever is substituted later


def hamming(a, b):
    """popcount of the xor of two 32-byte descriptors"""
    return int(np.unpackbits(np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8))).sum())


def mth_smallest(row, m):
    return sorted(int(x) for x in row)[m]


def key(median, rank):
    """what the choice minimises: the median first, then the largest rank (0 .. 63)"""
    return (int(median) << 6) | (63 - int(rank))


def observations(lids, ids):
    """landmark id -> [(keyframe id, position)], one per listed entry that holds it: the highest position there"""
    obs = {}
    for kf in ids:
        last = {}
        for i, l in enumerate(np.asarray(lids[kf]).tolist()):
            last[l] = i                                # a repeat inside the entry: the higher position
        for l, i in last.items():
            obs.setdefault(l, []).append((kf, i))
    return obs


def medians(descs):
    """per observation: its median distance to all the observations, itself included"""
    n = len(descs)
    bits = np.unpackbits(np.asarray(descs, np.uint8).reshape(n, 32), axis=1).astype(np.int32)
    d = (bits[:, None, :] != bits[None, :, :]).sum(axis=2)
    return [mth_smallest(d[a], (n - 1) // 2) for a in range(n)]


def choose(store, lids, ids):
    """landmark id -> (keyframe id, position, N) of the chosen observation"""
    out = {}
    for l, o in observations(lids, ids).items():
        med = medians([store[kf][0][i] for kf, i in o])
        best = min(range(len(o)), key=lambda a: (med[a], -o[a][0]))     # the least median, then the largest keyframe id
        out[l] = (o[best][0], o[best][1], len(o))
    return out


def union(store, lids, ids):
    """local_map_ref.union with every row's descriptor replaced by the chosen observation's -> (desc, world, landmark ids)"""
    desc, world, lid = _recent_union(store, lids, ids)
    chosen = choose(store, lids, ids)
    desc = desc.copy()
    for r, l in enumerate(lid.tolist()):
        kf, i, _ = chosen[l]
        desc[r] = store[kf][0][i]
    return desc, world, lid


def counts(lids, ids, row_lids):
    """per row of the union (its landmark ids given): N, the number of observations of its landmark"""
    obs = observations(lids, ids)
    return np.array([len(obs[l]) for l in np.asarray(row_lids).tolist()], np.int32)


class DistinctLocalMapTracker(lm.LocalMapTracker):
    """LocalMapTracker whose local map is the distinctive union.  self.unions gains, per union built, (rows, rows whose
    descriptor differs from the recent union's, the largest N)."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.unions = []

    def _union(self, store, lids, ids):
        got = union(store, lids, ids)
        recent = _recent_union(store, lids, ids)
        n = counts(lids, ids, got[2])
        self.unions.append((len(got[2]), int((got[0] != recent[0]).any(axis=1).sum()), int(n.max()) if len(n) else 0))
        return got

    def process(self, desc, xy, depth):
        before = lm.union
        lm.union = self._union
        try:
            return super().process(desc, xy, depth)
        finally:
            lm.union = before


def run(seq, depth, **kw):
    """the loop over a sequence on the distinctive union -> (rows, tracker), as local_map_ref.run"""
    params = dict(tr.SEQ_PARAMS)
    params.update(kw)
    trk = DistinctLocalMapTracker(depth=depth, cam=seq["cam"], **params)
    rows = [trk.process(fr["desc"], fr["xy"], fr["depth"]) for fr in seq["frames"]]
    return rows, trk
