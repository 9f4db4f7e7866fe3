"""Reference restatement of csrc/lm_table.hpp (not a test): the hash, the bucket count and a sequential linear-probing
insert, in numpy on np.uint64 arrays; and the hash's inverse, which makes landmark ids that land on a chosen bucket.
tests/test_lm_table_edges.py holds lm_hash and lm_bucket_count to the compiled header.  Shares no code with the product.

lm_hash is splitmix64's finaliser, a bijection of the 64-bit integers: an xor-shift x ^= x >> s is undone by repeating it
(x ^= x >> s, x ^= x >> 2s, ... until the shift leaves the word) and a multiplication by an odd constant by multiplying with
its inverse modulo 2^64.  A table of b buckets (a power of two) takes the low bits, hash & (b - 1): an id whose hash ends in
0xFFFF has the LAST bucket of every table of up to 65536 buckets as its home, whatever size a call gives its table."""
import numpy as np

M1, M2 = 0xbf58476d1ce4e5b9, 0x94d049bb133111eb
I1, I2 = pow(M1, -1, 1 << 64), pow(M2, -1, 1 << 64)
LAST = 0xFFFF


def _u64(x):
    return np.ascontiguousarray(np.asarray(x).astype(np.uint64, copy=True)).reshape(-1)


def lm_hash(ids):
    """lm_hash of every id -> np.uint64 array"""
    x = _u64(ids)
    x ^= x >> np.uint64(30)
    x *= np.uint64(M1)
    x ^= x >> np.uint64(27)
    x *= np.uint64(M2)
    x ^= x >> np.uint64(31)
    return x


def lm_unhash(h):
    """the id whose lm_hash is h"""
    x = _u64(h)
    x ^= (x >> np.uint64(31)) ^ (x >> np.uint64(62))
    x *= np.uint64(I2)
    x ^= (x >> np.uint64(27)) ^ (x >> np.uint64(54))
    x *= np.uint64(I1)
    x ^= (x >> np.uint64(30)) ^ (x >> np.uint64(60))
    return x


def lm_bucket_count(keys):
    b = 64
    while b < 2 * int(keys):
        b <<= 1
    return b


def home(ids, buckets):
    return (lm_hash(ids) & np.uint64(buckets - 1)).astype(np.int64)


def ids_with_hash_low(values, below=1 << 62, seed=0, at_least=0):
    """one landmark id in [at_least, below) per entry of `values`, its hash ending in those 16 bits; all distinct.  The upper
    48 hash bits are drawn at random and the preimages outside the range thrown away."""
    want = np.asarray(values, np.int64).reshape(-1)
    assert want.size == 0 or (want.min() >= 0 and want.max() <= 0xFFFF and 0 <= at_least < below <= 1 << 63)
    rng = np.random.default_rng(seed)
    out, seen = np.zeros(len(want), np.int64), set()
    todo = np.arange(len(want))
    while len(todo):
        rep = np.repeat(todo, 16)
        h = (rng.integers(0, 1 << 48, len(rep), dtype=np.uint64) << np.uint64(16)) | want[rep].astype(np.uint64)
        x = lm_unhash(h)
        ok = (x >= np.uint64(at_least)) & (x < np.uint64(below))
        left = []
        for p in todo.tolist():
            mine = x[ok & (rep == p)].tolist()
            mine = [m for m in mine if m not in seen]
            if mine:
                out[p] = mine[0]
                seen.add(mine[0])
            else:
                left.append(p)
        todo = np.array(left, np.int64)
    return out


def colliding(n, seed=0, below=1 << 62, at_least=0, low=LAST):
    """n distinct ids whose home is the last bucket of every table"""
    return ids_with_hash_low(np.full(n, low), below, seed, at_least)


def occupied(ids, buckets):
    """the keys inserted one after the other, each at the first free bucket from its home on (a key met again keeps its
    bucket) -> (bucket, probe length = steps from home) per key.  Which buckets end up occupied does not depend on the order
    of the insertions; which key sits in which bucket of a chain does."""
    keys = [int(k) for k in _u64(ids).tolist()]
    mask = buckets - 1
    assert buckets & mask == 0 and len(set(keys)) <= buckets
    table, at = {}, {}
    bucket, steps = np.zeros(len(keys), np.int64), np.zeros(len(keys), np.int64)
    for p, (k, h) in enumerate(zip(keys, home(ids, buckets).tolist())):
        if k not in at:
            s = 0
            while h in table:
                h, s = (h + 1) & mask, s + 1
            table[h], at[k] = k, (h, s)
        bucket[p], steps[p] = at[k]
    return bucket, steps
