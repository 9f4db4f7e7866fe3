"""Latency of landmark fusion (mslam_hip_kf_fuse), in the style of tools/pose_graph_latency.py: two sides of a loop, each
--keyframes (16) keyframes of --landmarks (1500) landmarks and their union, all in view of one camera; half of the drop
side's landmarks duplicate a landmark of the keep side (the same point within a few millimetres, its descriptor with a few
flipped bits), the other half are strangers.  Timed through the Python mirror: kf_fuse_search (which changes nothing) and
kf_fuse (the store is put back before every call, outside the timing), medians over --blocks blocks of --calls calls; with
the stage timers on (Context.set_profiling, mode 2) one more kf_fuse reports the event time of every launch (fuse_clear,
fuse_ids, fuse_project, fuse_bin, fuse_search, fuse_resolve, fuse_table, fuse_replace).  There is no pass / fail threshold.

usage: python tools/fuse_latency.py [--keyframes 16] [--landmarks 1500] [--calls 10] [--blocks 5] [--out profiles/fuse_latency.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

CAM = (525.0, 525.0, 319.5, 239.5)
KEEP, DROP = 0x7ffffffe, 0x7ffffffd


def flip_bits(rng, desc, bits):
    out = np.unpackbits(desc, axis=1)
    for row in out:
        row[rng.choice(256, bits, replace=False)] ^= 1
    return np.packbits(out, axis=1)


def make_sides(rng, n_kf, n_lm, width=640, height=480):
    """-> (keep keyframes, drop keyframes): lists of (desc, world, ids); the camera is the world frame"""
    def points(n):
        z = rng.uniform(1.6, 2.9, n)
        u, v = rng.uniform(1, width - 1, n), rng.uniform(1, height - 1, n)
        return np.stack([(u - CAM[2]) / CAM[0] * z, (v - CAM[3]) / CAM[1] * z, z], 1)

    n = n_kf * n_lm
    kw, kd = points(n), rng.integers(0, 256, (n, 32), dtype=np.uint8)
    dw, dd = points(n), rng.integers(0, 256, (n, 32), dtype=np.uint8)
    dup = rng.permutation(n)[:n // 2]
    dw[dup] = kw[dup] + rng.normal(0.0, 0.002, (len(dup), 3))
    dd[dup] = flip_bits(rng, kd[dup], 6)
    kl, dl = np.arange(n, dtype=np.int64), 10 ** 9 + np.arange(n, dtype=np.int64)
    cut = lambda a: [a[k * n_lm:(k + 1) * n_lm] for k in range(n_kf)]
    return list(zip(cut(kd), cut(kw), cut(kl))), list(zip(cut(dd), cut(dw), cut(dl)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=16)
    ap.add_argument("--landmarks", type=int, default=1500)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--radius", type=float, default=8.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_latency.json"))
    a = ap.parse_args()
    pkg = graft.load_package()
    n = a.keyframes * a.landmarks
    ctx = pkg.Context(width=0, height=0, max_keypoints=n)
    keep, drop = make_sides(np.random.default_rng(0), a.keyframes, a.landmarks)
    keep_ids, drop_ids = list(range(a.keyframes)), list(range(100, 100 + a.keyframes))

    def reset():
        for id, e in list(zip(keep_ids, keep)) + list(zip(drop_ids, drop)):
            ctx.kf_add(id, *e)
        return ctx.kf_union(KEEP, keep_ids), ctx.kf_union(DROP, drop_ids)

    args = dict(R=np.eye(3), t=np.zeros(3), radius=a.radius, max_distance=50, ratio=0.7, max_world_distance=0.1, focal=CAM[:2],
                principal=CAM[2:], width=640, height=480)
    sizes = reset()
    first = ctx.kf_fuse(KEEP, DROP, **args)
    search_ms, fuse_ms = [], []
    for _ in range(a.blocks):
        s, f = [], []
        for _ in range(a.calls):
            reset()
            t = time.perf_counter()
            ctx.kf_fuse_search(KEEP, DROP, **args)
            s.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            ctx.kf_fuse(KEEP, DROP, **args)
            f.append((time.perf_counter() - t) * 1e3)
        search_ms.append(float(np.median(s)))
        fuse_ms.append(float(np.median(f)))
    reset()
    ctx.set_profiling(2)
    ctx.stage_times()
    ctx.kf_fuse(KEEP, DROP, **args)
    stages = {}
    for name, ms in ctx.stage_times(cap=8192):
        if name.startswith("fuse_"):
            stages[name] = stages.get(name, 0.0) + float(ms)
    ctx.set_profiling(0)
    row = dict(keyframes=a.keyframes, landmarks=a.landmarks, union_sizes=list(sizes), store_entries=ctx.kf_size(),
               n_pairs=int(len(first["keep_lid"])), n_rewritten=int(first["n_rewritten"]), radius=a.radius,
               kf_fuse_search_ms=float(np.median(search_ms)), kf_fuse_ms=float(np.median(fuse_ms)),
               block_medians=dict(kf_fuse_search_ms=search_ms, kf_fuse_ms=fuse_ms), launch_ms=stages,
               device_ms=float(sum(stages.values())))
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
