"""Latency of multi-target landmark fusion (mslam_hip_kf_fuse_search_multi), in the style of tools/fuse_latency.py: a keep
union of --keep-keyframes (16) keyframes of --landmarks (1500) landmarks and, per n_drop in 1, 8, 64, that many target
keyframes of --landmarks landmarks, all in view of cameras a few centimetres apart; half of every target's landmarks
duplicate a landmark of the keep side (the same point within a few millimetres, its descriptor with a few flipped bits), the
other half are strangers.  Timed through the Python mirror, on the same store: one kf_fuse_search_multi over the n_drop
targets against a loop of n_drop kf_fuse_search calls, one per target under its pose (neither changes anything), medians
over --blocks blocks of --calls calls; with the stage timers on (Context.set_profiling, mode 2) one more multi call reports
the event time of every launch (fusem_*).  There is no pass / fail threshold.

usage: python tools/fuse_multi_latency.py [--keep-keyframes 16] [--landmarks 1500] [--calls 10] [--blocks 5]
                                          [--out profiles/fuse_multi_latency.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as graft  # noqa: E402
from fuse_latency import CAM, flip_bits  # noqa: E402

KEEP = 0x7ffffffe
N_DROP = (1, 8, 64)


def make_scene(rng, n_keep_kf, n_targets, n_lm, width=640, height=480):
    """-> (keep keyframes, target keyframes, R [n_targets, 3, 3], t [n_targets, 3]); the first camera is the world frame, the
    others are translated by up to 5 cm"""
    def points(n):
        z = rng.uniform(1.6, 2.9, n)
        u, v = rng.uniform(20, width - 20, n), rng.uniform(20, height - 20, n)
        return np.stack([(u - CAM[2]) / CAM[0] * z, (v - CAM[3]) / CAM[1] * z, z], 1)

    nk = n_keep_kf * n_lm
    kw, kd = points(nk), rng.integers(0, 256, (nk, 32), dtype=np.uint8)
    kl = np.arange(nk, dtype=np.int64)
    cut = lambda a: [a[k * n_lm:(k + 1) * n_lm] for k in range(n_keep_kf)]
    targets = []
    for m in range(n_targets):
        dw, dd = points(n_lm), rng.integers(0, 256, (n_lm, 32), dtype=np.uint8)
        dup, src = rng.permutation(n_lm)[:n_lm // 2], rng.permutation(nk)[:n_lm // 2]
        dw[dup] = kw[src] + rng.normal(0.0, 0.002, (len(dup), 3))
        dd[dup] = flip_bits(rng, kd[src], 6)
        targets.append((dd, dw, 10 ** 9 + m * n_lm + np.arange(n_lm, dtype=np.int64)))
    R = np.tile(np.eye(3), (n_targets, 1, 1))
    t = rng.uniform(-0.05, 0.05, (n_targets, 3))
    t[0] = 0.0
    return list(zip(cut(kd), cut(kw), cut(kl))), targets, R, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep-keyframes", type=int, default=16)
    ap.add_argument("--landmarks", type=int, default=1500)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--radius", type=float, default=8.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_multi_latency.json"))
    a = ap.parse_args()
    pkg = graft.load_package()
    ctx = pkg.Context(width=0, height=0, max_keypoints=a.keep_keyframes * a.landmarks)
    keep, targets, R, t = make_scene(np.random.default_rng(0), a.keep_keyframes, max(N_DROP), a.landmarks)
    keep_ids, drop_ids = list(range(a.keep_keyframes)), list(range(100, 100 + len(targets)))
    for id, e in list(zip(keep_ids, keep)) + list(zip(drop_ids, targets)):
        ctx.kf_add(id, *e)
    n_keep = ctx.kf_union(KEEP, keep_ids)
    args = dict(radius=a.radius, max_distance=50, ratio=0.7, max_world_distance=0.1, focal=CAM[:2], principal=CAM[2:], width=640,
                height=480)
    rows = []
    for n in N_DROP:
        ids = drop_ids[:n]

        def multi():
            return ctx.kf_fuse_search_multi(KEEP, ids, R[:n], t[:n], **args)

        def loop():
            return [ctx.kf_fuse_search(KEEP, ids[m], R[m], t[m], **args) for m in range(n)]

        first, singles = multi(), loop()
        multi_ms, loop_ms = [], []
        for _ in range(a.blocks):
            x, y = [], []
            for _ in range(a.calls):
                s = time.perf_counter()
                multi()
                x.append((time.perf_counter() - s) * 1e3)
                s = time.perf_counter()
                loop()
                y.append((time.perf_counter() - s) * 1e3)
            multi_ms.append(float(np.median(x)))
            loop_ms.append(float(np.median(y)))
        ctx.set_profiling(2)
        ctx.stage_times()
        multi()
        stages = {}
        for name, ms in ctx.stage_times(cap=8192):
            if name.startswith("fusem_"):
                stages[name] = stages.get(name, 0.0) + float(ms)
        ctx.set_profiling(0)
        rows.append(dict(n_drop=n, keep_landmarks=int(n_keep), target_landmarks=a.landmarks, n_pairs=int(len(first["keep_lid"])),
                         pairs_of_the_single_calls=int(sum(len(p["keep_lid"]) for p in singles)),
                         kf_fuse_search_multi_ms=float(np.median(multi_ms)), kf_fuse_search_loop_ms=float(np.median(loop_ms)),
                         block_medians=dict(multi_ms=multi_ms, loop_ms=loop_ms), launch_ms=stages,
                         device_ms=float(sum(stages.values()))))
        print(json.dumps(rows[-1]), flush=True)
    out = dict(keep_keyframes=a.keep_keyframes, landmarks=a.landmarks, radius=a.radius, store_entries=ctx.kf_size(), rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
