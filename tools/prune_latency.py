"""Latency of removing observations (mslam_hip_kf_remove_observations), in the style of tools/fuse_latency.py: a store of
--entries (64) entries of --landmarks (1500) landmarks; calls that name 1, 8 and 64 of the entries with 1 % and 50 % of each
named entry's landmarks.  Timed through the Python mirror (the named entries are put back before every call, outside the
timing), the median of --calls (100) calls per case; with the stage timers on (Context.set_profiling, mode 2) one more call
per case reports the event time of every stage (prune_upload, prune_compact).  For context, mslam_hip_kf_replace_ids — the
existing store-wide pass this one most resembles — is timed on the same store with the same number of rows.  There is no
pass / fail threshold.

usage: python tools/prune_latency.py [--entries 64] [--landmarks 1500] [--calls 100] [--out profiles/prune_latency.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=64)
    ap.add_argument("--landmarks", type=int, default=1500)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prune_latency.json"))
    a = ap.parse_args()
    pkg = graft.load_package()
    rng = np.random.default_rng(0)
    E, n = a.entries, a.landmarks
    ctx = pkg.Context(width=0, height=0, max_keypoints=n)
    store = [(rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.normal(size=(n, 3)), e * n + np.arange(n, dtype=np.int64))
             for e in range(E)]
    for e, (d, w, l) in enumerate(store):
        ctx.kf_add(e, d, w, lids=l)
    cases = []
    for named in (1, 8, E):
        for percent in (1, 50):
            take = max(1, n * percent // 100)
            kf = np.repeat(np.arange(named, dtype=np.int32), take)
            lid = np.concatenate([store[e][2][rng.choice(n, take, replace=False)] for e in range(named)])
            order = rng.permutation(len(kf))
            kf, lid = kf[order], lid[order]

            def reset():
                for e in range(named):
                    ctx.kf_add(e, *store[e][:2], lids=store[e][2])

            ms, rep = [], []
            for _ in range(a.calls):
                reset()
                t = time.perf_counter()
                got = ctx.kf_remove_observations(kf, lid)
                ms.append((time.perf_counter() - t) * 1e3)
                assert got["n_removed"] == len(kf)
            for _ in range(a.calls):
                t = time.perf_counter()
                ctx.kf_replace_ids(lid, lid)          # from == to: the same table and the same walk, nothing changes
                rep.append((time.perf_counter() - t) * 1e3)
            reset()
            ctx.set_profiling(2)
            ctx.stage_times()
            ctx.kf_remove_observations(kf, lid)
            stages = {}
            for name, t_ms in ctx.stage_times(cap=8192):
                if name.startswith("prune_"):
                    stages[name] = stages.get(name, 0.0) + float(t_ms)
            ctx.set_profiling(0)
            reset()
            cases.append(dict(entries_named=named, percent=percent, rows=int(len(kf)), kf_remove_observations_ms=float(np.median(ms)),
                              kf_replace_ids_ms=float(np.median(rep)), stage_ms=stages))
            print(json.dumps(cases[-1]), flush=True)
    row = dict(entries=E, landmarks=n, calls=a.calls, cases=cases)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
