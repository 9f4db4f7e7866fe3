"""Latency of the culling search (mslam_hip_kf_cull_search), in the style of tools/prune_latency.py: maps of --listed (64 and
1024) entries of about --landmarks (2000) landmarks each, laid out as a camera's run of keyframes would leave them (entry e
holds the ids of a window that slides over one sequence of landmarks, so that each landmark is held by --overlap (6)
consecutive entries), judged with --candidates (64) candidates: the last ones of the map, as the tracker names them.  Timed
through the Python mirror, the median of --calls (50) calls per case; with the stage timers on (Context.set_profiling, mode 2)
one more call per case reports the event time of every stage (cull_upload, cull_clear, cull_count, cull_greedy).
mslam_hip_kf_observers of 2000 ids is timed on the same maps.  The launch count of a call is computed next to the times: three
clears, two launches per 64 listed entries, one more launch.  There is no pass / fail threshold.

usage: python tools/cull_latency.py [--listed 64,1024] [--landmarks 2000] [--candidates 64] [--calls 50]
                                    [--out profiles/cull_latency.json]"""
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
    ap.add_argument("--listed", default="64,1024")
    ap.add_argument("--landmarks", type=int, default=2000)
    ap.add_argument("--candidates", type=int, default=64)
    ap.add_argument("--overlap", type=int, default=6)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cull_latency.json"))
    a = ap.parse_args()
    pkg = graft.load_package()
    rng = np.random.default_rng(0)
    n, step = a.landmarks, max(a.landmarks // a.overlap, 1)
    cases = []
    for E in [int(x) for x in a.listed.split(",")]:
        ctx = pkg.Context(width=0, height=0, max_keypoints=n)
        desc, world = rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.normal(size=(n, 3))
        for e in range(E):
            ctx.kf_add(e, desc, world, lids=e * step + rng.permutation(n).astype(np.int64))
        ids = np.arange(E, dtype=np.int32)
        cand = ids[-min(a.candidates, E):]
        asked = (E // 2) * step + np.arange(2000, dtype=np.int64)
        for _ in range(3):
            got = ctx.kf_cull_search(ids, cand)
            ctx.kf_observers(ids, asked)
        ms, obs = [], []
        for _ in range(a.calls):
            t = time.perf_counter()
            ctx.kf_cull_search(ids, cand)
            ms.append((time.perf_counter() - t) * 1e3)
        for _ in range(a.calls):
            t = time.perf_counter()
            ctx.kf_observers(ids, asked)
            obs.append((time.perf_counter() - t) * 1e3)
        ctx.set_profiling(2)
        ctx.stage_times()
        ctx.kf_cull_search(ids, cand)
        stages = {}
        for name, t_ms in ctx.stage_times(cap=8192):
            if name.startswith("cull_"):
                stages[name] = stages.get(name, 0.0) + float(t_ms)
        ctx.set_profiling(0)
        chunks = (E + 63) // 64
        cases.append(dict(listed=E, landmarks=n, candidates=int(len(cand)), culled=int(got["n_culled"]),
                          mean_landmarks=float(np.mean(got["n_landmarks"])), mean_redundant=float(np.mean(got["n_redundant"])),
                          clears=3, launches=2 * chunks + 1, kf_cull_search_ms=float(np.median(ms)),
                          kf_cull_search_min_ms=float(np.min(ms)), kf_cull_search_max_ms=float(np.max(ms)),
                          kf_observers_2000_ids_ms=float(np.median(obs)), stage_ms=stages))
        print(json.dumps(cases[-1]), flush=True)
        ctx.close()
    row = dict(calls=a.calls, overlap=a.overlap, cases=cases)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
