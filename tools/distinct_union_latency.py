"""What the DISTINCTIVE descriptor mode of the union costs (mslam_hip_set_union_descriptor): microseconds per
mslam_hip_kf_union call, its synchronisation included, in RECENT and in DISTINCTIVE mode, at the shape of
tools/track_latency.py --local-map: 16 keyframes of 1500 landmarks, entry k sharing its upper part with the lower part of
entry k + 1.  --stride 750 (the default) is that tool's scene exactly: a union of 12 750 rows, every landmark in one or two
keyframes, so every wave of the choice kernel returns after its ballot; --stride 375 makes a landmark live in up to four
keyframes (7 125 rows), --stride 100 in up to fifteen (3 000 rows).

The two modes are timed alternately, in blocks of --calls calls, so that drift of the machine hits both, and the whole
measurement is repeated (--runs) in the same process: the difference between the runs is the spread a difference between
the modes has to exceed.  Then one call per mode with in-place stage timing: the per-launch event times of every union_*
stage.  There is no pass threshold: the mode only adds work.

usage: python tools/distinct_union_latency.py [--stride 750] [--blocks 12] [--calls 100] [--runs 2] [--out file.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stride", type=int, default=750, help="landmark ids of entry k start at k * stride")
    ap.add_argument("--blocks", type=int, default=12)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    import reloc_ref as rr
    pkg = graft.load_package()
    n_kf, n_lm, U = 16, 1500, 0x7fffffff
    sc = rr.make_scene(seed=0, n_kf=n_kf, n_landmarks=n_lm, n_distractors=400)
    ids = sc["ids"]
    c = pkg.Context(width=0, height=0, max_keypoints=16384)
    for k, cid in enumerate(ids):
        c.kf_add(cid, *sc["store"][cid], lids=k * a.stride + np.arange(n_lm))
    modes = (("recent", pkg.UNION_DESC_RECENT), ("distinctive", pkg.UNION_DESC_DISTINCTIVE))

    def build(mode):
        def run():
            c.set_union_descriptor(mode)              # a host-side assignment
            return c.kf_union(U, ids)
        return run
    sides = [(name, build(mode)) for name, mode in modes]
    rows, descs = {}, {}
    for name, f in sides:
        rows[name] = f()
        descs[name] = c.kf_read(U)[0]
    assert rows["recent"] == rows["distinctive"] == (n_kf - 1) * a.stride + n_lm
    changed = int((descs["recent"] != descs["distinctive"]).any(axis=1).sum())
    for _ in range(30):
        for _, f in sides:
            f()
    runs = []
    for _ in range(a.runs):
        res = {name: [] for name, _ in sides}
        for _ in range(a.blocks):
            for name, f in sides:
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    f()                               # every call ends in a device synchronise
                res[name].append((time.perf_counter() - t0) / a.calls * 1e6)
        run = {k: dict(median_us=float(np.median(v)), min_us=float(np.min(v)), max_us=float(np.max(v)),
                       blocks=[round(x, 2) for x in v]) for k, v in res.items()}
        run["ratio"] = run["distinctive"]["median_us"] / run["recent"]["median_us"]
        runs.append(run)
    stages = {}
    for name, f in sides:
        c.set_profiling(2)
        f()
        stages[name] = [(n, round(ms * 1e3, 2)) for n, ms in c.stage_times() if n.startswith("union_")]
        c.set_profiling(0)
    out = dict(runs=runs, shape=dict(keyframes=n_kf, landmarks_per_keyframe=n_lm, stride=a.stride, union_rows=rows["recent"],
                                     rows_changed_by_the_mode=changed, calls_per_block=a.calls, blocks=a.blocks),
               union_stages_us=stages)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
