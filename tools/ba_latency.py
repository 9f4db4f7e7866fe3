"""Latency of mslam_hip_bundle_adjust over problem sizes (K keyframes, L landmarks, every landmark seen from `views`
keyframes, 5 mm noise, a start 0.1 rad and 5 cm off): milliseconds per solve and per trust-region iteration through the
Python mirror, arrays prepared beforehand, the median of --calls solves after one warm-up.  With the stage timers on
(mslam_hip_set_profiling mode 2) one more solve reports the time between the first and the last kernel of each batch of
iterations ("device"): wall minus device is what the host adds — validation, the two counting sorts, the upload, and one
wait on the mapped termination word per batch of four iterations.  There is no pass / fail threshold.

usage: python tools/ba_latency.py [--calls 20] [--out file.json]"""
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

SIZES = [(2, 200, 2), (8, 1000, 4), (16, 4000, 6), (32, 8000, 8), (64, 8000, 8), (64, 20000, 8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    import ba_ref
    pkg = graft.load_package()
    ctx = pkg.Context(width=0, height=0)
    rows = []
    for K, L, views in SIZES:
        sc = ba_ref.make_scene(K, L, K + L, noise=0.005, views=views, start_angle=0.1)
        args = (sc["poses"], sc["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"], sc["fixed"])
        res = ctx.bundle_adjust(*args)
        wall = []
        for _ in range(a.calls):
            t = time.perf_counter()
            res = ctx.bundle_adjust(*args)
            wall.append((time.perf_counter() - t) * 1e3)
        ctx.set_profiling(2)
        ctx.stage_times()
        ctx.bundle_adjust(*args)
        stages = ctx.stage_times()
        ctx.set_profiling(0)
        device = float(sum(ms for name, ms in stages if name.startswith("ba_")))
        batches = sum(1 for name, _ in stages if name == "ba_iterations")
        row = dict(K=K, L=L, M=int(len(sc["obs_kf"])), termination=res["termination"], iterations=res["iterations"],
                   ms_per_solve=float(np.median(wall)), ms_per_iteration=float(np.median(wall)) / max(res["iterations"], 1),
                   device_ms=device, batches=batches, host_ms=float(np.median(wall)) - device,
                   cost=[res["initial_cost"], res["final_cost"]])
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
