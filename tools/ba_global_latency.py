"""Latency of mslam_hip_bundle_adjust_global, in the style of tools/ba_latency.py: milliseconds per solve and per trust-region
iteration through the Python mirror, arrays prepared beforehand, the median of --calls solves after one warm-up, with
max_iterations = --iterations (4, as in the table of DESIGN 4.14) so that every row is the same amount of work per
iteration.  With the stage timers on (mslam_hip_set_profiling mode 2) one more solve reports the device time of the batches
of iterations and, inside them, of the three stages of the linear solver: solver_schur (the clear and the covisible-pair
Schur complement), solver_factor (the blocked Cholesky with the forward solve folded in) and solver_subst (the blocked
back-substitution); the old entry reports solver_schur and solver_factor_subst (k_ba_solve does both).

Two parts.  "old ground": the K = 64 rows of tools/ba_latency.py through the old and the new entry, interleaved call by call
in one process.  "trajectory": rings of K keyframes, 20 landmarks per group, every group seen from 8 consecutive keyframes,
K = 128 .. 1024, new entry only, with the number of covisible pairs against all pairs and the device memory in use after
the solve (hipMemGetInfo through torch).  There is no pass / fail threshold.

usage: python tools/ba_global_latency.py [--calls 10] [--iterations 4] [--sizes 128,256,512,1024] [--out file.json]"""
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

OLD_GROUND = [(64, 8000, 8), (64, 20000, 8)]


def used_mb():
    import torch
    free, total = torch.cuda.mem_get_info()
    return (total - free) / 2.0 ** 20


def staged(ctx, solve, args, iterations):
    ctx.set_profiling(2)
    ctx.stage_times()
    solve(*args, max_iterations=iterations)
    stages = ctx.stage_times()
    ctx.set_profiling(0)
    out = {}
    for name, ms in stages:
        if name.startswith("ba_") or name.startswith("solver_"):
            out[name] = out.get(name, 0.0) + float(ms)
    return out


def measure(ctx, solves, args, calls, iterations):
    """solves: {label: bound method}; the calls are interleaved label by label"""
    res, wall = {}, {k: [] for k in solves}
    for k, f in solves.items():
        res[k] = f(*args, max_iterations=iterations)
    for _ in range(calls):
        for k, f in solves.items():
            t = time.perf_counter()
            res[k] = f(*args, max_iterations=iterations)
            wall[k].append((time.perf_counter() - t) * 1e3)
    rows = {}
    for k, f in solves.items():
        it = max(res[k]["iterations"], 1)
        st = staged(ctx, f, args, iterations)
        rows[k] = dict(termination=res[k]["termination"], iterations=res[k]["iterations"], ms_per_solve=float(np.median(wall[k])),
                       ms_per_iteration=float(np.median(wall[k])) / it, device_ms=st.get("ba_iterations", 0.0) + st.get("ba_start_cost", 0.0),
                       stage_ms_per_iteration={n: v / it for n, v in st.items() if n.startswith("solver_")},
                       cost=[res[k]["initial_cost"], res[k]["final_cost"]])
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--sizes", default="128,256,512,1024")
    ap.add_argument("--out")
    a = ap.parse_args()
    import ba_global_cases as bg
    import ba_ref
    pkg = graft.load_package()
    ctx = pkg.Context(width=0, height=0)
    rows = []
    for K, L, views in OLD_GROUND:
        sc = ba_ref.make_scene(K, L, K + L, noise=0.005, views=views, start_angle=0.1)
        args = (sc["poses"], sc["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"], sc["fixed"])
        got = measure(ctx, {"old": ctx.bundle_adjust, "global": ctx.bundle_adjust_global}, args, a.calls, a.iterations)
        row = dict(part="old ground", K=K, L=L, M=int(len(sc["obs_kf"])), **got)
        rows.append(row)
        print(json.dumps(row), flush=True)
    base = used_mb()
    for K in [int(v) for v in a.sizes.split(",") if v]:
        sc = bg.trajectory(K, 20, 8, K)
        covisible, every = bg.pairs(sc)
        args = (sc["poses"], sc["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"], sc["fixed"])
        got = measure(ctx, {"global": ctx.bundle_adjust_global}, args, a.calls, a.iterations)
        row = dict(part="trajectory", K=K, L=int(len(sc["landmarks"])), M=int(len(sc["obs_kf"])), n=6 * (K - 1), covisible_pairs=len(covisible),
                   all_pairs=every, device_memory_mb=used_mb(), device_memory_before_mb=base, **got)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
