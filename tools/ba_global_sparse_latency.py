"""Latency of mslam_hip_bundle_adjust_global with the DENSE and the SPARSE linear solver (Context.set_ba_global_solver), in the
shape of tools/pose_graph_sparse_latency.py: milliseconds per solve and per trust-region iteration through the Python mirror,
arrays prepared beforehand, max_iterations = --iterations.  One process; where both solvers run, their solves are interleaved
(dense, sparse, dense, ...) after one warm-up each, and each reports the median of its --calls solves.  With the stage timers
on (Context.set_profiling, mode 2: timed in place) one more solve per solver reports the device time of the batches of
iterations and, inside them, of the three solver stages: solver_schur (the clear and the covisible pairs' Schur blocks),
solver_factor (DENSE: the blocked Cholesky over many workgroups; SPARSE: k_pgs_factor, one workgroup), solver_subst.

Scenes: the ring of tests/ba_global_cases.py, trajectory(K, 2, 3, K) (groups of 2 landmarks seen from 3 keyframes in a row,
the wrap is the loop), at K = 64, 256, 1024 with both solvers and at K = 1100, 4096, 16384 with SPARSE alone (DENSE ends at
1024); the ring of 1100 with its keyframe indices permuted (the reverse Cuthill-McKee order); and a map of 128 keyframes that
all see the same 200 landmarks (the envelope is the whole triangle: the dense pattern one workgroup has to walk alone) with
both.  There is no pass / fail threshold.

usage: python tools/ba_global_sparse_latency.py [--calls 5] [--iterations 4] [--sizes 64,256,1024,1100,4096,16384] [--no-shuffled]
                                                [--no-complete] [--out file.json]"""
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

OUTER = ("ba_iterations", "ba_start_cost")
INNER = ("solver_schur", "solver_factor", "solver_subst")


def staged(ctx, solve, iterations):
    ctx.set_profiling(2)
    ctx.stage_times()
    solve(iterations)
    stages = ctx.stage_times(cap=8192)
    ctx.set_profiling(0)
    out = {}
    for name, ms in stages:
        if name in OUTER or name in INNER:
            out[name] = out.get(name, 0.0) + float(ms)
    return out


def measure(ctx, sc, solvers, calls, iterations):
    """-> {solver: row}; the solves of the listed solvers interleaved"""
    def solve(kind, it):
        ctx.set_ba_global_solver(kind)
        return ctx.bundle_adjust_global(sc["poses"], sc["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"], sc["fixed"], max_iterations=it)
    res = {k: solve(k, iterations) for k in solvers}          # the warm-up: the buffers grow here
    wall = {k: [] for k in solvers}
    for _ in range(calls):
        for k in solvers:
            t = time.perf_counter()
            res[k] = solve(k, iterations)
            wall[k].append((time.perf_counter() - t) * 1e3)
    rows = {}
    for k in solvers:
        it = max(res[k]["iterations"], 1)
        st = staged(ctx, lambda n: solve(k, n), iterations)
        rows[k] = dict(termination=res[k]["termination"], iterations=res[k]["iterations"], ms_per_solve=float(np.median(wall[k])),
                       ms_per_iteration=float(np.median(wall[k])) / it, device_ms=sum(st.get(n, 0.0) for n in OUTER),
                       stage_ms_per_iteration={n: st.get(n, 0.0) / it for n in INNER},
                       cost=[res[k]["initial_cost"], res[k]["final_cost"]], solves_ms=wall[k])
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--sizes", default="64,256,1024,1100,4096,16384")
    ap.add_argument("--no-shuffled", action="store_true")
    ap.add_argument("--no-complete", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import ba_global_cases as bg
    import ba_global_sparse_cases as bc
    import ba_ref
    pkg = graft.load_package()
    ctx = pkg.Context(width=0, height=0)
    scenes = [("ring", K, bg.trajectory(K, 2, 3, K)) for K in [int(v) for v in a.sizes.split(",") if v]]
    if not a.no_shuffled:
        scenes.append(("shuffled", 1100, bc.scene("shuffled:1100")))
    if not a.no_complete:
        scenes.append(("complete", 128, ba_ref.make_scene(128, 200, 128, noise=0.005, start_angle=0.03, start_shift=0.03)))
    rows = []
    for kind, K, sc in scenes:
        an = pkg.ba_global_analyze(sc["fixed"], K, sc["obs_kf"], sc["obs_lm"], len(sc["landmarks"]))
        row = dict(scene=kind, K=K, M=int(len(sc["obs_kf"])), n=6 * an["n_free"], ordering=an["ordering"], envelope_blocks=an["envelope_blocks"],
                   n_pairs=an["n_pairs"])
        solvers = ["dense", "sparse"] if K <= pkg.BA_GLOBAL_MAX_KEYFRAMES else ["sparse"]
        row.update(measure(ctx, sc, solvers, a.calls, a.iterations))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
