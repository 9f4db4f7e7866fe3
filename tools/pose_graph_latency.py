"""Latency of mslam_hip_pose_graph, in the style of tools/ba_global_latency.py: milliseconds per solve and per trust-region
iteration through the Python mirror, arrays prepared beforehand, the median of --calls solves after one warm-up, with
max_iterations = --iterations (4, as in the tables of DESIGN 4.14 / 4.15).  With the stage timers on (Context.set_profiling,
mode 2: timed in place) one more solve reports the device time of the batches of iterations and, inside them, of the stages:
pg_blocks (k_pg_edges, k_pg_poses, k_pg_check), solver_schur (k_bag_clear and k_pg_assemble), solver_factor (the blocked
Cholesky with the forward solve folded in), solver_subst (the blocked back-substitution) and pg_step (k_pg_candidate,
k_pg_eval, k_pg_control).

The scenes are chains of K keyframes (tests/pose_graph_cases.py's drifted walk: K - 1 odometry edges, the chained odometry as
the start) closed by one loop edge from the first to the last keyframe; K = 64, 300, 1024, one process.  Beside every row the
same stages of mslam_hip_bundle_adjust_global at the same K (the ring of DESIGN 4.15: 20 landmarks per group, every group
seen from 8 consecutive keyframes), measured in the same process: the factorisation is the same kernels on a matrix of the
same size.  There is no pass / fail threshold.

usage: python tools/pose_graph_latency.py [--calls 10] [--iterations 4] [--sizes 64,300,1024] [--no-ba] [--out file.json]"""
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


def staged(ctx, solve, iterations, prefixes):
    ctx.set_profiling(2)
    ctx.stage_times()
    solve(iterations)
    stages = ctx.stage_times(cap=8192)
    ctx.set_profiling(0)
    out = {}
    for name, ms in stages:
        if name.startswith(prefixes):
            out[name] = out.get(name, 0.0) + float(ms)
    return out


def measure(ctx, solve, calls, iterations, outer):
    """solve(max_iterations) -> result dict; outer = the stage names that hold the whole device time"""
    res = solve(iterations)
    wall = []
    for _ in range(calls):
        t = time.perf_counter()
        res = solve(iterations)
        wall.append((time.perf_counter() - t) * 1e3)
    it = max(res["iterations"], 1)
    st = staged(ctx, solve, iterations, ("pg_", "ba_", "solver_"))
    return dict(termination=res["termination"], iterations=res["iterations"], ms_per_solve=float(np.median(wall)),
                ms_per_iteration=float(np.median(wall)) / it, device_ms=sum(st.get(n, 0.0) for n in outer),
                stage_ms_per_iteration={n: v / it for n, v in sorted(st.items()) if n not in outer},
                cost=[res["initial_cost"], res["final_cost"]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--sizes", default="64,300,1024")
    ap.add_argument("--no-ba", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import ba_global_cases as bg
    import pose_graph_cases as pc
    pkg = graft.load_package()
    ctx = pkg.Context(width=0, height=0)
    rows = []
    for K in [int(v) for v in a.sizes.split(",") if v]:
        sc = pc.drift_scene(K - 1, seed=K, step_noise=0.02, angle_noise=0.005)
        row = dict(K=K, E=int(len(sc["edge_a"])), n=6 * (K - 1))
        row["pose_graph"] = measure(ctx, lambda it: ctx.pose_graph(sc["poses"], sc["edge_a"], sc["edge_b"], sc["edge_meas"], None,
                                                                   sc["fixed"], max_iterations=it),
                                    a.calls, a.iterations, ("pg_iterations", "pg_start_cost"))
        if not a.no_ba:
            ba = bg.trajectory(K, 20, 8, K)
            row["bundle_adjust_global"] = measure(
                ctx, lambda it: ctx.bundle_adjust_global(ba["poses"], ba["landmarks"], ba["obs_kf"], ba["obs_lm"], ba["obs_cam"],
                                                         ba["fixed"], max_iterations=it),
                a.calls, a.iterations, ("ba_iterations", "ba_start_cost"))
            row["bundle_adjust_global"].update(L=int(len(ba["landmarks"])), M=int(len(ba["obs_kf"])))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
