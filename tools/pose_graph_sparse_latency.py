"""Latency of mslam_hip_pose_graph with the DENSE and the SPARSE linear solver (Context.set_pose_graph_solver), in the shape
of tools/pose_graph_latency.py: milliseconds per solve and per trust-region iteration through the Python mirror, arrays
prepared beforehand, max_iterations = --iterations (4).  One process; where both solvers run, their solves
are interleaved (dense, sparse, dense, ...) after one warm-up each, and each reports the median of its --calls solves.  With
the stage timers on (Context.set_profiling, mode 2: timed in place) one more solve per solver reports the device time of the
batches of iterations and, inside them, of the stages: pg_blocks, solver_schur (the clear and the assembly), solver_factor
(DENSE: the blocked Cholesky; SPARSE: k_pgs_factor, one workgroup), solver_subst, pg_step.

Scenes: the chains of DESIGN 4.17 (tests/pose_graph_cases.py's drifted walk closed by one loop edge) at K = 64, 300, 1024 with
both solvers and at K = 4096, 16384 with SPARSE alone (DENSE ends at 1024), and the K = 3000 revisit scene of
tests/pose_graph_sparse_cases.py (a band of 3 and 1200 revisits: the reverse Cuthill-McKee order, an envelope of 20970
blocks) with SPARSE alone, and a complete graph on 160 poses (the envelope is the whole triangle: the dense pattern one
workgroup has to walk alone) with both.  There is no pass / fail threshold.

usage: python tools/pose_graph_sparse_latency.py [--calls 10] [--iterations 4] [--sizes 64,300,1024,4096,16384] [--no-revisit] [--no-complete]
                                                 [--out file.json]"""
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

OUTER = ("pg_iterations", "pg_start_cost")


def staged(ctx, solve, iterations):
    ctx.set_profiling(2)
    ctx.stage_times()
    solve(iterations)
    stages = ctx.stage_times(cap=8192)
    ctx.set_profiling(0)
    out = {}
    for name, ms in stages:
        if name.startswith(("pg_", "solver_")):
            out[name] = out.get(name, 0.0) + float(ms)
    return out


def measure(ctx, sc, solvers, calls, iterations):
    """-> {solver: row}; the solves of the listed solvers interleaved"""
    def solve(kind, it):
        ctx.set_pose_graph_solver(kind)
        return ctx.pose_graph(sc["poses"], sc["edge_a"], sc["edge_b"], sc["edge_meas"], sc["sqrt_info"], sc["fixed"], max_iterations=it)
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
                       stage_ms_per_iteration={n: v / it for n, v in sorted(st.items()) if n not in OUTER},
                       cost=[res[k]["initial_cost"], res[k]["final_cost"]], solves_ms=wall[k])
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--sizes", default="64,300,1024,4096,16384")
    ap.add_argument("--no-revisit", action="store_true")
    ap.add_argument("--no-complete", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import pose_graph_cases as pc
    import pose_graph_sparse_cases as psc
    pkg = graft.load_package()
    ctx = pkg.Context(width=0, height=0)
    scenes = [("chain", K, pc.drift_scene(K - 1, seed=K, step_noise=0.02, angle_noise=0.005)) for K in [int(v) for v in a.sizes.split(",") if v]]
    if not a.no_revisit:
        scenes.append(("revisit", 3000, psc.scene("revisit3000")))
    if not a.no_complete:
        scenes.append(("complete", 160, pc.make_scene(160, psc.complete(160), 160)))
    rows = []
    for kind, K, sc in scenes:
        an = pkg.pose_graph_analyze(sc["fixed"], K, sc["edge_a"], sc["edge_b"])
        row = dict(scene=kind, K=K, E=int(len(sc["edge_a"])), n=6 * an["n_free"], ordering=an["ordering"], envelope_blocks=an["envelope_blocks"])
        solvers = ["dense", "sparse"] if K <= pkg.POSE_GRAPH_MAX_KEYFRAMES and kind != "revisit" else ["sparse"]
        row.update(measure(ctx, sc, solvers, a.calls, a.iterations))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
