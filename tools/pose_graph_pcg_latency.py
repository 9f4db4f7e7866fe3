"""Latency of mslam_hip_pose_graph with its three linear solvers: DENSE and SPARSE (Context.set_pose_graph_solver) and PCG
(Context.set_pose_graph_pcg), in the shape of tools/ba_global_pcg_latency.py: milliseconds per solve and per trust-region
iteration through the Python mirror (a host clock around a call that ends in a device synchronise), arrays prepared beforehand,
max_iterations = --iterations.  One process; the solvers that take a scene run interleaved (dense, sparse, pcg, dense, ...)
after one warm-up each, and each reports the median of its --calls solves.  With the stage timers on (Context.set_profiling,
mode 2: timed in place) one more solve per solver reports the device time inside the iterations per stage: solver_schur (the
assembly), then solver_factor / solver_subst (DENSE, SPARSE) or solver_precond / solver_cg (PCG).  For PCG the row also holds
the statistics of the timed solve: CG iterations per linear solve, and the launches per CG iteration that were enqueued (3 per
iteration, enqueued in batches of 32 between two looks at the device's decision).

Scenes (tests/pose_graph_pcg_cases.py): a chain of 1024 poses (thin: SPARSE's ground; CG runs into its cap there), revisit200,
the band-plus-random graph walk:K at K = 400, 1900, 4096, and random2048.  A solver that does not take a scene is recorded
with its error code; SPARSE is left out above --skip-sparse-above poses where its envelope fits, and recorded as not timed: one
workgroup walks the whole envelope there.  There is no pass / fail threshold.

usage: python tools/pose_graph_pcg_latency.py [--calls 3] [--iterations 4] [--chain 1024] [--walk 400,1900,4096] [--pcg 500:1e-6]
                                              [--skip-sparse-above 1000] [--out profiles/pose_graph_pcg_latency.json]"""
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
INNER = ("pg_blocks", "solver_schur", "solver_factor", "solver_subst", "solver_precond", "solver_cg", "pg_step")
CG_LAUNCHES, CG_BATCH = 3, 32        # k_pcg.hip: launches per CG iteration; pcg.hpp's kPcgBatch


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
    out["cg_batches"] = sum(1 for name, _ in stages if name == "solver_cg")
    return out


def measure(pkg, ctx, sc, solvers, calls, iterations, pcg):
    """-> {solver: row}; the solves of the listed solvers interleaved"""
    def solve(kind, it):
        ctx.set_pose_graph_pcg(kind == "pcg", *pcg)
        if kind != "pcg":
            ctx.set_pose_graph_solver(kind)
        return ctx.pose_graph(sc["poses"], sc["edge_a"], sc["edge_b"], sc["edge_meas"], sc["sqrt_info"], sc["fixed"], max_iterations=it)
    res, rows = {}, {}
    for k in list(solvers):                                   # the warm-up: the buffers grow here
        try:
            res[k] = solve(k, iterations)
        except pkg.MslamHipError as e:
            rows[k] = dict(error=e.code)
            solvers.remove(k)
    wall = {k: [] for k in solvers}
    for _ in range(calls):
        for k in solvers:
            t = time.perf_counter()
            res[k] = solve(k, iterations)
            wall[k].append((time.perf_counter() - t) * 1e3)
    for k in solvers:
        it = max(res[k]["iterations"], 1)
        st = staged(ctx, lambda n: solve(k, n), iterations)
        rows[k] = dict(termination=res[k]["termination"], iterations=res[k]["iterations"], ms_per_solve=float(np.median(wall[k])),
                       ms_per_iteration=float(np.median(wall[k])) / it, device_ms=sum(st.get(n, 0.0) for n in OUTER),
                       stage_ms_per_iteration={n: st[n] / it for n in INNER if n in st},
                       cost=[res[k]["initial_cost"], res[k]["final_cost"]], solves_ms=wall[k])
        if k == "pcg":
            cg = ctx.pose_graph_pcg_stats()
            enqueued = CG_LAUNCHES * CG_BATCH * st["cg_batches"]
            rows[k].update(cg=cg, cg_iterations_per_solve=cg["iterations"] / max(cg["solves"], 1),
                           launches_per_cg_iteration=enqueued / max(cg["iterations"], 1))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--chain", default="1024")
    ap.add_argument("--walk", default="400,1900,4096")
    ap.add_argument("--pcg", default="500:1e-6")
    ap.add_argument("--skip-sparse-above", type=int, default=1000, help="scenes above this K leave SPARSE out where it fits: its "
                    "factor walks the whole envelope on one workgroup there")
    ap.add_argument("--out")
    a = ap.parse_args()
    import pose_graph_pcg_cases as pcc
    pkg = graft.load_package()
    ctx = pkg.Context(width=0, height=0)
    pcg = (int(a.pcg.split(":")[0]), float(a.pcg.split(":")[1]))
    names = ["chain:%d" % int(v) for v in a.chain.split(",") if v] + ["revisit200"]
    names += ["walk:%d" % int(v) for v in a.walk.split(",") if v] + ["random2048"]
    rows = []
    for name in names:
        sc = pcc.scene(name)
        K = len(sc["poses"])
        an = pkg.pose_graph_analyze(sc["fixed"], K, sc["edge_a"], sc["edge_b"])
        pairs = {(min(x, y), max(x, y)) for x, y in zip(sc["edge_a"].tolist(), sc["edge_b"].tolist()) if not sc["fixed"][x] and not sc["fixed"][y]}
        row = dict(scene=name, K=K, E=int(len(sc["edge_a"])), n=6 * an["n_free"], ordering=an["ordering"], envelope_blocks=an["envelope_blocks"],
                   pcg_blocks=an["n_free"] + len(pairs), pcg_setting=list(pcg))
        solvers = ["dense", "sparse", "pcg"]
        if K > a.skip_sparse_above and an["fits"] and not name.startswith("chain"):
            solvers.remove("sparse")
            row["sparse"] = dict(skipped="fits, not timed")
        row.update(measure(pkg, ctx, sc, solvers, a.calls, a.iterations, pcg))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
