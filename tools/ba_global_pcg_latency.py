"""Latency of mslam_hip_bundle_adjust_global with its three linear solvers: DENSE and SPARSE (Context.set_ba_global_solver) and
PCG (Context.set_ba_global_pcg), in the shape of tools/ba_global_sparse_latency.py: milliseconds per solve and per trust-region
iteration through the Python mirror, arrays prepared beforehand, max_iterations = --iterations.  One process; the solvers that
take a scene run interleaved (dense, sparse, pcg, dense, ...) after one warm-up each, and each reports the median of its
--calls solves.  With the stage timers on (Context.set_profiling, mode 2: timed in place) one more solve per solver reports the
device time inside the iterations per stage: solver_schur, then solver_factor / solver_subst (DENSE, SPARSE) or solver_precond /
solver_cg (PCG).  For PCG the row also holds the statistics of the timed solve: CG iterations per linear solve, and the
launches per CG iteration that were enqueued (3 per iteration, enqueued in batches of 32 between two looks at the device's
decision: the launches after the end return at once but are launches all the same).

Scenes: the ring trajectory(K, 2, 3, K) at K = 256 and 1024 (thin covisibility: SPARSE's ground), the complete map of 128
keyframes and 200 landmarks (DENSE's), and the maps that revisit their ground of tests/ba_global_pcg_cases.py at K = 400,
1500, 1900, 4096 (at 1900 and 4096 neither DENSE nor SPARSE takes the problem).  A solver that does not take a scene is
recorded with its error code.  There is no pass / fail threshold.

usage: python tools/ba_global_pcg_latency.py [--calls 5] [--iterations 4] [--rings 256,1024] [--revisit 400,1500,1900,4096]
                                             [--no-complete] [--pcg 500:1e-6] [--skip-sparse-above 1000] [--out file.json]"""
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
INNER = ("solver_schur", "solver_factor", "solver_subst", "solver_precond", "solver_cg")
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
        ctx.set_ba_global_pcg(kind == "pcg", *pcg)
        if kind != "pcg":
            ctx.set_ba_global_solver(kind)
        return ctx.bundle_adjust_global(sc["poses"], sc["landmarks"], sc["obs_kf"], sc["obs_lm"], sc["obs_cam"], sc["fixed"], max_iterations=it)
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
            cg = ctx.ba_global_pcg_stats()
            enqueued = CG_LAUNCHES * CG_BATCH * st["cg_batches"]
            rows[k].update(cg=cg, cg_iterations_per_solve=cg["iterations"] / max(cg["solves"], 1),
                           launches_per_cg_iteration=enqueued / max(cg["iterations"], 1))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--rings", default="256,1024")
    ap.add_argument("--revisit", default="400,1500,1900,4096")
    ap.add_argument("--no-complete", action="store_true")
    ap.add_argument("--pcg", default="500:1e-6")
    ap.add_argument("--skip-sparse-above", type=int, default=1000, help="revisit scenes above this K leave SPARSE out where it fits: "
                    "its factor walks about 1e8 block products on one workgroup there")
    ap.add_argument("--out")
    a = ap.parse_args()
    import ba_global_cases as bg
    import ba_global_pcg_cases as pc
    import ba_ref
    pkg = graft.load_package()
    ctx = pkg.Context(width=0, height=0)
    pcg = (int(a.pcg.split(":")[0]), float(a.pcg.split(":")[1]))
    scenes = [("ring", K, bg.trajectory(K, 2, 3, K)) for K in [int(v) for v in a.rings.split(",") if v]]
    if not a.no_complete:
        scenes.append(("complete", 128, ba_ref.make_scene(128, 200, 128, noise=0.005, start_angle=0.03, start_shift=0.03)))
    scenes += [("revisit", K, pc.scene("revisit:%d" % K)) for K in [int(v) for v in a.revisit.split(",") if v]]
    rows = []
    for kind, K, sc in scenes:
        an = pkg.ba_global_analyze(sc["fixed"], K, sc["obs_kf"], sc["obs_lm"], len(sc["landmarks"]))
        row = dict(scene=kind, K=K, M=int(len(sc["obs_kf"])), n=6 * an["n_free"], ordering=an["ordering"], envelope_blocks=an["envelope_blocks"],
                   n_pairs=an["n_pairs"], pcg=list(pcg))
        solvers = ["dense", "sparse", "pcg"]
        if kind == "revisit" and K > a.skip_sparse_above and an["fits"]:
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
