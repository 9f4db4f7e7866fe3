"""Latency of mslam_hip_pose_graph_covariance (Context.pose_graph_covariance), in the shape of
tools/pose_graph_sparse_latency.py: milliseconds per call through the Python mirror (the median of --calls calls after one
warm-up, arrays prepared beforehand), and with the stage timers on (Context.set_profiling, mode 2: timed in place) the device
time of the call's stages: cov_blocks (k_pg_edges, k_pg_poses), solver_schur (the clear and the undamped assembly),
solver_factor (k_pgs_factor, one workgroup), cov_selinv (k_pgs_selinv, one workgroup) and cov_gather.  Next to them
solver_factor of one SPARSE solve iteration on the same envelope, the kernel cov_selinv walks backwards.

Scenes (tests/pose_graph_sparse_cases.py): loops:1025, loops:16384 (long and thin: two blocks per column but for one wide row)
and complete40 (the envelope is the whole triangle).  Every free pose that has an edge is requested, and the pairs of every
edge between two of them.  There is no pass / fail threshold: one workgroup walks the envelope alone by design.

usage: python tools/pose_graph_cov_latency.py [--calls 10] [--scenes loops:1025,loops:16384,complete40] [--out file.json]"""
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


def staged(ctx, call, prefixes):
    ctx.set_profiling(2)
    ctx.stage_times()
    call()
    stages = ctx.stage_times(cap=8192)
    ctx.set_profiling(0)
    out = {}
    for name, ms in stages:
        if name.startswith(prefixes):
            out[name] = out.get(name, 0.0) + float(ms)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--scenes", default="loops:1025,loops:16384,complete40")
    ap.add_argument("--out")
    a = ap.parse_args()
    import pose_graph_cov_ref as cr
    import pose_graph_sparse_cases as psc
    pkg = graft.load_package()
    ctx = pkg.Context(width=0, height=0)
    rows = []
    for name in [v for v in a.scenes.split(",") if v]:
        sc = psc.scene(name)
        K = len(sc["poses"])
        an = pkg.pose_graph_analyze(sc["fixed"], K, sc["edge_a"], sc["edge_b"])
        poses_of, pairs = cr.requests(sc)

        def cov():
            return ctx.pose_graph_covariance(sc["poses"], sc["edge_a"], sc["edge_b"], sc["edge_meas"], sc["sqrt_info"], sc["fixed"],
                                             poses_of=poses_of, pairs=pairs)

        def solve():
            ctx.set_pose_graph_solver("sparse")
            try:
                return ctx.pose_graph(sc["poses"], sc["edge_a"], sc["edge_b"], sc["edge_meas"], sc["sqrt_info"], sc["fixed"], max_iterations=1)
            finally:
                ctx.set_pose_graph_solver("dense")
        cov()                                       # the warm-up: the buffers grow here
        wall = []
        for _ in range(a.calls):
            t = time.perf_counter()
            cov()
            wall.append((time.perf_counter() - t) * 1e3)
        st = staged(ctx, cov, ("cov_", "solver_"))
        solve()
        it = staged(ctx, solve, ("solver_",))
        row = dict(scene=name, K=K, E=int(len(sc["edge_a"])), n=6 * an["n_free"], ordering=an["ordering"], envelope_blocks=an["envelope_blocks"],
                   P=int(len(poses_of)), Q=int(len(pairs)), ms_per_call=float(np.median(wall)), calls_ms=wall,
                   stage_ms={n: v for n, v in sorted(st.items())}, solve_solver_factor_ms=it.get("solver_factor", 0.0))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
