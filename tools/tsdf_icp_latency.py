"""Latency of frame-to-model alignment on the dense TSDF map (mslam_hip_tsdf_icp, k_icp.hip after k_tsdf_raycast.hip): a
640 x 480 depth frame against a 256^3 and a 512^3 volume with the default levels ((4, 4), (2, 5), (1, 10): 19 scheduled
iterations) and gates.  There is no pass / fail threshold: nothing earlier exists to compare with.

The scene: a 5.12 m cube in front of the first camera (voxel 2 cm / 1 cm, truncation 4 voxels, max_depth 3 m), filled from
analytic renders of the room corner of tests/tsdf_icp_ref.py with its apex at 2.4 m, seen from a few cameras that pan and slide
round the first one.  The frame is rendered 27 mm / 44 mrad away from the guess (tsdf_icp_ref.TRUE_POSE); the guess is the
first camera.

  stages      Context.set_profiling(2) puts HIP events round every launch: per call the sum of each stage's launches
              (tsdf_raycast 1, icp_frame 1, icp_linearize 19, icp_finish 19) and their total, the device time of a call
              without the gaps between the launches.
  host_ms     a host clock round Context.tsdf_icp with a host depth image (profiling off), which ends in the one device
              synchronise of the call: the upload of the frame (0.6 MB), 40 launches, the copy back, as a caller waits.
  host_dev_ms the same with the depth image already on the device.
  warm-up, then `reps` timed calls; median and quartiles.  launches: counted from the stage list.

usage: python tools/tsdf_icp_latency.py [--reps 9] [--dims 256 512] [--out profiles/tsdf_icp_latency.json]"""
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

EDGE = 5.12             # metres
W, H = 640, 480
CAM = (525.0, 525.0, 319.5, 239.5)
APEX = (0.05, -0.04, 2.4)
STAGES = ("tsdf_raycast", "icp_frame", "icp_linearize", "icp_finish")


def quartiles(ms):
    q = np.percentile(np.asarray(ms, np.float64), [25, 50, 75])
    return dict(median_ms=float(q[1]), q25_ms=float(q[0]), q75_ms=float(q[2]), n=len(ms))


def measure(pkg, dims, reps):
    import torch
    import tsdf_ref as tr
    import tsdf_icp_ref as ir
    voxel = EDGE / dims
    p = tr.params((dims,) * 3, voxel, (-EDGE / 2, -EDGE / 2, 0.2), None, 3.0, 16, W, H, 1.0 / 5000.0, CAM[:2], CAM[2:])
    poses = [(np.eye(3), np.zeros(3))]
    for a, b, t in ((0.2, 0.0, (0.3, 0.0, 0.0)), (-0.2, 0.05, (-0.3, 0.05, 0.0)), (0.1, -0.1, (0.1, -0.2, 0.05)),
                    (-0.1, 0.1, (-0.1, 0.2, 0.05))):
        poses.append((tr.rot(1, a) @ tr.rot(0, b), np.array(t)))
    ctx = pkg.Context(width=0, height=0)
    ctx.tsdf_create(**tr.create_kwargs(p))
    for q, (R, t) in enumerate(poses):
        ctx.tsdf_add_frame(q, ir.render_corner(p, R, t, APEX), R, t)
    depth = ir.render_corner(p, *ir.TRUE_POSE, APEX)
    d_depth = torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).cuda()
    torch.cuda.synchronize()
    I, Z = np.eye(3), np.zeros(3)
    out = dict(dims=dims, voxels=dims ** 3, volume_mib=dims ** 3 * 8 / 2 ** 20, voxel=voxel, frames=len(poses))
    ctx.set_profiling(2)
    ctx.stage_times(cap=4096)
    per_stage, totals, launches, res = {s: [] for s in STAGES}, [], None, None
    for r in range(reps + 2):                       # two warm-up calls
        res = ctx.tsdf_icp(d_depth.data_ptr(), I, Z)
        times = ctx.stage_times(cap=4096)
        assert all(name in STAGES for name, _ in times), sorted(set(name for name, _ in times))
        launches = {s: sum(1 for name, _ in times if name == s) for s in STAGES}
        if r >= 2:
            for s in STAGES:
                per_stage[s].append(float(sum(ms for name, ms in times if name == s)))
            totals.append(float(sum(ms for _, ms in times)))
    ctx.set_profiling(0)
    host, host_dev = [], []
    for r in range(reps + 2):
        t0 = time.perf_counter()
        got = ctx.tsdf_icp(depth, I, Z)
        t1 = time.perf_counter()
        got_dev = ctx.tsdf_icp(d_depth.data_ptr(), I, Z)
        t2 = time.perf_counter()
        if r >= 2:
            host.append((t1 - t0) * 1e3)
            host_dev.append((t2 - t1) * 1e3)
    assert got["R"].tobytes() == res["R"].tobytes() == got_dev["R"].tobytes() and got["record"].tobytes() == res["record"].tobytes()
    e0, e1 = ir.pose_error(I, Z, *ir.TRUE_POSE), ir.pose_error(res["R"], res["t"], *ir.TRUE_POSE)
    out.update(launches=launches, launches_per_call=sum(launches.values()), stages={s: quartiles(v) for s, v in per_stage.items()},
               device_total=quartiles(totals), host=quartiles(host), host_dev=quartiles(host_dev), status=int(res["status"]),
               iterations=int(res["iterations"]), pairs=int(res["count"]), pairs_per_level=[int(res["record"]["count"][res["record"]["level"] == l][-1]) for l in range(3)],
               rms_mm=float(1e3 * np.sqrt(res["cost"] / max(res["count"], 1))),
               start_error_mm_mrad=[1e3 * e0[0], 1e3 * e0[1]], end_error_mm_mrad=[1e3 * e1[0], 1e3 * e1[1]])
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--dims", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = graft.load_package()
    out = dict(tool="tsdf_icp_latency", reps=a.reps, width=W, height=H, levels=[list(l) for l in pkg.ICP_LEVELS], volumes=[])
    for dims in a.dims:
        out["volumes"].append(measure(pkg, dims, a.reps))
        print(json.dumps(out["volumes"][-1]), file=sys.stderr)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
