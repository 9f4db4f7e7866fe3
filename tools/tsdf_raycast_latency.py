"""Latency of the ray-cast of the dense TSDF map (mslam_hip_tsdf_raycast, k_tsdf_raycast.hip): a 640 x 480 render of a 256^3
and a 512^3 volume at the default parameters (step voxel / 2, coarse trunc / (2 step) = 4) and with coarse = 1, next to one
tsdf_extract of the same volume for scale.  There is no pass / fail threshold.

The scene: a 5.12 m cube in front of the first camera (voxel 2 cm / 1 cm, truncation 4 voxels, max_depth 3 m), filled from
analytic renders (tests/tsdf_ref.py) of a sphere of radius 0.5 m at 1.8 m in front of a wall at 2.7 m, seen from a few cameras
that pan and slide round the first one.  Two views are rendered: the first camera's and a tilted one.

  device_ms   the `tsdf_raycast` stage alone (Context.set_profiling(2): HIP events round the launch), the call rendering into
              device buffers: the kernel's time.
  host_ms     a host clock round Context.tsdf_raycast with host arrays, which ends in a device synchronise: launch, the
              kernel, 8.6 MB of copies back (depth, xyz, normal) and the synchronise, as a user of the host form waits.
  warm-up, then `reps` timed calls; median and quartiles.
  evaluations the field evaluations the numpy reference (tests/tsdf_raycast_ref.py) counts for the same view through a
              camera of 80 x 60 pixels (every 8th ray), for both strides: the work ratio the coarse stride is there to buy,
              to be read next to the ratio of the two device times.  nominal_bytes = evaluations x 64 (8 corners of 8 B) x 64
              rays per reference ray, over device time: the rate at which the kernel's loads are SERVED (mostly by the vector
              cache: the 64 rays of a wave's 8 x 8 tile touch a few dozen distinct voxels per sample), not a DRAM rate.

usage: python tools/tsdf_raycast_latency.py [--reps 9] [--dims 256 512] [--out profiles/tsdf_raycast_latency.json]"""
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
SUB = 8                 # the reference counts every SUB-th ray in both directions


def quartiles(ms):
    q = np.percentile(np.asarray(ms, np.float64), [25, 50, 75])
    return dict(median_ms=float(q[1]), q25_ms=float(q[0]), q75_ms=float(q[2]), n=len(ms))


def make_frames(p):
    """depth images of the sphere in front of the wall, and their world -> camera poses"""
    import tsdf_ref as tr
    poses = [(np.eye(3), np.zeros(3))]
    for a, b, t in ((0.2, 0.0, (0.3, 0.0, 0.0)), (-0.2, 0.05, (-0.3, 0.05, 0.0)), (0.1, -0.1, (0.1, -0.2, 0.05)),
                    (-0.1, 0.1, (-0.1, 0.2, 0.05)), (0.3, 0.0, (0.5, 0.0, 0.1))):
        poses.append((tr.rot(1, a) @ tr.rot(0, b), np.array(t)))
    frames = []
    for R, t in poses:
        ball = tr.render_sphere(p, R, t, centre=(0.0, 0.0, 1.8), radius=0.5)
        wall = tr.render_plane(p, R, t, (0.0, 0.0, 1.0), 2.7)
        frames.append((np.where(ball > 0, ball, wall).astype(np.uint16), R, t))
    return frames


def stage_ms(ctx):
    return float(sum(ms for name, ms in ctx.stage_times(cap=4096) if name == "tsdf_raycast"))


def measure(pkg, dims, reps):
    import torch
    import tsdf_ref as tr
    import tsdf_raycast_ref as rr
    voxel = EDGE / dims
    p = tr.params((dims,) * 3, voxel, (-EDGE / 2, -EDGE / 2, 0.2), None, 3.0, 16, W, H, 1.0 / 5000.0, CAM[:2], CAM[2:])
    frames = make_frames(p)
    ctx = pkg.Context(width=0, height=0)
    ctx.tsdf_create(**tr.create_kwargs(p))
    for q, (d, R, t) in enumerate(frames):
        ctx.tsdf_add_frame(q, d, R, t)
    out = dict(dims=dims, voxels=dims ** 3, volume_mib=dims ** 3 * 8 / 2 ** 20, voxel=voxel, frames=len(frames), views=[])
    S, Wt = ctx.tsdf_read()
    sub = dict(width=W // SUB, height=H // SUB, focal=(CAM[0] / SUB, CAM[1] / SUB), principal=((CAM[2] - (SUB - 1) / 2) / SUB,
                                                                                               (CAM[3] - (SUB - 1) / 2) / SUB))
    d_depth = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    d_xyz = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    d_nrm = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ptrs = (d_depth.data_ptr(), d_xyz.data_ptr(), d_nrm.data_ptr())
    views = {"first": (np.eye(3), np.zeros(3)), "tilted": (tr.rot(1, -0.25) @ tr.rot(0, 0.1), np.array([-0.4, 0.15, 0.1]))}
    for name, (R, t) in views.items():
        row = dict(view=name)
        for label, coarse in (("default", None), ("coarse_1", 1)):
            q = ctx.tsdf_raycast_params(R, t, coarse=coarse)
            ctx.set_profiling(2)
            ctx.stage_times(cap=4096)
            dev, host, hits = [], [], 0
            for r in range(reps + 2):                       # two warm-up calls
                hits = ctx.tsdf_raycast(R, t, coarse=coarse, out=ptrs, with_hits=True)
                ms = stage_ms(ctx)
                if r >= 2:
                    dev.append(ms)
            ctx.set_profiling(0)
            for r in range(reps + 2):
                t0 = time.perf_counter()
                got = ctx.tsdf_raycast(R, t, coarse=coarse)
                ms = (time.perf_counter() - t0) * 1e3
                if r >= 2:
                    host.append(ms)
            assert got[0].tobytes() == d_depth.cpu().numpy().tobytes()    # both forms: the same image
            stats = rr.raycast(S, Wt, p, R, t, camera=sub, coarse=coarse, with_stats=True)[3]
            dq = quartiles(dev)
            nominal = stats["evaluations"] * 64 * SUB * SUB
            row[label] = dict(coarse=q.coarse, step=q.step, z_far=q.z_far, samples=stats["n_last"] + 1, hits=int(hits), device=dq,
                              host=quartiles(host), reference_evaluations=stats["evaluations"], reference_rays=sub["width"] * sub["height"],
                              reference_hits=stats["hits"], nominal_bytes=nominal,
                              nominal_tb_per_s=nominal / (dq["median_ms"] * 1e-3) / 1e12)
        row["device_ratio_fine_over_coarse"] = row["coarse_1"]["device"]["median_ms"] / row["default"]["device"]["median_ms"]
        row["evaluation_ratio_fine_over_coarse"] = row["coarse_1"]["reference_evaluations"] / row["default"]["reference_evaluations"]
        out["views"].append(row)
    ex = []
    for r in range(reps + 2):
        t0 = time.perf_counter()
        xyz, _ = ctx.tsdf_extract(1)
        if r >= 2:
            ex.append((time.perf_counter() - t0) * 1e3)
    out["extract"] = dict(quartiles(ex), points=int(len(xyz)))
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--dims", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = graft.load_package()
    out = dict(tool="tsdf_raycast_latency", reps=a.reps, width=W, height=H, volumes=[])
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
