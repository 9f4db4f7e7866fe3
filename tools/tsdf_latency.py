"""Latency of the dense TSDF map (mslam_hip_tsdf_*, k_tsdf.hip) at 256^3 and 512^3 voxels with 640 x 480 frames.  There is no
pass / fail threshold.

The scene: a 5.12 m cube in front of the camera (voxel 2 cm / 1 cm, truncation 4 voxels, max_depth 3 m), depth images of a wavy
wall 1.6 .. 2.4 m away, cameras that pan and slide a little round the first one.  Every timed call goes through the Python mirror
and ends in a device synchronise (every mslam_hip_tsdf_* call drains the context's stream), so a host clock round the call is
the time a user waits: upload, launches and synchronise included.

  add_frame       one frame: a 600 KB upload and one sweep with one entry; the median over the frames added.
  update_poses    n = 1, 64, 512 frames moved between two pose sets, alternating: 2 n entries, ceil(2 n / 64) sweeps.
                  bytes = sweeps x 16 B x voxels (8 B read + 8 B written per voxel and sweep: the upper bound, a voxel that no
                  entry changes is not written) over the call's time, next to the 6.3 TB/s the memory system achieves.  The sweep
                  is f64 arithmetic per (voxel, entry) as well, so the figure says how far from a pure copy the call is.
  extract         the count call and the fill (Context.tsdf_extract), and the number of points.
  batch           what justifies the batched launch: update_poses of n = 64 frames (2 sweeps of 64 entries) against the same
                  128 entries as single-entry launches of the same kernel (remove_frame, then add_frame at the new pose, per
                  frame).  Both as host time and as device time of the `tsdf_sweep` stage alone (Context.set_profiling(2)),
                  which leaves the uploads of the unbatched path out.

usage: python tools/tsdf_latency.py [--reps 7] [--frames 512] [--dims 256 512] [--out profiles/tsdf_latency.json]"""
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

ACHIEVABLE_TBS = 6.3    # HBM, achievable (the microarchitecture notes' figure)
EDGE = 5.12             # metres
W, H = 640, 480
CAM = (525.0, 525.0, 319.5, 239.5)


def quartiles(ms):
    q = np.percentile(np.asarray(ms, np.float64), [25, 50, 75])
    return dict(median_ms=float(q[1]), q25_ms=float(q[0]), q75_ms=float(q[2]), n=len(ms))


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def make_frames(n, seed):
    """n depth images and two pose sets (world -> camera)"""
    import tsdf_ref as tr
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    depths, a, b = [], [], []
    for q in range(n):
        z = 2.0 + 0.4 * np.sin(u / 47.0 + 0.1 * q) * np.cos(v / 61.0 - 0.07 * q)
        depths.append(np.rint(z * 5000.0).astype(np.uint16))
        for out in (a, b):
            R = tr.rot(1, rng.uniform(-0.3, 0.3)) @ tr.rot(0, rng.uniform(-0.15, 0.15))
            out.append((R, rng.uniform(-0.4, 0.4, 3) * np.array([1.0, 0.5, 0.3])))
    return depths, a, b


def sweep_ms(ctx):
    return float(sum(ms for name, ms in ctx.stage_times(cap=4096) if name == "tsdf_sweep"))


def measure(pkg, dims, depths, pa, pb, reps):
    n_frames = len(depths)
    voxels = dims ** 3
    ctx = pkg.Context(width=0, height=0)
    ctx.tsdf_create((dims,) * 3, EDGE / dims, (-EDGE / 2, -EDGE / 2, 0.2), None, 3.0, max(n_frames, 1), W, H, 1.0 / 5000.0, CAM[:2], CAM[2:])
    out = dict(dims=dims, voxels=voxels, volume_mib=voxels * 8 / 2 ** 20)
    add = [timed(lambda q=q: ctx.tsdf_add_frame(q, depths[q], *pa[q]))[0] for q in range(n_frames)]
    out["add_frame"] = quartiles(add[2:])
    where = [pa, pb]
    side = 0
    out["update_poses"] = []
    for n in (1, 64, 512):
        if n > n_frames:
            continue
        ids = list(range(n))
        ts = []
        for r in range(reps + 1):
            side ^= 1
            P = where[side]
            ms, moved = timed(lambda: ctx.tsdf_update_poses(ids, np.stack([P[q][0] for q in ids]), np.stack([P[q][1] for q in ids])))
            assert moved == n
            if r:
                ts.append(ms)
        # (frames n .. stay where they are; frames below n are now at where[side])
        sweeps = -(-2 * n // pkg.TSDF_CHUNK)
        q = quartiles(ts)
        nbytes = sweeps * 16 * voxels
        out["update_poses"].append(dict(q, frames=n, entries=2 * n, sweeps=sweeps, bytes=nbytes,
                                        tb_per_s=nbytes / (q["median_ms"] * 1e-3) / 1e12, achievable_tb_per_s=ACHIEVABLE_TBS))
        # every list leaves its frames on the same side for the next one
        if side != 0:
            P = where[0]
            ctx.tsdf_update_poses(ids, np.stack([P[q][0] for q in ids]), np.stack([P[q][1] for q in ids]))
            side = 0
    ex = []
    for r in range(reps + 1):
        ms, (xyz, nrm) = timed(lambda: ctx.tsdf_extract(1))
        if r:
            ex.append(ms)
    out["extract"] = dict(quartiles(ex), points=int(len(xyz)))
    # the batch against single-entry launches, n = 64 frames between the two pose sets
    n = min(64, n_frames)
    ids = list(range(n))
    batched, single, batched_dev, single_dev = [], [], [], []
    ctx.set_profiling(2)
    ctx.stage_times(cap=4096)
    for r in range(reps + 1):
        side ^= 1
        P = where[side]
        ms, _ = timed(lambda: ctx.tsdf_update_poses(ids, np.stack([P[q][0] for q in ids]), np.stack([P[q][1] for q in ids])))
        dev = sweep_ms(ctx)
        side ^= 1
        P = where[side]

        def one_by_one():
            for q in ids:
                ctx.tsdf_remove_frame(q)
                ctx.tsdf_add_frame(q, depths[q], *P[q])
        ms1, _ = timed(one_by_one)
        dev1 = sweep_ms(ctx)
        if r:
            batched.append(ms), single.append(ms1), batched_dev.append(dev), single_dev.append(dev1)
    ctx.set_profiling(0)
    out["batch"] = dict(frames=n, entries=2 * n, batched_host=quartiles(batched), single_host=quartiles(single),
                        batched_sweep_device=quartiles(batched_dev), single_sweep_device=quartiles(single_dev),
                        device_ratio=float(np.median(single_dev) / np.median(batched_dev)))
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--dims", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = graft.load_package()
    depths, pa, pb = make_frames(a.frames, 3)
    out = dict(tool="tsdf_latency", reps=a.reps, frames=a.frames, width=W, height=H, chunk=pkg.TSDF_CHUNK, volumes=[])
    for dims in a.dims:
        out["volumes"].append(measure(pkg, dims, depths, pa, pb, a.reps))
        print(json.dumps(out["volumes"][-1]), file=sys.stderr)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
