"""Latency of RANSAC rigid alignment (mslam_hip_align_ransac) next to RANSAC PnP (mslam_hip_pnp_ransac) on the same
correspondences, and of Context.track in both pose modes on the synthetic tracking sequence.  There is no pass / fail threshold.

Part 1, per (n, outlier share): one scene of tests/align_ref.py (noise 5 mm).  The alignment sees (world point, camera point);
PnP sees (world point, the camera point's projection with the TUM intrinsics), so both problems have the same inliers.  Both run
100 hypotheses at most, confidence 0.99 (the early exit on), max_distance 0.05 m / 5 px.  Timed through the Python mirror: a host
clock around a call that uploads the points, runs one workgroup and ends in a device synchronise — so what is compared is the
call a user makes, copies and launch included, not the kernel alone.  After --warmup calls of each, --calls calls alternate
(align, pnp, align, ...); the medians and the quartiles are reported, with the inlier counts of both.

Part 2: Context.track over tests/track_ref.make_sequence() (32 frames) against keyframe 0's successors as the reference loop
inserts them, once per mode per frame, alternating the modes per frame, --track-rounds times; the median per-call time of each
mode and how many frames each tracked.  With the stage timers on (Context.set_profiling, mode 2) one more pass reports the
device time of the pose stage alone (pnp_ransac / align_ransac) per frame.

usage: python tools/align_latency.py [--calls 200] [--warmup 20] [--track-rounds 5] [--out profiles/align_latency.json]"""
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

CAM = (525.0, 525.0, 319.5, 239.5)


def quartiles(ms):
    q = np.percentile(np.asarray(ms), [25, 50, 75])
    return dict(median_ms=float(q[1]), q25_ms=float(q[0]), q75_ms=float(q[2]))


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def part_estimators(ctx, ar, calls, warmup):
    rows = []
    for n in (100, 500, 2000):
        for outl in (0.0, 0.3, 0.6):
            src, dst, R, t, good = ar.scene(1000 + n, n, outl, 0.005)
            d = dst.astype(np.float64)
            img = np.stack([CAM[0] * d[:, 0] / d[:, 2] + CAM[2], CAM[1] * d[:, 1] / d[:, 2] + CAM[3]], 1).astype(np.float32)
            align = lambda: ctx.align_ransac(src, dst, 0.05, 100, 7)
            pnp = lambda: ctx.pnp_ransac(src, img, CAM[:2], CAM[2:], iterations=100, reprojection_error=5.0, seed=7)
            for _ in range(warmup):
                align(), pnp()
            ta, tp, ra, rp = [], [], None, None
            for _ in range(calls):
                ms, ra = timed(align)
                ta.append(ms)
                ms, rp = timed(pnp)
                tp.append(ms)
            rows.append(dict(n=n, outliers=outl, align=dict(quartiles(ta), inliers=None if ra is None else int(ra[2].sum())),
                             pnp=dict(quartiles(tp), inliers=None if rp is None else int(rp[2].sum()))))
            print(rows[-1], file=sys.stderr)
    return rows


def part_track(pkg, tr, tar, rounds):
    seq = tr.make_sequence(seed=0)
    rows, trk = tar.run_reference(seq, 0.05)                  # the stores and references of the loop, frame by frame
    ctx = pkg.Context(width=0, height=0, max_keypoints=1024)
    times = {"pnp": [], "align": []}
    tracked = {"pnp": 0, "align": 0}
    stage = {"pnp": [], "align": []}

    def steps():
        for f in range(1, len(rows)):
            ids = [i for i in trk.ids if i <= max(r["keyframe"] for r in rows[:f])]
            yield f, ids, rows[f - 1]["reference"], seq["frames"][f]
    loaded = None
    for rnd in range(rounds + 2):                             # round 0: warm-up; the last: stage timers on
        staged = rnd == rounds + 1
        for f, ids, ref_id, fr in steps():
            if loaded != ids:
                ctx.kf_clear()
                for i in ids:
                    ctx.kf_add(i, *trk.store[i])
                loaded = ids
            for mode in (("pnp", "align") if f % 2 else ("align", "pnp")):
                ctx.set_track_pose(mode, 0.05 if mode == "align" else 0.0)
                if staged:
                    ctx.set_profiling(2)
                    ctx.stage_times()
                ms, res = timed(lambda: ctx.track(fr["desc"], fr["xy"], fr["depth"], ref_id, ids, -1, seed=f,
                                                  new_keyframe_min_landmarks=tr.SEQ_PARAMS["new_keyframe_min_landmarks"]))
                if staged:
                    st = dict((k, v) for k, v in ctx.stage_times(cap=256))
                    ctx.set_profiling(0)
                    stage[mode].append(float(st.get("align_ransac" if mode == "align" else "pnp_ransac", np.nan)))
                elif rnd >= 1:
                    times[mode].append(ms)
                    tracked[mode] += int(bool(res["tracked"])) if rnd == 1 else 0
    ctx.close()
    return {m: dict(quartiles(times[m]), tracked_frames=tracked[m], frames=len(rows) - 1,
                    pose_stage_device_ms_median=float(np.nanmedian(stage[m]))) for m in times}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--track-rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = graft.load_package()
    graft.load_oracle().lib()
    import align_ref as ar
    import track_align_ref as tar
    import track_ref as tr
    ctx = pkg.Context(width=0, height=0)
    out = dict(tool="align_latency", calls=a.calls, warmup=a.warmup, estimators=part_estimators(ctx, ar, a.calls, a.warmup))
    ctx.close()
    out["track"] = part_track(pkg, tr, tar, a.track_rounds)
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
