#!/usr/bin/env python3
"""Tracking rate of HipKeyframeTracker over one recorded stream, frame by frame and in windows.

A tests/track_ref.py::make_sequence stream (default 256 frames) is tracked by processSensorData, one Context.track call per
frame, and by process_window at windows 4 / 16 / 64, one Context.track_window call per window.  The runs alternate in blocks
(per frame, window 4, 16, 64, then again) and are repeated in one process on one context, so the second repetition finds
every scratch buffer allocated.  Prints one JSON line: frames/s of every run, the window calls made and the share of frames
that were computed behind an event and discarded.  Nothing is fixed in advance: a window form that loses is reported as such.

    python tools/track_throughput.py [--frames 256] [--repeats 2] [--windows 4,16,64] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as graft  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--windows", default="4,16,64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import track_ref as tr
    pkg = graft.load_package()
    seq = tr.make_sequence(seed=0, n_frames=a.frames)
    fr = seq["frames"]
    descs, xys, depths = [x["desc"] for x in fr], [x["xy"] for x in fr], [x["depth"] for x in fr]
    ctx = pkg.Context(width=0, height=0, max_keypoints=1024)
    modes = [("per_frame", None)] + [("window_%d" % int(w), int(w)) for w in a.windows.split(",")]
    runs = {name: [] for name, _ in modes}
    shape = {}
    for rep in range(a.repeats):
        for name, window in modes:
            ctx.kf_clear()
            t = pkg.HipKeyframeTracker(ctx, focal=tr.CAM[:2], principal=tr.CAM[2:], **tr.SEQ_PARAMS)
            ctx.sync()
            t0 = time.perf_counter()
            if window is None:
                rows = [t.processSensorData(d, p, z) for d, p, z in zip(descs, xys, depths)]
            else:
                rows = t.process_window(descs, xys, depths, window=window)
            ctx.sync()
            dt = time.perf_counter() - t0
            runs[name].append(len(rows) / dt)
            summary = dict(keyframes=[f for f, r in enumerate(rows) if r["keyframe"] >= 0], tracked=sum(bool(r["tracked"]) for r in rows),
                           calls=t.window_calls if window else len(rows) - 1,
                           discarded_share=(t.window_discarded / t.window_computed) if window and t.window_computed else 0.0)
            if name in shape and (shape[name]["keyframes"], shape[name]["tracked"]) != (summary["keyframes"], summary["tracked"]):
                raise SystemExit("%s: two repetitions tracked the stream differently" % name)
            shape[name] = summary
    base = max(runs["per_frame"])
    out = dict(tool="track_throughput", frames=a.frames, repeats=a.repeats, keypoints_per_frame=sum(len(d) for d in descs) / len(descs),
               modes={name: dict(frames_per_s=max(v), frames_per_s_runs=v, speedup_over_per_frame=max(v) / base, **shape[name])
                      for name, v in runs.items()})
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
