"""Latency of landmark culling (mslam_hip_kf_cull_landmarks), in the style of tools/cull_latency.py.  Maps of --listed
(16, 64 and 4096) entries laid out as a camera's run of keyframes leaves them: entry e holds `shared` ids of a window that
slides over one sequence of landmarks, so that each of those is held by --overlap (6) consecutive entries, and `own` ids
nobody else holds (part B's never-seen-again landmarks); --landmarks gives shared + own per map size (1000 = 700 + 300 for
the tracker's shapes, 300 = 200 + 100 at 4096 entries).  The candidates are two entries --age (2) from the end of the map, as
the tracker names them (it names one per keyframe; two bounds it from above).  Timed through the Python mirror:
  - the fused call on a fresh map (it removes the candidates' own landmarks), one sample per refill, the median of --fills;
  - the fused call again on the same map (nothing is left to cull: the counts, flags and gather alone), median of --calls;
  - the search on a fresh map, median of --calls;
  - mslam_hip_kf_cull on the same map with the same candidates and ratio = 1.0, which culls nothing and so leaves the map as
    it is: the yardstick, median of --calls.
With the stage timers on (Context.set_profiling, mode 2) one more fused call on a fresh map reports the event time of every
stage (lmcull_upload, cull_clear, cull_count, lmcull_judge, lmcull_gather, lmcull_compact).
--walk: HipKeyframeTracker(local_map_depth=2, local_ba=True) over tests/lm_cull_ref.py's sequence with and without lm_cull:
the wall time of the lm_cull step per keyframe (the call and the backend's bookkeeping), the frame time, and the size of the
last union.  There is no pass / fail threshold.

usage: python tools/lm_cull_latency.py [--listed 16,64,4096] [--landmarks 1000,1000,300] [--calls 30] [--fills 5] [--walk]
                                       [--out profiles/lm_cull_latency.json]"""
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


def fill(ctx, E, n, own, overlap, rng, desc, world):
    ctx.kf_clear()
    shared = n - own
    step = max(shared // overlap, 1)
    for e in range(E):
        lids = np.concatenate([e * step + rng.permutation(shared), (1 << 40) + e * n + np.arange(own)]).astype(np.int64)
        ctx.kf_add(e, desc, world, lids=lids)


def timed(f, calls):
    ms = []
    for _ in range(calls):
        t = time.perf_counter()
        f()
        ms.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def walk(pkg):
    import lm_cull_ref as lc
    import track_ref as tr
    seq = lc.sequence()
    out = {}
    for on in (False, True):
        ctx = pkg.Context(width=0, height=0, max_keypoints=2048)
        t = pkg.HipKeyframeTracker(ctx, focal=tr.CAM[:2], principal=tr.CAM[2:], local_map_depth=lc.DEPTH, local_ba=True, lm_cull=on,
                                   **lc.PARAMS)
        made, real = [], t._lm_cull

        def spy(new_id, t=t, made=made, real=real):
            t0, before = time.perf_counter(), len(t.lm_cull_results)
            real(new_id)
            if len(t.lm_cull_results) > before:      # a call was made: the step's wall time
                made.append((time.perf_counter() - t0) * 1e3)
        t._lm_cull = spy
        frame_ms, unions = [], []
        for fr in seq["frames"]:
            t0 = time.perf_counter()
            o = t.processSensorData(fr["desc"], fr["xy"], fr["depth"])
            frame_ms.append((time.perf_counter() - t0) * 1e3)
            assert o["tracked"]
            unions.append(len(ctx.kf_read_ids(t.LOCAL_MAP_ID)) if len(t.ids) > 1 else 0)
        out["lm_cull" if on else "plain"] = dict(
            keyframes=len(t.ids), store_landmarks=int(sum(len(ctx.kf_read_ids(k)) for k in t.ids)), last_union=int(unions[-1]),
            frame_ms_median=float(np.median(frame_ms[1:])), lm_cull_calls=len(t.lm_cull_results),
            lm_cull_step_ms_median=float(np.median(made)) if made else 0.0, lm_cull_step_ms_max=float(np.max(made)) if made else 0.0,
            removed=[int(r["n_removed"]) for r in t.lm_cull_results])
        ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--listed", default="16,64,4096")
    ap.add_argument("--landmarks", default="1000,1000,300")
    ap.add_argument("--own", type=float, default=0.3, help="the share of an entry's landmarks nobody else holds")
    ap.add_argument("--overlap", type=int, default=6)
    ap.add_argument("--age", type=int, default=2)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--fills", type=int, default=5)
    ap.add_argument("--walk", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_cull_latency.json"))
    a = ap.parse_args()
    pkg = graft.load_package()
    rng = np.random.default_rng(0)
    cases = []
    for E, n in zip([int(x) for x in a.listed.split(",")], [int(x) for x in a.landmarks.split(",")]):
        own = int(round(a.own * n))
        ctx = pkg.Context(width=0, height=0, max_keypoints=n)
        desc, world = rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.normal(size=(n, 3))
        ids = np.arange(E, dtype=np.int32)
        cand = ids[max(E - a.age - 2, 0):max(E - a.age, 1)]
        fills = a.fills if E <= 256 else 2
        fill(ctx, E, n, own, a.overlap, rng, desc, world)
        ctx.kf_cull_landmarks(ids, cand)       # warm-up: allocations and code objects
        fresh = []
        for _ in range(fills):
            fill(ctx, E, n, own, a.overlap, rng, desc, world)
            t = time.perf_counter()
            got = ctx.kf_cull_landmarks(ids, cand)
            fresh.append((time.perf_counter() - t) * 1e3)
        again = timed(lambda: ctx.kf_cull_landmarks(ids, cand), a.calls)
        fill(ctx, E, n, own, a.overlap, rng, desc, world)
        search = timed(lambda: ctx.kf_cull_landmarks_search(ids, cand), a.calls)
        kf_cull = timed(lambda: ctx.kf_cull(ids, cand, ratio=1.0), a.calls)
        assert ctx.kf_size() == E
        ctx.set_profiling(2)
        ctx.stage_times()
        ctx.kf_cull_landmarks(ids, cand)
        stages = {}
        for name, t_ms in ctx.stage_times(cap=8192):
            if name.startswith("cull_") or name.startswith("lmcull_"):
                stages[name] = stages.get(name, 0.0) + float(t_ms)
        ctx.set_profiling(0)
        chunks = (E + 63) // 64
        cases.append(dict(listed=E, landmarks=n, own=own, candidates=int(len(cand)), found=int(len(got["landmark_ids"])),
                          removed=int(got["n_removed"]), clears=3, launches=2 * chunks + 3,
                          kf_cull_landmarks_fresh_ms=float(np.median(fresh)), kf_cull_landmarks_fresh_min_ms=float(np.min(fresh)),
                          kf_cull_landmarks_again_ms=again[0], kf_cull_landmarks_again_min_ms=again[1], kf_cull_landmarks_again_max_ms=again[2],
                          kf_cull_landmarks_search_ms=search[0], kf_cull_ratio_1_ms=kf_cull[0], kf_cull_ratio_1_min_ms=kf_cull[1],
                          stage_ms=stages))
        print(json.dumps(cases[-1]), flush=True)
        ctx.close()
    row = dict(calls=a.calls, fills=a.fills, overlap=a.overlap, age=a.age, cases=cases)
    if a.walk:
        row["walk"] = walk(pkg)
        print(json.dumps(row["walk"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
