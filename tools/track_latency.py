"""Latency of one mslam_hip_track call that inserts a keyframe (about 1900 query keypoints, a reference entry of 600
landmarks, 8 vote ids) against the composition it replaces on the same inputs: mslam_hip_backproject, mslam_hip_relocalize
with one candidate and the depth mask, the vote in numpy on copies of the entries read beforehand, and the entry assembled
on the host and uploaded with mslam_hip_kf_add.  Both go through the Python mirror with arrays prepared beforehand; the two
are timed alternately, in blocks, so that drift of the machine hits both, and the whole measurement is repeated (--runs) in
the same process: the difference between the runs is the spread a difference between the sides has to exceed.

usage: python tools/track_latency.py [--blocks 12] [--calls 100] [--runs 2] [--out file.json] [--trace new|old]
       (--trace: a short run of one side only, for rocprofv3 --kernel-trace --stats)

--local-map: tracking against the local map instead (16 keyframes of 1500 landmarks, each sharing half of them with the
next one, so their union holds 12750; the same query).  Timed alternately, in blocks, in the same process: the union
build on its own (mslam_hip_kf_union of the 16 entries, one synchronisation), the track step against the union, and the
single-reference track step against one of the 16 entries.  A tracker pays the build only when the reference keyframe
changes or a keyframe is added, the step every frame.

--local-map --guided <radius>: every track step gets the scene's true pose as its guess, and two more sides join the
alternation: the step against the union and against the single entry with mslam_hip_set_guided_match(radius,
--max-distance) on (the setter is switched per call: a host-side assignment)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=12)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out")
    ap.add_argument("--trace", choices=["new", "old"])
    ap.add_argument("--local-map", action="store_true")
    ap.add_argument("--guided", type=float, default=0.0, metavar="RADIUS")
    ap.add_argument("--max-distance", type=int, default=256, help="the guided sides' distance gate")
    a = ap.parse_args()
    import reloc_ref as rr
    import track_ref as tr
    pkg = graft.load_package()
    if a.local_map:
        return local_map(a, pkg, rr)
    sc = rr.make_scene(seed=0, n_kf=8, n_landmarks=600, n_distractors=1360)        # 540 + 1360 = 1900 query keypoints
    ids, ref_id, new_id = sc["ids"], sc["target_id"], 500
    desc, xy = sc["desc"], sc["xy"]
    # a depth image consistent with the query: the landmark's camera z at its pixel, a 2 .. 4 m slope elsewhere
    depth = np.tile(((2.0 + 2.0 * np.arange(640) / 640) * 5000).astype(np.uint16), (480, 1))
    world = sc["store"][ref_id][1]
    for i, l in enumerate(sc["from_landmark"]):
        x, y = int(xy[i, 0]), int(xy[i, 1])
        if l >= 0 and 0 <= x < 640 and 0 <= y < 480:
            depth[y, x] = np.uint16(round(float((sc["R"] @ world[l] + sc["t"])[2]) * 5000))
    c = pkg.Context(width=0, height=0, max_keypoints=2048)
    for cid in ids:
        c.kf_add(cid, *sc["store"][cid])
    copies = {cid: c.kf_read(cid) for cid in ids}
    kw = dict(seed=1, new_keyframe_min_landmarks=1 << 20)                           # every tracked step requires a keyframe

    def new():
        return c.track(desc, xy, depth, ref_id, ids, new_id, with_entry=True, **kw)

    def old():
        xyz, valid = c.backproject(depth, xy)
        r = c.relocalize(desc, xy, [ref_id], valid=valid, seed=1, min_inliers=0, with_pairs=True)
        w = r["candidates"][0]
        R, t = tr.po.rodrigues(w["rvec"]), w["tvec"]
        counts, best = tr.vote(copies, ids, R, t)
        e = tr.build_entry(desc, xyz, valid, r["pairs"][0], r["inliers"][0], copies[ref_id][1], R, t, 3.0)
        c.kf_add(new_id, e["desc"], e["world"])
        return w, counts, best, e
    # same answer (the composition's pose goes through rvec: the lifted points agree to rounding, the rest exactly)
    rn = new()
    gd, gw = c.kf_read(new_id)
    w, counts, best, e = old()
    assert rn["tracked"] and rn["keyframe_added"] and rn["n_inliers"] == w["n_inliers"] and rn["n_entry"] == len(e["kp"])
    assert np.array_equal(rn["vote_counts"], counts) and rn["vote_best"] == best
    assert np.array_equal(rn["entry_kp"], e["kp"]) and np.array_equal(gd, e["desc"]) and np.abs(gw - e["world"]).max() < 1e-9
    if a.trace:
        f = new if a.trace == "new" else old
        for _ in range(50):
            f()
        return
    for _ in range(30):
        new(), old()
    runs = []
    for _ in range(a.runs):
        res = {"new": [], "old": []}
        for _ in range(a.blocks):
            for name, f in (("new", new), ("old", old)):
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    f()                               # every call ends in a device synchronise
                res[name].append((time.perf_counter() - t0) / a.calls * 1e6)
        runs.append({k: dict(median_us=float(np.median(v)), min_us=float(np.min(v)), max_us=float(np.max(v)),
                             blocks=[round(x, 2) for x in v]) for k, v in res.items()})
    out = dict(runs=runs, shape=dict(query=len(desc), reference_landmarks=600, vote_ids=len(ids), calls_per_block=a.calls,
                                     blocks=a.blocks),
               step=dict(n_matches=rn["n_matches"], n_correspondences=rn["n_correspondences"], n_inliers=rn["n_inliers"],
                         n_entry=rn["n_entry"], n_inherited=rn["n_inherited"]))
    text = json.dumps(out, indent=1)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


def local_map(a, pkg, rr):
    n_kf, n_lm, U = 16, 1500, 0x7fffffff
    sc = rr.make_scene(seed=0, n_kf=n_kf, n_landmarks=n_lm, n_distractors=400)
    ids, ref_id, new_id = sc["ids"], sc["target_id"], 500
    desc, xy = sc["desc"], sc["xy"]
    depth = np.tile(((2.0 + 2.0 * np.arange(640) / 640) * 5000).astype(np.uint16), (480, 1))
    world = sc["store"][ref_id][1]
    for i, l in enumerate(sc["from_landmark"]):
        x, y = int(xy[i, 0]), int(xy[i, 1])
        if l >= 0 and 0 <= x < 640 and 0 <= y < 480:
            depth[y, x] = np.uint16(round(float((sc["R"] @ world[l] + sc["t"])[2]) * 5000))
    c = pkg.Context(width=0, height=0, max_keypoints=16384)
    for k, cid in enumerate(ids):                       # entry k shares its upper half with the lower half of entry k + 1
        c.kf_add(cid, *sc["store"][cid], lids=k * (n_lm // 2) + np.arange(n_lm))
    kw = dict(seed=1, new_keyframe_min_landmarks=1 << 20)
    if a.guided > 0:
        R = sc["R"]
        th = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
        kw.update(rvec=th / (2 * np.sin(th)) * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]), tvec=sc["t"])

    def guided(step):
        def run():
            c.set_guided_match(a.guided, a.max_distance, 640, 480)
            try:
                return step()
            finally:
                c.set_guided_match(0.0, 256, 640, 480)
        return run

    def build():
        return c.kf_union(U, ids)

    def step_map():
        return c.track(desc, xy, depth, U, ids, new_id, with_entry=True, **kw)

    def step_single():
        return c.track(desc, xy, depth, ref_id, ids, new_id, with_entry=True, **kw)
    n_union = build()
    rm, rs = step_map(), step_single()
    assert n_union == (n_kf + 1) * (n_lm // 2) and rm["tracked"] and rs["tracked"] and rm["keyframe_added"] and rs["keyframe_added"]
    sides = (("union_build", build), ("track_local_map", step_map), ("track_single_reference", step_single))
    if a.guided > 0:
        sides += (("track_local_map_guided", guided(step_map)), ("track_single_reference_guided", guided(step_single)))
        gm, gs = sides[3][1](), sides[4][1]()
        assert gm["tracked"] and gs["tracked"]
    for _ in range(30):
        for _, f in sides:
            f()
    runs = []
    for _ in range(a.runs):
        res = {name: [] for name, _ in sides}
        for _ in range(a.blocks):
            for name, f in sides:
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    f()                               # every call ends in a device synchronise
                res[name].append((time.perf_counter() - t0) / a.calls * 1e6)
        runs.append({k: dict(median_us=float(np.median(v)), min_us=float(np.min(v)), max_us=float(np.max(v)),
                             blocks=[round(x, 2) for x in v]) for k, v in res.items()})
    c.set_profiling(2)
    build()
    stages = [(n, round(ms * 1e3, 2)) for n, ms in c.stage_times() if n.startswith("union_")]
    c.set_profiling(0)
    out = dict(runs=runs, shape=dict(query=len(desc), keyframes=n_kf, landmarks_per_keyframe=n_lm, union_landmarks=n_union,
                                     vote_ids=len(ids), calls_per_block=a.calls, blocks=a.blocks),
               union_stages_us=stages,
               step_local_map=dict(n_matches=rm["n_matches"], n_correspondences=rm["n_correspondences"], n_inliers=rm["n_inliers"]),
               step_single=dict(n_matches=rs["n_matches"], n_correspondences=rs["n_correspondences"], n_inliers=rs["n_inliers"]))
    if a.guided > 0:
        out["guided_radius"], out["guided_max_distance"] = a.guided, a.max_distance
        out["step_local_map_guided"] = dict(n_matches=gm["n_matches"], n_correspondences=gm["n_correspondences"], n_inliers=gm["n_inliers"])
        out["step_single_guided"] = dict(n_matches=gs["n_matches"], n_correspondences=gs["n_correspondences"], n_inliers=gs["n_inliers"])
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
