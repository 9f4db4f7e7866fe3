"""Stage times of the guided matching stage (guided_bin + match_guided + ratio_guided) against the brute-force stage it
replaces (match_knn2 + ratio_compact) inside the same tracking call, from mslam_hip_set_profiling(ctx, 1)'s events.  The
brute-force side is the mode switched off on the same context: the two are run alternately, call by call, so drift of the
machine hits both.  Shapes: one frame of 1900 keypoints against an entry of 1900 landmarks; the same frame against a union
of 8000 landmarks; a window of 64 such frames against the 1900-landmark entry.  The guess is the true pose, the radius 15 px.

usage: python tools/guided_stage_times.py [--rounds 30] [--radius 15] [--out file.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402

BRUTE = ("match_knn2", "ratio_compact")
GUIDED = ("guided_bin", "match_guided", "ratio_guided")


def rvec_of(R):
    th = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    if th < 1e-12:
        return np.zeros(3)
    return th / (2 * np.sin(th)) * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--radius", type=float, default=15.0)
    ap.add_argument("--out")
    a = ap.parse_args()
    import reloc_ref as rr
    pkg = graft.load_package()
    sc = rr.make_scene(seed=0, n_kf=1, n_landmarks=1900, target=0, n_distractors=190, drop=0.1)    # 1710 + 190 keypoints
    desc, xy = sc["desc"], sc["xy"]
    depth = np.full((480, 640), 10000, np.uint16)
    rng = np.random.default_rng(1)
    d, w = sc["store"][sc["target_id"]]
    others = np.stack([rng.uniform(-1.6, 1.6, 6100), rng.uniform(-1.2, 1.2, 6100), rng.uniform(2.5, 6.0, 6100)], 1)
    union = (np.concatenate([d, rng.integers(0, 256, (6100, 32), dtype=np.uint8)]), np.concatenate([w, (others - sc["t"]) @ sc["R"]]))
    c = pkg.Context(width=0, height=0, max_keypoints=8192)
    c.kf_add(1, d, w)
    c.kf_add(2, *union)
    guess = dict(rvec=rvec_of(sc["R"]), tvec=sc["t"])
    S = 64
    shapes = {
        "row_1900x1900": lambda: c.track(desc, xy, depth, 1, [1], -1, seed=1, **guess),
        "row_1900x8000_union": lambda: c.track(desc, xy, depth, 2, [1], -1, seed=1, **guess),
        "window_64x1900x1900": lambda: c.track_window([desc] * S, [xy] * S, [depth] * S, 1, [1], -1, 0, seed=1, **guess)[0][0],
    }
    out = dict(radius=a.radius, rounds=a.rounds, keypoints=len(desc), shapes={})
    for name, call in shapes.items():
        res = {"brute": [], "guided": []}
        info = {}
        for r in range(-5, a.rounds):                  # five warm-up rounds
            for side, radius, stages in (("brute", 0.0, BRUTE), ("guided", a.radius, GUIDED)):
                c.set_guided_match(radius, 256, 640, 480)
                c.set_profiling(1)                     # (starts a fresh list of stage events)
                rec = call()
                times = dict()
                for n, ms in c.stage_times():
                    times[n] = times.get(n, 0.0) + ms * 1e3
                assert all(s in times for s in stages), (side, sorted(times))
                if r >= 0:
                    res[side].append(sum(times[s] for s in stages))
                info[side] = dict(n_matches=rec["n_matches"], n_correspondences=rec["n_correspondences"], n_inliers=rec["n_inliers"],
                                  stages_us={s: round(times[s], 2) for s in stages})
        c.set_profiling(0)
        out["shapes"][name] = {side: dict(median_us=round(float(np.median(v)), 2), min_us=round(float(np.min(v)), 2),
                                          max_us=round(float(np.max(v)), 2), last=info[side]) for side, v in res.items()}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
