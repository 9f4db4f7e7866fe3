"""Latency of one mslam_hip_relocalize call (4 candidates x ~1900 query keypoints x ~600 landmarks) against the composition
that gives the same answer from host pointers: 4 x mslam_hip_match + 4 x mslam_hip_pnp_ransac.  Both go through ctypes with
arrays prepared beforehand; the two are timed alternately, in blocks, so that drift of the machine hits both.

usage: python tools/reloc_latency.py [--blocks 15] [--calls 200] [--trace new|old]   (--trace: a short run of one side only,
       for rocprofv3 --kernel-trace --stats)"""
import argparse
import ctypes as C
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
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--trace", choices=["new", "old"])
    a = ap.parse_args()
    import reloc_ref as rr
    pkg = graft.load_package()
    sc = rr.make_scene(seed=0, n_landmarks=600, n_distractors=1360)        # 540 + 1360 = 1900 query keypoints
    cand = sc["ids"]
    c = pkg.Context(width=0, height=0, max_keypoints=1024)
    for cid in cand:
        c.kf_add(cid, *sc["store"][cid])
    desc, xy = sc["desc"], sc["xy"]
    kd = {cid: sc["store"][cid][0] for cid in cand}
    kw32 = {cid: sc["store"][cid][1].astype(np.float32) for cid in cand}

    def new():
        return c.relocalize(desc, xy, cand, seed=1)

    def old():
        out = []
        for k, cid in enumerate(cand):
            fi, ti = c.match(desc, kd[cid])
            if len(fi) < 4:
                out.append(None)
                continue
            out.append(c.pnp_ransac(kw32[cid][ti], xy[fi], seed=1 + k))
        return out
    # same answer
    rn, ro = new(), old()
    for k, o in enumerate(ro):
        cn = rn["candidates"][k]
        assert (o is None) == (cn["status"] == 0)
        if o is not None:
            assert int(o[2].sum()) == cn["n_inliers"] and np.abs(o[0] - cn["rvec"]).max() < 1e-9 and np.abs(o[1] - cn["tvec"]).max() < 1e-9
    if a.trace:
        f = new if a.trace == "new" else old
        for _ in range(50):
            f()
        return
    for _ in range(50):
        new(), old()
    res = {"new": [], "old": []}
    for _ in range(a.blocks):
        for name, f in (("new", new), ("old", old)):
            t0 = time.perf_counter()
            for _ in range(a.calls):
                f()                                   # every call ends in a device synchronise
            res[name].append((time.perf_counter() - t0) / a.calls * 1e6)
    out = {k: dict(median_us=float(np.median(v)), min_us=float(np.min(v)), max_us=float(np.max(v)), blocks=[round(x, 2) for x in v])
           for k, v in res.items()}
    out["shape"] = dict(candidates=len(cand), query=len(desc), landmarks=600, calls_per_block=a.calls)
    out["inliers"] = [cn["n_inliers"] for cn in rn["candidates"]]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
