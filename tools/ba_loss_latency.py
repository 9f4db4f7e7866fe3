"""What the loss function of bundle adjustment costs (mslam_hip_set_ba_loss): milliseconds per solve and per trust-region
iteration of mslam_hip_bundle_adjust for
    parent    a libmslam_hip.so built from the parent commit (--parent), which has no loss kernels,
    parent2   a second context of that same library: parent against parent2 is the run-to-run spread of one binary,
    none      this tree's library with loss NONE (the kernels of before are launched),
    none2     a second context of the same: the spread of this binary,
    huber, cauchy   this tree's library with the loss set (the *_loss kernels), scale --scale,
all through the same ctypes calls on arrays prepared beforehand, one context each, on one device.  The variants are
interleaved: every round solves each of them once, in an order rotated per round, so drift of the clocks or of the box falls
on all alike.  Reported per variant: the median over --rounds rounds after one warm-up round, the quartiles, and the
iterations the solve took; a loss changes the minimisation, so the iteration counts differ and ms per iteration is the
number to compare.  The problems are tools/ba_latency.py's sizes with one observation in twelve spoilt by 0.4 m, so that
the loss has something to do.  --max-iterations 1 makes every variant run the same launches from the same state (the start
cost, one full iteration with its Jacobian kernels, the outlier mask), so the difference between `none` and a loss is then the
cost of the weights alone.  There is no pass / fail threshold; `none` slower than `parent` beyond the parent / parent2
spread would be a defect.

usage: python tools/ba_loss_latency.py --parent path/to/parent/libmslam_hip.so [--rounds 30] [--scale 0.02] [--max-iterations 100]
       [--out file.json]"""
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

SIZES = [(2, 200, 2), (8, 1000, 4), (16, 4000, 6), (64, 8000, 8)]


class Solver:
    """one context of one library, driven through the C ABI directly"""

    def __init__(self, pkg, library, loss=None):
        self.pkg, self.L = pkg, library
        library.mslam_hip_create.argtypes = [C.POINTER(pkg.Params), C.POINTER(C.c_void_p)]
        library.mslam_hip_destroy.argtypes = [C.c_void_p]
        library.mslam_hip_destroy.restype = None
        self.h = C.c_void_p()
        params = pkg.default_params(width=0, height=0)
        if library.mslam_hip_create(C.byref(params), C.byref(self.h)) != 0:
            raise RuntimeError("mslam_hip_create failed")
        if loss is not None and library.mslam_hip_set_ba_loss(self.h, int(loss[0]), C.c_double(loss[1])) != 0:
            raise RuntimeError("mslam_hip_set_ba_loss failed")

    def solve(self, sc, max_iterations=100):
        poses, lms = sc["poses"].copy(), sc["landmarks"].copy()
        summary = self.pkg.BaSummary()
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        t = time.perf_counter()
        rc = self.L.mslam_hip_bundle_adjust(self.h, p(poses), p(sc["fixed"]), len(poses), p(lms), len(lms), p(sc["obs_kf"]),
                                            p(sc["obs_lm"]), p(sc["obs_cam"]), len(sc["obs_kf"]), int(max_iterations), C.c_double(0.15), None,
                                            C.byref(summary))
        ms = (time.perf_counter() - t) * 1e3
        if rc != 0:
            raise RuntimeError("mslam_hip_bundle_adjust returned %d" % rc)
        return ms, summary.iterations, summary.termination

    def close(self):
        self.L.mslam_hip_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--scale", type=float, default=0.02)
    ap.add_argument("--max-iterations", type=int, default=100)
    ap.add_argument("--out")
    a = ap.parse_args()
    import ba_ref
    pkg = graft.load_package()
    mine, parent = pkg.lib(), C.CDLL(os.path.abspath(a.parent))
    solvers = {"parent": Solver(pkg, parent), "none": Solver(pkg, mine), "parent2": Solver(pkg, parent), "none2": Solver(pkg, mine),
               "huber": Solver(pkg, mine, (pkg.BA_LOSS_HUBER, a.scale)), "cauchy": Solver(pkg, mine, (pkg.BA_LOSS_CAUCHY, a.scale))}
    names = list(solvers)
    rows = []
    for K, L, views in SIZES:
        sc = ba_ref.make_scene(K, L, K + L, noise=0.005, views=views, start_angle=0.1)
        rng = np.random.default_rng(K + L)
        M = len(sc["obs_kf"])
        bad = rng.choice(M, size=M // 12, replace=False)
        sc["obs_cam"][bad] += 0.4 * rng.normal(size=(len(bad), 3))
        for k in ("poses", "landmarks", "obs_cam"):
            sc[k] = np.ascontiguousarray(sc[k], np.float64)
        for k in ("obs_kf", "obs_lm"):
            sc[k] = np.ascontiguousarray(sc[k], np.int32)
        sc["fixed"] = np.ascontiguousarray(sc["fixed"], np.uint8)
        times = {n: [] for n in names}
        info = {}
        for r in range(a.rounds + 1):
            for i in range(len(names)):
                n = names[(i + r) % len(names)]
                ms, it, term = solvers[n].solve(sc, a.max_iterations)
                info[n] = (it, term)
                if r > 0:
                    times[n].append(ms)
        row = dict(K=K, L=L, M=M, rounds=a.rounds, max_iterations=a.max_iterations)
        for n in names:
            q1, med, q3 = np.percentile(times[n], [25, 50, 75])
            row[n] = dict(ms=float(med), q1=float(q1), q3=float(q3), iterations=info[n][0], termination=info[n][1],
                          ms_per_iteration=float(med) / max(info[n][0], 1))
        rows.append(row)
        print(json.dumps(row), flush=True)
    for s in solvers.values():
        s.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
