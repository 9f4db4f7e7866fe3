"""What the loss of the pose graph and of min-MSE PnP costs (mslam_hip_set_pose_graph_loss, mslam_hip_set_pnp_mse_loss):
milliseconds per call and per trust-region iteration of mslam_hip_pose_graph (DENSE and SPARSE) on one graph and of
mslam_hip_pnp_min_mse_batch_dev on one batch, for
    parent    a libmslam_hip.so built from the parent commit (--parent), which has neither setting,
    parent2   a second context of that same library: parent against parent2 is the run-to-run spread of one binary,
    none      this tree's library with loss NONE (the kernels of before are launched),
    none2     a second context of the same: the spread of this binary,
    huber, cauchy   this tree's library with the loss set (the *_loss kernels),
all through the same ctypes calls on arrays prepared beforehand, one context each, on one device.  The variants are
interleaved: every round runs each of them once, in an order rotated per round, so drift of the clocks or of the box falls on
all alike.  Reported per variant: the median over --rounds rounds after one warm-up round, the quartiles, and the iterations
the solve took; a loss changes the minimisation, so the iteration counts differ and ms per iteration is the number to compare.
A pose-graph call is timed by the host clock (the call ends in a device synchronise and a download); the PnP batch, which is
asynchronous, between two mslam_hip_sync calls; mslam_hip_pose_graph_edge_weights (one launch, this tree only) the same way as
the solve.  Every row also says whether `none` returned the parent's bytes.  The graph: a chain of --poses
poses with a loop edge every 10 poses and one false loop in 25, noise 0.01 (tests/pose_graph_loss_ref.py's construction).  The
batch: --problems problems of --points points, tests/test_mse_pnp.py's scene64 with 20 % wrong image points.  There is no
pass / fail threshold; `none` slower than `parent` beyond the parent / parent2 spread would be a defect.

usage: python tools/robust_loss_latency.py --parent path/to/parent/libmslam_hip.so [--rounds 30] [--poses 400] [--problems 1024]
       [--points 256] [--out file.json]"""
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

PG_SCALE, PNP_SCALE = 0.1, 2.0
CAM = (525.0, 525.0, 319.5, 239.5)


class Library:
    """one context of one library, driven through the C ABI directly; `setter` names the loss setting to use, if any"""

    def __init__(self, pkg, library, setter=None, loss=None):
        self.pkg, self.L = pkg, library
        library.mslam_hip_create.argtypes = [C.POINTER(pkg.Params), C.POINTER(C.c_void_p)]
        library.mslam_hip_destroy.argtypes = [C.c_void_p]
        library.mslam_hip_destroy.restype = None
        library.mslam_hip_sync.argtypes = [C.c_void_p]
        self.h = C.c_void_p()
        params = pkg.default_params(width=0, height=0)
        if library.mslam_hip_create(C.byref(params), C.byref(self.h)) != 0:
            raise RuntimeError("mslam_hip_create failed")
        if loss is not None and getattr(library, setter)(self.h, int(loss[0]), C.c_double(loss[1])) != 0:
            raise RuntimeError(setter + " failed")

    def pose_graph(self, sc, sparse):
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        poses = sc["poses"].copy()
        summary = self.pkg.BaSummary()
        if self.L.mslam_hip_set_pose_graph_solver(self.h, 1 if sparse else 0) != 0:
            raise RuntimeError("mslam_hip_set_pose_graph_solver failed")
        t = time.perf_counter()
        rc = self.L.mslam_hip_pose_graph(self.h, p(poses), p(sc["fixed"]), len(poses), p(sc["edge_a"]), p(sc["edge_b"]), p(sc["edge_meas"]),
                                         None, len(sc["edge_a"]), 100, C.byref(summary))
        ms = (time.perf_counter() - t) * 1e3
        if rc != 0:
            raise RuntimeError("mslam_hip_pose_graph returned %d" % rc)
        return ms, summary.iterations, summary.termination, poses

    def edge_weights(self, sc):
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        chi2, weight = np.zeros(len(sc["edge_a"])), np.zeros(len(sc["edge_a"]))
        t = time.perf_counter()
        rc = self.L.mslam_hip_pose_graph_edge_weights(self.h, p(sc["poses"]), len(sc["poses"]), p(sc["edge_a"]), p(sc["edge_b"]),
                                                      p(sc["edge_meas"]), None, len(sc["edge_a"]), p(chi2), p(weight))
        ms = (time.perf_counter() - t) * 1e3
        if rc != 0:
            raise RuntimeError("mslam_hip_pose_graph_edge_weights returned %d" % rc)
        return ms, 1, 0, weight

    def pnp_batch(self, b):
        b["d_pose"].copy_(b["pose0"])
        b["torch"].cuda.synchronize()
        self.L.mslam_hip_sync(self.h)
        t = time.perf_counter()
        rc = self.L.mslam_hip_pnp_min_mse_batch_dev(self.h, C.c_void_p(b["d_obj"].data_ptr()), C.c_void_p(b["d_img"].data_ptr()),
                                                    C.c_void_p(b["d_n"].data_ptr()), b["P"], b["cap"], *[C.c_double(v) for v in CAM],
                                                    C.c_void_p(b["d_pose"].data_ptr()), C.c_void_p(b["d_info"].data_ptr()))
        self.L.mslam_hip_sync(self.h)
        ms = (time.perf_counter() - t) * 1e3
        if rc != 0:
            raise RuntimeError("mslam_hip_pnp_min_mse_batch_dev returned %d" % rc)
        info = b["d_info"].cpu().numpy()
        return ms, float(np.mean(info[:, 1])), int(np.max(info[:, 0])), b["d_pose"].cpu().numpy()

    def close(self):
        self.L.mslam_hip_destroy(self.h)


def measure(what, variants, run, rounds):
    """-> the row of one workload: run(variant) -> (ms, iterations, termination, output), interleaved and rotated"""
    names = list(variants)
    times, info, outputs = {n: [] for n in names}, {}, {}
    for r in range(rounds + 1):
        for i in range(len(names)):
            n = names[(i + r) % len(names)]
            ms, it, term, out = run(variants[n])
            info[n], outputs[n] = (it, term), out
            if r > 0:
                times[n].append(ms)
    row = dict(what=what, rounds=rounds)
    for n in names:
        q1, med, q3 = np.percentile(times[n], [25, 50, 75])
        row[n] = dict(ms=float(med), q1=float(q1), q3=float(q3), iterations=info[n][0], termination=info[n][1],
                      ms_per_iteration=float(med) / max(info[n][0], 1))
    if "parent" in outputs and "none" in outputs:
        row["none_returns_the_parents_bytes"] = bool(outputs["parent"].tobytes() == outputs["none"].tobytes())
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--poses", type=int, default=400)
    ap.add_argument("--problems", type=int, default=1024)
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import pose_graph_cases as pc
    import pose_graph_loss_ref as pl
    from test_mse_pnp import perturbed, scene64
    if not torch.cuda.is_available():
        raise SystemExit("robust_loss_latency: no GPU; a time from a CPU says nothing")
    pkg = graft.load_package()
    mine, parent = pkg.lib(), C.CDLL(os.path.abspath(a.parent))

    def variants(setter, scale):
        return {"parent": Library(pkg, parent), "none": Library(pkg, mine), "parent2": Library(pkg, parent), "none2": Library(pkg, mine),
                "huber": Library(pkg, mine, setter, (pkg.BA_LOSS_HUBER, scale)), "cauchy": Library(pkg, mine, setter, (pkg.BA_LOSS_CAUCHY, scale))}

    rows = []
    # ---- the pose graph ----
    K = a.poses
    loops = [(k, k + 10) for k in range(0, K - 10, 10)]
    false = [(k, (k + K // 2) % K) for k in range(5, K, 25)]
    sc = pc.make_scene(K, pc.chain(K, 0) + loops + false, 7, noise=0.01)
    sc = pl.spoil(sc, np.arange(K - 1 + len(loops), K - 1 + len(loops) + len(false)), 7)
    for k in ("poses", "edge_meas"):
        sc[k] = np.ascontiguousarray(sc[k], np.float64)
    for k in ("edge_a", "edge_b"):
        sc[k] = np.ascontiguousarray(sc[k], np.int32)
    sc["fixed"] = np.ascontiguousarray(sc["fixed"], np.uint8)
    pg = variants("mslam_hip_set_pose_graph_loss", PG_SCALE)
    for sparse in (False, True):
        row = measure("pose_graph %s K %d E %d" % ("sparse" if sparse else "dense", K, len(sc["edge_a"])), pg,
                      lambda v: v.pose_graph(sc, sparse), a.rounds)
        rows.append(row)
        print(json.dumps(row), flush=True)
    row = measure("pose_graph_edge_weights E %d" % len(sc["edge_a"]), {n: pg[n] for n in ("none", "huber", "cauchy")},
                  lambda v: v.edge_weights(sc), a.rounds)
    rows.append(row)
    print(json.dumps(row), flush=True)
    for v in pg.values():
        v.close()
    # ---- the PnP batch ----
    P, cap = a.problems, a.points
    obj, img, pose = np.zeros((P, cap, 3)), np.zeros((P, cap, 2)), np.zeros((P, 6))
    for p in range(P):
        o, i, x = scene64(9000 + p, n=cap, noise=0.5, outliers=0.2)
        obj[p], img[p], pose[p] = o, i, perturbed(x, p)
    dev = torch.device("cuda")
    batch = dict(torch=torch, P=P, cap=cap, d_obj=torch.from_numpy(obj).to(dev), d_img=torch.from_numpy(img).to(dev),
                 d_n=torch.full((P,), cap, dtype=torch.int32, device=dev), pose0=torch.from_numpy(pose).to(dev),
                 d_pose=torch.from_numpy(pose).to(dev), d_info=torch.zeros((P, 4), dtype=torch.float64, device=dev))
    pnp = variants("mslam_hip_set_pnp_mse_loss", PNP_SCALE)
    row = measure("pnp_min_mse_batch_dev P %d n %d" % (P, cap), pnp, lambda v: v.pnp_batch(batch), a.rounds)
    rows.append(row)
    print(json.dumps(row), flush=True)
    for v in pnp.values():
        v.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
