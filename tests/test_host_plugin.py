"""The C++ host side: the plugin is loaded through the reference's loader contract
(loadFactoryMethod<T>(lib, alias), plugin_loader.hpp:20-24 — cf. test/plugin_loader_test.cpp:17-21) and
driven in RgbdFeatureFrontend's call order; its output is compared with the oracle by checksum."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "modular-slam_amd", "host")
HARNESS = os.path.join(HOST, "mslam_harness")
PLUGIN = os.path.join(HOST, "libmslam_hip_plugin.so")


def _fnv(data, h=0x811C9DC5):
    for b in data:
        h = ((h ^ b) * 0x01000193) & 0xFFFFFFFF
    return h


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", HOST])
    return True


def test_plugin_exports_boost_style_aliases(built):
    out = subprocess.check_output(["nm", "-D", PLUGIN]).decode()
    for alias in ("hipOrbDetectorFactory", "hipCvOrbDetectorFactory", "hipOrbMatcherFactory", "hipOrbRelocalizerFactory",
                  "loopDetection", "hipRansacPnpFactory"):
        assert any(line.split()[-1] == alias and line.split()[-2] in "DdBb" for line in out.splitlines()), alias
    sec = subprocess.check_output(["readelf", "-S", PLUGIN]).decode()
    assert "boostdll" in sec  # the section BOOST_DLL_ALIAS uses


def test_loader_resolves_factories_without_gpu(built):
    # same assertion as the reference's plugin loader test: the factory function loads and can be called
    r = subprocess.run([HARNESS, PLUGIN], capture_output=True, text=True)
    assert r.returncode == 0 and "loaded ok" in r.stdout
    # append_decorations: "mslam_hip_plugin" -> "libmslam_hip_plugin.so"
    r = subprocess.run([HARNESS, os.path.join(HOST, "mslam_hip_plugin")], capture_output=True, text=True)
    assert r.returncode == 0 and "loaded ok" in r.stdout
    r = subprocess.run([HARNESS, os.path.join(HOST, "no_such_plugin")], capture_output=True, text=True)
    assert r.returncode == 1 and "cannot load library" in r.stderr


@pytest.mark.gpu
def test_plugin_detect_match_parity(built, orc, bundled_frames, tmp_path):
    paths = []
    for i, f in enumerate(bundled_frames):
        p = tmp_path / ("f%d.bgr" % i)
        p.write_bytes(f.tobytes())
        paths.append(str(p))
    r = subprocess.run([HARNESS, PLUGIN, "640", "480"] + paths, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    dets = [orc.detect(f, orc.params()) for f in bundled_frames]
    for i, d in enumerate(dets):
        h = 0x811C9DC5
        for k in range(len(d["xy"])):
            h = _fnv(struct.pack("<Q", k), h)
            h = _fnv(struct.pack("<dd", float(d["xy"][k, 0]), float(d["xy"][k, 1])), h)
            h = _fnv(d["desc"][k].tobytes(), h)
        assert "frame %d keypoints %d fnv %08x" % (i, len(d["xy"]), h) in lines
    fi, ti = orc.match(dets[1]["desc"], dets[0]["desc"])
    h = 0x811C9DC5
    for a, b in zip(fi, ti):
        h = _fnv(struct.pack("<QQ", int(a), int(b)), h)
    assert "match 1 pairs %d fnv %08x" % (len(fi), h) in lines
    # the same two frames as a TUM RGB-D sequence (PNG files + association list) give the same lines
    assoc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tum", "associations.txt")
    r2 = subprocess.run([HARNESS, PLUGIN, "--tum", assoc], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stderr
    assert r2.stdout.strip().splitlines() == lines


@pytest.mark.gpu
def test_plugin_bow_boundary(built, orc, synth_frames, tmp_path):
    """relocalizer + loop-detector factories on ONE shared database (the frontend feeds keyframes only through
    IRelocalizer::addKeyframe, rgbd_feature_frontend.cpp:176, and asks ILoopDetector::detectLoop(), :202):
    detectLoop() after every addKeyframe, relocalize() for every frame, removeKeyframe() — against the oracle."""
    import synth
    voc = tmp_path / "orbvoc.dbow3"
    blob = synth.make_vocabulary(10, 4, seed=5)
    voc.write_bytes(blob)
    order = [0, 1, 2, 0, 3, 1, 4]                       # revisits: frame 3 == frame 0, frame 5 == frame 1
    paths = []
    for i, fi in enumerate(order):
        p = tmp_path / ("k%d.bgr" % i)
        p.write_bytes(synth_frames[fi].tobytes())
        paths.append(str(p))
    r = subprocess.run([HARNESS, PLUGIN, "--bow", str(voc), "640", "480"] + paths, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    V = orc.Vocabulary(blob)
    dets = [orc.detect(synth_frames[fi], orc.params()) for fi in order]
    vecs = [V.bow_vector(d["desc"]) for d in dets]

    def ranked(q, live):
        sc = sorted(((orc.bow_score_l1(*vecs[q], *vecs[e]), e) for e in live), key=lambda x: (-x[0], x[1]))
        return [e for s, e in sc if s > 0]

    for t in range(len(order)):
        best = ranked(t, range(t))
        exp = "keyframe %d keypoints %d loop %d" % (t, len(dets[t]["xy"]), 100 + best[0] if best else -1)
        assert exp in lines, (exp, lines)
    assert "keyframe 3 keypoints %d loop 100" % len(dets[3]["xy"]) in lines      # the revisit of frame 0 is found
    n = len(order)
    for t in range(n):
        assert "relocalize %d: %s" % (t, " ".join(str(100 + e) for e in ranked(t, range(n))[:4])) in lines
    assert "after remove 0: %s" % " ".join(str(100 + e) for e in ranked(0, range(1, n))[:4]) in lines


@pytest.mark.gpu
def test_plugin_cv_orb_detector(built, orc, bundled_frames, tmp_path):
    """hipCvOrbDetectorFactory: the OrbOpenCvDetector drop-in (orb_feature.cpp:25,33-65) through the loader"""
    paths = []
    for i, f in enumerate(bundled_frames):
        p = tmp_path / ("f%d.bgr" % i)
        p.write_bytes(f.tobytes())
        paths.append(str(p))
    env = dict(os.environ, MSLAM_HARNESS_DETECTOR="cvorb")
    r = subprocess.run([HARNESS, PLUGIN, "640", "480"] + paths, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    dets = [orc.cvorb_detect(f, orc.cvorb_params()) for f in bundled_frames]
    for i, d in enumerate(dets):
        h = 0x811C9DC5
        for k in range(len(d["xy"])):
            h = _fnv(struct.pack("<Q", k), h)
            h = _fnv(struct.pack("<dd", float(d["xy"][k, 0]), float(d["xy"][k, 1])), h)
            h = _fnv(d["desc"][k].tobytes(), h)
        assert "frame %d keypoints %d fnv %08x" % (i, len(d["xy"]), h) in lines
    fi, ti = orc.match(dets[1]["desc"], dets[0]["desc"])
    h = 0x811C9DC5
    for a, b in zip(fi, ti):
        h = _fnv(struct.pack("<QQ", int(a), int(b)), h)
    assert "match 1 pairs %d fnv %08x" % (len(fi), h) in lines


@pytest.mark.gpu
@pytest.mark.parametrize("negative_w", [False, True, "four_inliers"])
def test_plugin_pnp(built, tmp_path, negative_w):
    """hipRansacPnpFactory: the OpenCvRansacPnp drop-in (cv_ransac_pnp.cpp:14-85) through the loader — sensor pose in,
    sensor pose out (the adapter does the world->camera inversions of :42-50 and :65-78 around the solver).  The initial
    orientation is also passed as -q (w < 0: the same rotation; Eigen::AngleAxisd folds the sign into the axis,
    cv_ransac_pnp.cpp:44-48): the extrinsic guess, and so the result, must not change.  "four_inliers": a scene whose best
    hypothesis explains exactly 4 points — below the consensus floor of 5, so the adapter returns nullopt."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import mslam_pnp_oracle as po
    from test_pnp import CAM, scene, rot_err
    obj, img, R, t, good = scene(21, n=500, outliers=0.25)
    if negative_w == "four_inliers":
        from test_pnp_edges import four_inlier_scene
        obj, img = four_inlier_scene()[:2]
        assert max(po.consensus(obj, img, CAM, seed=0)["counts"]) == 4     # the plugin samples with seed 0
    # the sensor pose (world frame) that corresponds to the camera transform (R, t): orientation R^T, position -R^T t
    Rs, ps = R.T, -R.T @ t
    # start from a perturbed sensor pose (what the frontend passes: the previous frame's pose)
    R0s = Rs @ po.rodrigues([0.01, 0.02, -0.015])
    p0s = ps + np.array([0.03, -0.02, 0.04])

    def quat(Rm):   # w, x, y, z
        w = np.sqrt(max(0.0, 1 + np.trace(Rm))) / 2
        return np.array([w, (Rm[2, 1] - Rm[1, 2]) / (4 * w), (Rm[0, 2] - Rm[2, 0]) / (4 * w), (Rm[1, 0] - Rm[0, 1]) / (4 * w)])
    path = tmp_path / "scene.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(obj)))
        for P, uv in zip(obj.astype(np.float64), img.astype(np.float64)):
            f.write(struct.pack("<5d", *P, *uv))
        f.write(struct.pack("<7d", *p0s, *(-quat(R0s) if negative_w else quat(R0s))))
        f.write(struct.pack("<4d", *CAM))
    r = subprocess.run([HARNESS, PLUGIN, "--pnp", str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    if negative_w == "four_inliers":
        assert "pnp none" in r.stdout.splitlines() and "Didnt find pnp solution" in r.stderr, (r.stdout, r.stderr)
        return
    line = [l for l in r.stdout.splitlines() if l.startswith("pnp position")][0].split()
    pos = np.array([float(x) for x in line[2:5]])
    q = np.array([float(x) for x in line[6:10]])
    n_in = int(line[11])
    w, x, y, z = q
    Rq = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    assert rot_err(Rq, Rs) < 0.1 and np.linalg.norm(pos - ps) < 0.03          # ground truth (sensor pose)
    ref = po.pnp_ransac(obj, img, CAM, seed=0, guess=(R0s.T, -R0s.T @ p0s))
    assert n_in == int(ref["mask"].sum())
    assert rot_err(Rq, ref["R"].T) < 1e-5 and np.linalg.norm(pos - (-ref["R"].T @ ref["t"])) < 1e-6
