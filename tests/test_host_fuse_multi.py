"""Multi-target landmark fusion through the plugin loader: `mslam_harness <plugin> --fuse-multi <scene>`
(IMultiLandmarkFuser::fuseLandmarksMulti on the relocalizer adapter, which owns the store) on scenes written by
tests/fuse_multi_ref.py, against the restatement: the pairs, the count of rewritten landmarks and every entry's ids after
the replacement.  Without a GPU: the plugin exports what it exported before and calls the new C ABI, and the harness reads
a scene's header and refuses a malformed one before it loads the plugin."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fuse_multi_ref as fm
import fuse_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "modular-slam_amd", "host")
HARNESS = os.path.join(HOST, "mslam_harness")
PLUGIN = os.path.join(HOST, "libmslam_hip_plugin.so")


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", HOST])
    return True


def test_harness_interface_and_adapter_know_the_multi_fusion(built):
    assert "--fuse-multi" in open(os.path.join(HOST, "harness.cpp")).read()
    hdr = open(os.path.join(HOST, "mslam_interfaces.hpp")).read()
    assert "class IMultiLandmarkFuser" in hdr and "class ILandmarkFuser" in hdr
    out = subprocess.check_output(["nm", "-D", PLUGIN]).decode()
    for alias in ("hipOrbDetectorFactory", "hipCvOrbDetectorFactory", "hipOrbMatcherFactory", "hipOrbRelocalizerFactory",
                  "loopDetection", "hipRansacPnpFactory"):                  # what the plugin exported before
        assert any(line.split()[-1] == alias and line.split()[-2] in "DdBb" for line in out.splitlines()), alias
    undefined = [line.split()[-1] for line in out.splitlines() if " U " in line]
    assert "mslam_hip_kf_fuse_multi" in undefined and "mslam_hip_kf_fuse" in undefined   # the plugin calls both C entry points


def _scenes():
    a = fm.random_case(3, 1024)
    rng = np.random.default_rng(3)
    dl = np.concatenate([d[2] for d in a["drops"]])
    others = [(rng.integers(0, 256, (40, 32), dtype=np.uint8), rng.normal(size=(40, 3)), np.concatenate([dl[:30], 7000 + np.arange(10)]))]
    return [(a, others), (fm.hand_case("a_before_b"), [])]


def _write(path, case, others):
    kw = case["kw"]
    fm.write_scene(str(path), case["keep"], case["drops"], case["Rs"], case["ts"], case["radius"], kw["cam"], kw["width"], kw["height"],
                   kw["max_distance"], kw["ratio"], kw["max_world_distance"], others)


def test_harness_reads_the_scene_header_without_a_gpu(built, tmp_path):
    """a scene with a foreign magic, one cut short inside the poses and one with fewer entries than targets are refused with
    exit code 5 before the plugin is loaded"""
    case, others = _scenes()[1]
    good = tmp_path / "good.bin"
    _write(good, case, others)
    raw = good.read_bytes()
    assert raw[:4] == b"MSFM" and int.from_bytes(raw[20:24], "little") == len(case["drops"])
    few = bytearray(raw)
    few[20:24] = (64).to_bytes(4, "little")                                  # 64 targets: the poses run past the entries
    for name, data in (("magic", b"MSFU" + raw[4:]), ("short", raw[:100]), ("few", bytes(few))):
        p = tmp_path / (name + ".bin")
        p.write_bytes(data)
        r = subprocess.run([HARNESS, PLUGIN, "--fuse-multi", str(p)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 5 and "not a multi-target fusion scene" in r.stderr, (name, r.returncode, r.stderr)


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1])
def test_harness_fuse_multi_equals_the_reference(built, tmp_path, which):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth
    case, others = _scenes()[which]
    voc = tmp_path / "orbvoc.dbow3"
    voc.write_bytes(synth.make_vocabulary(10, 3))
    path = tmp_path / "fuse_multi.bin"
    _write(path, case, others)
    r = subprocess.run([HARNESS, PLUGIN, "--fuse-multi", str(path)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, MSLAM_ORB_VOCABULARY=str(voc)))
    assert r.returncode == 0, r.stderr
    store = dict(enumerate([case["keep"]] + list(case["drops"]) + others))
    n_drop = len(case["drops"])
    pairs, new, n = fm.fuse_multi(store, 0, list(range(1, 1 + n_drop)), case["Rs"], case["ts"], case["radius"], **case["kw"])
    lines = r.stdout.strip().splitlines()
    head = [l for l in lines if l.startswith("fuse-multi pairs ")]
    assert head == ["fuse-multi pairs %d rewritten %d" % (len(pairs["keep_pos"]), n)] and (which or len(pairs["keep_pos"]) > 20)
    got = [tuple(int(x) for x in l.split()[1:]) for l in lines if l.startswith("pair ")]
    assert got == list(zip(pairs["target"].tolist(), pairs["keep_pos"].tolist(), pairs["drop_pos"].tolist(), pairs["keep_lid"].tolist(),
                           pairs["drop_lid"].tolist(), pairs["dist"].tolist()))
    ids = {int(l.split()[1]): [int(x) for x in l.split()[3:]] for l in lines if l.startswith("entry ")}
    assert ids == {k: fr.entry(*v)[2].tolist() for k, v in new.items()}
