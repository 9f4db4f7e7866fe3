"""Landmark fusion through the plugin loader: `mslam_harness <plugin> --fuse <scene>` (ILandmarkFuser::fuseLandmarks on the
relocalizer adapter, which owns the store) on two small scenes written by tests/fuse_ref.py, against the restatement: the
pairs, the count of rewritten landmarks and every entry's ids after the replacement."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fuse_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "modular-slam_amd", "host")
HARNESS = os.path.join(HOST, "mslam_harness")
PLUGIN = os.path.join(HOST, "libmslam_hip_plugin.so")


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", HOST])
    return True


def test_harness_and_adapter_know_the_fusion(built):
    assert "--fuse" in open(os.path.join(HOST, "harness.cpp")).read()
    assert "class ILandmarkFuser" in open(os.path.join(HOST, "mslam_interfaces.hpp")).read()
    out = subprocess.check_output(["nm", "-DC", PLUGIN]).decode()
    assert "mslam_hip_kf_fuse" in out                                       # the plugin calls the new C ABI


def _scenes():
    a = fr.random_case(21, 120, 150, shared=4)
    rng = np.random.default_rng(2)
    dl = a["drop"][2]
    others = [(rng.integers(0, 256, (40, 32), dtype=np.uint8), rng.normal(size=(40, 3)), np.concatenate([dl[:30], 7000 + np.arange(10)]))]
    b = fr.hand_case("two_claim_one")
    return [(a, others), (b, [])]


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1])
def test_harness_fuse_equals_the_reference(built, tmp_path, which):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth
    case, others = _scenes()[which]
    kw = case["kw"]
    voc = tmp_path / "orbvoc.dbow3"
    voc.write_bytes(synth.make_vocabulary(10, 3))
    path = tmp_path / "fuse.bin"
    fr.write_scene(str(path), case["keep"], case["drop"], kw["R"], kw["t"], case["radius"], kw["cam"], kw["width"], kw["height"],
                   kw["max_distance"], kw["ratio"], kw["max_world_distance"], others)
    r = subprocess.run([HARNESS, PLUGIN, "--fuse", str(path)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, MSLAM_ORB_VOCABULARY=str(voc)))
    assert r.returncode == 0, r.stderr
    store = dict(enumerate([case["keep"], case["drop"]] + others))
    pairs, new, n = fr.fuse(store, 0, 1, radius=case["radius"], **kw)
    lines = r.stdout.strip().splitlines()
    head = [l for l in lines if l.startswith("fuse pairs ")]
    assert head == ["fuse pairs %d rewritten %d" % (len(pairs["keep_pos"]), n)] and (which or len(pairs["keep_pos"]) > 20)
    got = [tuple(int(x) for x in l.split()[1:]) for l in lines if l.startswith("pair ")]
    assert got == list(zip(pairs["keep_pos"].tolist(), pairs["drop_pos"].tolist(), pairs["keep_lid"].tolist(), pairs["drop_lid"].tolist(),
                           pairs["dist"].tolist()))
    ids = {int(l.split()[1]): [int(x) for x in l.split()[3:]] for l in lines if l.startswith("entry ")}
    assert ids == {k: fr.entry(*v)[2].tolist() for k, v in new.items()}
