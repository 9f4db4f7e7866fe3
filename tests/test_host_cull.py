"""Keyframe culling through the plugin loader: `mslam_harness <plugin> --cull <scene>` (IKeyframeCuller::cullKeyframes on
the relocalizer adapter, which owns the store and the BoW database) on two scenes written by tests/cull_ref.py, against the
restatement: the count, every candidate's verdict and counts, and the entries the adapter still holds."""
import os
import subprocess
import sys

import pytest

import cull_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "modular-slam_amd", "host")
HARNESS = os.path.join(HOST, "mslam_harness")
PLUGIN = os.path.join(HOST, "libmslam_hip_plugin.so")


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", HOST])
    return True


def test_harness_interface_and_adapter_know_the_culling(built):
    harness = open(os.path.join(HOST, "harness.cpp")).read()
    assert "--cull" in harness and "IKeyframeCuller" in harness
    assert "class IKeyframeCuller" in open(os.path.join(HOST, "mslam_interfaces.hpp")).read()
    assert "public IKeyframeCuller" in open(os.path.join(HOST, "mslam_hip_plugin.cpp")).read()
    out = subprocess.check_output(["nm", "-DC", PLUGIN]).decode()
    assert "mslam_hip_kf_cull_search" in out                              # the plugin calls the new C ABI


def _scenes():
    sizes = [1 + (37 * e) % 300 for e in range(70)]
    sizes[:4] = [256, 257, cr.STRIDE + 1, 1]
    store = cr.random_case(43, sizes, pool=1200, repeats=0.1)
    ids = sorted(store)
    a = (store, ids[:-2], ids[5:40][::-1] + ids[:5], dict(min_observers=8, ratio=0.6, min_landmarks=20))   # two entries not listed
    lids, listed, cand, kw, _ = cr.chain_case()
    return [a, (cr.store_of(lids), listed, cand, kw)]


def test_the_scenes_cull_some_and_keep_some():
    for store, ids, cand, kw in _scenes():
        res = cr.cull_search(store, ids, cand, **kw)
        assert 0 < res["n_culled"] < len(cand)


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1])
def test_harness_cull_equals_the_reference(built, tmp_path, which):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth
    store, ids, cand, kw = _scenes()[which]
    voc = tmp_path / "orbvoc.dbow3"
    voc.write_bytes(synth.make_vocabulary(10, 3))
    path = tmp_path / "cull.bin"
    cr.write_scene(str(path), store, ids, cand, **kw)
    r = subprocess.run([HARNESS, PLUGIN, "--cull", str(path)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, MSLAM_ORB_VOCABULARY=str(voc)))
    assert r.returncode == 0, r.stderr
    new, ref = cr.cull(store, ids, cand, **kw)
    lines = r.stdout.strip().splitlines()
    assert [l for l in lines if l.startswith("cull ")] == ["cull culled %d" % ref["n_culled"]]
    rows = [tuple(int(x) for x in l.split()[1:]) for l in lines if l.startswith("cand ")]
    assert rows == [(p, k, int(c), int(nl), int(nr))
                    for p, (k, c, nl, nr) in enumerate(zip(cand, ref["culled"], ref["n_landmarks"], ref["n_redundant"]))]
    left = [l for l in lines if l.startswith("remaining")]
    assert len(left) == 1 and [int(x) for x in left[0].split()[1:]] == [k for k in store if k in new]
