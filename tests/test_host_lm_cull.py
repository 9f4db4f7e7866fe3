"""Landmark culling through the plugin loader: `mslam_harness <plugin> --cull-landmarks <scene>`
(ILandmarkCuller::cullLandmarks on the relocalizer adapter, which owns the store) on two scenes written by
tests/lm_cull_ref.py, against the restatement: the counts, every culled id with its observer count, and every entry's size
afterwards."""
import os
import subprocess
import sys

import pytest

import cull_ref as cr
import lm_cull_ref as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "modular-slam_amd", "host")
HARNESS = os.path.join(HOST, "mslam_harness")
PLUGIN = os.path.join(HOST, "libmslam_hip_plugin.so")


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", HOST])
    return True


def test_harness_interface_and_adapter_know_the_landmark_culling(built):
    harness = open(os.path.join(HOST, "harness.cpp")).read()
    assert "--cull-landmarks" in harness and "ILandmarkCuller" in harness and "MSLC" in harness
    iface = open(os.path.join(HOST, "mslam_interfaces.hpp")).read()
    assert "class ILandmarkCuller" in iface and "cullLandmarks" in iface and "removeLandmarks" in iface
    assert "public ILandmarkCuller" in open(os.path.join(HOST, "mslam_hip_plugin.cpp")).read()
    out = subprocess.check_output(["nm", "-DC", PLUGIN]).decode()
    assert "mslam_hip_kf_cull_landmarks" in out and "mslam_hip_kf_remove_landmarks" in out      # the plugin calls the new C ABI


def _scenes():
    sizes = [1 + (37 * e) % 300 for e in range(70)]
    sizes[:4] = [256, 257, 600, 1]
    store = cr.random_case(43, sizes, pool=3000, repeats=0.1)
    ids = sorted(store)
    a = (store, ids[:-2], ids[5:40][::-1] + ids[:5], 3)                    # two entries not listed
    lids, listed, cand, mo = lc.hand_case("unlisted_holder")               # and an entry that holds a culled id and is not listed
    return [a, (cr.store_of(lids), listed, cand, mo)]


def test_the_scenes_cull_some_landmarks_and_keep_some():
    for store, ids, cand, mo in _scenes():
        new, res = lc.cull_landmarks(store, ids, cand, mo)
        assert 0 < res["n_removed"] < sum(len(store[k][2]) for k in cand)
        assert len(res["landmark_ids"]) > 0 and any(len(new[k][2]) > 0 for k in cand)


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1])
def test_harness_cull_landmarks_equals_the_reference(built, tmp_path, which):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth
    store, ids, cand, mo = _scenes()[which]
    voc = tmp_path / "orbvoc.dbow3"
    voc.write_bytes(synth.make_vocabulary(10, 3))
    path = tmp_path / "lmcull.bin"
    lc.write_scene(str(path), store, ids, cand, mo)
    r = subprocess.run([HARNESS, PLUGIN, "--cull-landmarks", str(path)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, MSLAM_ORB_VOCABULARY=str(voc)))
    assert r.returncode == 0, r.stderr
    new, ref = lc.cull_landmarks(store, ids, cand, mo)
    lines = r.stdout.strip().splitlines()
    assert [l for l in lines if l.startswith("lmcull ")] == ["lmcull found %d removed %d" % (len(ref["landmark_ids"]), ref["n_removed"])]
    rows = [tuple(int(x) for x in l.split()[1:]) for l in lines if l.startswith("lm ")]
    assert rows == list(zip(ref["landmark_ids"].tolist(), ref["observers"].tolist()))
    left = [tuple(int(x) for x in l.split()[1:]) for l in lines if l.startswith("entry ")]
    assert left == [(k, len(new[k][2])) for k in store]
