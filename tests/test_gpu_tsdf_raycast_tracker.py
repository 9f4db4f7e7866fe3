"""HipKeyframeTracker.dense_render on the GPU: the view of the tracker's dense map from the latest tracked pose equals
Context.tsdf_raycast at that pose and the numpy reference (tests/tsdf_raycast_ref.py) on a fresh integration of the keyframes,
bit for bit; a tracker without dense_map refuses it; and rendering changes nothing: a run that renders after every frame
returns the poses, records and volume of a run that never does."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_ref as tk  # noqa: E402
import tsdf_ref as tr  # noqa: E402
import tsdf_raycast_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu

DENSE = dict(dims=(32, 24, 20), voxel=0.25, origin=(-1.5, -3.0, 0.0), max_depth=4.5, max_frames=64)
UPDATE = (1e-7, 1e-7)
N_FRAMES = 8
SMALL = dict(width=23, height=17, focal=(22.0, 23.0), principal=(11.0, 8.0))    # a viewer's camera, not the volume's


@pytest.fixture(scope="module")
def sequence():
    return tk.make_sequence(seed=0)


def run(pkg, seq, render, **kw):
    c = pkg.Context(width=0, height=0, max_keypoints=4096)
    t = pkg.HipKeyframeTracker(c, focal=tk.CAM[:2], principal=tk.CAM[2:], local_map_depth=2, local_ba=True, **dict(tk.SEQ_PARAMS, **kw))
    rows, views = [], []
    for f in seq["frames"][:N_FRAMES]:
        rows.append(t.processSensorData(f["desc"], f["xy"], f["depth"]))
        if render:
            views.append(t.dense_render(camera=SMALL))
    return c, t, rows, views


@pytest.fixture(scope="module")
def runs(pkg, sequence):
    quiet = run(pkg, sequence, False, dense_map=DENSE, dense_update=UPDATE)
    drawn = run(pkg, sequence, True, dense_map=DENSE, dense_update=UPDATE)
    yield quiet, drawn
    quiet[0].close()
    drawn[0].close()


def test_render_equals_raycast_and_the_reference(runs, sequence):
    c, t, rows, views = runs[1]
    assert len(t.ids) >= 2 and rows[-1]["tracked"]
    got = t.dense_render(camera=SMALL)
    R, tv = rows[-1]["R"], rows[-1]["tvec"]
    direct = c.tsdf_raycast(R, tv, camera=SMALL)
    for a, b in zip(got, direct):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(got, views[-1]):                      # the render after the last frame, made during the run
        assert a.tobytes() == b.tobytes()
    p = tr.params(DENSE["dims"], DENSE["voxel"], DENSE["origin"], None, DENSE["max_depth"], DENSE["max_frames"], sequence["width"],
                  sequence["height"], 1.0 / 5000.0, tk.CAM[:2], tk.CAM[2:])
    depth_of = {r["keyframe"]: sequence["frames"][f]["depth"] for f, r in enumerate(rows) if r["keyframe"] >= 0}
    S, W = tr.fresh(p, [(depth_of[k],) + t.dense_poses[k] for k in t.ids])
    ref = rr.raycast(S, W, p, R, tv, camera=SMALL)
    hits = int((ref[0] > 0).sum())
    print("dense_render: %d of %d pixels hit over %d keyframes" % (hits, ref[0].size, len(t.ids)))
    assert hits > 0
    for a, b in zip(got, ref):
        assert a.tobytes() == b.tobytes()
    # an explicit pose and the keywords of tsdf_raycast go through; the default camera is the volume's
    other = t.dense_render(np.eye(3), np.zeros(3), camera=SMALL, min_weight=2, normals=False)
    want = c.tsdf_raycast(np.eye(3), np.zeros(3), camera=SMALL, min_weight=2, normals=False)
    assert other[2] is None and other[0].tobytes() == want[0].tobytes() and other[1].tobytes() == want[1].tobytes()
    assert t.dense_render(coarse=1)[0].shape == (sequence["height"], sequence["width"])


def test_rendering_changes_nothing(runs):
    (c0, t0, a, _), (c1, t1, b, views) = runs
    assert len(views) == N_FRAMES and any((v[0] > 0).any() for v in views)
    assert t0.ids == t1.ids and len(t0.ba_results) == len(t1.ba_results) and t0.dense_results == t1.dense_results
    for f, (x, y) in enumerate(zip(a, b)):
        assert (x["tracked"], x["n_inliers"], x["keyframe"], x["reference"], x["relocalized"]) == \
               (y["tracked"], y["n_inliers"], y["keyframe"], y["reference"], y["relocalized"]), f
        assert x["R"].tobytes() == y["R"].tobytes() and x["tvec"].tobytes() == y["tvec"].tobytes() and x["rvec"].tobytes() == y["rvec"].tobytes(), f
    for k in t0.ids:
        assert c0.kf_read(k)[1].tobytes() == c1.kf_read(k)[1].tobytes()
        assert t0.backend.poses[k].tobytes() == t1.backend.poses[k].tobytes()
        assert t0.dense_poses[k][0].tobytes() == t1.dense_poses[k][0].tobytes() and t0.dense_poses[k][1].tobytes() == t1.dense_poses[k][1].tobytes()
    S0, W0 = c0.tsdf_read()
    S1, W1 = c1.tsdf_read()
    assert np.array_equal(S0, S1) and np.array_equal(W0, W1) and W0.any()


def test_render_needs_the_dense_map(pkg, sequence):
    c = pkg.Context(width=0, height=0, max_keypoints=4096)
    t = pkg.HipKeyframeTracker(c, focal=tk.CAM[:2], principal=tk.CAM[2:], local_map_depth=2, **tk.SEQ_PARAMS)
    f = sequence["frames"][0]
    t.processSensorData(f["desc"], f["xy"], f["depth"])
    with pytest.raises(pkg.MslamHipError) as e:
        t.dense_render()
    assert e.value.code == pkg.E_INVALID
    # with the option but before the first keyframe there is no volume yet
    t2 = pkg.HipKeyframeTracker(c, focal=tk.CAM[:2], principal=tk.CAM[2:], dense_map=DENSE)
    with pytest.raises(pkg.MslamHipError) as e:
        t2.dense_render()
    assert e.value.code == pkg.E_INVALID
    with pytest.raises(pkg.MslamHipError):
        c.tsdf_info()
    c.close()
