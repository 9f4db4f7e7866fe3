"""HipKeyframeTracker(dense_map=...) on the GPU: after a run with local BA the volume equals the reference's fresh integration
(tests/tsdf_ref.py) of the keyframes' depth images at tracker.dense_poses, bit for bit, although keyframes were re-integrated
on the way; and the option changes nothing else: the same run without it returns the same poses and records."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_ref as tk  # noqa: E402
import tsdf_ref as tr  # noqa: E402

pytestmark = pytest.mark.gpu

# 8 x 6 x 5 m round the wall the sequence's camera slides along, coarse: the test is about the bookkeeping.  max_depth 4.5 m takes
# in the whole background (2 .. 4 m), so that the keyframes' views overlap
DENSE = dict(dims=(32, 24, 20), voxel=0.25, origin=(-1.5, -3.0, 0.0), max_depth=4.5, max_frames=64)
# any pose the back end moved by more than a tenth of a micrometre / microradian is re-integrated: local BA moves the keyframes
# of this sequence by the depth quantisation's share, far more than that (the test prints what it saw)
UPDATE = (1e-7, 1e-7)


@pytest.fixture(scope="module")
def sequence():
    return tk.make_sequence(seed=0)


def run(pkg, seq, window=None, **kw):
    c = pkg.Context(width=0, height=0, max_keypoints=4096)
    t = pkg.HipKeyframeTracker(c, focal=tk.CAM[:2], principal=tk.CAM[2:], local_map_depth=2, local_ba=True, **dict(tk.SEQ_PARAMS, **kw))
    fr = seq["frames"]
    if window is None:
        rows = [t.processSensorData(f["desc"], f["xy"], f["depth"]) for f in fr]
    else:
        rows = t.process_window([f["desc"] for f in fr], [f["xy"] for f in fr], [f["depth"] for f in fr], window=window)
    return c, t, rows


def ref_params(seq):
    return tr.params(DENSE["dims"], DENSE["voxel"], DENSE["origin"], None, DENSE["max_depth"], DENSE["max_frames"], seq["width"], seq["height"],
                     1.0 / 5000.0, tk.CAM[:2], tk.CAM[2:])


def check_volume(pkg, c, t, rows, seq):
    p = ref_params(seq)
    info, n = c.tsdf_info()
    assert n == len(t.ids) == len(t.dense_poses) >= 3
    assert (info.trunc, info.max_depth, info.width, info.height) == (1.0, 4.5, seq["width"], seq["height"])
    depth_of = {r["keyframe"]: seq["frames"][f]["depth"] for f, r in enumerate(rows) if r["keyframe"] >= 0}
    assert sorted(depth_of) == sorted(t.ids)
    frames = [(depth_of[k],) + t.dense_poses[k] for k in t.ids]
    ref = tr.fresh(p, frames)
    assert ref[1].max() >= 2 and np.any(ref[0] < 0)
    S, W = c.tsdf_read()
    assert np.array_equal(W, ref[1]) and np.array_equal(S, ref[0])
    for k in t.ids:
        R, tt = c.tsdf_get_frame(k)
        assert R.tobytes() == t.dense_poses[k][0].tobytes() and tt.tobytes() == t.dense_poses[k][1].tobytes()
    # the CPU side: keyframes were re-integrated, and the poses they ended at are not the tracked poses they came in with
    moved = sum(r["moved"] for r in t.dense_results)
    assert all(r["moved"] == len(r["listed"]) for r in t.dense_results)
    assert len(t.dense_results) == len(t.ba_results)
    tracked = {r["keyframe"]: (r["step"]["R"], r["step"]["tvec"]) for r in rows if r["keyframe"] > 0}
    change = {k: t.dense_pose_change(np.asarray(R, np.float64).reshape(3, 3), np.asarray(tv, np.float64), *t.dense_poses[k])
              for k, (R, tv) in tracked.items()}
    print("re-integrated %d times over %d updates; tracked -> final pose change per keyframe (m, rad): %s" % (
        moved, len(t.dense_results), {k: ("%.2e" % d, "%.2e" % a) for k, (d, a) in change.items()}))
    assert moved >= 1
    assert any(d > UPDATE[0] or a > UPDATE[1] for d, a in change.values())
    # every retained keyframe is within the bound of its back-end pose
    for k in t.ids:
        pose = t.backend.poses[k]
        R = pkg.quaternion_to_rotation(pose[:4]).T
        d, a = t.dense_pose_change(*t.dense_poses[k], R, -R @ pose[4:])
        assert d <= UPDATE[0] and a <= UPDATE[1], (k, d, a)
    xyz, nrm = c.tsdf_extract(2)
    rx, rn = tr.extract(ref[0], ref[1], p, 2)
    assert xyz.tobytes() == rx.tobytes() and nrm.tobytes() == rn.tobytes()


@pytest.fixture(scope="module")
def runs(pkg, sequence):
    plain = run(pkg, sequence)
    dense = run(pkg, sequence, dense_map=DENSE, dense_update=UPDATE)
    yield plain, dense
    plain[0].close()
    dense[0].close()


def test_volume_follows_the_keyframe_poses(pkg, runs, sequence):
    c, t, rows = runs[1]
    check_volume(pkg, c, t, rows, sequence)


def test_volume_follows_over_windows(pkg, sequence):
    c, t, rows = run(pkg, sequence, window=4, dense_map=DENSE, dense_update=UPDATE)
    check_volume(pkg, c, t, rows, sequence)
    c.close()


def test_culled_keyframes_leave_the_volume(pkg):
    """kf_cull on tests/cull_ref.triple_walk() (every frame a keyframe, the middle ones become redundant): the volume holds the
    keyframes that are left, at their current poses"""
    import cull_ref as cr
    seq = cr.triple_walk()
    c = pkg.Context(width=0, height=0, max_keypoints=4096)
    t = pkg.HipKeyframeTracker(c, focal=tk.CAM[:2], principal=tk.CAM[2:], local_map_depth=cr.WALK_DEPTH, local_ba=True, kf_cull=True,
                               dense_map=DENSE, dense_update=UPDATE, **cr.WALK_PARAMS)
    rows = [t.processSensorData(f["desc"], f["xy"], f["depth"]) for f in seq["frames"]]
    gone = [k for r in t.cull_results for k in r["culled"]]
    print("culled %s, left %s, re-integrated %d times" % (gone, t.ids, sum(r["moved"] for r in t.dense_results)))
    assert len(gone) >= 2 and not set(gone) & set(t.ids)
    assert sorted(t.dense_poses) == sorted(t.ids) and c.tsdf_info()[1] == len(t.ids)
    depth_of = {r["keyframe"]: seq["frames"][f]["depth"] for f, r in enumerate(rows) if r["keyframe"] >= 0}
    ref = tr.fresh(ref_params(seq), [(depth_of[k],) + t.dense_poses[k] for k in t.ids])
    S, W = c.tsdf_read()
    assert W.max() >= 2 and np.array_equal(W, ref[1]) and np.array_equal(S, ref[0])
    for k in gone:
        with pytest.raises(pkg.MslamHipError):
            c.tsdf_get_frame(k)
    c.close()


def test_volume_follows_a_loop_closure_and_global_ba(pkg):
    """the ring walk of tests/loop_walk.py closes one loop and runs the global solve behind it: one update follows each of
    close_loop and global_ba, and the volume holds every keyframe at the pose it ended at"""
    import loop_walk
    import synth
    seq = loop_walk.ring_sequence()
    dense = dict(dims=(32, 12, 32), voxel=0.25, origin=(-4.0, -1.5, -4.0), max_depth=4.5, max_frames=64)
    c = pkg.Context(width=0, height=0, max_keypoints=4096)
    c.bow_load(synth.make_vocabulary(10, 3))
    t = pkg.HipKeyframeTracker(c, focal=tk.CAM[:2], principal=tk.CAM[2:], local_map_depth=2, local_ba=True,
                               new_keyframe_min_landmarks=200, loop_closure=True, loop_min_gap=5, loop_global_ba=True,
                               dense_map=dense, dense_update=UPDATE)
    rows = [t.processSensorData(f["desc"], f["xy"], f["depth"]) for f in seq["frames"]]
    closed = [a for a in t.loop_results if a["loop"] is not None and a["result"]["termination"] != 2]
    assert len(closed) == 1 and "global_ba" in closed[0]
    assert len(t.dense_results) == len(t.ba_results) + 2                 # local BA per keyframe, then close_loop and global_ba
    print("ring: %d keyframes, updates moved %s" % (len(t.ids), [r["moved"] for r in t.dense_results]))
    at_closure = t.dense_results[closed[0]["keyframe"]]    # keyframe k's local BA is update k - 1; close_loop's comes right after it
    assert at_closure["moved"] >= 2
    p = tr.params(dense["dims"], dense["voxel"], dense["origin"], None, dense["max_depth"], dense["max_frames"], seq["width"],
                  seq["height"], 1.0 / 5000.0, tk.CAM[:2], tk.CAM[2:])
    depth_of = {r["keyframe"]: seq["frames"][f]["depth"] for f, r in enumerate(rows) if r["keyframe"] >= 0}
    assert sorted(depth_of) == sorted(t.ids) == sorted(t.dense_poses)
    ref = tr.fresh(p, [(depth_of[k],) + t.dense_poses[k] for k in t.ids])
    S, W = c.tsdf_read()
    assert W.max() >= 2 and np.array_equal(W, ref[1]) and np.array_equal(S, ref[0])
    for k in t.ids:
        pose = t.backend.poses[k]
        R = pkg.quaternion_to_rotation(pose[:4]).T
        d, a = t.dense_pose_change(*t.dense_poses[k], R, -R @ pose[4:])
        assert d <= UPDATE[0] and a <= UPDATE[1], (k, d, a)
    c.close()


def test_without_dense_map_nothing_changes(pkg, runs):
    (c0, t0, a), (c1, t1, b) = runs
    assert t0.dense_map is None and t0.dense_poses == {} and t0.dense_results == []
    with pytest.raises(pkg.MslamHipError):
        c0.tsdf_info()                      # no volume was ever created
    assert t0.ids == t1.ids and len(t0.ba_results) == len(t1.ba_results)
    for f, (x, y) in enumerate(zip(a, b)):
        assert (x["tracked"], x["n_inliers"], x["keyframe"], x["reference"], x["relocalized"]) == \
               (y["tracked"], y["n_inliers"], y["keyframe"], y["reference"], y["relocalized"]), f
        assert x["R"].tobytes() == y["R"].tobytes() and x["tvec"].tobytes() == y["tvec"].tobytes() and x["rvec"].tobytes() == y["rvec"].tobytes(), f
    for k in t0.ids:
        assert c0.kf_read(k)[1].tobytes() == c1.kf_read(k)[1].tobytes()
        assert t0.backend.poses[k].tobytes() == t1.backend.poses[k].tobytes()
    for x, y in zip(t0.ba_results, t1.ba_results):
        assert x["final_cost"] == y["final_cost"] and x["iterations"] == y["iterations"]


def test_dense_options_are_checked(pkg):
    with pytest.raises(pkg.MslamHipError):
        pkg.HipKeyframeTracker(None, dense_update=(0.1, 0.1))             # needs dense_map
    with pytest.raises(pkg.MslamHipError):
        pkg.HipKeyframeTracker(None, dense_map=dict(dims=(4, 4, 4), voxel=0.1))    # no origin
    with pytest.raises(pkg.MslamHipError):
        pkg.HipKeyframeTracker(None, dense_map=dict(DENSE, colour=True))
    t = pkg.HipKeyframeTracker(None, dense_map=dict(dims=(4, 4, 4), voxel=0.25, origin=(0, 0, 0)))
    assert t.dense_update == (0.125, 0.25 / 6.0) and t.dense_map["max_depth"] == 3.0                          # voxel / 2, voxel / (2 max_depth)
