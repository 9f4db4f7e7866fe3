"""The dense TSDF map on the GPU (k_tsdf.hip) against the numpy reference tests/tsdf_ref.py.  Both sides evaluate the same
separately rounded IEEE operations, so S and W from tsdf_read equal the reference bit for bit, and the extraction gives the
same count and order with xyz and normal equal bit for bit: no tolerance anywhere.  The shapes are the smallest at which the
kernel's tiling (a wave owns 16 x 4 x 1 voxels, a workgroup 4 such tiles along z; MSLAM_HIP_TSDF_CHUNK = 64 entries per sweep;
extraction: 256 consecutive voxels per workgroup) can go wrong."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_ref as tr  # noqa: E402

pytestmark = pytest.mark.gpu

CHUNK = tr.CHUNK


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(width=0, height=0)
    yield c
    c.close()


def load(ctx, p, frames, ids=None):
    ctx.tsdf_create(**tr.create_kwargs(p))
    for q, (d, R, t) in enumerate(frames):
        ctx.tsdf_add_frame(q if ids is None else ids[q], d, R, t)


def same_volume(ctx, ref, what=""):
    S, W = ctx.tsdf_read()
    assert S.dtype == np.int32 and S.shape == ref[0].shape
    assert np.array_equal(W, ref[1]), (what, "W", int((W != ref[1]).sum()))
    assert np.array_equal(S, ref[0]), (what, "S", int((S != ref[0]).sum()))


def same_surface(ctx, ref, p, min_weight, what=""):
    xyz, nrm = ctx.tsdf_extract(min_weight)
    rx, rn = tr.extract(ref[0], ref[1], p, min_weight)
    assert len(xyz) == len(rx), (what, len(xyz), len(rx))
    assert xyz.tobytes() == rx.tobytes(), what
    assert nrm.tobytes() == rn.tobytes(), what
    return len(xyz)


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, (p, frames) in tr.shape_cases().items():
        out[name] = (p, frames, tr.fresh(p, frames))
    return out


@pytest.mark.parametrize("name", ["ny_not_block", "below_one_wave", "nx_crosses_wave", "plane_many_groups"])
def test_shapes(ctx, cases, name):
    p, frames, ref = cases[name]
    assert ref[1].max() >= 1 and np.any(ref[0] < 0) and np.any(ref[0] > 0)
    load(ctx, p, frames)
    same_volume(ctx, ref, name)
    n1 = same_surface(ctx, ref, p, 1, name)
    n2 = same_surface(ctx, ref, p, 2, name)
    print("%s: %d / %d points" % (name, n1, n2))
    assert n1 > 0
    if name == "plane_many_groups":
        # a condition on the input: the rows come from many of the extraction's workgroups (256 consecutive voxels each)
        groups = np.unique(tr.extract(ref[0], ref[1], p, 1, with_index=True)[2] // 256)
        assert len(groups) >= 64


def test_camera_inside_and_blind_frame(ctx):
    """the camera sits inside the volume: voxels behind it and beside the frustum stay untouched; a frame that looks away from
    the volume changes nothing"""
    p, frames = tr.sphere_scene((24, 20, 32), origin=(-0.6, -0.5, -0.2))
    ref = tr.fresh(p, frames)
    assert not tr.fresh(p, frames[:1])[1][:4].any() and ref[1].any()    # the slabs behind the first camera stay empty under it
    load(ctx, p, frames)
    same_volume(ctx, ref)
    same_surface(ctx, ref, p, 1)
    # a camera far behind the volume that looks the other way
    p2, frames2 = tr.sphere_scene()
    load(ctx, p2, frames2)
    before = tr.fresh(p2, frames2)
    R, t = tr.rot(1, np.pi), np.array([0.0, 0.0, -3.0])
    blind = frames2[0][0]
    after = tr.integrate(before[0].copy(), before[1].copy(), p2, blind, R, t)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])    # the reference sees nothing either
    ctx.tsdf_add_frame(77, blind, R, t)
    same_volume(ctx, before)
    assert ctx.tsdf_info()[1] == 4
    ctx.tsdf_remove_frame(77)
    same_volume(ctx, before)


@pytest.mark.parametrize("max_depth", [1.0, np.inf])
def test_depth_values(ctx, max_depth):
    """raw 0, 1 and 65535, and values either side of max_depth = 1 m (raw 5000)"""
    rng = np.random.default_rng(5)
    p = tr.params((24, 20, 16), 0.05, (-0.6, -0.5, 0.6), 0.2, max_depth=max_depth)
    values = np.array([0, 1, 65535, 4998, 4999, 5000, 5001, 5002, 4500, 5500, 4000], np.uint16)
    frames = []
    for R, t in tr.SPHERE_POSES:
        frames.append((values[rng.integers(0, len(values), (p["height"], p["width"]))], R, t))
    ref = tr.fresh(p, frames)
    one = tr.fresh(tr.params((24, 20, 16), 0.05, (-0.6, -0.5, 0.6), 0.2, max_depth=np.inf if max_depth == 1.0 else 1.0), frames)
    assert not np.array_equal(one[1], ref[1])    # the cut matters on this input
    load(ctx, p, frames)
    same_volume(ctx, ref)
    same_surface(ctx, ref, p, 1)
    assert ctx.tsdf_info()[0].max_depth == max_depth


def many_frames(n, seed):
    """n frames on the 24 x 20 x 16 sphere volume: the three renders under perturbed poses, and a second pose for each"""
    rng = np.random.default_rng(seed)
    p, base = tr.sphere_scene(max_frames=256)
    frames, moved = [], []
    for q in range(n):
        d, R, t = base[q % 3]
        R0 = tr.rot(int(rng.integers(0, 3)), rng.uniform(-0.05, 0.05)) @ R
        frames.append((d, R0, t + rng.uniform(-0.05, 0.05, 3)))
        moved.append((tr.rot(int(rng.integers(0, 3)), rng.uniform(-0.05, 0.05)) @ R0, frames[-1][2] + rng.uniform(-0.05, 0.05, 3)))
    return p, frames, moved


@pytest.fixture(scope="module")
def big():
    return many_frames(2 * CHUNK + 2, 11)


@pytest.mark.parametrize("n", [1, CHUNK // 2, CHUNK // 2 + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 2])
def test_update_poses(ctx, big, n):
    """n moved frames are 2 n entries: one sweep that is exactly full (n = CHUNK / 2) and one entry pair more, then the frame
    counts round CHUNK and 2 CHUNK (two full sweeps at n = CHUNK, a third with two entries at CHUNK + 1)"""
    p, frames, moved = big
    frames, moved = frames[:n], moved[:n]
    load(ctx, p, frames, ids=[100 + 3 * q for q in range(n)])
    ids = [100 + 3 * q for q in range(n)][::-1]    # any order
    Rs = np.stack([moved[q][0] for q in range(n)][::-1])
    ts = np.stack([moved[q][1] for q in range(n)][::-1])
    assert ctx.tsdf_update_poses(ids, Rs, ts) == n
    final = [(frames[q][0], moved[q][0], moved[q][1]) for q in range(n)]
    same_volume(ctx, tr.fresh(p, final), n)
    for q in (0, n - 1):
        R, t = ctx.tsdf_get_frame(100 + 3 * q)
        assert R.tobytes() == np.ascontiguousarray(moved[q][0]).tobytes() and t.tobytes() == moved[q][1].tobytes()
    # the same poses again: nothing moves
    assert ctx.tsdf_update_poses(ids, Rs, ts) == 0
    assert ctx.tsdf_update_poses([], np.zeros((0, 9)), np.zeros((0, 3))) == 0
    same_volume(ctx, tr.fresh(p, final), n)


def test_update_mixed_list(ctx, big):
    """moved frames among bit-identical ones; a pose that differs in its last bit counts as moved"""
    p, frames, moved = big
    n = 9
    load(ctx, p, frames[:n])
    pick = [1, 4, 5, 8]
    final = [(frames[q][0],) + (moved[q] if q in pick else frames[q][1:]) for q in range(n)]
    t_bit = final[2][2].copy()
    t_bit[0] = np.nextafter(t_bit[0], 1.0)
    final[2] = (final[2][0], final[2][1], t_bit)
    ids = list(range(n))
    got = ctx.tsdf_update_poses(ids, np.stack([f[1] for f in final]), np.stack([f[2] for f in final]))
    assert got == len(pick) + 1
    same_volume(ctx, tr.fresh(p, final))
    same_surface(ctx, tr.fresh(p, final), p, 2)


def test_remove_and_rebuild(ctx, cases):
    p, frames, ref = cases["ny_not_block"]
    load(ctx, p, frames)
    ctx.tsdf_remove_frame(1)
    rest = tr.fresh(p, [frames[0], frames[2]])
    same_volume(ctx, rest)
    same_surface(ctx, rest, p, 1)
    assert ctx.tsdf_info()[1] == 2
    ctx.tsdf_remove_frame(0)
    ctx.tsdf_remove_frame(2)
    same_volume(ctx, tr.zeros(p))
    xyz, nrm = ctx.tsdf_extract(1)
    assert xyz.shape == (0, 3) and nrm.shape == (0, 3)    # an empty volume: n = 0 and OK
    # create over a volume with frames: zeros again and the ids are free
    load(ctx, p, frames)
    assert ctx.tsdf_info()[1] == 3
    ctx.tsdf_create(**tr.create_kwargs(p))
    assert ctx.tsdf_info()[1] == 0
    same_volume(ctx, tr.zeros(p))
    ctx.tsdf_add_frame(0, *frames[0])
    same_volume(ctx, tr.fresh(p, frames[:1]))


def test_add_frame_from_device(ctx, cases):
    import torch
    p, frames, ref = cases["ny_not_block"]
    ctx.tsdf_create(**tr.create_kwargs(p))
    keep = []
    for q, (d, R, t) in enumerate(frames):
        dev = torch.from_numpy(d.view(np.int16).copy()).cuda()
        keep.append(dev)
        ctx.tsdf_add_frame(q, dev.data_ptr(), R, t)
        dev.zero_()    # the image was copied: the caller's buffer is free again
    torch.cuda.synchronize()
    same_volume(ctx, ref)
    ctx.tsdf_update_poses([1], frames[1][1][None], (frames[1][2] + 0.01)[None])
    same_volume(ctx, tr.fresh(p, [frames[0], (frames[1][0], frames[1][1], frames[1][2] + 0.01), frames[2]]))


def refused(pkg, code, call, *args):
    with pytest.raises(pkg.MslamHipError) as e:
        call(*args)
    assert e.value.code == code, e.value


def test_errors_leave_everything_untouched(pkg, ctx, cases):
    p, frames, ref = cases["ny_not_block"]
    p3 = dict(p, max_frames=3)
    load(ctx, p3, frames)
    d, R, t = frames[0]
    I, z = np.eye(3), np.zeros(3)

    def unchanged():
        same_volume(ctx, ref)
        assert ctx.tsdf_info()[1] == 3
        for q in range(3):
            Rq, tq = ctx.tsdf_get_frame(q)
            assert np.array_equal(Rq, frames[q][1]) and np.array_equal(tq, frames[q][2])

    refused(pkg, pkg.E_CAPACITY, ctx.tsdf_add_frame, 3, d, R, t)                  # a fourth frame
    unchanged()
    refused(pkg, pkg.E_INVALID, ctx.tsdf_add_frame, 1, d, R, t)                   # the id exists
    unchanged()
    moved = np.stack([tr.rot(0, 0.1), tr.rot(1, 0.1)])
    refused(pkg, pkg.E_INVALID, ctx.tsdf_update_poses, [0, 0], moved, np.zeros((2, 3)))    # listed twice
    unchanged()
    refused(pkg, pkg.E_INVALID, ctx.tsdf_update_poses, [0, 9], moved, np.zeros((2, 3)))    # unknown, behind a valid move
    unchanged()
    refused(pkg, pkg.E_INVALID, ctx.tsdf_get_frame, 9)
    refused(pkg, pkg.E_INVALID, ctx.tsdf_remove_frame, 9)
    unchanged()
    bad = moved.copy()
    bad[1, 2, 1] = np.nan
    refused(pkg, pkg.E_INVALID, ctx.tsdf_update_poses, [0, 1], bad, np.zeros((2, 3)))      # a NaN in R, behind a valid move
    unchanged()
    refused(pkg, pkg.E_INVALID, ctx.tsdf_update_poses, [0], I[None], np.array([[0.0, np.inf, 0.0]]))
    unchanged()
    ctx.tsdf_remove_frame(2)
    refused(pkg, pkg.E_INVALID, ctx.tsdf_add_frame, 2, d, bad[1], z)              # add with a NaN: nothing is retained
    ctx.tsdf_add_frame(2, *frames[2])
    unchanged()
    refused(pkg, pkg.E_INVALID, ctx.tsdf_extract, 0)                              # min_weight < 1
    # a capacity one short: the count comes back, no row is written
    import ctypes as C
    rx, _ = tr.extract(ref[0], ref[1], p, 1)
    xyz = np.full((len(rx), 3), 7.0, np.float32)
    n = C.c_int(0)
    rc = ctx.L.mslam_hip_tsdf_extract(ctx._h, 1, xyz.ctypes.data_as(C.c_void_p), None, len(rx) - 1, C.byref(n))
    assert rc == pkg.E_CAPACITY and n.value == len(rx) and np.all(xyz == 7.0)
    rc = ctx.L.mslam_hip_tsdf_extract(ctx._h, 1, xyz.ctypes.data_as(C.c_void_p), None, len(rx), C.byref(n))
    assert rc == pkg.OK and n.value == len(rx) and xyz.tobytes() == rx.tobytes()
    unchanged()
    # parameters outside their ranges: the volume that exists stays
    for k, v in (("dims", (0, 4, 4)), ("dims", (1 << 11, 1 << 10, 1 << 10)), ("voxel", 0.0), ("voxel", np.nan), ("trunc", -1.0),
                 ("trunc", np.inf), ("max_depth", 0.0), ("max_depth", np.nan), ("max_frames", 0), ("max_frames", 32769),
                 ("origin", (0.0, np.inf, 0.0)), ("focal", (0.0, 40.0)), ("focal", (40.0, np.nan)), ("width", 0)):
        refused(pkg, pkg.E_INVALID, lambda kw: ctx.tsdf_create(**kw), dict(tr.create_kwargs(p3), **{k: v}))
    unchanged()
    # no volume at all
    ctx.tsdf_destroy()
    ctx.tsdf_destroy()
    for call, args in ((ctx.tsdf_info, ()), (ctx.tsdf_add_frame, (0, 0x1000, I, z)), (ctx.tsdf_get_frame, (0,)),
                       (ctx.tsdf_update_poses, ([0], I[None], z[None])), (ctx.tsdf_remove_frame, (0,)), (ctx.tsdf_extract, (1,))):
        refused(pkg, pkg.E_INVALID, call, *args)
