"""The ray-cast of the dense TSDF map on the GPU (k_tsdf_raycast.hip) against the numpy reference tests/tsdf_raycast_ref.py.
Both sides evaluate the same separately rounded IEEE f64 operations, so depth, xyz and normal are compared by .tobytes(): no
tolerance anywhere.  The shapes are the smallest at which the kernel can go wrong: a wave owns 8 x 8 pixels and a workgroup
16 x 16, so 40 x 30, 23 x 17, 1 x 1 and 65 x 1 leave partial tiles in both directions; the volumes are those of
tests/test_gpu_tsdf.py; the march is run with every coarse stride that takes another path."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_ref as tr  # noqa: E402
import tsdf_raycast_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu

I, Z = np.eye(3), np.zeros(3)
TILTED = (tr.rot(1, -0.12) @ tr.rot(0, 0.07), np.array([-0.1, 0.05, 0.02]))
BLIND = (tr.rot(1, np.pi), np.array([0.0, 0.0, -3.0]))
ODD = dict(width=23, height=17, focal=(22.0, 23.0), principal=(11.0, 8.0))


def scenes():
    s = dict(tr.shape_cases())
    return {"sphere": s["ny_not_block"], "long": s["nx_crosses_wave"], "plane": s["plane_many_groups"],
            "small": tr.sphere_scene((9, 7, 5), voxel=0.1, origin=(-0.45, -0.35, 0.55), trunc=0.3),
            "open": tr.sphere_scene(max_depth=np.inf)}


# name -> (scene, R, t, keywords of tsdf_raycast, hits: None = at least one hit and one miss, 0 = none, "all" = every pixel)
CASES = {
    # tile edges
    "40x30": ("sphere", I, Z, {}, None),
    "23x17_axis_rays": ("sphere", I, Z, dict(camera=ODD), None),
    "1x1": ("sphere", I, Z, dict(camera=dict(width=1, height=1, focal=(40.0, 40.0), principal=(0.0, 0.0))), "all"),
    "65x1": ("sphere", I, Z, dict(camera=dict(width=65, height=1, focal=(40.0, 40.0), principal=(32.0, 0.0))), None),
    # volume edges
    "small": ("small", I, Z, {}, None),
    "long": ("long", I, Z, {}, None),
    "plane": ("plane", I, Z, {}, None),
    "open_default_far": ("open", I, Z, {}, None),
    # poses
    "tilted": ("sphere", *TILTED, {}, None),
    "tilted_odd_plane": ("plane", *TILTED, dict(camera=ODD), None),
    "tilted_long": ("long", *TILTED, {}, None),
    "inside": ("sphere", I, np.array([0.0, 0.0, -0.65]), dict(z_near=0.01), "all"),
    "blind": ("sphere", *BLIND, {}, 0),
    "behind_surface": ("sphere", I, Z, dict(z_near=0.9), 0),
    # march
    "coarse_1": ("sphere", I, Z, dict(coarse=1), None),
    "coarse_2": ("sphere", I, Z, dict(coarse=2), None),
    "coarse_beyond": ("sphere", I, Z, dict(coarse=1 << 24), None),
    "step_voxel": ("sphere", I, Z, dict(step=0.05), None),
    "z_far_cut": ("sphere", I, Z, dict(z_far=0.75), None),
    "one_sample": ("sphere", I, Z, dict(z_near=0.8, z_far=0.8), 0),
    "min_weight_2": ("sphere", I, Z, dict(min_weight=2), None),
    "min_weight_3": ("sphere", I, Z, dict(min_weight=3), None),
    "tilted_min_weight_2_coarse_3": ("plane", *TILTED, dict(min_weight=2, coarse=3), None),
}


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(width=0, height=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def world():
    """scene name -> (params, frames, (S, W)), and the reference renders, computed once each"""
    vols = {name: (p, frames, tr.fresh(p, frames)) for name, (p, frames) in scenes().items()}
    return vols, {}


def reference(world, name):
    vols, done = world
    if name not in done:
        scene, R, t, kw, _ = CASES[name]
        p, _, (S, W) = vols[scene]
        done[name] = rr.raycast(S, W, p, R, t, **kw)
    return done[name]


def load(ctx, p, frames):
    ctx.tsdf_create(**tr.create_kwargs(p))
    for q, (d, R, t) in enumerate(frames):
        ctx.tsdf_add_frame(q, d, R, t)


def same(got, ref, what=""):
    for g, r, part in zip(got, ref, ("depth", "xyz", "normal")):
        assert g.dtype == np.float32 and g.shape == r.shape, (what, part)
        assert g.tobytes() == r.tobytes(), (what, part, int((g != r).sum()))


@pytest.mark.parametrize("name", list(CASES))
def test_cases(ctx, world, name):
    scene, R, t, kw, expect = CASES[name]
    p, frames, _ = world[0][scene]
    ref = reference(world, name)
    hits = int((ref[0] > 0).sum())
    print("%s: %d of %d pixels hit" % (name, hits, ref[0].size))
    # conditions on the inputs: a degenerate case cannot pass silently
    if expect is None:
        assert 0 < hits < ref[0].size
    else:
        assert hits == (ref[0].size if expect == "all" else 0)
    assert np.all((np.linalg.norm(ref[2], axis=-1) > 0) <= (ref[0] > 0))
    load(ctx, p, frames)
    depth, xyz, nrm, n = ctx.tsdf_raycast(R, t, with_hits=True, **kw)
    same((depth, xyz, nrm), ref, name)
    assert n == hits


def test_case_conditions(world):
    """what the cases are there for holds on the reference"""
    # 23 x 17 with principal (11, 8) and R = I: column 11 and row 8 are rays parallel to the volume's faces, and they hit
    ref = reference(world, "23x17_axis_rays")
    assert (11.0 - ODD["principal"][0]) / ODD["focal"][0] == 0.0 and np.any(ref[0][:, 11] > 0) and np.any(ref[0][8, :] > 0)
    # a stride beyond the last sample walks every sample, as coarse = 1 does; the default stride differs from both
    one, far, dflt = reference(world, "coarse_1"), reference(world, "coarse_beyond"), reference(world, "40x30")
    for a, b in zip(one, far):
        assert a.tobytes() == b.tobytes()
    assert one[0].tobytes() != dflt[0].tobytes()
    # the cut removes hits; min_weight removes some
    full = int((dflt[0] > 0).sum())
    assert 0 < int((reference(world, "z_far_cut")[0] > 0).sum()) < full
    assert int((reference(world, "min_weight_3")[0] > 0).sum()) < int((reference(world, "min_weight_2")[0] > 0).sum()) < full


def test_volume_changes(ctx, world):
    """after tsdf_update_poses and tsdf_remove_frame the render is the reference's on a fresh integration of what is retained"""
    p, frames, _ = world[0]["sphere"]
    load(ctx, p, frames)
    R1, t1 = tr.rot(1, 0.23) @ frames[1][1], frames[1][2] + np.array([0.01, -0.02, 0.015])
    assert ctx.tsdf_update_poses([1], R1[None], t1[None]) == 1
    ctx.tsdf_remove_frame(2)
    S, W = tr.fresh(p, [frames[0], (frames[1][0], R1, t1)])
    ref = rr.raycast(S, W, p, *TILTED)
    assert 0 < int((ref[0] > 0).sum()) < ref[0].size and ref[0].tobytes() != reference(world, "tilted")[0].tobytes()
    same(ctx.tsdf_raycast(*TILTED), ref)


def test_call_forms(ctx, world):
    import torch
    p, frames, vol = world[0]["sphere"]
    ref = reference(world, "tilted")
    load(ctx, p, frames)
    before = ctx.tsdf_read()
    first = ctx.tsdf_raycast(*TILTED)
    same(first, ref)
    same(ctx.tsdf_raycast(*TILTED), ref)                               # two calls in a row
    depth, xyz, nrm = ctx.tsdf_raycast(*TILTED, normals=False)         # normal = NULL
    assert nrm is None and depth.tobytes() == ref[0].tobytes() and xyz.tobytes() == ref[1].tobytes()
    # xyz = NULL through the C ABI
    q = ctx.tsdf_raycast_params(*TILTED)
    R, t = np.ascontiguousarray(TILTED[0]), np.ascontiguousarray(TILTED[1])
    d2, n2, hits = np.full((30, 40), 7.0, np.float32), np.full((30, 40, 3), 7.0, np.float32), C.c_int(-1)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)    # noqa: E731
    assert ctx.L.mslam_hip_tsdf_raycast(ctx._h, C.byref(q), vp(R), vp(t), vp(d2), None, vp(n2), C.byref(hits)) == 0
    assert d2.tobytes() == ref[0].tobytes() and n2.tobytes() == ref[2].tobytes() and hits.value == int((ref[0] > 0).sum())
    # the device form into torch buffers
    t_depth = torch.full((30, 40), 7.0, dtype=torch.float32, device="cuda")
    t_xyz = torch.full((30, 40, 3), 7.0, dtype=torch.float32, device="cuda")
    t_nrm = torch.full((30, 40, 3), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    n = ctx.tsdf_raycast(*TILTED, out=(t_depth.data_ptr(), t_xyz.data_ptr(), t_nrm.data_ptr()), with_hits=True)
    assert n == int((ref[0] > 0).sum())
    same((t_depth.cpu().numpy(), t_xyz.cpu().numpy(), t_nrm.cpu().numpy()), ref)
    t_depth.fill_(7.0)
    torch.cuda.synchronize()
    assert ctx.tsdf_raycast(*TILTED, out=(t_depth.data_ptr(), None, None)) is None    # depth only, enqueued
    ctx.sync()
    assert t_depth.cpu().numpy().tobytes() == ref[0].tobytes()
    after = ctx.tsdf_read()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and np.array_equal(after[0], vol[0])


def test_errors_leave_everything_untouched(pkg, ctx, world):
    p, frames, vol = world[0]["sphere"]
    load(ctx, p, frames)
    good = ctx.tsdf_raycast_params(I, Z)
    R, t = np.ascontiguousarray(I), np.ascontiguousarray(Z)
    depth, xyz, nrm = (np.full(s, 7.0, np.float32) for s in ((30, 40), (30, 40, 3), (30, 40, 3)))
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)    # noqa: E731

    def call(q, R=R, t=t, depth=depth, h=None, form="mslam_hip_tsdf_raycast"):
        hits = C.c_int(-5)
        rc = getattr(ctx.L, form)(ctx._h if h is None else h, None if q is None else C.byref(q), vp(R), vp(t), vp(depth), vp(xyz),
                                  vp(nrm), C.byref(hits))
        assert rc == pkg.OK or hits.value == -5    # a refused call leaves *n_hits alone too
        return rc

    def changed(**kw):
        q = pkg.TsdfRaycastParams.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    E = pkg.E_INVALID
    bad = [dict(width=0), dict(height=0), dict(width=-1), dict(width=1 << 16, height=(1 << 14) + 1), dict(fx=0.0), dict(fy=0.0),
           dict(fx=np.nan), dict(fy=np.nan), dict(cx=np.inf), dict(cy=np.nan), dict(z_near=-0.1), dict(z_near=np.nan),
           dict(z_near=np.inf), dict(z_far=np.inf), dict(z_far=np.nan), dict(z_near=0.5, z_far=0.4), dict(step=0.0),
           dict(step=-0.1), dict(step=np.nan), dict(step=np.inf), dict(z_near=0.0, z_far=1.0, step=1.0 / (1 << 20)), dict(coarse=0),
           dict(coarse=-3), dict(min_weight=0)]
    for form in ("mslam_hip_tsdf_raycast", "mslam_hip_tsdf_raycast_dev"):    # (refused before a pointer is looked at)
        for kw in bad:
            assert call(changed(**kw), form=form) == E, (form, kw)
        Rn, ti = R.copy(), t.copy()
        Rn[1, 2], ti[0] = np.nan, np.inf
        assert call(good, R=Rn, form=form) == E and call(good, t=ti, form=form) == E
        assert call(None, form=form) == E and call(good, R=None, form=form) == E and call(good, t=None, form=form) == E
        assert call(good, depth=None, form=form) == E
        assert getattr(ctx.L, form)(None, C.byref(good), vp(R), vp(t), vp(depth), vp(xyz), vp(nrm), None) == E
    assert np.all(depth == 7.0) and np.all(xyz == 7.0) and np.all(nrm == 7.0)
    S, W = ctx.tsdf_read()
    assert np.array_equal(S, vol[0]) and np.array_equal(W, vol[1]) and ctx.tsdf_info()[1] == 3
    # one sample short of the limit is fine, and the call still works after all the refusals
    assert call(changed(z_near=0.0, z_far=0.001, step=0.001 / ((1 << 20) - 0.5))) == pkg.OK
    assert call(good) == pkg.OK and depth.tobytes() == reference(world, "40x30")[0].tobytes()
    with pytest.raises(pkg.MslamHipError) as e:
        ctx.tsdf_raycast(I, Z, camera=dict(width=0, height=4, focal=(1.0, 1.0), principal=(0.0, 0.0)))
    assert e.value.code == E
    # no volume
    ctx.tsdf_destroy()
    depth[:] = 7.0
    assert call(good) == E and call(good, form="mslam_hip_tsdf_raycast_dev") == E and np.all(depth == 7.0)
    with pytest.raises(pkg.MslamHipError) as e:
        ctx.tsdf_raycast(I, Z)
    assert e.value.code == E
