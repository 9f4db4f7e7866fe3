"""Frame-to-model point-to-plane ICP on the GPU (k_icp.hip) against the numpy reference tests/tsdf_icp_ref.py.  Both sides
evaluate the same separately rounded IEEE f64 operations and add in the same tree, so R, t, the result struct, the whole
record and the sums of a linearisation are compared by .tobytes(): no tolerance anywhere.  The cases are the reference's SOLVES
and LINEARIZES (tests/test_tsdf_icp.py checks on the CPU that each of them meets what it is there for): a workgroup owns 256
consecutive pixels of a level, so 40 x 30 (4.7 chunks), 23 x 17, 1 x 1 and 65 x 1 frames and the strides 1, 2, 3, 4 leave partial
chunks and partial waves everywhere; 160 x 120 has 75 chunks, more than the 64 rows of partials the finish kernel stages at a time."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_ref as tr  # noqa: E402
import tsdf_raycast_ref as rr  # noqa: E402
import tsdf_icp_ref as ir  # noqa: E402

pytestmark = pytest.mark.gpu

I, Z = ir.I3, ir.Z3


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(width=0, height=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def world():
    return ir.world(), {}


def reference(world, name):
    w, done = world
    if name not in done:
        done[name] = ir.solve_case(w, name)
    return done[name]


def same_solve(got, ref, what=""):
    assert got["R"].tobytes() == np.ascontiguousarray(ref["R"]).tobytes(), (what, "R", got["R"], ref["R"])
    assert got["t"].tobytes() == np.ascontiguousarray(ref["t"]).tobytes(), (what, "t")
    assert bytes(got["result"]) == ir.result_bytes(ref), (what, "result", got["status"], got["iterations"], got["count"],
                                                          ref["status"], ref["iterations"], ref["count"])
    assert got["record"].tobytes() == ref["record"].tobytes(), (what, "record")


def run_solve(ctx, w, name, **more):
    frame_key, model_key, guess, kw, _, _ = ir.SOLVES[name]
    mcam, Rm, tm, xyz, nrm = w["model"][model_key]
    return ctx.icp_point_plane(w["depth"][frame_key], w["cam"][frame_key], xyz, nrm, mcam, Rm, tm, *guess, **dict(kw, **more))


@pytest.mark.parametrize("name", list(ir.SOLVES))
def test_solves(ctx, world, name):
    ref = reference(world, name)
    want = ir.SOLVES[name][4]
    print("%s: status %d after %d linearisations, %d pairs, sum r^2 %.6g" % (name, ref["status"], ref["iterations"], ref["count"],
                                                                            ref["cost"]))
    assert want is None or ref["status"] == want
    same_solve(run_solve(ctx, world[0], name), ref, name)


@pytest.mark.parametrize("name", list(ir.LINEARIZES))
def test_linearizes(ctx, world, name):
    w = world[0]
    frame_key, model_key, pose, stride = ir.LINEARIZES[name]
    mcam, Rm, tm, xyz, nrm = w["model"][model_key]
    A, g, count, cost = ir.linearize_case(w, name)
    print("%s: %d pairs, sum r^2 %.6g" % (name, count, cost))
    gA, gg, gcount, gcost = ctx.icp_linearize(w["depth"][frame_key], w["cam"][frame_key], xyz, nrm, mcam, Rm, tm, *pose, stride=stride)
    assert gcount == count
    assert gA.tobytes() == A.tobytes() and gg.tobytes() == g.tobytes()
    assert np.float64(gcost).tobytes() == np.float64(cost).tobytes()


def load(ctx, p, frames):
    ctx.tsdf_create(**tr.create_kwargs(p))
    for q, (d, R, t) in enumerate(frames):
        ctx.tsdf_add_frame(q, d, R, t)


def test_call_forms_and_repeats(ctx, world):
    import torch
    w = world[0]
    ref = reference(world, "small_default_levels")
    first = run_solve(ctx, w, "small_default_levels")
    same_solve(first, ref)
    same_solve(run_solve(ctx, w, "small_default_levels"), ref)    # the same call twice in a row
    same_solve(run_solve(ctx, w, "frame_65x1"), reference(world, "frame_65x1"))    # a degenerate solve in between
    same_solve(run_solve(ctx, w, "small_default_levels"), ref)
    # the device form
    mcam, Rm, tm, xyz, nrm = w["model"]["small"]
    t_d = torch.from_numpy(np.ascontiguousarray(w["depth"]["small"]).view(np.int16)).cuda()    # the same 16 bits
    t_xyz, t_nrm = torch.from_numpy(xyz).cuda(), torch.from_numpy(nrm).cuda()
    torch.cuda.synchronize()
    got = ctx.icp_point_plane(t_d.data_ptr(), w["cam"]["small"], t_xyz.data_ptr(), t_nrm.data_ptr(), mcam, Rm, tm, I, Z, **ir.SMALL)
    same_solve(got, ref, "device form")
    # no record through the C ABI
    q = ctx.icp_params(w["cam"]["small"], mcam, **ir.SMALL)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)    # noqa: E731
    d, Rg, tg = np.ascontiguousarray(w["depth"]["small"]), np.ascontiguousarray(I), np.ascontiguousarray(Z)
    R, t, res = np.zeros((3, 3)), np.zeros(3), type(first["result"])()
    assert ctx.L.mslam_hip_icp_point_plane(ctx._h, C.byref(q), vp(d), vp(xyz), vp(nrm), vp(Rg), vp(tg), vp(Rg), vp(tg), vp(R), vp(t),
                                           C.byref(res), None, 0) == 0
    assert R.tobytes() == ref["R"].tobytes() and t.tobytes() == ref["t"].tobytes() and bytes(res) == ir.result_bytes(ref)


def tsdf_reference(w, vol, p, depth, guess, raycast=None, **kw):
    _, xyz, nrm = rr.raycast(*vol, p, *guess, **(raycast or {}))
    mcam = rr.camera_of(p) if not raycast or "camera" not in raycast else raycast["camera"]
    return ir.solve(depth, ir.frame_camera(p), (xyz, nrm), mcam, *guess, *guess, **kw)


def test_tsdf_icp(ctx, world):
    import torch
    w = world[0]
    p, frames, vol, depth = w["p"]["small"], w["frames"]["small"], w["vol"]["small"], w["depth"]["small"]
    load(ctx, p, frames)
    before = ctx.tsdf_read()
    for guess, raycast in ((ir.OFF, None), ((I, Z), dict(camera=ir.ODD, coarse=1))):
        ref = tsdf_reference(w, vol, p, depth, guess, raycast, **ir.SMALL)
        assert ref["status"] == ir.ITERATIONS
        got = ctx.tsdf_icp(depth, *guess, raycast=raycast, **ir.SMALL)
        same_solve(got, ref, "tsdf_icp")
        # equal to tsdf_raycast followed by icp_point_plane
        _, xyz, nrm = ctx.tsdf_raycast(*guess, **(raycast or {}))
        mcam = ir.ODD if raycast else rr.camera_of(p)
        same_solve(ctx.icp_point_plane(depth, ir.frame_camera(p), xyz, nrm, mcam, *guess, **ir.SMALL), ref, "two calls")
    t_d = torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).cuda()
    torch.cuda.synchronize()
    same_solve(ctx.tsdf_icp(t_d.data_ptr(), I, Z, raycast=dict(camera=ir.ODD, coarse=1), **ir.SMALL), ref, "tsdf_icp_dev")
    after = ctx.tsdf_read()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    # after tsdf_update_poses and tsdf_remove_frame the model is the retained frames'
    R1, t1 = tr.rot(1, 0.23) @ frames[1][1], frames[1][2] + np.array([0.01, -0.02, 0.015])
    assert ctx.tsdf_update_poses([1], R1[None], t1[None]) == 1
    ctx.tsdf_remove_frame(2)
    vol2 = tr.fresh(p, [frames[0], (frames[1][0], R1, t1)])
    ref2 = tsdf_reference(w, vol2, p, depth, (I, Z), **ir.SMALL)
    assert ref2["R"].tobytes() != tsdf_reference(w, vol, p, depth, (I, Z), **ir.SMALL)["R"].tobytes()
    same_solve(ctx.tsdf_icp(depth, I, Z, **ir.SMALL), ref2, "after volume changes")
    ctx.tsdf_destroy()


def test_errors_leave_everything_untouched(pkg, ctx, world):
    w = world[0]
    p, frames = w["p"]["small"], w["frames"]["small"]
    load(ctx, p, frames)
    mcam, Rm, tm, xyz, nrm = w["model"]["small"]
    cam, depth = w["cam"]["small"], np.ascontiguousarray(w["depth"]["small"])
    good = ctx.icp_params(cam, mcam, **ir.SMALL)
    ray = ctx.tsdf_raycast_params(I, Z)
    Rg, tg = np.ascontiguousarray(I), np.ascontiguousarray(Z)
    R, t, rec = np.full((3, 3), 7.0), np.full(3, 7.0), np.full(19, 7, np.uint8).repeat(32)
    A, g = np.full(21, 7.0), np.full(6, 7.0)
    res = pkg.IcpResult()
    res.status, res.cost = -5, 7.0
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)    # noqa: E731
    ref_q = lambda q: None if q is None else C.byref(q)    # noqa: E731

    def solve(q, form="mslam_hip_icp_point_plane", depth=depth, xyz=xyz, nrm=nrm, Rm=Rg, tm=tg, R0=Rg, t0=tg, R=R, t=t, result=res,
              record=rec, capacity=19, h=None, ray=ray):
        h = ctx._h if h is None else h
        out = None if result is None else C.byref(result)
        if form.startswith("mslam_hip_tsdf"):
            return getattr(ctx.L, form)(h, ref_q(q), ref_q(ray), vp(depth), vp(R0), vp(t0), vp(R), vp(t), out, vp(record), capacity)
        return getattr(ctx.L, form)(h, ref_q(q), vp(depth), vp(xyz), vp(nrm), vp(Rm), vp(tm), vp(R0), vp(t0), vp(R), vp(t), out,
                                    vp(record), capacity)

    def linearize(q, stride=1, depth=depth, R=Rg, A=A):
        n, cost = C.c_int(-5), C.c_double(7.0)
        rc = ctx.L.mslam_hip_icp_linearize(ctx._h, ref_q(q), vp(depth), vp(xyz), vp(nrm), vp(Rg), vp(tg), vp(R), vp(tg), stride, vp(A),
                                           vp(g), C.byref(n), C.byref(cost))
        assert rc == pkg.OK or (n.value == -5 and cost.value == 7.0)
        return rc

    def changed(**kw):
        q = pkg.IcpParams.from_buffer_copy(good)
        for k, v in kw.items():
            if isinstance(v, tuple):
                for i, x in enumerate(v):
                    getattr(q, k)[i] = x
            else:
                setattr(q, k, v)
        return q

    E = pkg.E_INVALID
    frame_side = [dict(width=0), dict(height=0), dict(width=-1), dict(width=1 << 13, height=(1 << 11) + 1), dict(fx=0.0), dict(fy=0.0),
                  dict(fx=np.nan), dict(fy=np.inf), dict(cx=np.inf), dict(cy=np.nan), dict(factor=np.nan), dict(factor=np.inf),
                  dict(max_depth=0.0), dict(max_depth=-1.0), dict(max_depth=np.nan)]
    model_side = [dict(model_width=0), dict(model_height=-2), dict(model_width=1 << 16, model_height=(1 << 14) + 1), dict(mfx=0.0),
                  dict(mfy=0.0), dict(mfx=np.nan), dict(mfy=-np.inf), dict(mcx=np.nan), dict(mcy=np.inf)]
    rest = [dict(n_levels=0), dict(n_levels=5), dict(n_levels=-1), dict(stride=(4, 0, 1, 0)), dict(stride=(-1, 2, 1, 0)),
            dict(iterations=(4, 5, 0, 0)), dict(iterations=(4, -5, 10, 0)), dict(iterations=(100, 100, 57, 0)),
            dict(n_levels=4, stride=(1, 1, 1, 1), iterations=(64, 64, 64, 65)), dict(dist_max=0.0), dict(dist_max=-0.1),
            dict(dist_max=np.nan), dict(dist_max=np.inf), dict(cos_min=1.0000001), dict(cos_min=-1.0000001), dict(cos_min=np.nan),
            dict(min_pairs=5), dict(min_pairs=-1), dict(rot_tol=-1e-9), dict(trans_tol=-1e-9), dict(rot_tol=np.nan),
            dict(trans_tol=np.inf)]
    bad_pose, bad_t = Rg.copy(), tg.copy()
    bad_pose[2, 1], bad_t[1] = np.nan, -np.inf
    for form in ("mslam_hip_icp_point_plane", "mslam_hip_icp_point_plane_dev", "mslam_hip_tsdf_icp", "mslam_hip_tsdf_icp_dev"):
        tsdf = form.startswith("mslam_hip_tsdf")
        # (refused before a pointer is looked at: the _dev forms may be given host pointers here)
        for kw in frame_side + rest + ([] if tsdf else model_side):
            assert solve(changed(**kw), form) == E, (form, kw)
        assert solve(good, form, capacity=18) == E, form
        assert solve(good, form, R0=bad_pose) == E and solve(good, form, t0=bad_t) == E, form
        for name in ("depth", "R0", "t0", "R", "t", "result"):
            assert solve(good, form, **{name: None}) == E, (form, name)
        assert solve(None, form) == E and solve(good, form, h=C.c_void_p(None)) == E, form
        if tsdf:
            assert solve(good, form, ray=None) == E
            for kw in (dict(width=0), dict(fx=0.0), dict(cy=np.nan), dict(step=0.0), dict(coarse=0), dict(min_weight=0),
                       dict(z_near=-1.0)):
                q = pkg.TsdfRaycastParams.from_buffer_copy(ray)
                for k, v in kw.items():
                    setattr(q, k, v)
                assert solve(good, form, ray=q) == E, (form, kw)
            # a frame camera that is not the volume's
            for kw in (dict(width=39), dict(fx=40.5), dict(cy=14.0), dict(factor=1.0 / 1000.0), dict(max_depth=2.5)):
                assert solve(changed(**kw), form) == E, (form, kw)
        else:
            assert solve(good, form, Rm=bad_pose) == E and solve(good, form, tm=bad_t) == E, form
            for name in ("xyz", "nrm", "Rm", "tm"):
                assert solve(good, form, **{name: None}) == E, (form, name)
    for kw in frame_side + model_side + rest:
        assert linearize(changed(**kw)) == E, kw
    assert linearize(good, stride=0) == E and linearize(good, stride=-4) == E and linearize(None) == E
    assert linearize(good, depth=None) == E and linearize(good, R=bad_pose) == E and linearize(good, A=None) == E
    assert np.all(R == 7.0) and np.all(t == 7.0) and np.all(rec == 7) and np.all(A == 7.0) and np.all(g == 7.0)
    assert res.status == -5 and res.cost == 7.0
    S, W = ctx.tsdf_read()
    assert np.array_equal(S, w["vol"]["small"][0]) and np.array_equal(W, w["vol"]["small"][1]) and ctx.tsdf_info()[1] == 3
    # a capacity that just fits, 256 iterations in all, and the calls still work after all the refusals
    rec19 = np.zeros(19, ir.RECORD)
    assert solve(good, record=rec19, capacity=19) == pkg.OK
    ref = reference(world, "small_default_levels")
    assert R.tobytes() == ref["R"].tobytes() and rec19.tobytes() == ref["record"].tobytes() and bytes(res) == ir.result_bytes(ref)
    assert solve(changed(n_levels=4, stride=(4, 4, 4, 4), iterations=(64, 64, 64, 64)), record=None, capacity=0) == pkg.OK
    most = ir.solve(depth, cam, (xyz, nrm), mcam, I, Z, I, Z, levels=((4, 64),) * 4, **ir.SMALL)
    assert most["iterations"] == 256 and bytes(res) == ir.result_bytes(most) and R.tobytes() == most["R"].tobytes()
    assert linearize(good) == pkg.OK and A.tobytes() == ir.linearize_case(w, "stride_1")[0].tobytes()
    with pytest.raises(pkg.MslamHipError) as e:
        ctx.icp_point_plane(depth, cam, xyz, nrm, mcam, Rm, tm, levels=())
    assert e.value.code == E
    with pytest.raises(pkg.MslamHipError) as e:
        ctx.icp_point_plane(depth, cam, xyz, nrm, mcam, Rm, tm, levels=((1, 1),) * 5)
    assert e.value.code == E
    # no volume
    ctx.tsdf_destroy()
    R[:] = 7.0
    assert solve(good, "mslam_hip_tsdf_icp") == E and solve(good, "mslam_hip_tsdf_icp_dev") == E and np.all(R == 7.0)
    with pytest.raises(pkg.MslamHipError) as e:
        ctx.tsdf_icp(depth, I, Z)
    assert e.value.code == E
