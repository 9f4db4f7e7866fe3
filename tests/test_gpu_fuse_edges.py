"""Landmark fusion on the MI355X away from the default frame: k_fuse_search's cell walk at four frame extents and four radii
(one larger than the frame: brute force), and the projection under a real pose, depths of 0.5 .. 4 m and the TUM camera with
a 3-D gate that bites — pairs, ids and counts exactly, stores read back and compared as bytes, against tests/fuse_ref.py,
which evaluates the projection in the kernel's order of operations.  tests/test_lm_table_edges.py proves on the CPU that
every case has pairs and that the gate decides some of them.  (The sizes at which the resolution takes a second and third
pass are part of fuse_ref.SIZES and run in tests/test_gpu_fuse.py.)"""
import numpy as np
import pytest

import fuse_ref as fr
from test_gpu_fuse import _args, _fill, _same_pairs, _same_store

pytestmark = pytest.mark.gpu

K = 1280


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(width=0, height=0, max_keypoints=K)
    yield c
    c.close()


@pytest.mark.parametrize("width,height", fr.FRAMES)
def test_frames_and_radii(ctx, width, height):
    for nk, nd in fr.FRAME_SIZES:
        case = fr.frame_case(nk, nd, width, height)
        store = {1: case["keep"], 2: case["drop"]}
        _fill(ctx, store)
        total = 0
        for radius in fr.frame_radii(width, height):
            ref = fr.search(case["keep"], case["drop"], radius=radius, **case["kw"])
            got = ctx.kf_fuse_search(1, 2, **dict(_args(case), radius=radius))
            print("%d x %d, %d / %d, radius %g: %d pairs" % (width, height, nk, nd, radius, len(ref["keep_pos"])))
            _same_pairs(got, ref, (nk, nd, radius))
            total += len(ref["keep_pos"])
        assert total > 0
        _same_store(ctx, store, "search changes nothing")
        pairs, new, n = fr.fuse(store, 1, 2, radius=radius, **case["kw"])          # the brute-force radius, then the replacement
        fused = ctx.kf_fuse(1, 2, **dict(_args(case), radius=radius))
        _same_pairs(fused, pairs, "fuse")
        assert fused["n_rewritten"] == n
        _same_store(ctx, new, "fuse")


@pytest.mark.parametrize("nk,nd", fr.POSED_SIZES)
def test_real_pose_and_camera(ctx, nk, nd):
    case = fr.posed_case(40 + nk, nk, nd, shared=5)
    rng = np.random.default_rng(nk)
    dl = case["drop"][2]

    def other(ids):
        return (rng.integers(0, 256, (len(ids), 32), dtype=np.uint8), rng.normal(size=(len(ids), 3)), ids)

    store = {1: case["keep"], 2: case["drop"], 3: other(np.concatenate([dl[::3], dl[:40], 9000000 + np.arange(30)])), 4: other(dl[1::2])}
    _fill(ctx, store)
    ref = fr.search(case["keep"], case["drop"], radius=case["radius"], **case["kw"])
    _same_pairs(ctx.kf_fuse_search(1, 2, **_args(case)), ref, "search")
    open_ = dict(case["kw"], max_world_distance=np.inf)                             # the same scene with the gate off
    _same_pairs(ctx.kf_fuse_search(1, 2, **dict(_args(case), max_world_distance=np.inf)),
                fr.search(case["keep"], case["drop"], radius=case["radius"], **open_), "no gate")
    _same_store(ctx, store, "search changes nothing")
    pairs, new, n = fr.fuse(store, 1, 2, radius=case["radius"], **case["kw"])
    got = ctx.kf_fuse(1, 2, **_args(case))
    _same_pairs(got, ref, "fuse")
    assert got["n_rewritten"] == n > len(ref["keep_pos"]) >= 30
    _same_store(ctx, new, "fuse")                                                   # entries 3 and 4: ids and world points
    assert any(new[k][1].tobytes() != fr.entry(*store[k])[1].tobytes() for k in (3, 4))
