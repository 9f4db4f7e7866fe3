"""tests/points_ref.py on the CPU: the numpy reference equals the oracle's back-projection bit for bit, and the shared
inputs plant what tests/test_gpu_points_edges.py relies on (so that the GPU tests cannot pass vacuously)."""
import numpy as np
import pytest

import points_ref as pr


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("w,h", pr.SIZES)
def test_reference_equals_oracle(orc, w, h):
    depth = pr.make_depth(w, h, seed=w + h)
    xy = pr.make_coordinates(w, h, 5000, seed=3 * w + h)
    none = pr.has_no_depth(xy, w, h)
    for factor in pr.FACTORS:
        ref_xyz, ref_ok = pr.backproject(depth, xy, factor, pr.FOCAL, pr.PRINCIPAL)
        orc_xyz, orc_ok = orc.backproject(depth, xy, factor, pr.FOCAL, pr.PRINCIPAL)
        assert np.array_equal(ref_ok, orc_ok), (w, h, factor, np.nonzero(ref_ok != orc_ok)[0][:8])
        assert _same_bits(ref_xyz, orc_xyz), (w, h, factor)
        assert not ref_ok[none].any() and not ref_xyz[none].view(np.uint64).any()
        assert not ref_xyz[~ref_ok].view(np.uint64).any()                # an invalid point is +0.0 three times
        assert np.isfinite(ref_xyz).all()
        if (w, h) != (1, 1):
            assert 0.05 < ref_ok.mean() < 0.95, (w, h, factor, ref_ok.mean())


def test_edge_list_plants_what_it_claims():
    """every row of the edge list: which side of the contract it is on, from the contract's wording alone"""
    w, h = 37, 23
    e = pr.edge_coordinates(w, h)
    none = pr.has_no_depth(e, w, h)
    inside = [tuple(map(float, r)) for r in e[~none]]
    assert inside == [(-0.5, float(np.float32(-0.99))), (float(np.float32(w - 0.01)), float(np.float32(h - 0.01)))]
    assert np.isnan(e[:3]).any(1).all() and none[:3].all()
    assert int(np.isinf(e).any(1).sum()) == 4
    # the two inside rows sit in the corner pixels
    depth = np.zeros((h, w), np.uint16)
    depth[0, 0], depth[h - 1, w - 1] = 5000, 10000
    xyz, ok = pr.backproject(depth, e)
    assert np.array_equal(ok, ~none) and list(xyz[ok, 2]) == [1.0, 2.0]
    # make_depth: row 0 and column 0 have depth everywhere, about 30 % of the rest has none
    for (w, h) in pr.SIZES:
        d = pr.make_depth(w, h, seed=1)
        assert d[0].all() and d[:, 0].all()
        if w * h > 1:
            assert 0.2 < (d[1:, 1:] == 0).mean() < 0.4


def test_truncation_and_threshold_rules_are_observable():
    """-0.5 is pixel 0 (truncation, not floor); depth * factor == FLT_EPSILON is invalid (>, not >=); the product is a
    float product (f64 would put 3 * (1/3) elsewhere)"""
    depth = np.array([[7, 0], [0, 9]], np.uint16)
    xyz, ok = pr.backproject(depth, [(-0.5, -0.5), (-1.0, 0.0), (1.99, 1.99), (2.0, 1.0)], factor=1.0)
    assert list(ok) == [True, False, True, False] and list(xyz[:, 2]) == [7.0, 0.0, 9.0, 0.0]
    row = np.array([[0, 1, 2, 65535]], np.uint16)
    xy = [(0.5, 0), (1.5, 0), (2.5, 0), (3.5, 0)]
    for factor, want in zip(pr.FACTOR_EDGES, pr.FACTOR_EDGES_VALID):
        xyz, ok = pr.backproject(row, xy, factor, pr.FOCAL, pr.PRINCIPAL)
        assert list(ok) == want, factor
    xyz, ok = pr.backproject(row, xy, float("inf"), pr.FOCAL, pr.PRINCIPAL)
    assert np.isinf(xyz[1:]).all() and not xyz[0].any()
    xyz, ok = pr.backproject(np.array([[3]], np.uint16), [(0, 0)], factor=1.0 / 3.0)
    assert xyz[0, 2] == 1.0 and 3.0 * float(np.float32(1.0 / 3.0)) != 1.0


def test_factor_edges_equal_oracle(orc):
    row = np.array([[0, 1, 2, 65535]], np.uint16)
    xy = np.array([(0.5, 0), (1.5, 0), (2.5, 0), (3.5, 0)], np.float32)
    for factor in pr.FACTOR_EDGES:
        ref_xyz, ref_ok = pr.backproject(row, xy, factor, pr.FOCAL, pr.PRINCIPAL)
        orc_xyz, orc_ok = orc.backproject(row, xy, factor, pr.FOCAL, pr.PRINCIPAL)
        assert np.array_equal(ref_ok, orc_ok) and _same_bits(ref_xyz, orc_xyz), factor

