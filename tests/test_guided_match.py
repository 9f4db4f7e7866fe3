"""Guided matching without a GPU: tests/guided_match_ref.py against hand-computed cases and against the oracle's brute-force
knn-2, the proof that every planted scene tests/test_gpu_guided_match.py runs is what it claims to be, and the four new
entry points in the header and in the built library."""
import os
import re

import numpy as np
import pytest

import guided_match_ref as gr
import reloc_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["mslam_hip_match_guided_knn2", "mslam_hip_match_guided", "mslam_hip_set_guided_match", "mslam_hip_get_guided_match"]
RADII = [0.5, 15.0, 47.5]


def _knn2(sc, radius):
    return gr.knn2(sc["kp_desc"], sc["kp_xy"], sc["lm_desc"], sc["lm_world"], sc["R"], sc["t"], radius, sc["cam"], sc["width"],
                   sc["height"])


def _match(sc, radius, max_distance=256, ratio=0.7):
    return gr.match(sc["kp_desc"], sc["kp_xy"], sc["lm_desc"], sc["lm_world"], sc["R"], sc["t"], radius, max_distance, ratio,
                    sc["cam"], sc["width"], sc["height"])


def test_the_header_declares_and_the_library_exports_the_new_entry_points(pkg):
    hdr = open(os.path.join(ROOT, "include", "mslam_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mslam_hip_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in pkg.ABI_SYMBOLS, name
        assert hasattr(pkg.lib(), name), name
    assert pkg.lib().mslam_hip_abi_version() == 5      # additions only


def test_reference_on_a_hand_computed_case():
    """three landmarks, four keypoints, IDENTITY_CAM (u = X, v = Y), radius 2, worked out by hand"""
    ld = np.zeros((3, 32), np.uint8)
    kd = np.zeros((4, 32), np.uint8)
    kd[0, 0], kd[1, 0], kd[2, 0], kd[3, 0] = 0b1, 0b11, 0b1, 0b111          # distances 1, 2, 1, 3 from every landmark
    xy = np.array([(10, 10), (11, 11), (12, 10), (30, 30)], np.float32)
    world = np.array([(10, 10, 1), (31, 31, 1), (50, 50, 1)], np.float64)
    i0, i1, d0, d1, nc = gr.knn2(kd, xy, ld, world, np.eye(3), np.zeros(3), 2.0, gr.IDENTITY_CAM, 64, 64)
    # landmark 0: keypoints 0, 1, 2 within 2 px; distances 1, 2, 1 -> 0 then 2 (tie to the lower index).  1: keypoint 3
    # alone.  2: nothing.
    assert nc.tolist() == [3, 1, 0]
    assert i0.tolist() == [0, 3, -1] and i1.tolist() == [2, -1, -1]
    assert d0.tolist() == [1, 3, gr.ABSENT] and d1.tolist() == [1, gr.ABSENT, gr.ABSENT]
    fi, ti = gr.match(kd, xy, ld, world, np.eye(3), np.zeros(3), 2.0, 256, 0.7, gr.IDENTITY_CAM, 64, 64)
    assert (fi.tolist(), ti.tolist()) == ([3], [1])                          # 0: d0 == d1 fails; 1: a lone candidate passes
    fi, ti = gr.match(kd, xy, ld, world, np.eye(3), np.zeros(3), 2.0, 2, 0.7, gr.IDENTITY_CAM, 64, 64)
    assert len(fi) == 0                                                      # ... unless its distance exceeds the gate
    # a frame of 11 x 64: keypoints 1, 2 (x >= 11) and 3 leave it
    assert gr.knn2(kd, xy, ld, world, np.eye(3), np.zeros(3), 2.0, gr.IDENTITY_CAM, 11, 64)[4].tolist() == [1, 0, 0]
    # the projection: t = (-20, -20, 0) at Z = 1 moves landmark 0 out of the frame, landmark 1 to (11, 11) — keypoints 0, 1, 2
    # within 2 px, distances 1, 2, 1 — and landmark 2 onto keypoint 3
    assert gr.knn2(kd, xy, ld, world, np.eye(3), np.array([-20.0, -20.0, 0.0]), 2.0, gr.IDENTITY_CAM, 64, 64)[0].tolist() == [-1, 0, 3]


@pytest.mark.parametrize("n_kp,n_lm,size", [(2, 9, (20, 20)), (65, 64, (100, 80)), (700, 65, (640, 480)), (64, 7, (4114, 102))])
def test_whole_frame_radius_is_brute_force_on_the_in_frame_keypoints(orc, n_kp, n_lm, size):
    sc = gr.random_scene(n_kp * 1000 + n_lm, n_kp, n_lm, *size)
    sc["kp_xy"][0] = (-1.0, 3.0)                       # one keypoint out of the frame
    sc["lm_world"][0, 2] = -1.0                        # one landmark behind the camera
    got = _knn2(sc, float(max(size)) + 10.0)
    inside = np.flatnonzero(gr.in_frame(sc["kp_xy"], *size))
    assert 0 not in inside and len(inside) >= 1
    front = gr.project(sc["lm_world"], sc["R"], sc["t"], sc["cam"])[2] > 0
    assert not front[0] and got[4][0] == 0 and got[0][0] == -1
    if len(inside) < 2:
        return
    b0, b1, e0, e1 = orc.match_knn2_raw(sc["kp_desc"][inside], sc["lm_desc"])
    # the landmarks project at most 10 px beyond the frame: with radius = the larger extent + 10 every in-frame keypoint
    # is a candidate of every landmark in front of the camera
    assert (got[4][front] == len(inside)).all()
    assert np.array_equal(got[0][front], inside[b0][front]) and np.array_equal(got[1][front], inside[b1][front])
    assert np.array_equal(got[2][front], e0[front]) and np.array_equal(got[3][front], e1[front])


@pytest.mark.parametrize("radius", RADII)
def test_edge_scene_is_what_it_claims(radius):
    sc = gr.edge_scene(radius)
    xy, world = sc["kp_xy"].astype(np.float64), sc["lm_world"]
    u, v, c2 = gr.project(world, sc["R"], sc["t"], sc["cam"])
    assert np.array_equal(u[:8], world[:8, 0]) and np.array_equal(v[:8], world[:8, 1])      # u = X exactly
    assert c2[8] == 0 and c2[9] < 0 and np.isinf(u[10]) and np.isnan(u[11]) and u[15] > 9e299 and v[15] < -9e299 and np.isfinite(u[15]) and c2[15] > 0
    n_cand = _knn2(sc, radius)[4]
    for j, want in sc["expect"].items():
        got = np.flatnonzero(gr.candidates(sc["kp_xy"], u[j], v[j], c2[j], 640, 480, radius)).tolist()
        assert got == want and n_cand[j] == len(want), (j, got, want)
    # landmark 0: which side of <= each planted point is on (keypoints 0 .. 9 are its own)
    dx, dy = np.abs(xy[:10, 0] - 100.0), np.abs(xy[:10, 1] - 100.0)
    assert dx[0] == radius and dx[1] == radius and dy[2] == radius and dy[3] == radius and dx[4] == radius and dy[4] == radius
    assert dx[6] > radius and dx[7] > radius and dy[8] > radius and dy[9] > radius
    assert np.nextafter(np.float32(100 + radius), np.float32(np.inf)) == sc["kp_xy"][6, 0]
    assert sc["expect"][0] == [0, 1, 2, 3, 4, 5]
    # cells (32 px): landmark 1's window lies in one cell, 2's in two, 3's in four — for the radius below half a cell
    if radius < 16:
        cells = lambda j: {(int(x) >> 5, int(y) >> 5) for x, y in sc["kp_xy"][sc["expect"][j]]}
        lo, hi = world[1:4, :2] - radius, world[1:4, :2] + radius
        span = ((np.floor(hi) // 32 - np.floor(lo) // 32 + 1).prod(1)).astype(int).tolist()
        assert span == [1, 2, 4], span
        assert len(cells(1)) == 1 and len(cells(2)) == 2 and len(cells(3)) == 4
    # the borders: the window reaches past the frame on the side named
    assert world[4, 0] - radius < 0 and world[5, 0] + radius >= 640 and world[6, 1] - radius < 0 and world[7, 1] + radius >= 480
    assert all(len(sc["expect"][j]) == 1 for j in (4, 5, 6, 7))
    # the keypoints that are not numbers or not in the frame, next to landmarks 12, 13, 14
    bad = ~gr.in_frame(sc["kp_xy"], 640, 480)
    assert bad.sum() == 6 and np.isnan(sc["kp_xy"][bad]).any() and np.isinf(sc["kp_xy"][bad]).any()
    assert (sc["kp_xy"][bad][:, 0] == 640.0).sum() == 1 and (sc["kp_xy"][bad][:, 0] == -0.25).sum() == 1
    zero = sc["kp_xy"][:, 0] == 0.0
    assert np.signbit(sc["kp_xy"][zero, 0]).any() and gr.in_frame(sc["kp_xy"], 640, 480)[zero].all()   # x = -0.0 is in
    assert len(sc["expect"][12]) == 1 and len(sc["expect"][13]) == (radius >= 2) and len(sc["expect"][14]) == (radius >= 1)


def test_tie_scene_is_what_it_claims():
    sc = gr.tie_scene()
    i0, i1, d0, d1, nc = _knn2(sc, sc["radius"])
    first = np.cumsum([0] + [len(v) for v in sc["plan"].values()])[:-1]
    assert nc.tolist() == [len(v) for v in sc["plan"].values()]
    for j, dists in sc["plan"].items():               # the planted distances are the Hamming distances
        assert gr.hamming(sc["kp_desc"][first[j]:first[j] + len(dists)], sc["lm_desc"][j]).tolist() == dists
    A = int(gr.ABSENT)
    assert d0.tolist() == [3, 0, 200, 255, 256, 0, 9] and d1.tolist() == [3, 256, A, 256, A, A, 10]
    assert (i0 - first).tolist() == [0, 0, 0, 0, 0, 0, 2] and i1[0] == first[0] + 1 and i1[6] == first[6]   # ties: the lower index
    assert np.array_equal(sc["kp_desc"][first[0]], sc["kp_desc"][first[0] + 1])
    for md, want in ((0, [1, 5]), (255, [1, 2, 5]), (256, [1, 2, 4, 5])):
        fi, ti = _match(sc, sc["radius"], md)
        assert ti.tolist() == want and fi.tolist() == i0[want].tolist(), (md, ti)
    # the ratio: landmark 6 (9 against 10) passes from 0.9 on (9 < 0.91 * 10), landmark 0 (3 against 3) from ratio > 1
    assert 6 not in _match(sc, sc["radius"], 256, 0.9)[1] and 6 in _match(sc, sc["radius"], 256, 0.91)[1]
    assert 0 not in _match(sc, sc["radius"], 256, 1.0)[1] and 0 in _match(sc, sc["radius"], 256, 1.01)[1]


def test_crowded_scene_is_what_it_claims():
    sc = gr.crowded_scene()
    cells = {(int(x) >> 5, int(y) >> 5) for x, y in sc["kp_xy"]}
    assert cells == {(10, 7)} and len(sc["kp_xy"]) == 3000
    assert _knn2(sc, sc["radius"])[4].tolist() == [0, 3000, 0]


def test_mode_frames_keep_clear_of_the_window_edges(orc):
    """the mode's inputs go through the library's own rvec -> R: no (landmark, keypoint) pair may lie within 1e-6 px of a
    window edge, so that a last-bit difference in R cannot flip a membership (a point 6 m away moves by far less)"""
    m = gr.mode_frames()
    for radius in (15.0, 47.5):
        for fr in m["frames"]:
            for cid, (_, world) in m["store"].items():
                margin = gr.min_edge_margin(fr["xy"], world, m["guess"][0], m["guess"][1], radius)
                assert margin > 1e-6, (radius, cid, margin)
    # and the frames are what they claim: 17 of them, different sizes, frame 12 far away
    assert len(m["frames"]) == 17 and len({len(f["desc"]) for f in m["frames"]}) > 10
    assert rr.rot_err(m["guess"][0], m["truth"][0]) == pytest.approx(0.3, abs=1e-6)
    assert np.linalg.norm(m["guess"][1] - m["truth"][1]) == pytest.approx(0.005, abs=1e-9)


def test_twins_scene_is_what_it_claims(orc):
    tw = gr.twins_scene()
    ld, world = tw["store"][0]
    n, radius = len(ld), tw["radius"]
    assert np.array_equal(ld, ld[tw["twin"]]) and (tw["twin"] != np.arange(n)).all()
    # every landmark's own keypoint and its twin's are 6 bits away from it; no other keypoint comes within 64 bits
    for j in range(n):
        d = gr.hamming(tw["desc"], ld[j])
        assert d[tw["own"][j]] == 6 and d[tw["own"][tw["twin"][j]]] == 6
        d[[tw["own"][j], tw["own"][tw["twin"][j]]]] = 999
        assert d.min() > 64, (j, d.min())
    # brute force: d0 == d1 for every landmark -> the oracle matches nothing
    b0, b1, d0, d1 = orc.match_knn2_raw(tw["desc"], ld)
    assert (d0 == 6).all() and (d1 == 6).all()
    assert len(rr.match(tw["desc"], ld, 0.7)[0]) == 0
    # twins lie more than 2 radii apart in the image; under the perturbed guess every landmark's own keypoint stays inside
    # its window and its twin's keypoint outside, clear of the edge by more than 1e-6 px
    guess = gr.perturbed(tw["R"], tw["t"], 0.5, 0.01)
    u, v, c2 = gr.project(world, guess[0], guess[1])
    assert (c2 > 0).all()
    xy = tw["xy"].astype(np.float64)
    for j in range(n):
        cand = gr.candidates(tw["xy"], u[j], v[j], c2[j], 640, 480, radius)
        assert cand[tw["own"][j]] and not cand[tw["own"][tw["twin"][j]]], j
    own, other = xy[tw["own"]], xy[tw["own"][tw["twin"]]]
    assert (np.abs(own - other).max(1) > 2 * radius).all()
    assert gr.min_edge_margin(tw["xy"], world, guess[0], guess[1], radius) > 1e-6
    # so the guided matcher finds every landmark's own keypoint
    fi, ti = gr.match(tw["desc"], tw["xy"], ld, world, guess[0], guess[1], radius)
    assert np.array_equal(ti, np.arange(n)) and np.array_equal(fi, tw["own"])
