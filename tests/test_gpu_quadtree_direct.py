"""GPU parity of the quadtree selection in its direct form (k_quadtree_direct) and in the list-pass form it leaves the
other (level, frame) pairs to, stage by stage as test_gpu_parity.py: on every level DBG_CANDIDATES must be the oracle's
FAST candidates and DBG_SELECTED the oracle's quadtree() of them, with the direct form on and with
MSLAM_HIP_QUAD_DIRECT=0; which form a level takes is asserted through debug_quad_direct_levels().  The frames
(tests/quadtree_direct_frames.py) are the smallest at which the form can go wrong; tests/test_quadtree_direct_ref.py
proves on the CPU that they reach their regimes."""
import numpy as np
import pytest

import quadtree_direct_frames as F

pytestmark = pytest.mark.gpu

FORMS = ["direct", "passes"]


def _ctx(pkg, W, H, p, **kw):
    return pkg.Context(width=W, height=H, n_levels=p["n_levels"], scale_factor=p["scale_factor"], ini_fast_thr=p["ini_fast_thr"],
                       min_fast_thr=p["min_fast_thr"], min_node_area=p["min_node_area"], **kw)


def _set_form(monkeypatch, form):
    if form == "passes":
        monkeypatch.setenv("MSLAM_HIP_QUAD_DIRECT", "0")
    else:
        monkeypatch.delenv("MSLAM_HIP_QUAD_DIRECT", raising=False)


def _assert_levels(pkg, orc, c, slot, frame, p, ref, what):
    """ref: F.level_lists of the frame.  Returns the candidate count per level."""
    n = []
    for l, (w, h, s, cand) in enumerate(ref):
        got = c.debug_keypoints(pkg.DBG_CANDIDATES, slot, l)
        assert np.array_equal(got, cand), (what, "FAST candidates level %d" % l, len(got), len(cand))
        want = F.oracle_select(orc, got, w, h, s, p["min_node_area"])
        sel = c.debug_keypoints(pkg.DBG_SELECTED, slot, l)
        assert len(sel) == len(want) and np.array_equal(sel, want), (what, "selection level %d" % l, len(sel), len(want))
        n.append(len(got))
    return n


@pytest.fixture(scope="module")
def single_refs(orc):
    cases = dict(F.single_cases())
    cases.update(F.fallback_cases())
    return {name: (frame, p, F.level_lists(orc, frame, p)) for name, (frame, p) in cases.items()}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(F.single_cases()) + list(F.fallback_cases()))
def test_single_frame(pkg, orc, single_refs, monkeypatch, name, form):
    frame, p, ref = single_refs[name]
    _set_form(monkeypatch, form)
    H, W = frame.shape[:2]
    c = _ctx(pkg, W, H, p)
    eligible = F.eligible_levels(W, H, p)
    assert eligible == [name in F.single_cases()] * p["n_levels"]      # every level, or (the fallback cases) none
    assert c.debug_quad_direct_levels() == (eligible if form == "direct" else [False] * p["n_levels"]), (name, form)
    c.detect(frame)
    n = _assert_levels(pkg, orc, c, 0, frame, p, ref, (name, form))
    assert max(n) <= pkg.QUAD_DIRECT_MAX_CANDIDATES == F.DIRECT_MAX_CANDIDATES        # (the eligible levels ran direct)
    c.close()


@pytest.fixture(scope="module")
def batch_refs(orc):
    frames = F.batch_frames()
    return frames, {key: [F.level_lists(orc, f, p) for f in frames]
                    for key, p in (("all", F.BATCH_P), ("mixed", F.BATCH_MIXED_P))}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("key", ["all", "mixed"])
def test_batch(pkg, orc, batch_refs, monkeypatch, key, form):
    """9 frames in one batched call: a flat frame (N = 0), a noise frame whose level 0 is beyond the direct instance (the
    list-pass instance takes that pair in the same call), textured frames.  `mixed`: level 1 is not eligible, so the direct
    kernel and the three list-pass instances all have pairs."""
    import torch
    frames, refs = batch_refs
    p = F.BATCH_P if key == "all" else F.BATCH_MIXED_P
    _set_form(monkeypatch, form)
    c = _ctx(pkg, F.BATCH_W, F.BATCH_H, p, max_batch=len(frames), max_keypoints=32768, max_candidates=65536)
    eligible = F.eligible_levels(F.BATCH_W, F.BATCH_H, p)
    assert eligible == ([True, True, True] if key == "all" else [True, False, True])
    assert c.debug_quad_direct_levels() == (eligible if form == "direct" else [False] * 3)
    dev = torch.from_numpy(np.ascontiguousarray(np.stack(frames))).cuda()
    c.detect_batch_dev(dev.data_ptr(), len(frames))
    c.sync()
    direct_pairs = other_pairs = 0
    for t, frame in enumerate(frames):
        n = _assert_levels(pkg, orc, c, t, frame, p, refs[key][t], (key, form, "frame %d" % t))
        for l, x in enumerate(n):
            if eligible[l] and x <= F.DIRECT_MAX_CANDIDATES:
                direct_pairs += 1
            else:
                other_pairs += 1
    assert np.array_equal(c.debug_counts(pkg.DBG_CANDIDATES, len(frames))[F.BATCH_FLAT], [0, 0, 0])
    assert direct_pairs >= 16 and other_pairs >= (3 if key == "all" else 11), (direct_pairs, other_pairs)
    del dev
    c.close()
