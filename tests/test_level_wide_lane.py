"""The level kernels (k_level.hip: gray + blur, resize + blur) at the shapes where a lane that owns eight adjacent pixels
of a row can go wrong: level widths of every residue mod 8 (a row that ends in the middle of its last lane, or in the
middle of a quad), rows wider than one wave, the narrowest pyramids, row blocks that end short, batches on both sides of
the 8-frame switch between the batched and the handful-of-frames launches, a frame boundary inside a wave, both detector
modes (INTER_LINEAR and INTER_LINEAR_EXACT) and both layouts of the blurred slab.  Every raw plane and every blurred plane
of every frame is compared with the oracle's, bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_LEVELS = 4
BATCHES = (1, 7, 8, 9)
# (W, H).  200 / 204 / 236: level 0 is 0 and 4 (mod 8) and the upper levels reach the odd residues; 524: a row is more than
# one wave's 62 productive lanes, eight pixels each; 80: the narrowest pyramid whose level 0 has dword columns; 77: the
# narrowest one the context accepts (its smallest level is 45 px, one more than two borders and an overlap).  Heights: 120 and
# 131 are not 6 k + 2 and no multiple of the row blocks taken (the last block of a level is short), all are below 380 (2-row
# blocks for fewer than 8 frames), and every level is small enough for the shortened blocks of the batched launches.
SHAPES = ((200, 120), (204, 120), (236, 131), (524, 122), (80, 120), (77, 118))
_cache = {}


def _frames(W, H):
    """9 frames: seeded noise, one constant, one horizontal ramp; frames 0 and 8 differ"""
    rng = np.random.default_rng(1000 * W + H)
    fr = rng.integers(0, 256, (9, H, W, 3), dtype=np.uint8)
    fr[3] = 93
    fr[5] = (np.arange(W, dtype=np.uint32) * 255 // (W - 1)).astype(np.uint8)[None, :, None]
    assert not np.array_equal(fr[0], fr[8])
    return fr


def _reference(orc, W, H, cv):
    """frames and, per frame, the oracle's (raw planes, blurred planes): computed once per shape and mode, never modified"""
    key = (W, H, cv)
    if key not in _cache:
        fr = _frames(W, H)
        planes = []
        for f in fr:
            pyr = (orc.cvorb_pyramid(orc.gray(f), orc.cvorb_params(n_levels=N_LEVELS)) if cv
                   else orc.pyramid(orc.gray(f), orc.params(n_levels=N_LEVELS)))
            planes.append((pyr, [orc.gaussian_blur7(im) for im in pyr]))
        _cache[key] = (fr, planes)
    return _cache[key]


def _check(pkg, orc, monkeypatch, W, H, tiled, cv):
    import torch
    monkeypatch.setenv("MSLAM_HIP_TILED_BLUR", tiled)
    fr, planes = _reference(orc, W, H, cv)
    kw = dict(detector=pkg.DETECTOR_CV_ORB, n_features=500) if cv else {}
    c = pkg.Context(width=W, height=H, max_batch=max(BATCHES), n_levels=N_LEVELS, max_keypoints=16384, max_candidates=65536, **kw)
    try:
        dev = torch.from_numpy(fr).cuda()
        for n in BATCHES:
            c.detect_batch_dev(dev.data_ptr(), n)
            c.sync()
            for f in range(n):
                for l in range(N_LEVELS):
                    what = "%dx%d tiled=%s cv=%s batch of %d, frame %d, level %d" % (W, H, tiled, cv, n, f, l)
                    assert np.array_equal(c.debug_image(pkg.DBG_PYRAMID, f, l), planes[f][0][l]), "raw plane: " + what
                    assert np.array_equal(c.debug_image(pkg.DBG_BLURRED, f, l), planes[f][1][l]), "blurred plane: " + what
    finally:
        c.close()


def test_level_widths_cover_every_residue(orc):
    """the shapes above reach level widths of all eight residues mod 8, in both detector modes' geometry"""
    seen, seen_cv = set(), set()
    for W, H in SHAPES:
        seen |= {int(w) % 8 for w in orc.level_geometry(W, H, orc.params(n_levels=N_LEVELS))[0][:N_LEVELS]}
        seen_cv |= {int(w) % 8 for w in orc.cvorb_geometry(W, H, orc.cvorb_params(n_levels=N_LEVELS))[0][:N_LEVELS]}
    assert seen == set(range(8)) and seen_cv == set(range(8)), (seen, seen_cv)
    assert max(W for W, _ in SHAPES) >= 520 and all(H < 380 for _, H in SHAPES)
    assert any((H - 2) % 6 for _, H in SHAPES)


@pytest.mark.parametrize("tiled", ["1", "0"])
@pytest.mark.parametrize("W,H", SHAPES)
def test_distributed_levels(pkg, orc, monkeypatch, W, H, tiled):
    _check(pkg, orc, monkeypatch, W, H, tiled, False)


@pytest.mark.parametrize("tiled", ["1", "0"])
@pytest.mark.parametrize("W,H", [(204, 120), (236, 131)])
def test_cv_orb_levels(pkg, orc, monkeypatch, W, H, tiled):
    _check(pkg, orc, monkeypatch, W, H, tiled, True)


def test_smallest_context(pkg):
    """77 px is the narrowest 4-level pyramid the context accepts: one pixel less is refused"""
    with pytest.raises(pkg.MslamHipError):
        pkg.Context(width=76, height=118, n_levels=N_LEVELS)
