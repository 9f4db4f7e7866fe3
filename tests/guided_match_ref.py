"""Reference restatement of guided matching (not a test): the semantics include/mslam_hip.h states at
mslam_hip_match_guided_knn2, in numpy, as a double loop — over the landmarks in Python, over the keypoints elementwise —
and its composition with tests/reloc_ref.py, tests/track_ref.py and tests/track_window_ref.py into what the mode of
mslam_hip_set_guided_match makes of relocalize, track and track_window.  Shares no code with the product.

Every f64 expression is written out elementwise in the order the header states, so numpy rounds each operation on its own
as the library (built with -ffp-contract=off) does.

Also here: the planted scenes tests/test_guided_match.py proves and tests/test_gpu_guided_match.py runs."""
import numpy as np

import reloc_ref as rr
import track_ref as tr
import track_window_ref as twr
from reloc_ref import po

CAM = rr.CAM
ABSENT = np.int32(2**31 - 1)
IDENTITY_CAM = (1.0, 1.0, 0.0, 0.0)      # with R = I, t = 0 and Z = 1: u = X, v = Y exactly


def project(world, R, t, cam=CAM):
    """-> (u, v, c2) per world point: c_r = ((R[r][0] X + R[r][1] Y) + R[r][2] Z) + t[r], u = (c0 / c2) fx + cx,
    v = (c1 / c2) fy + cy"""
    w = np.asarray(world, np.float64).reshape(-1, 3)
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64).reshape(3)
    X, Y, Z = w[:, 0], w[:, 1], w[:, 2]
    c = [((R[r, 0] * X + R[r, 1] * Y) + R[r, 2] * Z) + t[r] for r in range(3)]
    with np.errstate(all="ignore"):
        u = (c[0] / c[2]) * np.float64(cam[0]) + np.float64(cam[2])
        v = (c[1] / c[2]) * np.float64(cam[1]) + np.float64(cam[3])
    return u, v, c[2]


def in_frame(xy, width, height):
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    x, y = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(x) & np.isfinite(y) & (x >= 0) & (x < np.float64(width)) & (y >= 0) & (y < np.float64(height))


def candidates(xy, u, v, c2, width, height, radius):
    """the keypoints that are candidates of ONE landmark (its u, v, c2) -> bool [n_kp]"""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    x, y = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
    with np.errstate(invalid="ignore"):
        if not c2 > 0:
            return np.zeros(len(xy), bool)
        return in_frame(xy, width, height) & (np.abs(x - u) <= np.float64(radius)) & (np.abs(y - v) <= np.float64(radius))


def hamming(desc, one):
    return np.unpackbits(np.asarray(desc, np.uint8).reshape(-1, 32) ^ np.asarray(one, np.uint8).reshape(1, 32), axis=1).sum(1).astype(np.int64)


def knn2(kp_desc, kp_xy, lm_desc, lm_world, R, t, radius, cam=CAM, width=640, height=480):
    """-> (idx0, idx1, dist0, dist1, n_cand), each [n_lm] int32: per landmark the two candidates of least Hamming distance,
    ties to the lower keypoint index; absent: index -1, distance INT32_MAX"""
    kd = np.asarray(kp_desc, np.uint8).reshape(-1, 32)
    ld = np.asarray(lm_desc, np.uint8).reshape(-1, 32)
    u, v, c2 = project(lm_world, R, t, cam)
    n = len(ld)
    idx = np.full((2, n), -1, np.int32)
    dist = np.full((2, n), ABSENT, np.int32)
    n_cand = np.zeros(n, np.int32)
    for j in range(n):
        cand = np.flatnonzero(candidates(kp_xy, u[j], v[j], c2[j], width, height, radius))
        n_cand[j] = len(cand)
        if len(cand) == 0:
            continue
        d = hamming(kd[cand], ld[j])
        order = np.lexsort((cand, d))[:2]            # by distance, then by keypoint index
        for r, o in enumerate(order):
            idx[r, j], dist[r, j] = cand[o], d[o]
    return idx[0], idx[1], dist[0], dist[1], n_cand


def accept(d0, d1, max_distance, ratio):
    if d0 == ABSENT or d0 > max_distance:
        return False
    return bool(d1 == ABSENT or float(d0) < ratio * float(d1))


def match(kp_desc, kp_xy, lm_desc, lm_world, R, t, radius, max_distance=256, ratio=0.7, cam=CAM, width=640, height=480):
    """-> (from = keypoint indices, to = landmark indices), by landmark"""
    i0, _, d0, d1, _ = knn2(kp_desc, kp_xy, lm_desc, lm_world, R, t, radius, cam, width, height)
    keep = [j for j in range(len(i0)) if accept(d0[j], d1[j], max_distance, ratio)]
    return i0[keep].astype(np.int32), np.array(keep, np.int32)


def min_edge_margin(kp_xy, lm_world, R, t, radius, cam=CAM, width=640, height=480):
    """the least distance, over every (landmark with c2 > 0, in-frame keypoint) pair and both axes, of |x - u| from the
    radius: a pose whose projections move by less than this cannot flip a membership"""
    xy = np.asarray(kp_xy, np.float32).reshape(-1, 2)[in_frame(kp_xy, width, height)].astype(np.float64)
    u, v, c2 = project(lm_world, R, t, cam)
    best = np.inf
    for j in np.flatnonzero(c2 > 0):
        if len(xy):
            best = min(best, np.abs(np.abs(xy[:, 0] - u[j]) - radius).min(), np.abs(np.abs(xy[:, 1] - v[j]) - radius).min())
    return best


# ---- the mode: reloc_ref / track_ref / track_window_ref with the guided matcher in the matcher's place ------------------

def relocalize(desc, xy, store, cand_ids, guess, radius, max_distance=256, width=640, height=480, cam=CAM, valid=None, ratio=0.7,
               iterations=100, thr=5.0, seed=0, min_inliers=60, confidence=0.99):
    """reloc_ref.relocalize with a guess (R0, t0): every candidate's landmarks are matched by `match` under that pose"""
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    cands = []
    for pos, cid in enumerate(cand_ids):
        kd, kw = store[cid]
        fi, ti = match(desc, xy, kd, kw, guess[0], guess[1], radius, max_distance, ratio, cam, width, height)
        keep = np.ones(len(fi), bool) if valid is None else np.asarray(valid).reshape(-1)[fi] != 0
        obj = np.asarray(kw, np.float64).reshape(-1, 3)[ti[keep]].astype(np.float32)
        img = xy[fi[keep]]
        res = po.pnp_ransac(obj, img, cam, iterations, thr, seed + pos, guess, confidence) if len(obj) >= 4 else None
        cands.append(dict(pairs=(fi, ti), n_matches=len(fi), n_correspondences=len(obj), status=0 if res is None else 1,
                          n_inliers=0 if res is None else int(res["mask"].sum()), R=None if res is None else res["R"],
                          t=None if res is None else res["t"], mask=np.zeros(len(obj), bool) if res is None else res["mask"]))
    return dict(best=rr.rank([c["status"] for c in cands], [c["n_inliers"] for c in cands], min_inliers), candidates=cands)


def track(desc, xy, depth, store, ref_id, guess, radius, max_distance=256, vote_ids=(), cam=CAM, factor=tr.FACTOR, ratio=0.7,
          iterations=100, thr=5.0, seed=0, min_matched_points=10, new_keyframe_min_landmarks=30, z_max=3.0, want_keyframe=True,
          width=None, height=None):
    """track_ref.track with the guided matcher; the window's frame extent defaults to the depth image's"""
    h, w = np.asarray(depth).shape
    xyz, valid = tr._oracle().backproject(depth, xy, factor, cam[:2], cam[2:])
    c = relocalize(desc, xy, store, [ref_id], guess, radius, max_distance, w if width is None else width,
                   h if height is None else height, cam, valid, ratio, iterations, thr, seed, 0)["candidates"][0]
    tracked = bool(c["status"]) and c["n_correspondences"] >= min_matched_points
    required = tracked and c["n_inliers"] < new_keyframe_min_landmarks
    out = dict(pairs=c["pairs"], mask=c["mask"], n_matches=c["n_matches"], n_correspondences=c["n_correspondences"],
               n_inliers=c["n_inliers"], status=c["status"], R=c["R"], t=c["t"], tracked=tracked, keyframe_required=required,
               vote_counts=np.zeros(len(vote_ids), np.int32), vote_best=-1, vote_best_count=0, entry=None, xyz=xyz, valid=valid)
    if tracked and len(vote_ids):
        out["vote_counts"], out["vote_best"] = tr.vote(store, vote_ids, c["R"], c["t"], cam, w, h)
        out["vote_best_count"] = int(out["vote_counts"][out["vote_best"]])
    if required and want_keyframe:
        out["entry"] = tr.build_entry(desc, xyz, valid, c["pairs"], c["mask"], store[ref_id][1], c["R"], c["t"], z_max)
    return out


def track_window(descs, xys, depths, store, ref_id, guess, radius, max_distance=256, vote_ids=(), ref_vote_pos=-1, seed=0, **kw):
    """track_window_ref.track_window with the guided matcher: frame s is `track` with seed + s and the one shared guess
    -> (steps, first_event)"""
    steps, first = [], len(descs)
    for s in range(len(descs)):
        st = track(descs[s], xys[s], depths[s], store, ref_id, guess, radius, max_distance, vote_ids, seed=seed + s,
                   want_keyframe=False, **kw)
        steps.append(st)
        if first == len(descs) and twr.is_event(st, len(vote_ids), ref_vote_pos):
            first = s
    return steps, first


# ---- planted scenes --------------------------------------------------------------------------------------------------------

def rvec_of(R):
    th = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    if th < 1e-12:
        return np.zeros(3)
    return th / (2 * np.sin(th)) * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])


def random_scene(seed, n_kp, n_lm, width, height, spread=8.0):
    """n_lm landmarks at Z = 1 whose projections (IDENTITY_CAM, R = I, t = 0: u = X, v = Y) are uniform over the frame and a
    little beyond, n_kp keypoints uniform over the frame; a third of the keypoints (where there are landmarks) sit within
    `spread` px of a landmark and carry its descriptor with a few flipped bits, so windows hold near and far candidates"""
    rng = np.random.default_rng(seed)
    world = np.stack([rng.uniform(-10, width + 10, n_lm), rng.uniform(-10, height + 10, n_lm), np.ones(n_lm)], 1)
    ld = rng.integers(0, 256, (n_lm, 32), dtype=np.uint8)
    xy = rng.uniform(0, [width, height], (n_kp, 2))
    kd = rng.integers(0, 256, (n_kp, 32), dtype=np.uint8)
    if n_lm and n_kp:
        near = rng.choice(n_kp, n_kp // 3, replace=False)
        src = rng.integers(0, n_lm, len(near))
        xy[near] = world[src, :2] + rng.uniform(-spread, spread, (len(near), 2))
        kd[near] = rr._flip_bits(rng, ld[src], 5)
    xy = xy.astype(np.float32)
    xy[:, 0] = np.clip(xy[:, 0], 0, np.nextafter(np.float32(width), np.float32(0)))
    xy[:, 1] = np.clip(xy[:, 1], 0, np.nextafter(np.float32(height), np.float32(0)))
    return dict(kp_desc=kd, kp_xy=xy, lm_desc=ld, lm_world=world, R=np.eye(3), t=np.zeros(3), cam=IDENTITY_CAM, width=width,
                height=height)


def edge_scene(radius, width=640, height=480):
    """Exact window edges (IDENTITY_CAM: u = X).  Landmarks and what each one's window holds:
      0  at (100, 100): keypoints exactly at u +- radius (in) and nextafter beyond (out), on both axes, plus the centre
      1  at (208, 336), the centre of a 32-px cell: with radius < 16 inside one cell;  2 at (416, 336): on a cell edge in x,
         2 cells;  3 at (512, 128): on a cell corner, 4 cells  (larger radii: 9 and more cells)
      4 .. 7  at the four frame borders: the window is clamped
      8  c2 = 0;  9  c2 < 0;  10  c2 = 1e-300 (u overflows to inf);  11  a NaN world point;  15  c2 = 1e-300 with
         u = 1e300, v = -1e300 (finite, far beyond any int): no candidates
      12 at (300, 200): keypoints at x = NaN and y = inf next to it are out; one real keypoint is in
      13 at (2, 60): a keypoint at x = -0.0 is in, one at x = -0.25 is out
      14 at (width - 1, 60): a keypoint at x = width is out, the one at nextafter(width, 0) is in (radius >= 1)
    Landmarks lie more than 2 x 47.5 px apart on an axis: for every radius up to 47.5 no window holds another's keypoints.
    -> the scene and `expect` = {landmark: sorted keypoint indices of its window}"""
    assert (width, height) == (640, 480) and radius <= 47.5
    r = np.float64(radius)
    f32 = np.float32
    kp, expect = [], {}

    def add(j, pts_in, pts_out):
        ids = []
        for p in pts_in:
            ids.append(len(kp))
            kp.append(p)
        for p in pts_out:
            kp.append(p)
        expect[j] = sorted(expect.get(j, []) + ids)

    def beyond(c, sign):                   # the f32 next to c + sign r, away from c
        edge = f32(c + sign * r)
        assert np.float64(edge) == c + sign * r, "the edge is not an f32"
        return np.nextafter(edge, f32(np.inf * sign))

    lm = [(100.0, 100.0, 1.0)]
    add(0, [(100 + r, 100), (100 - r, 100), (100, 100 + r), (100, 100 - r), (100 + r, 100 - r), (100, 100)],
        [(beyond(100.0, 1), 100), (beyond(100.0, -1), 100), (100, beyond(100.0, 1)), (100, beyond(100.0, -1))])
    for j, c in ((1, (208.0, 336.0)), (2, (416.0, 336.0)), (3, (512.0, 128.0))):
        lm.append(c + (1.0,))
        q = min(r, 15.0) / 2
        add(j, [(c[0] - q, c[1] - q), (c[0] + q, c[1] + q), (c[0] - q, c[1] + q), (c[0] + q, c[1] - q)], [])
    for j, c in ((4, (0.0, 240.0)), (5, (width - 0.5, 240.0)), (6, (320.0, 0.0)), (7, (320.0, height - 0.5))):
        lm.append(c + (1.0,))
        add(j, [(min(max(c[0], 0), width - 0.5), min(max(c[1], 0), height - 0.5))], [])
    lm += [(5.0, 5.0, 0.0), (5.0, 5.0, -1.0), (1e10, 1e10, 1e-300), (np.nan, 50.0, 1.0)]
    for j in (8, 9, 10, 11):
        expect[j] = []
    lm.append((300.0, 200.0, 1.0))
    add(12, [(300.25, 200.25)], [(np.nan, 200.0), (300.0, np.inf), (np.nan, np.nan), (-np.inf, 200.0)])
    lm.append((2.0, 60.0, 1.0))
    add(13, [(-0.0, 60.0)] if r >= 2 else [], [(-0.25, 60.0)] + ([] if r >= 2 else [(-0.0, 60.0)]))
    lm.append((width - 1.0, 60.0, 1.0))
    add(14, [(np.nextafter(f32(width), f32(0)), 60.0)] if r >= 1 else [], [(float(width), 60.0)])
    lm.append((1.0, -1.0, 1e-300))
    expect[15] = []
    rng = np.random.default_rng(3)
    return dict(kp_desc=rng.integers(0, 256, (len(kp), 32), dtype=np.uint8), kp_xy=np.array(kp, np.float32),
                lm_desc=rng.integers(0, 256, (len(lm), 32), dtype=np.uint8), lm_world=np.array(lm, np.float64), R=np.eye(3),
                t=np.zeros(3), cam=IDENTITY_CAM, width=width, height=height, expect=expect)


def tie_scene():
    """One landmark window (radius 10 round (50, 50)) for each acceptance case, far apart; descriptors by distance from the
    landmark's: landmark -> [(keypoint offset, distance)], and what knn-2 / acceptance make of it.
      0  two equal descriptors at distance 3: the lower index wins, d0 == d1 is rejected
      1  distances 0 and 256: accepted (0 < 0.7 * 256)
      2  a single candidate at distance 200: accepted without a ratio test up to max_distance >= 200
      3  distances 255 and 256 -> rejected by the ratio test whatever max_distance is
      4  a single candidate at distance 256: accepted only with max_distance = 256
      5  a single candidate at distance 0: accepted with every max_distance
      6  distances 10, 10, 9 (in index order): the 9 first, then the lower index of the two 10s"""
    rng = np.random.default_rng(4)
    plan = {0: [3, 3], 1: [0, 256], 2: [200], 3: [255, 256], 4: [256], 5: [0], 6: [10, 10, 9]}
    lm_desc = rng.integers(0, 256, (len(plan), 32), dtype=np.uint8)
    lm_world, kd, kxy = [], [], []
    for j, dists in plan.items():
        c = (50.0 + 60.0 * j, 50.0)
        lm_world.append(c + (1.0,))
        for k, d in enumerate(dists):
            row = np.unpackbits(lm_desc[j])
            row[:d] ^= 1                              # the first d bits flipped: equal d -> equal descriptors
            kd.append(np.packbits(row))
            kxy.append((c[0] + k - 1.0, c[1] + 0.5 * k))
    return dict(kp_desc=np.array(kd, np.uint8), kp_xy=np.array(kxy, np.float32), lm_desc=lm_desc, lm_world=np.array(lm_world),
                R=np.eye(3), t=np.zeros(3), cam=IDENTITY_CAM, width=640, height=480, radius=10.0, plan=plan)


def crowded_scene(n_in=3000, n_lm=3):
    """n_in keypoints inside the one cell [320, 352) x [224, 256) and nothing else; landmark 1 sits at the cell's centre and,
    with radius 16, sees them all; landmarks 0 and 2 sit 100 px to its sides and see none"""
    rng = np.random.default_rng(5)
    xy = np.stack([rng.uniform(320.5, 351.5, n_in), rng.uniform(224.5, 255.5, n_in)], 1).astype(np.float32)
    lm_world = np.array([(236.0, 240.0, 1.0), (336.0, 240.0, 1.0), (436.0, 240.0, 1.0)][:n_lm])
    return dict(kp_desc=rng.integers(0, 256, (n_in, 32), dtype=np.uint8), kp_xy=xy, lm_desc=rng.integers(0, 256, (n_lm, 32), dtype=np.uint8),
                lm_world=lm_world, R=np.eye(3), t=np.zeros(3), cam=IDENTITY_CAM, width=640, height=480, radius=16.0)


def perturbed(R, t, deg, metres, seed=0):
    """the pose (R, t) turned by `deg` degrees about a random axis and moved by `metres`"""
    rng = np.random.default_rng(seed)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    d = rng.normal(size=3)
    d *= metres / np.linalg.norm(d)
    return po.rodrigues(axis * np.radians(deg)) @ R, t + d


def twins_scene(seed=0, n_pairs=150, radius=15.0, flip=6, n_distractors=300, width=640, height=480):
    """reloc_ref.make_scene's geometry (camera-frame box, one known pose) with every landmark descriptor used by TWO
    landmarks whose projections lie more than 4 radii apart on an axis (so that their windows stay disjoint under a guess
    that moves projections by up to a radius), every landmark seen by its own keypoint: its descriptor with `flip` flipped
    bits (independent flips: each twin's keypoint is at distance `flip` from both landmarks), plus distractors with random
    descriptors, shuffled; a depth image with a valid depth everywhere.
    -> dict(store = {0: (desc, world)}, desc, xy, depth, R, t, own = keypoint of each landmark, twin = landmark's twin)"""
    rng = np.random.default_rng(seed)
    R = po.rodrigues(rng.normal(size=3) * 0.3)
    t = rng.normal(size=3) * 0.2 + np.array([0.1, -0.1, 0.3])
    n = 2 * n_pairs

    def draw(k):
        return np.stack([rng.uniform(-1.4, 1.4, k), rng.uniform(-1.0, 1.0, k), rng.uniform(2.5, 6.0, k)], 1)

    def image(p):
        return np.stack([CAM[0] * p[:, 0] / p[:, 2] + CAM[2], CAM[1] * p[:, 1] / p[:, 2] + CAM[3]], 1)

    a = draw(n_pairs)
    b = draw(n_pairs)
    for _ in range(1000):
        bad = np.abs(image(a) - image(b)).max(1) <= 4 * radius
        if not bad.any():
            break
        b[bad] = draw(int(bad.sum()))
    assert not bad.any()
    cam_pts = np.concatenate([a, b])
    world = (cam_pts - t) @ R
    half = rng.integers(0, 256, (n_pairs, 32), dtype=np.uint8)
    ld = np.concatenate([half, half])
    twin = np.concatenate([np.arange(n_pairs) + n_pairs, np.arange(n_pairs)])
    img, ok = po.project(R, t, world.astype(np.float32).astype(np.float64), CAM)
    assert ok.all() and (img[:, 0] >= 1).all() and (img[:, 0] < width - 1).all() and (img[:, 1] >= 1).all() and (img[:, 1] < height - 1).all()
    qd = np.concatenate([rr._flip_bits(rng, ld, flip), rng.integers(0, 256, (n_distractors, 32), dtype=np.uint8)])
    qxy = np.concatenate([img, rng.uniform(1, [width - 1, height - 1], (n_distractors, 2))]).astype(np.float32)
    perm = rng.permutation(len(qd))
    own = np.argsort(perm)[:n]                         # position of landmark j's keypoint after the shuffle
    depth = np.full((height, width), 10000, np.uint16)
    return dict(store={0: (ld, world)}, desc=qd[perm].copy(), xy=qxy[perm].copy(), depth=depth, R=R, t=t, own=own, twin=twin,
                radius=radius, n_distractors=n_distractors)


def mode_frames(seed=0, S=17, far_at=12):
    """What the mode tests run on: track_ref.make_sequence's frame 0 lifted into keyframe 0 (as the loop does) with two
    more entries for relocalize (1: a decoy, 2: strangers), and S
    query frames that are shuffled 85 % subsets of its frame 2 (one depth image, so one true pose), frame `far_at` being a
    shuffled frame 16 instead (the camera 5.6 m away: under the shared guess its landmarks project elsewhere and the frame
    is not tracked); the guess is frame 2's true pose perturbed by 0.3 degrees / 5 mm.
    -> dict(store, frames = [dict(desc, xy, depth)], guess = (R, t), truth = (R, t))"""
    seq = tr.make_sequence(seed=0)
    f0 = seq["frames"][0]
    xyz, valid = tr._oracle().backproject(f0["depth"], f0["xy"], tr.FACTOR, CAM[:2], CAM[2:])
    keep = valid & (xyz[:, 2] <= 3.0)
    store = {0: (f0["desc"][keep].copy(), xyz[keep].copy())}
    rng = np.random.default_rng(seed + 100)
    d0, w0 = store[0]
    store[1] = (d0.copy(), w0[rng.permutation(len(w0))].copy())                    # a decoy: the same descriptors elsewhere
    store[2] = (rng.integers(0, 256, (300, 32), dtype=np.uint8), w0[:300] + 0.5)  # and an entry of strangers
    frames = []
    for s in range(S):
        src = seq["frames"][16 if s == far_at else 2]
        n = len(src["desc"])
        pick = rng.permutation(n)[:int(0.85 * n) + s]
        frames.append(dict(desc=src["desc"][pick].copy(), xy=src["xy"][pick].copy(), depth=src["depth"]))
    truth = (seq["frames"][2]["R"], seq["frames"][2]["t"])
    return dict(store=store, frames=frames, guess=perturbed(truth[0], truth[1], 0.3, 0.005, seed), truth=truth)
