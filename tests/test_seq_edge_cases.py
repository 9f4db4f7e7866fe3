"""The inputs of tests/test_gpu_seq_edges.py, on the CPU references alone: every builder of tests/seq_edge_cases.py meets the
condition it is named for."""
import numpy as np
import pytest

import reloc_ref as rr
import seq_edge_cases as sec
import track_ref as tr


@pytest.fixture(autouse=True)
def _oracle(orc):
    """(the references call the oracle library: built before the first case)"""


def test_track_hands_its_capacity_to_build_entry():
    tc = sec.twin_case(3)
    cut, uncut = sec.twin_track(3)["entry"], sec.twin_track(3, None)["entry"]
    assert len(cut["kp"]) == tc["K"] < len(uncut["kp"])
    for k in ("desc", "world", "src", "kp"):
        assert np.array_equal(cut[k], uncut[k][:tc["K"]]), k
    assert cut["n_inherited"] == uncut["n_inherited"]


def test_twins_overflow_the_entry_and_repeat_keypoints():
    tc = sec.twin_case(3)
    K, step = tc["K"], sec.twin_track(3, None)
    e = step["entry"]
    na = e["n_inherited"]
    distinct = len(set(e["kp"][:na].tolist()))
    print("three copies: nq", K, "reference entry", len(tc["store"][0][0]), "matches", step["n_matches"], "correspondences",
          step["n_correspondences"], "inliers", step["n_inliers"], "uncut entry", len(e["kp"]), "inherited", na, "distinct", distinct)
    assert K == len(tc["frame"]["desc"]) == 227 and len(tc["store"][0][0]) <= K       # the store takes the reference entry
    assert (step["n_matches"], step["n_correspondences"], step["n_inliers"]) == (165, 153, 153) and step["keyframe_required"]
    assert len(e["kp"]) == 271 >= K + 20 and na == 153 < K                            # cut inside part B, 20 and more lost
    assert distinct == 51 and np.bincount(e["kp"][:na]).max() == 3                    # part A repeats its keypoints
    assert not np.isin(e["kp"][na:], e["kp"][:na]).any()
    assert len(set(tc["lids"].tolist())) == len(tc["lids"])
    # two copies: repeats, no cut
    t2 = sec.twin_case(2)
    e2 = sec.twin_track(2)["entry"]
    assert t2["K"] == K and (len(e2["kp"]), e2["n_inherited"]) == (220, 102) and len(set(e2["kp"][:102].tolist())) == 51
    assert np.array_equal(e2["kp"], sec.twin_track(2, None)["entry"]["kp"])


def test_the_cut_entry_tracks_the_next_frame():
    tc = sec.twin_case(3)
    e, nx = sec.twin_track(3)["entry"], tc["next"]
    assert len(nx["desc"]) == tc["K"]
    step = tr.track(nx["desc"], nx["xy"], nx["depth"], {9: (e["desc"], e["world"])}, 9, [9], seed=2, guess=sec.IDENTITY)
    print("next frame against the cut entry:", step["n_matches"], step["n_correspondences"], step["n_inliers"])
    assert step["tracked"] and step["n_inliers"] >= 30


def test_the_twin_window_has_its_event_at_frame_1():
    w, tc = sec.twin_window(), sec.twin_case(3)
    print("window inliers", [s["n_inliers"] for s in w["steps"]], "kf_min", w["kf_min"], "first", w["first"])
    assert w["first"] == 1 and all(len(x["desc"]) <= tc["K"] for x in w["frames"])
    assert w["steps"][0]["tracked"] and not w["steps"][0]["keyframe_required"] and w["steps"][1]["keyframe_required"]
    single = sec.twin_track(3, None)
    assert np.array_equal(w["entry"]["kp"], single["entry"]["kp"]) and np.array_equal(w["entry"]["world"], single["entry"]["world"])


@pytest.mark.parametrize("k", range(8))
def test_k_correspondences(k):
    full, r = sec.few_full()["candidates"][0], sec.few_ref(k)["candidates"][0]
    assert len(sec.few_scene()["desc"]) == 1838 and full["n_matches"] == 538 and full["mask"].all()
    assert (r["n_matches"], r["n_correspondences"]) == (538, k)
    assert (r["status"], r["n_inliers"]) == ((0, 0) if k <= 4 else (1, k)) and int(r["mask"].sum()) == r["n_inliers"]
    d = sec.few_depth(k)["ref"]
    print(k, "track:", d["n_matches"], d["n_correspondences"], d["status"], d["tracked"])
    assert d["n_correspondences"] == k and d["n_matches"] > 50 and not d["tracked"] and d["entry"] is None and not d["vote_counts"].any()


@pytest.mark.parametrize("n", sec.FULL_SIZES)
def test_full_rows_match_every_landmark(n):
    for n_cand in (2, 64):
        r = sec.full_ref(n, n_cand)
        for c, o in zip(r["candidates"], sec.full_rows(n, n_cand)["offsets"]):
            assert c["n_matches"] == c["n_correspondences"] == n                       # m == n: a full row when n is 256 or 512
            assert np.array_equal(c["pairs"][1], np.arange(n)) and np.array_equal(c["pairs"][0], o + np.arange(n))


@pytest.mark.parametrize("pattern", sec.VALID_PATTERNS)
def test_valid_patterns_empty_what_they_name(pattern):
    n = 512
    v = sec.pattern_valid(n, pattern)
    c0 = sec.full_ref(n, 2, pattern)["candidates"][0]
    on = v[c0["pairs"][0]]
    want = {"wave0": n - 64, "chunk_64_319": n - 256, "alternate": n // 2, "none": 0, "last_only": 1}[pattern]
    assert c0["n_matches"] == n and c0["n_correspondences"] == want == int(on.sum())
    if pattern == "wave0":
        assert not on[:64].any() and on[64:].all()
    if pattern == "chunk_64_319":
        assert on[:64].all() and not on[64:320].any() and on[320:].all()
    if pattern == "last_only":
        assert on[-1]


def test_z_max_equality_decides_a_part_b_keypoint():
    zc = sec.zmax_case()
    i, z = zc["i"], zc["z"]
    below = float(np.nextafter(z, 0))
    at, under, all_ = sec.zmax_entry(z), sec.zmax_entry(below), sec.zmax_entry(np.inf)
    assert 0 < below < z <= 3.0 and i in at["kp"][at["n_inherited"]:] and i not in under["kp"]
    assert len(under["kp"]) < len(at["kp"]) < len(all_["kp"]) and at["n_inherited"] == under["n_inherited"] == all_["n_inherited"] > 0
    st = zc["ref"]
    used = st["pairs"][0][st["valid"][st["pairs"][0]] != 0]
    assert len(all_["kp"]) - all_["n_inherited"] == int(st["valid"].sum()) - len(set(used.tolist()))      # inf keeps every valid keypoint


def test_the_big_query_uses_the_upper_half_of_the_bitmap():
    g = sec.upper_used()
    step, e = g["ref"], g["ref"]["entry"]
    na = e["n_inherited"]
    print("big query: matches", step["n_matches"], "correspondences", step["n_correspondences"], "inliers", na, "entry", len(e["kp"]))
    assert len(g["desc"]) == 33000 and g["lead"] >= 32768 and len(g["store"][0][0]) == 200 and len(e["kp"]) <= g["K"]
    assert step["keyframe_required"] and na > 100 and e["kp"][:na].min() >= 32768
    matched = step["pairs"][0][step["valid"][step["pairs"][0]] != 0]
    assert matched.min() >= 32768 and not np.isin(e["kp"][na:], matched).any()
    assert (e["kp"][na:] >= 32768).any() and (e["kp"][na:] < 32768).any()           # part B reads both halves
    assert step["valid"].all() and len(e["kp"]) < 33000                               # z_max cuts part B


def test_rankings():
    cand, mi, r = sec.ranking_ref("no_model")
    assert len(cand) == 64 and r["best"] == -1 and not any(c["status"] for c in r["candidates"])
    cand, mi, r = sec.ranking_ref("last")
    assert r["best"] == 63 and [c["status"] for c in r["candidates"]] == [0] * 63 + [1]
    n_in = r["candidates"][63]["n_inliers"]
    cand, mi, r = sec.ranking_ref("at_min")
    assert mi == n_in and r["best"] == 63
    cand, mi, r = sec.ranking_ref("below_min")
    assert mi == n_in + 1 and r["best"] == -1 and r["candidates"][63]["n_inliers"] == n_in


def test_query_of_entry_finds_its_pose():
    sc = sec.few_scene()
    d, w = sc["store"][sc["target_id"]]
    w = w @ sc["R"].T + sc["t"]                                   # in front of the identity camera
    qd, qxy = sec.query_of_entry(d, w, seed=1)
    c = rr.relocalize(qd, qxy, {0: (d, w)}, [0], seed=1)["candidates"][0]
    assert c["status"] and c["n_inliers"] > 200
