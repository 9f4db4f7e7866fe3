"""Removing observations without a GPU: the entry point is exported, declared and listed; tests/prune_ref.py's restatement
holds the rules of include/mslam_hip.h's statement on hand cases (the GPU tests then hold the library to the restatement);
HipBackend.remove_observations against its restatement; HipBackend.local_ba(prune=True) on a stub context that solves with
tests/ba_ref.py, on the three planted scenes; the margin of the flags the GPU test rests on; the constructor's guard."""
import inspect
import os
import re

import numpy as np
import pytest

import ba_ref
import prune_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mslam_hip_kf_remove_observations"


def test_symbol_is_exported_declared_and_listed(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mslam_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint %s\s*\(" % NAME, hdr)
    assert NAME in pkg.ABI_SYMBOLS and hasattr(pkg.lib(), NAME)
    assert pkg.lib().mslam_hip_abi_version() == 5
    assert callable(pkg.Context.kf_remove_observations) and callable(pkg.HipBackend.remove_observations)
    assert inspect.signature(pkg.HipBackend.local_ba).parameters["prune"].default is False
    assert inspect.signature(pkg.HipBackend.global_ba).parameters["prune"].default is False
    assert inspect.signature(pkg.HipKeyframeTracker.__init__).parameters["ba_prune"].default is False


def _same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_order_is_kept_and_an_unnamed_entry_is_untouched():
    store, kf, lid = pr.hand_case("order")
    new, removed, n = pr.remove_observations(store, kf, lid)
    assert new[1][2].tolist() == [11, 12, 14, 15] and removed.tolist() == [1, 1] and n == 2
    keep = [1, 2, 4, 5]
    assert _same(new[1], (store[1][0][keep], store[1][1][keep], store[1][2][keep]))
    assert new[2] is store[2] and _same(new[2], store[2])      # entry 2 holds id 10 too: only the named entry loses it


def test_a_repeat_inside_an_entry_and_a_row_listed_twice():
    store, kf, lid = pr.hand_case("repeat_inside")
    new, removed, n = pr.remove_observations(store, kf, lid)
    assert new[1][2].tolist() == [10, 13]
    assert removed.tolist() == [2, 1, 2]       # both rows for id 11 report its two positions ...
    assert n == 3                              # ... which are counted once
    assert new[2][2].tolist() == [11, 12]


def test_an_absent_id_and_an_emptied_entry():
    store, kf, lid = pr.hand_case("absent")
    new, removed, n = pr.remove_observations(store, kf, lid)
    assert new[1][2].tolist() == [10, 11, 13] and removed.tolist() == [0, 1] and n == 1
    store, kf, lid = pr.hand_case("emptied")
    new, removed, n = pr.remove_observations(store, kf, lid)
    assert sorted(new) == [1, 2] and len(new[1][2]) == 0 and new[1][0].shape == (0, 32) and new[1][1].shape == (0, 3)
    assert removed.tolist() == [1, 1] and n == 2 and _same(new[2], store[2])


def test_errors_of_the_restatement():
    store, _, _ = pr.hand_case("absent")
    with pytest.raises(KeyError):
        pr.remove_observations(store, [7], [10])
    with pytest.raises(ValueError):
        pr.remove_observations(store, [1], [-1])
    new, removed, n = pr.remove_observations(store, [], [])
    assert n == 0 and len(removed) == 0 and new[1] is store[1]


def test_random_case_counts():
    store, kf, lid = pr.random_case(3, [0, 1, 40, 300])
    new, removed, n = pr.remove_observations(store, kf, lid)
    assert n == sum(len(store[k][2]) - len(new[k][2]) for k in store) > 50
    distinct = {}
    for k, l, r in zip(kf.tolist(), lid.tolist(), removed.tolist()):
        assert distinct.setdefault((k, l), r) == r
    assert sum(distinct.values()) == n and len(distinct) < len(kf)


# ---- the backend ----------------------------------------------------------------------------------------------------------
def _backend(pkg):
    b = pkg.HipBackend(None)
    rng = np.random.default_rng(5)
    I = (0, 0, 0, 1, 0, 0, 0)
    b.add_keyframe(3, I, [10, 11, 12, 11], rng.normal(size=(4, 3)))     # 11 twice in keyframe 3
    b.add_keyframe(5, I, [11, 12, 13], rng.normal(size=(3, 3)))
    b.add_keyframe(4, I, [12, 13, 14], rng.normal(size=(3, 3)))
    return b


@pytest.mark.parametrize("pairs", [[(3, 11)], [(3, 12)], [(3, 10), (3, 10)], [(3, 12), (5, 12), (4, 12)], [(9, 10), (3, 99)], [],
                                   [(5, 13), (3, 11), (4, 14)]])
def test_backend_remove_observations_against_the_restatement(pkg, pairs):
    b = _backend(pkg)
    obs, lms, anchor, n = pr.backend_remove(b.obs, b.landmarks, b.anchor, pairs)
    assert b.remove_observations(pairs) == n
    assert sorted(b.obs) == sorted(obs)
    for k in obs:
        assert b.obs[k][0].tolist() == obs[k][0].tolist() and b.obs[k][1].tobytes() == obs[k][1].tobytes()
    assert b.anchor == anchor and sorted(b.landmarks) == sorted(lms)
    assert all(b.landmarks[l].tobytes() == lms[l].tobytes() for l in lms)


def test_backend_reanchors_and_drops_orphans(pkg):
    b = _backend(pkg)
    assert b.anchor[12] == 3 and b.anchor[10] == 3
    assert b.remove_observations([(3, 12)]) == 1
    assert b.anchor[12] == 4                        # keyframes 4 and 5 still observe 12: the smallest id
    assert b.remove_observations([(3, 11)]) == 2    # both positions
    assert b.anchor[11] == 5 and b.obs[3][0].tolist() == [10]
    assert b.remove_observations([(3, 10)]) == 1    # nobody observes 10 any more
    assert 10 not in b.landmarks and 10 not in b.anchor and len(b.obs[3][0]) == 0 and b.obs[3][1].shape == (0, 3)
    assert b.remove_observations([(3, 10), (77, 1)]) == 0


class StubContext:
    """Context.bundle_adjust's arguments and result, solved by tests/ba_ref.py"""

    def __init__(self):
        self.calls = 0

    def bundle_adjust(self, poses, landmarks, obs_kf, obs_lm, obs_cam, fixed=None, max_iterations=100, outlier_threshold=0.15):
        self.calls += 1
        res = ba_ref.bundle_adjust(poses, landmarks, obs_kf, obs_lm, obs_cam, fixed, max_iterations)
        mask = ba_ref.outliers(res["poses"], res["landmarks"], obs_kf, obs_lm, obs_cam, outlier_threshold)
        return dict(poses=res["poses"], landmarks=res["landmarks"], outlier=mask, termination=res["termination"],
                    iterations=res["iterations"], n_outliers=int(mask.sum()), initial_cost=res["initial_cost"],
                    final_cost=res["final_cost"])

    bundle_adjust_global = bundle_adjust


def _graph(K):
    return {k: set(range(K)) - {k} for k in range(K)}


def check_pruned(res, ref, sc):
    """what the CPU and the GPU tests ask of a pruned solve on a planted scene"""
    planted = {(int(sc["obs_kf"][m]), int(sc["obs_lm"][m])) for m in ref["planted"]}
    pairs = res["pruned"]["pairs"]
    assert planted <= set(pairs)
    assert len(res["outlier_observations"]) == 0 and not res["outlier"].any()      # the second solve flags nothing
    e1 = pr.max_position_error(res["pruned"]["first"]["poses"], sc["truth_poses"])
    e2 = pr.max_position_error(res["poses"], sc["truth_poses"])
    print("pruned BA: %d pairs (%d planted), max position error %.4f -> %.4f m" % (len(pairs), len(planted), e1, e2))
    assert e2 <= e1 / 5.0
    return e1, e2


@pytest.mark.parametrize("which", range(len(pr.BA_SCENES)))
def test_local_ba_prune_on_a_stub_context(pkg, which):
    ref = pr.pruned_reference(which)
    sc = ref["scene"]
    K = len(sc["poses"])
    ctx = StubContext()
    b = pr.backend_of(pkg, ctx, sc)
    m_before = sum(len(v[0]) for v in b.obs.values())
    res = b.local_ba(0, _graph(K), prune=True)
    assert ctx.calls == 2 and res["keyframes"] == list(range(K))
    check_pruned(res, ref, sc)
    pairs = res["pruned"]["pairs"]
    assert pairs == sorted(set(zip(sc["obs_kf"][ref["mask"]].tolist(), sc["obs_lm"][ref["mask"]].tolist())))
    assert sum(len(v[0]) for v in b.obs.values()) == m_before - int(ref["mask"].sum()) == len(res["outlier"])
    assert res["pruned"]["first"]["n_outliers"] == int(ref["mask"].sum()) and "pruned" not in res["pruned"]["first"]
    assert not ref["mask2"].any()
    # a landmark all of whose observations were flagged is gone from the backend
    for l in range(len(sc["landmarks"])):
        assert (l in b.landmarks) == bool(ref["keep"][sc["obs_lm"] == l].any())


def test_prune_off_and_nothing_to_prune(pkg):
    sc = ba_ref.make_scene(4, 20, 9, noise=0.002, views=3)
    ctx = StubContext()
    b = pr.backend_of(pkg, ctx, sc)
    res = b.local_ba(0, _graph(4))
    assert ctx.calls == 1 and "pruned" not in res
    res = b.global_ba(prune=True)                   # nothing is flagged: no second solve
    assert ctx.calls == 2 and res["pruned"]["pairs"] == [] and res["pruned"]["first"]["termination"] == res["termination"]


def test_a_failed_first_solve_prunes_nothing(pkg):
    sc, _ = pr.planted_scene(*pr.BA_SCENES[0])
    ctx = StubContext()
    b = pr.backend_of(pkg, ctx, sc)
    b.obs[1][1][0, 0] = np.nan                      # the initial evaluation fails
    before = {k: v[0].copy() for k, v in b.obs.items()}
    res = b.local_ba(0, _graph(len(sc["poses"])), prune=True)
    assert res["termination"] == 2 and ctx.calls == 1 and res["pruned"]["pairs"] == []
    assert all(np.array_equal(before[k], b.obs[k][0]) for k in before)


@pytest.mark.parametrize("which", range(len(pr.BA_SCENES)))
def test_no_residual_of_the_first_solve_lies_at_the_threshold(which):
    """the condition the GPU test rests on: then the device and the reference flag the same rows"""
    ref = pr.pruned_reference(which)
    assert np.min(np.abs(ref["r2"] - 0.15 * 0.15)) > 1e-6


def test_ba_prune_needs_local_ba(pkg):
    with pytest.raises(pkg.MslamHipError) as e:
        pkg.HipKeyframeTracker(None, local_map_depth=2, ba_prune=True)
    assert e.value.code == pkg.E_INVALID
