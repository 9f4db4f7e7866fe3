"""Window tracking, CPU side: tests/track_window_ref.py against tests/track_ref.py — a window equals S independent steps, the
window loop equals the frame-by-frame loop run with the same guess policy — and the proof that the inputs the GPU tests
share (tests/track_window_cases.py) produce the event kinds and positions they claim."""
import numpy as np
import pytest

import track_ref as tr
import track_window_cases as cases
import track_window_ref as twr


@pytest.fixture(scope="module")
def sequence(orc):
    seq = tr.make_sequence(seed=0)
    rows, trk = tr.run_reference(seq)
    return seq, rows, trk


def _same_step(a, b):
    assert np.array_equal(a["pairs"][0], b["pairs"][0]) and np.array_equal(a["pairs"][1], b["pairs"][1])
    assert np.array_equal(a["mask"], b["mask"])
    for k in ("n_matches", "n_correspondences", "n_inliers", "status", "tracked", "keyframe_required", "vote_best", "vote_best_count"):
        assert a[k] == b[k], k
    assert np.array_equal(a["vote_counts"], b["vote_counts"])
    if a["status"]:
        assert np.array_equal(a["R"], b["R"]) and np.array_equal(a["t"], b["t"])


def test_the_default_sequence_has_the_planted_events(sequence):
    seq, rows, trk = sequence
    tracked, inserted, switched = tr.summarize(rows)
    assert all(tracked) and inserted[:3] == [0, 6, 11] and switched == [25]
    r = tr.KeyframeTracker(cam=tr.CAM, **tr.SEQ_PARAMS)
    flags = []
    for f in cases.FAILURE_ORDER:
        fr = seq["frames"][f]
        o = r.process(fr["desc"], fr["xy"], fr["depth"])
        flags.append((o["tracked"], o["relocalized"], o["keyframe"]))
    assert [k for k, x in enumerate(flags) if x[2] >= 0] == [0, 6, 11]
    assert flags[13][:2] == (False, True) and flags[14][:2] == (True, False)


def test_a_window_equals_independent_steps(sequence):
    seq, rows, trk = sequence
    for name in ("at_last", "vote", "failure"):
        inp = cases.case_inputs(seq, rows, trk, name)
        steps, first, entry = cases.run_case_ref(inp)
        assert len(steps) == len(inp["frames"])
        events = []
        for s, fr in enumerate(inp["frames"]):
            alone = tr.track(fr["desc"], fr["xy"], fr["depth"], inp["store"], inp["ref"], inp["ids"], seed=inp["seed"] + s,
                             guess=inp["guess"], new_keyframe_min_landmarks=cases.KF_MIN)
            _same_step(steps[s], alone)
            events.append(twr.is_event(alone, len(inp["ids"]), inp["pos"]))
            if s == first and alone["entry"] is not None:
                assert entry is not None
                for k in ("desc", "world", "src", "kp"):
                    assert np.array_equal(entry[k], alone["entry"][k]), k
        assert first == (events.index(True) if True in events else len(events))
        assert (entry is not None) == (first < len(steps) and steps[first]["keyframe_required"])


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_the_planted_cases_produce_their_events(sequence, name):
    seq, rows, trk = sequence
    inp = cases.case_inputs(seq, rows, trk, name)
    steps, first, entry = cases.run_case_ref(inp)
    kinds = {s: cases.kind(st, len(inp["ids"]), inp["pos"]) for s, st in enumerate(steps)}
    assert first == inp["first"], (first, kinds)
    assert {s: k for s, k in kinds.items() if k} == inp["kinds"], kinds
    # a stopped window is the same up to its event
    short, first2, entry2 = cases.run_case_ref(inp, stop_at_event=True)
    assert first2 == first and len(short) == min(first + 1, len(steps)) and (entry is None) == (entry2 is None)


def test_the_ragged_and_small_inputs_are_what_they_claim(orc):
    for S, at in ((65, 64), (256, 255)):
        sc = cases.small_scene(S, at)
        fr = sc["frames"]
        assert len(fr) == S and all(x["depth"].shape == (48, 64) for x in fr) and len(sc["store"][0][0]) == 200
        assert len(fr[at]["desc"]) == 35 and min(len(x["desc"]) for k, x in enumerate(fr) if k != at) > 100
        if S == 65:                                    # (the 256-frame reference runs once, in the GPU test)
            steps, first, entry = twr.track_window([x["desc"] for x in fr], [x["xy"] for x in fr], [x["depth"] for x in fr],
                                                   sc["store"], 0, [0], 0, cam=sc["cam"], guess=sc["guess"])
            assert first == at and steps[at]["tracked"] and steps[at]["keyframe_required"] and entry is not None
            assert all(st["tracked"] and not st["keyframe_required"] for st in steps[:at])


@pytest.mark.parametrize("window", [1, 4, 32])
def test_the_window_loop_equals_the_frame_by_frame_loop_with_the_shared_guess(sequence, window):
    seq, rows, trk = sequence
    for order in (list(range(len(seq["frames"]))), cases.FAILURE_ORDER):
        fr = [seq["frames"][f] for f in order]
        w = twr.WindowTracker(cam=tr.CAM, **tr.SEQ_PARAMS)
        got = w.process_window([x["desc"] for x in fr], [x["xy"] for x in fr], [x["depth"] for x in fr], window)
        r = twr.SharedGuessTracker(window, cam=tr.CAM, **tr.SEQ_PARAMS)
        ref = [r.process(x["desc"], x["xy"], x["depth"]) for x in fr]
        assert len(got) == len(ref) == len(fr)
        for k in ("keyframe", "reference", "tracked", "relocalized", "n_inliers"):
            assert [o[k] for o in got] == [o[k] for o in ref], k
        assert all(np.array_equal(a["R"], b["R"]) and np.array_equal(a["t"], b["t"]) for a, b in zip(got, ref))
        assert w.ids == r.ids and all(np.array_equal(w.store[i][1], r.store[i][1]) for i in w.ids)
        if window == 1 and len(order) == len(rows):                     # window 1 is the frame-by-frame loop itself
            assert [o["reference"] for o in got] == [o["reference"] for o in rows]
            assert all(np.array_equal(a["R"], b["R"]) for a, b in zip(got, rows))
            assert w.discarded == 0 and w.window_calls == len(rows) - 1
        if window == 32 and len(order) == len(rows):
            assert w.window_calls < len(rows) / 2 and [f for f, o in enumerate(got) if o["keyframe"] >= 0] == [0, 6, 11, 30]
