"""Reference composition of window tracking (not a test): mslam_hip_track_window put together from tests/track_ref.py —
S independent track_ref.track calls against one store entry (seed + s, one shared guess, no insertion), the event rule, the
event frame's entry by track_ref.build_entry — and the process_window loop on track_ref.KeyframeTracker's state.  Shares no
code with the product."""
import numpy as np

import reloc_ref as rr
import track_ref as tr


def is_event(step, n_vote, ref_vote_pos):
    """the frame at which the front end's state would change: not tracked, a keyframe required, or the vote names another
    keyframe than the current reference (position ref_vote_pos of the vote list; -1: votes never count)"""
    return bool(not step["tracked"] or step["keyframe_required"]
                or (n_vote > 0 and ref_vote_pos >= 0 and step["vote_best"] != ref_vote_pos))


def track_window(descs, xys, depths, store, ref_id, vote_ids=(), ref_vote_pos=-1, cam=tr.CAM, factor=tr.FACTOR, ratio=0.7,
                 iterations=100, thr=5.0, seed=0, guess=None, min_matched_points=10, new_keyframe_min_landmarks=30, z_max=3.0,
                 want_keyframe=True, stop_at_event=False):
    """-> (steps = [track_ref.track's dict per frame, entry = None], first_event = the first event's index or S,
    entry = the event frame's new entry or None).  stop_at_event: frames behind the first event are not computed (the
    loop discards them anyway); steps then ends at the event."""
    S = len(descs)
    steps, first = [], S
    for s in range(S):
        st = tr.track(descs[s], xys[s], depths[s], store, ref_id, vote_ids, cam, factor, ratio, iterations, thr, seed + s, guess,
                      min_matched_points, new_keyframe_min_landmarks, z_max, want_keyframe=False)
        steps.append(st)
        if first == S and is_event(st, len(vote_ids), ref_vote_pos):
            first = s
            if stop_at_event:
                break
    entry = None
    if first < S and steps[first]["keyframe_required"] and want_keyframe:
        e = steps[first]
        entry = tr.build_entry(descs[first], e["xyz"], e["valid"], e["pairs"], e["mask"], store[ref_id][1], e["R"], e["t"], z_max)
    return steps, first, entry


class WindowTracker(tr.KeyframeTracker):
    """HipKeyframeTracker.process_window's loop: track_window on the next `window` frames with the current pose as the
    guess and seed + absolute frame index, accept the frames up to and including the first event, handle the event as
    KeyframeTracker.process does, continue behind it."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.window_calls = self.computed = self.discarded = 0

    def process_window(self, descs, xys, depths, window=16, stop_at_event=True):
        out, i, N = [], 0, len(descs)
        while i < N:
            if self.reference is None:
                out.append(self.process(descs[i], xys[i], depths[i]))
                i += 1
                continue
            ids = self.ids[-64:]
            pos = ids.index(self.reference) if self.reference in ids else -1
            S = min(window, N - i) if pos >= 0 else 1        # a reference outside the vote list: frame by frame
            seed0 = self.seed + self.frame
            steps, first, entry = track_window(descs[i:i + S], xys[i:i + S], depths[i:i + S], self.store, self.reference, ids, pos,
                                               self.cam, self.factor, self.ratio, self.iterations, self.thr, seed0,
                                               (self.R, self.t), self.min_matched_points, self.new_keyframe_min_landmarks,
                                               self.z_max, stop_at_event=stop_at_event)
            n_acc = min(first + 1, S)
            self.window_calls += 1
            self.computed += S
            self.discarded += S - n_acc
            for s in range(n_acc):
                st = steps[s]
                o = dict(tracked=st["tracked"], n_inliers=st["n_inliers"], keyframe=-1, relocalized=False)
                if st["tracked"]:
                    self.R, self.t = st["R"], st["t"]
                    if st["vote_best"] >= 0:
                        self.reference = ids[st["vote_best"]]
                    if s == first and entry is not None:
                        new_id = self.ids[-1] + 1
                        self.store[new_id] = (entry["desc"], entry["world"])
                        self.ids.append(new_id)
                        self.reference = o["keyframe"] = new_id
                else:
                    best = rr.relocalize(descs[i + s], xys[i + s], self.store, ids, self.cam, ratio=self.ratio,
                                         iterations=self.iterations, thr=self.thr, seed=seed0 + s,
                                         min_inliers=self.reloc_min_inliers)["best"]
                    if best >= 0:
                        self.reference, o["relocalized"] = ids[best], True
                o.update(R=np.array(self.R, copy=True), t=np.array(self.t, copy=True), reference=self.reference)
                out.append(o)
            self.frame += n_acc
            i += n_acc
        return out


class SharedGuessTracker(tr.KeyframeTracker):
    """KeyframeTracker run frame by frame, with process_window's guess policy stated on its own: the guess is the pose at
    the start of a run of at most `window` frames, and a run ends behind a frame that inserts a keyframe, changes the
    reference or fails."""

    def __init__(self, window, **kw):
        super().__init__(**kw)
        self.window, self.left, self.guess = window, 0, None

    def process(self, desc, xy, depth):
        if self.reference is None:
            return super().process(desc, xy, depth)
        if self.left == 0 or self.reference not in self.ids[-64:]:
            self.guess, self.left = (self.R, self.t), self.window
        pose, before = (self.R, self.t), self.reference
        self.R, self.t = self.guess                       # what the base class passes as the guess
        o = super().process(desc, xy, depth)
        if not o["tracked"]:                              # the pose stays the last tracked one, not the guess
            self.R, self.t = pose
            o["R"], o["t"] = np.array(self.R, copy=True), np.array(self.t, copy=True)
        self.left -= 1
        if not o["tracked"] or o["keyframe"] >= 0 or self.reference != before:
            self.left = 0
        return o
