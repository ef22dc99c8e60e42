"""The host rule of the track-morph streams (include/world_class_track_morph.h, wc_track_morph) restated in plain Python / numpy:
which frames a push forms and from which entry, the flush, and the ring's numbering.  The frames themselves are delegated to
tests/morph_rule.morph.  A helper of tests/test_track_morph_rule.py and tests/test_gpu_track_morph.py, not a test module.

Per stream with delay D: n rows received.  A push of c rows with c positions: row i (since the reset) with i >= D forms frame
t = i - D from A's row t and the track at the entry of row i; after the push the rows max(n - D, 0) .. n - 1 wait.  The flush takes
K = min(D + 1, n) entries for the rows n - K .. n - 1 and forms the frames max(n - D, 0) .. n - 1 from the last min(D, n) of them.
Every row that is ever kept takes the next number of a sequence and sits in slot number % cap, cap = max_delay + min(max_delay,
max_frames)."""
import numpy as np

import morph_rule as mr


def ring_cap(max_delay, max_frames):
    return max_delay + min(max_delay, max_frames)


class Stream:
    def __init__(self, delay, max_delay=None, max_frames=1):
        self.delay = int(delay)
        self.cap = ring_cap(self.delay if max_delay is None else max_delay, max_frames)
        self.n = 0          # rows received
        self.seq = 0        # number of the oldest row that waits
        self.ended = False

    def formed(self):
        """frames formed so far = the first row that still waits"""
        return self.n if self.ended else max(self.n - self.delay, 0)

    def pending(self):
        return self.n - self.formed()

    def held(self):
        """{row: slot} of the rows that wait"""
        k = self.formed()
        return {r: (self.seq + r - k) % self.cap for r in range(k, self.n)}

    def count(self, c):
        """frames_out of a push of c rows"""
        return max(self.n + c - self.delay, 0) - max(self.n - self.delay, 0)

    def push(self, c):
        """c rows arrive.  Returns (frames, keeps): frames [(t, source, entry)], source ("push", row of the push) or ("ring", slot),
        entry the index among the push's positions; keeps [(row of the push, slot)]"""
        assert not self.ended and c >= 0
        old_n, old_keep, held = self.n, self.formed(), self.held()
        self.n += c
        keep = self.formed()
        frames = [(t, ("push", t - old_n) if t >= old_n else ("ring", held[t]), t + self.delay - old_n) for t in range(old_keep, keep)]
        fresh = self.seq + (old_n - old_keep)  # the next unused number
        self.seq = self.seq + (keep - old_keep) if keep < old_n else fresh
        keeps = [(r - old_n, (self.seq + r - keep) % self.cap) for r in range(max(keep, old_n), self.n)]
        return frames, keeps

    def flush(self):
        """Returns (frames, K): frames [(t, ("ring", slot), entry among the stream's K tail entries)]"""
        assert not self.ended and self.delay > 0 and self.n > 0
        k, held = self.formed(), self.held()
        K = min(self.delay + 1, self.n)
        c = self.n - k
        frames = [(t, ("ring", held[t]), K - c + (t - k)) for t in range(k, self.n)]
        self.seq += c
        self.ended = True
        return frames, K


def consumed(positions, tail, delay):
    """the entry every frame 0 .. n - 1 consumes: the pushed positions from row `delay` on, then the last min(delay, n) of the tail
    (tail: K = min(delay + 1, n) doubles, or None when delay == 0)"""
    positions = np.asarray(positions, dtype=np.float64)
    n = len(positions)
    if delay == 0:
        return positions.copy()
    tail = np.asarray(tail, dtype=np.float64)
    assert len(tail) == min(delay + 1, n)
    return np.concatenate([positions[delay:], tail[len(tail) - min(delay, n):]])


def drive(a, b, positions, cuts, delay, tail=None, settings=None, max_delay=None, max_frames=None, stale=np.nan):
    """All rows of the voice a = (f0, sp, ap) through one stream onto the track b, cut into pushes of the sizes in cuts, then (with
    delay > 0 and rows) the flush at `tail`.  The rows that wait go through a ring of cap slots that starts out full of `stale`
    and is written only by the keeps.  settings(k) -> (weight, f0_weight) of call k (the flush is call len(cuts)); None: (0, 0).
    Returns a list per call of (f0, sp, ap) of the frames formed, each frame morph_rule.morph at pos_a = t."""
    a = tuple(np.asarray(v, dtype=np.float64) for v in a)
    positions = np.asarray(positions, dtype=np.float64)
    assert sum(cuts) == len(a[0]) == len(positions)
    s = Stream(delay, max_delay, max(cuts) if max_frames is None else max_frames)
    ring = [np.full((s.cap,) + v.shape[1:], stale) for v in a]
    out, o = [], 0

    def form(k, frames, rows, entries):
        w, wf = (0.0, 0.0) if settings is None else settings(k)
        m = len(frames)
        if m == 0:
            return tuple(v[:0].copy() for v in a)
        src = tuple(np.array([rows[q][i] if kind == "push" else ring[q][i] for _, (kind, i), _ in frames]).reshape((m,) + a[q].shape[1:]) for q in range(3))
        # (morph at pos_a = arange(m) on the m rows the frames use is morph at pos_a = t on all rows: a whole position reads one row)
        return mr.morph(src, b, np.arange(m, dtype=np.float64), np.array([entries[e] for _, _, e in frames]), np.full(m, w), np.full(m, wf))

    for k, c in enumerate(cuts):
        rows = tuple(v[o:o + c] for v in a)
        frames, keeps = s.push(c)
        assert len(frames) == max(o + c - delay, 0) - max(o - delay, 0)
        res = form(k, frames, rows, positions[o:o + c])
        for r, slot in keeps:  # (behind the frames: no frame of this push reads a slot this push writes)
            for q in range(3):
                ring[q][slot] = rows[q][r]
        out.append(res)
        o += c
    if delay > 0 and s.n > 0:
        frames, K = s.flush()
        assert len(np.atleast_1d(tail)) == K
        out.append(form(len(cuts), frames, None, np.asarray(tail, dtype=np.float64)))
    return out


def cuttings(n, patterns=((1,), (6,), (0, 1, 6), (3, 0, 5, 1))):
    """push sizes that feed n rows along each cycled pattern"""
    res = []
    for pat in patterns:
        cuts, left, k = [], n, 0
        while left:
            c = min(pat[k % len(pat)], left)
            cuts.append(c)
            left -= c
            k += 1
        res.append(cuts)
    return res
