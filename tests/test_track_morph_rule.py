"""CPU tests of the track-morph streams' host rule (tests/track_morph_rule.py, the restatement of
include/world_class_track_morph.h): the frames over any cutting of the rows are morph_rule.morph on everything at pos_a = arange,
the flush's entries belong to the right rows, the slots a push writes never meet slots that are still held, and behind
tests/align_lag_rule.follow the positions consumed are that rule's settled values plus its tail."""
import numpy as np
import pytest

import align_lag_rule as al
import morph_rule as mr
import track_morph_rule as tm
from align_window_rule import followable

BINS = 5


def _voice(n, seed):
    """n rows of a small voice: F0 with unvoiced stretches, positive sp rows, ap rows in (0, 1)"""
    rng = np.random.default_rng(seed)
    f0 = rng.uniform(80.0, 300.0, n)
    f0[rng.uniform(size=n) < 0.3] = 0.0
    return f0, rng.uniform(1e-4, 1e-2, (n, BINS)), rng.uniform(0.01, 0.99, (n, BINS))


def _positions(n, m, seed):
    """whole, half-integer and arbitrary positions that fall, repeat and leave [0, m - 1], with a NaN and both infinities"""
    rng = np.random.default_rng(seed)
    pos = np.round(rng.uniform(-2.0, m + 1.0, n) * 2) / 2
    pos[::5] = rng.uniform(0.0, m - 1.0, len(pos[::5]))
    pos[3::7] = pos[2::7][:len(pos[3::7])]
    if n > 12:
        pos[[4, 9, 11]] = [np.nan, np.inf, -np.inf]
    return pos


def _settings(k):
    return mr.WEIGHTS[k % 8], mr.WEIGHTS[(k + 3) % 8]


def _cat(calls, q):
    return np.concatenate([c[q] for c in calls])


@pytest.mark.parametrize("delay", [0, 1, 3, 5])
@pytest.mark.parametrize("m", [1, 40])
def test_frames_over_any_cutting_equal_the_whole_morph(delay, m):
    n = 57
    a, b, pos = _voice(n, 10 + m), _voice(m, 20 + m), _positions(n, m, 30 + delay)
    tail = _positions(min(delay + 1, n), m, 40 + delay) if delay else None
    used = tm.consumed(pos, tail, delay)
    assert len(used) == n
    want = mr.morph(a, b, np.arange(n, dtype=np.float64), used, np.zeros(n) + 0.25, np.zeros(n) + 0.75)
    assert np.isnan(want[0]).any() and np.isfinite(want[0]).any()
    for cuts in tm.cuttings(n):
        calls = tm.drive(a, b, pos, cuts, delay, tail, settings=lambda k: (0.25, 0.75), max_delay=5, max_frames=6)
        assert len(calls) == len(cuts) + (1 if delay else 0)
        for q in range(3):
            assert np.array_equal(_cat(calls, q), want[q], equal_nan=True), (cuts[:4], q)
        # the count per call is arithmetic on counts alone
        at = np.cumsum([0] + cuts)
        assert [len(c[0]) for c in calls[:len(cuts)]] == [max(e - delay, 0) - max(s - delay, 0) for s, e in zip(at, at[1:])]


def test_each_frame_takes_the_settings_of_the_call_that_forms_it():
    n, m, delay = 23, 9, 3
    a, b, pos = _voice(n, 1), _voice(m, 2), _positions(n, m, 3)
    tail = _positions(4, m, 4)
    cuts = tm.cuttings(n, [(0, 1, 6)])[0]
    calls = tm.drive(a, b, pos, cuts, delay, tail, settings=_settings, max_delay=5, max_frames=6)
    w = np.concatenate([np.full(len(c[0]), _settings(k)[0]) for k, c in enumerate(calls)])
    wf = np.concatenate([np.full(len(c[0]), _settings(k)[1]) for k, c in enumerate(calls)])
    want = mr.morph(a, b, np.arange(n, dtype=np.float64), tm.consumed(pos, tail, delay), w, wf)
    assert len(set(w)) > 4
    for q in range(3):
        assert np.array_equal(_cat(calls, q), want[q], equal_nan=True)


@pytest.mark.parametrize("n,frames,first_entry", [(2, [0, 1], 0), (5, [0, 1, 2, 3, 4], 0), (6, [1, 2, 3, 4, 5], 1), (60, [55, 56, 57, 58, 59], 1)])
def test_flush_entries_belong_to_the_right_rows(n, frames, first_entry):
    """D = 5 at n < D, n = D, n = D + 1 and n >> D: the tail holds K = min(D + 1, n) entries for the rows n - K .. n - 1; the flush
    forms the rows that wait, and skips the first entry exactly when a push has formed its frame (n > D)"""
    D = 5
    s = tm.Stream(D, 5, 6)
    for c in tm.cuttings(n, [(6, 1, 0)])[0]:
        s.push(c)
    assert s.formed() == max(n - D, 0) and s.pending() == min(D, n)
    held = s.held()
    got, K = s.flush()
    assert K == min(D + 1, n)
    assert [t for t, _, _ in got] == frames and [e for _, _, e in got] == list(range(first_entry, K))
    # entry e of the tail is row n - K + e
    assert all(n - K + e == t for t, _, e in got)
    assert [slot for _, (kind, slot), _ in got] == [held[t] for t in frames] and all(kind == "ring" for _, (kind, _), _ in got)
    assert s.ended and s.pending() == 0 and s.formed() == n


@pytest.mark.parametrize("delay", [1, 3, 5])
@pytest.mark.parametrize("max_delay,max_frames", [(5, 6), (5, 2), (7, 200)])
def test_slots_of_a_push_never_meet_slots_still_held(delay, max_delay, max_frames):
    """what lets a failed push leave the last good state: the slots a push writes are disjoint from the slots the state before it
    holds (which its own frames read), the rows that wait are always where the numbering says, and never more than `delay`"""
    rng = np.random.default_rng(delay * 100 + max_frames)
    s = tm.Stream(delay, max_delay, max_frames)
    assert s.cap == max_delay + min(max_delay, max_frames)
    where = {}  # row -> slot, as written
    for _ in range(400):
        c = int(rng.integers(0, min(max_frames, 9) + 1))
        before, n0 = s.held(), s.n
        frames, keeps = s.push(c)
        written = [slot for _, slot in keeps]
        assert len(set(written)) == len(written) and not set(written) & set(before.values())
        assert all(0 <= slot < s.cap for slot in written)
        for t, (kind, i), e in frames:
            assert 0 <= e < c and (kind == "push" and i == t - n0 or kind == "ring" and where[t] == i)
        for r, slot in keeps:
            where[n0 + r] = slot
        now = s.held()
        assert len(now) == min(delay, s.n) <= delay and all(where[r] == slot for r, slot in now.items())
        assert len(set(now.values())) == len(now)


def test_row_index_modulo_cap_would_not_do():
    """the reason for the sequence numbering: with slot = row % cap a push of 6 rows at D = 5, cap = 10 lands on a held row"""
    held = {r % 10 for r in range(0, 5)}
    assert {r % 10 for r in range(6, 11)} & held


@pytest.mark.parametrize("lag", [1, 3])
def test_composed_with_the_alignment_rule_it_consumes_settled_plus_tail(lag):
    voice, track, _ = followable(0)
    voice, track = voice[:40], track[:70]
    n, m = len(voice), len(track)
    tails = []
    cuts = tm.cuttings(n, [(3, 0, 5, 1)])[0]
    _, _, settled = al.follow(voice, track, 0, 8, lag=lag, cuts=cuts, tails=tails)
    tail = tails[-1]
    assert len(tail) == lag + 1 and np.isfinite(settled).all()
    a, b = _voice(n, 5), _voice(m, 6)
    used = np.concatenate([settled[lag:], tail[1:]])
    assert np.array_equal(used, tm.consumed(settled, tail, lag))
    # frame t sits at the settled value reported with row t + lag: where row t lies on the path behind row t + lag
    for t in (0, 7, n - lag - 1):
        f = al.follower(track, 0, 8, lag=lag)
        f.push(voice[:t + lag + 1])
        assert used[t] == f.tail()[0]
    calls = tm.drive(a, b, settled, cuts, lag, tail, settings=_settings, max_delay=3, max_frames=5)
    w = np.concatenate([np.full(len(c[0]), _settings(k)[0]) for k, c in enumerate(calls)])
    wf = np.concatenate([np.full(len(c[0]), _settings(k)[1]) for k, c in enumerate(calls)])
    want = mr.morph(a, b, np.arange(n, dtype=np.float64), used, w, wf)
    for q in range(3):
        assert np.array_equal(_cat(calls, q), want[q], equal_nan=True)
