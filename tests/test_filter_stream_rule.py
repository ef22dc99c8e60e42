"""CPU tests of the filter streams' rule (tests/filter_stream_rule.py, include/world_class_filter_stream.h): the bounded-state recursion
equals filter_rule.frame_filter bit for bit under every kind of cut, T and C are monotone, C(T(n, F)) <= n, the latency bound holds and
is reached, the minimal capacities leave no dead end, and three one-line mistakes are each caught."""
import math

import numpy as np
import pytest

import filter_rule as fr
import filter_stream_rule as fsr

# (fs, fft_size, frame_period_ms, n): hops 1, 1.5, 40, 64.49999999999999 (ties), 80 and 512 (the largest at 2048)
SETTINGS = ((8000, 512, 0.125, 37), (8000, 512, 0.1875, 41), (8000, 512, 5.0, 203), (22050, 512, 64.5 / 22.05, 330), (16000, 512, 5.0, 401),
            (48000, 2048, 512 / 48.0, 1290))
HOPS = (1.0, 1.5, 40.0, 64.49999999999999, 80.0, 512.0)
CUTS = ("one_sample", "rows_first", "samples_first", "random")


def test_the_settings_are_the_hops_the_issue_names():
    assert tuple(fr.hop(fp, fs) for fs, _, fp, _ in SETTINGS) == HOPS
    assert all(fr.accepts(fs, N, fp) for fs, N, fp, _ in SETTINGS)


_cases = {}


def case(setting, mode, kind, nan_row=None):
    """(x, rows, y of the whole call), computed once"""
    key = (setting, mode, kind, nan_row)
    if key not in _cases:
        fs, N, fp, n = setting
        x = np.random.default_rng(11 + n).normal(size=n)
        rows = fr.mode_rows("envelope" if kind == fr.POWER else "noise", mode, fr.segments(n, fp, fs), N, kind, seed=n)
        if nan_row is not None:
            rows[nan_row, 5] = np.nan
        _cases[key] = (x, rows, fr.frame_filter(x, rows, kind, fs, N, fp))
    return _cases[key]


@pytest.mark.parametrize("how", CUTS)
@pytest.mark.parametrize("mode", fr.ROW_MODES)
@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "hop%g" % fr.hop(s[2], s[0]))
def test_the_recursion_is_the_whole_call_bit_for_bit(setting, mode, how):
    fs, N, fp, n = setting
    for kind in (fr.POWER, fr.LOG):
        x, rows, want = case(setting, mode, kind)
        got = fsr.one_call(fs, N, fp, kind, x, rows, fsr.cut(how, n, len(rows), fp, fs, seed=n))
        assert got.shape == want.shape and np.array_equal(got, want), (kind, np.abs(got - want).max())


@pytest.mark.parametrize("how", CUTS + ("hop_and_row", "all_at_once"))
@pytest.mark.parametrize("setting", (SETTINGS[0], SETTINGS[2], SETTINGS[3]), ids=lambda s: "hop%g" % fr.hop(s[2], s[0]))
def test_a_nan_row_next_to_a_push_border(setting, how):
    """the N samples from a_2 are NaN and nothing else, and the rest is the whole call's bits (one_sample and hop_and_row put a push
    border on either side of every sample of the row's span)"""
    fs, N, fp, n = setting
    x, rows, want = case(setting, "exact", fr.LOG, nan_row=2)
    a2 = fr.span(2, n, fp, fs)[0]
    assert np.array_equal(np.isnan(want), (np.arange(n) >= a2) & (np.arange(n) < a2 + N)) and np.isnan(want).any()
    got = fsr.one_call(fs, N, fp, fr.LOG, x, rows, fsr.cut(how, n, len(rows), fp, fs, seed=3))
    assert np.array_equal(got, want, equal_nan=True)


def test_a_reset_stream_is_a_fresh_one_and_an_ended_one_takes_nothing():
    fs, N, fp, n = SETTINGS[2]
    x, rows, want = case(SETTINGS[2], "exact", fr.POWER)
    st = fsr.Stream(fs, N, fp, fr.POWER, n, len(rows))
    st.push(x[:150], rows[:3])
    assert st.T == 3 and st.C == 81 and np.abs(st.tail).max() > 0
    st.reset()
    assert (st.n, st.F, st.T, st.C) == (0, 0, 0, 0)
    got = np.concatenate([st.push(x[:99], rows[:1]), st.push(x[99:], rows[1:], flush=True)])
    assert np.array_equal(got, want)
    with pytest.raises(fsr.Refused, match="has ended"):
        st.push(x[:1])
    assert len(st.push(flush=True)) == 0 and st.pending_samples == 0 and st.pending_rows == 0


@pytest.mark.parametrize("h_setting", SETTINGS, ids=lambda s: "hop%g" % fr.hop(s[2], s[0]))
def test_counts_are_monotone_and_never_ahead_of_the_samples(h_setting):
    fs, _, fp, _ = h_setting
    h = fr.hop(fp, fs)
    top = int(6 * h) + 8
    T = np.array([[fsr.segments_done(n, F, fp, fs) for F in range(10)] for n in range(top)])
    C = np.array([[fsr.committed(t, fp, fs) for t in row] for row in T])
    assert (np.diff(T, axis=0) >= 0).all() and (np.diff(T, axis=1) >= 0).all()
    assert (np.diff(C, axis=0) >= 0).all() and (np.diff(C, axis=1) >= 0).all()
    assert (C <= np.arange(top)[:, None]).all() and (T <= np.arange(10)[None, :]).all()
    for n in range(top):
        for F in range(10):
            t = T[n, F]
            assert fr.centre(t, fp, fs) <= n and (t == F or fr.centre(t + 1, fp, fs) > n)      # the largest such T
            assert t <= fr.segments(n, fp, fs) if n else t == 0                                 # the flush has segments T .. S - 1 left


@pytest.mark.parametrize("fs,fp,bound", [(8000, 5.0, 78), (48000, 512 / 48.0, 1022), (22050, 64.5 / 22.05, 128), (8000, 0.125, 0), (8000, 0.1875, 2)])
def test_the_latency_bound_holds_and_is_reached(fs, fp, bound):
    assert fsr.latency_bound(fp, fs) == bound
    h = fr.hop(fp, fs)
    top = int(40 * h) + 5
    behind = [n - fsr.committed(fsr.segments_done(n, top, fp, fs), fp, fs) for n in range(top)]
    assert max(behind) <= bound
    if h == math.floor(h):
        assert max(behind) == bound         # an integer hop reaches it one sample in front of a centre
    assert bound < fsr.min_pending_samples(fp, fs)


@pytest.mark.parametrize("setting", SETTINGS[:5], ids=lambda s: "hop%g" % fr.hop(s[2], s[0]))
def test_minimal_capacities_leave_no_dead_end(setting):
    """max_pending_samples = 2 ceil(h), max_pending_rows = 1: from every state reachable by pushes of one sample or one row, one of
    the two is accepted (it makes progress: n or F grows), and a full sample window waits for rows"""
    fs, _, fp, _ = setting
    cap_s = fsr.min_pending_samples(fp, fs)
    top = int(5 * fr.hop(fp, fs)) + 3
    seen, todo, full = set(), [(0, 0)], 0
    while todo:
        n, F = todo.pop()
        if (n, F) in seen or n > top:
            continue
        seen.add((n, F))
        c = fsr.Counts(fs, fp, cap_s, 1)
        c.n, c.F = n, F
        c.T = fsr.segments_done(n, F, fp, fs)
        c.C = fsr.committed(c.T, fp, fs)
        assert 0 <= c.pending_samples <= cap_s and 0 <= c.pending_rows <= 1
        ok_s, ok_r = c.refusal(1, 0, 0) is None, c.refusal(0, 1, 0) is None
        assert ok_s or ok_r, (n, F)
        if c.pending_samples == cap_s:
            full += 1
            assert c.T == c.F and ok_r and not ok_s
        if c.pending_rows == 1:
            assert ok_s and not ok_r
        todo += [(n + 1, F)] * ok_s + [(n, F + 1)] * ok_r
    assert full > 0 and max(n for n, _ in seen) == top


def test_the_refusals_on_counts():
    c = fsr.Counts(8000, 5.0, 80, 2)
    assert c.refusal(-1, 0, 0) == fsr.NEGATIVE and c.refusal(0, -1, 0) == fsr.NEGATIVE
    assert c.refusal(81, 0, 0) == fsr.NO_FIT and c.refusal(0, 3, 0) == fsr.NO_FIT and c.refusal(80, 2, 0) is None
    assert c.refusal(5, 0, 1) == fsr.NO_ROW and c.refusal(0, 0, 1) is None and c.refusal(5, 1, 1) is None
    c.n = c.C = fsr.MAX_SAMPLES - 3
    assert c.refusal(4, 0, 0) == fsr.TOO_LONG and c.refusal(3, 0, 0) is None
    c.ended = True
    assert c.refusal(1, 0, 0) == fsr.ENDED and c.refusal(0, 1, 1) == fsr.ENDED and c.refusal(0, 0, 1) is None


@pytest.mark.parametrize("mistake", fsr.MISTAKES)
def test_each_one_line_mistake_is_caught(mistake):
    """hop 40 with a row per segment; the cut puts a push border on a centre (n == c_T: `<` waits a push longer and then lacks ...
    nothing, so the border case is held on the counts), resets in mid-stream, and gives two rows for five segments"""
    fs, N, fp, n = SETTINGS[2]
    x, rows, want = case(SETTINGS[2], "exact", fr.POWER)
    if mistake == "lt_for_le":
        assert fsr.segments_done(80, 9, fp, fs) == 2 and fsr.segments_done(80, 9, fp, fs, mistake) == 1
        st = fsr.Stream(fs, N, fp, fr.POWER, n, len(rows), mistake)
        assert len(st.push(x[:80], rows)) == 1 and len(fsr.Stream(fs, N, fp, fr.POWER, n, len(rows)).push(x[:80], rows)) == 41
    elif mistake == "tail_kept_at_reset":
        def run(m):
            st = fsr.Stream(fs, N, fp, fr.POWER, n, len(rows), m)
            st.push(x[::-1][:150], rows[:3])
            st.reset()
            return np.concatenate([st.push(x[:99], rows[:1]), st.push(x[99:], rows[1:], flush=True)])
        assert np.array_equal(run(None), want) and not np.array_equal(run(mistake), want)
    else:
        held = rows[:2]
        whole = fr.frame_filter(x, rows[:3], fr.POWER, fs, N, fp)      # the third row arrives late
        pushes = [(200, 2, 0), (3, 1, 1)]
        assert np.array_equal(fsr.one_call(fs, N, fp, fr.POWER, x, rows[:3], pushes), whole)
        got = fsr.one_call(fs, N, fp, fr.POWER, x, rows[:3], pushes, mistake=mistake)
        assert len(got) == len(whole) and not np.array_equal(got, whole)
        assert np.array_equal(fsr.one_call(fs, N, fp, fr.POWER, x, held, [(203, 2, 1)], mistake=mistake), fr.frame_filter(x, held, fr.POWER, fs, N, fp))
