"""CPU tests that pin the rule of the settled positions (tests/align_lag_rule.py, the checker of tests/test_gpu_align_lag.py)
against the whole call's rule (tests/align_ex_rule.py): for an unwindowed stream the settled position of row i is b_on_a[max(i - L,
0)] of the whole call on rows 0..i with an open end, and the tail is the end of b_on_a on all rows, bit for bit; nothing depends
on how the rows are cut into pushes; a window over the whole track changes nothing; integer costs make every tie; a NaN row; lag 0
is the position; and a path never leaves the cells its stream computed, however narrow the window."""
import numpy as np
import pytest

import align_ex_rule as aex
import align_lag_rule as alr
import align_stream_rule as asr
import align_window_rule as awr
from align_rule import local_costs

N = 40
LAGS = [1, 2, 5, 39, 40, 60]
_prefix = {}


def _voice(m, dims=6):
    rng = np.random.default_rng(7000 + m)
    return rng.standard_normal((N, dims)), rng.standard_normal((m, dims))


def _prefixes(key, open_begin, costs):
    """b_on_a of the whole call with an open end on every prefix of the cost matrix: made once per key"""
    k = (key, open_begin)
    if k not in _prefix:
        flags = (aex.OPEN_BEGIN if open_begin else 0) | aex.OPEN_END
        _prefix[k] = [aex.align(None, None, 0, 0, flags=flags, costs=costs[:i + 1]) for i in range(len(costs))]
    return _prefix[k]


def _check_against_the_whole_call(costs, key, open_begin, lag, base):
    refs = _prefixes(key, open_begin, costs)
    f = alr.LagFollower(base, lag)
    pos, cost, settled = f.push_costs(costs)
    for i, ref in enumerate(refs):
        assert cost[i].tobytes() == np.float64(ref["cost"]).tobytes()
        if np.isfinite(ref["cost"]):
            assert pos[i] == ref["span"][1]
            assert settled[i].tobytes() == ref["b_on_a"][max(i - lag, 0)].tobytes(), (i, lag)
        else:
            assert np.isnan(pos[i]) and np.isnan(settled[i])
    k = min(lag + 1, len(costs))
    if np.isfinite(refs[-1]["cost"]):
        assert f.tail().tobytes() == refs[-1]["b_on_a"][-k:].tobytes()
    else:
        assert np.isnan(f.tail()).all() and len(f.tail()) == k
    return pos, cost, settled


@pytest.mark.parametrize("lag", LAGS)
@pytest.mark.parametrize("open_begin", [False, True])
@pytest.mark.parametrize("m", [1, 2, 9, 33])
def test_settled_is_the_whole_calls_b_on_a_on_every_prefix(m, open_begin, lag):
    a, b = _voice(m)
    costs = local_costs(a, b, 1, 6)
    _check_against_the_whole_call(costs, ("rows", m), open_begin, lag, asr.Follower(m=m, open_begin=open_begin))


@pytest.mark.parametrize("lag", LAGS)
@pytest.mark.parametrize("open_begin", [False, True])
@pytest.mark.parametrize("m", [1, 2, 9, 33])
def test_certain_ties(m, open_begin, lag):
    """integer-valued costs of 0 to 2: Dd == Du == Dl occurs, and the scan meets equal minima"""
    costs = np.random.default_rng(7100 + m).integers(0, 3, (N, m)).astype(np.float64)
    _check_against_the_whole_call(costs, ("ties", m), open_begin, lag, asr.Follower(m=m, open_begin=open_begin))
    if m >= 9:  # the ties are there: neighbours of a row of D are equal
        f = asr.Follower(m=m, open_begin=open_begin)
        f.push_costs(costs[:N - 1])
        prev = np.array(f.state)
        assert (prev[:-1] == prev[1:]).any()


@pytest.mark.parametrize("lag", LAGS)
@pytest.mark.parametrize("open_begin", [False, True])
@pytest.mark.parametrize("m", [1, 2, 9, 33])
def test_a_window_over_the_whole_track_gives_the_unwindowed_settled_values(m, open_begin, lag):
    a, b = _voice(m)
    costs = local_costs(a, b, 1, 6)
    for width, back, hop in ((m, 0, 1), (m + 5, min(3, m - 1), 3), (m, m - 1, 64)):
        base = awr.WindowFollower(m=m, open_begin=open_begin, width=width, back=back, hop=hop)
        _check_against_the_whole_call(costs, ("rows", m), open_begin, lag, base)


@pytest.mark.parametrize("cuts", [[1] * N, [N], [7, 0, 33], [39, 1], [1, 39], [10, 10, 10, 10]])
def test_the_result_does_not_depend_on_the_pushes(cuts):
    a, b = _voice(33)
    wins = [None, (6, 2, 1, False), (6, 2, 4, True), (9, 0, 7, False), (33, 32, 64, True), (3, 1, 3, False)]
    for open_begin in (False, True):
        for k, win in enumerate(wins):
            lag = LAGS[k]
            want_tail, got_tail = [], []
            want = alr.follow(a, b, 1, 6, open_begin, lag, win, tails=want_tail)
            got = alr.follow(a, b, 1, 6, open_begin, lag, win, cuts, tails=got_tail)
            for g, w in zip(got, want):
                assert g.tobytes() == w.tobytes(), (open_begin, win, lag)
            assert got_tail[-1].tobytes() == want_tail[-1].tobytes()
            plain = asr.follow(a, b, 1, 6, open_begin) if win is None else awr.follow(a, b, 1, 6, open_begin, *win)
            assert got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes()  # the lag changes neither


@pytest.mark.parametrize("open_begin", [False, True])
def test_the_tail_behind_every_push_is_the_whole_calls(open_begin):
    a, b = _voice(9)
    costs = local_costs(a, b, 1, 6)
    refs = _prefixes(("rows", 9), open_begin, costs)
    for lag in LAGS:
        f = alr.LagFollower(asr.Follower(m=9, open_begin=open_begin), lag)
        for i in range(N):
            f.push_costs(costs[i:i + 1])
            k = min(lag + 1, i + 1)
            assert f.tail().tobytes() == refs[i]["b_on_a"][-k:].tobytes(), (lag, i)


def test_lag_zero_is_the_position():
    a, b = _voice(33)
    for win in (None, (6, 2, 4, True)):
        pos, cost, settled = alr.follow(a, b, 1, 6, True, 0, win)
        assert settled.tobytes() == pos.tobytes()


@pytest.mark.parametrize("open_begin", [False, True])
def test_a_nan_row_in_the_middle_of_a_voice(open_begin):
    """no cell wins in or behind a NaN row (tests/test_align_window_rule.py): settled is NaN from there on and so is the tail; the
    rows before it are the whole call's.  A NaN row of the TRACK leaves the columns in front of it alone: the voice goes on"""
    a, b = _voice(9)
    a = a.copy()
    a[17] = np.nan
    with np.errstate(invalid="ignore"):
        costs = local_costs(a, b, 1, 6)
    for lag in (1, 5, 60):
        pos, cost, settled = _check_against_the_whole_call(costs, "nan_a", open_begin, lag, asr.Follower(m=9, open_begin=open_begin))
        assert not np.isnan(settled[:17]).any() and np.isnan(settled[17:]).all()
    a, b = _voice(9)
    b = b.copy()
    b[6] = np.nan
    with np.errstate(invalid="ignore"):
        costs = local_costs(a, b, 1, 6)
    for lag in (1, 5, 60):
        pos, cost, settled = _check_against_the_whole_call(costs, "nan_b", open_begin, lag, asr.Follower(m=9, open_begin=open_begin))
        assert not np.isnan(settled).any() and (pos[1:] < 6).all()


def test_a_path_never_leaves_the_cells_its_stream_computed():
    """consequence 5: the walks of align_lag_rule raise where they would read a choice that no row kernel stored.  Narrow windows
    that move every row, on voices that can and cannot be followed; and the settled positions, unlike the monotone positions, may fall"""
    voice, track, _ = awr.followable(0)
    rng = np.random.default_rng(7200)
    falls = 0
    for a in (voice, rng.standard_normal(voice.shape)):
        for win in ((2, 1, 1, False), (8, 3, 1, True), (24, 8, 8, True), (5, 4, 64, False)):
            for lag in (1, 10, 50):
                tails = []
                pos, cost, settled = alr.follow(a, track, 0, 8, True, lag, win, cuts=[50, 50, 50], tails=tails)
                ok = ~np.isnan(pos)
                assert ok.any() and not np.isnan(settled[ok]).any()
                assert (settled[ok] <= pos[ok]).all() and (settled[ok] * 2 == np.round(settled[ok] * 2)).all()
                falls += int((np.diff(settled[ok]) < 0).sum())
    assert falls > 0
