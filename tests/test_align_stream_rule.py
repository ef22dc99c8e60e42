"""CPU tests that pin the rule of the alignment streams (tests/align_stream_rule.py, the checker of tests/test_gpu_align_stream.py)
to the rule of the whole-utterance call (tests/align_ex_rule.py): at every row i the stream's cost is the cost of
align(a[:i + 1], b, pattern 0, band 0, flags | OPEN_END) bit for bit and its position is span[1] where that total is finite and NaN
exactly where it is not -- for random rows, integer-valued cost matrices with ties, rows of NaN / inf, both flags -- and nothing
depends on how the rows are cut into pushes."""
import numpy as np
import pytest

import align_ex_rule as ax
import align_stream_rule as asr

SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (7, 40), (40, 7), (23, 31), (40, 40)]


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _assert_prefixes(pos, cost, whole):
    """whole(i): align_ex_rule's dict for rows 0..i"""
    for i in range(len(pos)):
        r = whole(i)
        if np.isnan(r["cost"]):
            assert np.isnan(cost[i]), i
        else:
            assert _bits(cost[i]) == _bits(r["cost"]), (i, cost[i], r["cost"])
        if np.isfinite(r["cost"]):
            assert pos[i] == float(r["span"][1]), (i, pos[i], r["span"])
        else:
            assert np.isnan(pos[i]), (i, pos[i])


@pytest.mark.parametrize("open_begin", [False, True])
@pytest.mark.parametrize("n,m", SHAPES)
def test_random_rows_equal_the_whole_call_at_every_prefix(n, m, open_begin):
    rng = np.random.default_rng(1000 * n + m)
    a, b = rng.standard_normal((n, 6)), rng.standard_normal((m, 6))
    pos, cost = asr.follow(a, b, 1, 6, open_begin)
    flags = (ax.OPEN_BEGIN if open_begin else 0) | ax.OPEN_END
    _assert_prefixes(pos, cost, lambda i: ax.align(a[:i + 1], b, 1, 6, 0, 0, flags))
    assert np.isfinite(cost).all() and not np.isnan(pos).any()


@pytest.mark.parametrize("open_begin", [False, True])
def test_integer_costs_with_ties_equal_the_whole_call_at_every_prefix(open_begin):
    """costs of 0 to 2: every comparison of the rule meets equal operands somewhere, and the open-end scan meets equal minima"""
    rng = np.random.default_rng(77 + open_begin)
    flags = (ax.OPEN_BEGIN if open_begin else 0) | ax.OPEN_END
    ties = 0
    for n, m in SHAPES + [(11, 5), (5, 11)]:
        d = rng.integers(0, 3, (n, m)).astype(np.float64)
        f = asr.Follower(m=m, open_begin=open_begin)
        pos, cost = f.push_costs(d)
        _assert_prefixes(pos, cost, lambda i: ax.align(None, None, 0, 0, 0, 0, flags, costs=d[:i + 1]))
        ties += int(m > 1 and open_begin and (d[0] == d[0].min()).sum() > 1)
        assert f.rows == n
    assert not open_begin or ties > 0


@pytest.mark.parametrize("open_begin", [False, True])
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_rows_that_are_not_finite(open_begin, bad):
    """after a row that is not finite no cell ever wins again: the position is NaN from there on.  The cost of a NaN row is NaN; the
    rows behind it take the left step from +inf (both comparisons with NaN fail), so their cost is +inf, as behind an inf row"""
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal((12, 4)), rng.standard_normal((9, 4))
    a[5] = bad
    pos, cost = asr.follow(a, b, 0, 4, open_begin)
    flags = (ax.OPEN_BEGIN if open_begin else 0) | ax.OPEN_END
    _assert_prefixes(pos, cost, lambda i: ax.align(a[:i + 1], b, 0, 4, 0, 0, flags))
    assert np.isfinite(cost[:5]).all() and not np.isnan(pos[:5]).any()
    assert np.isnan(pos[5:]).all()
    assert np.isnan(cost[5]) if np.isnan(bad) else cost[5] == np.inf
    assert (cost[6:] == np.inf).all()


def test_a_track_row_that_is_not_finite_blocks_its_column_only():
    rng = np.random.default_rng(6)
    a, b = rng.standard_normal((10, 4)), rng.standard_normal((8, 4))
    b[3, 2] = np.inf
    for open_begin in (False, True):
        pos, cost = asr.follow(a, b, 0, 4, open_begin)
        flags = (ax.OPEN_BEGIN if open_begin else 0) | ax.OPEN_END
        _assert_prefixes(pos, cost, lambda i: ax.align(a[:i + 1], b, 0, 4, 0, 0, flags))
        assert (pos != 3.0).all() and np.isfinite(cost).all()


def test_coefficients_outside_the_window_are_not_read():
    rng = np.random.default_rng(7)
    a, b = rng.standard_normal((9, 8)), rng.standard_normal((13, 8))
    want = asr.follow(a, b, 2, 6)
    a[:, :2], a[:, 6:], b[:, :2], b[:, 6:] = np.nan, np.inf, -np.inf, np.nan
    got = asr.follow(a, b, 2, 6)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


@pytest.mark.parametrize("cuts", [[1] * 30, [30], [7, 0, 23], [29, 1], [1, 29], [10, 10, 10]])
def test_the_result_does_not_depend_on_the_pushes(cuts):
    rng = np.random.default_rng(8)
    a, b = rng.standard_normal((30, 5)), rng.standard_normal((17, 5))
    for open_begin in (False, True):
        want, got = asr.follow(a, b, 1, 5, open_begin), asr.follow(a, b, 1, 5, open_begin, cuts)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


def test_an_open_beginning_finds_a_phrase_inside_the_track():
    """rows 20..29 of the track pushed as the voice: cost 0.0 and position 20 + i at every row, known without either rule"""
    b = np.random.default_rng(9).standard_normal((40, 5))
    pos, cost = asr.follow(b[20:30], b, 0, 5, True)
    assert (cost == 0.0).all() and pos.tolist() == [20.0 + i for i in range(10)]
