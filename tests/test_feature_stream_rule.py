"""CPU tests of THE rule of include/world_class_feature_stream.h as tests/feature_stream_rule.py states it: the bounded-state
recursion the kernels run equals the definition (features_rule.pack on every prefix) bit for bit, on contours written to reach
every branch -- and the recursion's own trace says that they did; the counts; consequences 4, 5 and 7 with the converse of 7; the
place and the size of the step of point 8."""
import functools

import numpy as np
import pytest

import feature_stream_rule as fs
import features_rule as fr

ND, N_AP, FILL = 3, 2, -3.25
LAGS = [0, 1, 2, 5, 64]


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@functools.lru_cache(maxsize=None)
def case(name, lag, ring):
    """F0, supplied logs (not numpy's: any finite values do, so seeded noise), coded rows of one contour"""
    v = fs.contours(lag, ring)[name]
    rng = np.random.default_rng(len(name) * 1000 + lag)
    n = len(v)
    f0 = fs.f0_of(v, rng)
    logs = rng.uniform(4.0, 6.5, n)   # read on the voiced rows alone
    sp, ap = rng.standard_normal((n, ND)), -rng.uniform(0.0, 40.0, (n, N_AP))
    if name == "NaN, 0, negative and +inf":
        assert np.isnan(f0).any() and (f0 == 0).any() and (f0 < 0).any() and np.isinf(f0).any()
        sp[4, 1], ap[6, 0] = np.nan, np.inf   # values that are not finite travel through
    return f0, logs, sp, ap


def random_cuts(n, rng, most):
    cuts = [0]
    while sum(cuts) < n:
        cuts.append(int(min(rng.integers(0, most + 1), n - sum(cuts))))
    return cuts + [0]


def check(name, lag, orders, max_rows, max_lag, cuts_of, trace):
    ring = fs.ring_rows(max_rows, max_lag)
    f0, logs, sp, ap = case(name, lag, ring)
    want = fs.by_prefixes(ND, N_AP, orders, lag, FILL, f0, sp, ap, logs)
    got, tail = fs.stream(ND, N_AP, orders, lag, FILL, f0, sp, ap, cuts_of(len(f0)), logs, max_rows, max_lag, trace)
    assert _same(np.concatenate(got), want[0]) and _same(tail, want[1]), (name, lag, orders, max_rows, max_lag)
    assert len(want[0]) == max(len(f0) - lag, 0) and len(tail) == min(lag, len(f0))


NAMES = sorted(fs.contours(5, 14))


@pytest.mark.parametrize("lag", LAGS)
@pytest.mark.parametrize("orders", [1, 2, 3])
def test_the_recursion_equals_the_definition_bit_for_bit(orders, lag):
    """every contour in the smallest ring its lag allows, one row per push (max_lag = lag, max_rows_per_push = 1), and in pushes of
    up to 8 rows with zeros among them; what each contour is named for shows in the recursion's trace"""
    rng = np.random.default_rng(10 * lag + orders)
    for name in NAMES:
        small, wide = set(), set()
        check(name, lag, orders, 1, lag, lambda n: [1] * n, small)
        check(name, lag, orders, 8, lag, lambda n: random_cuts(n, rng, 8), wide)
        both = small | wide
        if name == "all unvoiced":
            assert "fill" in both and both <= {"fill", "the successor counts as 0.0", "the window wraps"}
        elif name == "a single voiced row":
            assert {"fill", "leading run", "voiced", "hold"} <= small and {"fill", "leading run", "voiced", "hold"} <= wide
            assert "interpolated" not in both
        elif name == "a leading run":
            assert {"fill", "leading run", "voiced"} <= small and "hold" not in both and "interpolated" not in both
        elif name == "a trailing run":
            assert {"voiced", "hold"} <= small and not both & {"fill", "leading run", "interpolated"}
        elif name == "runs of L - 1, L and L + 1":
            assert {"voiced", "hold", "interpolated"} <= small and {"voiced", "hold", "interpolated"} <= wide
            assert "a voiced row beyond the prefix is not seen" in wide   # (one row per push has no row beyond the prefix in its ring)
            assert "a voiced row beyond the prefix is not seen" not in small
        elif name == "a run longer than the ring":
            for t in (small, wide):
                assert {"left end is the carried record", "the carried record advances", "hold", "interpolated", "the window wraps"} <= t
        elif name == "two runs inside one push":
            assert "interpolated" in both and "the carried record advances" in both
        else:
            assert {"interpolated", "voiced"} <= both
        assert ("the successor counts as 0.0" in small) and ("the successor counts as 0.0" in wide)   # lag 0, or the flush's last row


@pytest.mark.parametrize("lag", [0, 1, 2])
def test_the_smallest_handle(lag):
    """max_lag = 2 with max_rows_per_push = 1: a ring of four rows, at every lag it allows"""
    assert fs.ring_rows(1, 2) == 4
    for name in NAMES:
        for orders in (1, 3):
            trace = set()
            check(name, lag, orders, 1, 2, lambda n: [1] * n, trace)
        if name == "a run longer than the ring":
            assert "left end is the carried record" in trace and "the window wraps" in trace


def test_counts():
    assert [fs.emitted(t, 3) for t in range(7)] == [0, 0, 0, 0, 1, 2, 3]
    assert fs.emitted(5, 0) == 5 and fs.emitted(-1, 0) == -1 and fs.emitted(0, -1) == -1
    rng = np.random.default_rng(1)
    for lag in LAGS:
        for n in (0, 1, lag, lag + 1, lag + 9):
            f0, sp, ap = np.full(n, 100.0), np.zeros((n, ND)), np.zeros((n, N_AP))
            cuts = random_cuts(n, rng, 4)
            got, tail = fs.stream(ND, N_AP, 2, lag, FILL, f0, sp, ap, cuts, max_rows_per_push=4)
            done = 0
            for k, rows in zip(cuts, got):
                assert len(rows) == fs.emitted(done + k, lag) - fs.emitted(done, lag)
                done += k
            assert sum(len(r) for r in got) == fs.emitted(n, lag) and len(tail) == min(lag, n)   # a stream with no rows flushes nothing


def whole_call(orders, f0, logs, sp, ap):
    return fr.pack([len(f0)], ND, N_AP, orders, f0, sp, ap, FILL, logs=logs)


def test_consequence_4_a_lag_beyond_the_stream_is_the_whole_call():
    for name in NAMES:
        f0, logs, sp, ap = case(name, 5, 14)
        n = len(f0)
        for lag in (n, n + 3):
            got, tail = fs.stream(ND, N_AP, 3, lag, FILL, f0, sp, ap, [8] * (n // 8) + [n % 8], logs, 8, lag)
            assert sum(len(r) for r in got) == 0 and _same(tail, whole_call(3, f0, logs, sp, ap))


def test_consequence_5_lag_0_emits_each_row_as_the_last_of_its_prefix():
    f0, logs, sp, ap = case("runs of L - 1, L and L + 1", 5, 14)
    for orders in (1, 2, 3):
        got, tail = fs.stream(ND, N_AP, orders, 0, FILL, f0, sp, ap, [1] * len(f0), logs)
        assert len(tail) == 0
        cols, _ = fr.columns(ND, N_AP, orders)
        for i, row in enumerate(np.concatenate(got)):
            assert _same(row, whole_call(orders, f0[:i + 1], logs[:i + 1], sp[:i + 1], ap[:i + 1])[i])
            if orders > 1 and i > 0:   # the successor counts as 0.0
                x, xm = sp[i, 0], sp[i - 1, 0]
                assert row[cols[0][1]] == 0.5 * (0.0 - xm)
                assert orders < 3 or row[cols[0][2]] == (xm + 0.0) - 2.0 * x


@pytest.mark.parametrize("lag", [1, 2, 5, 64])
def test_consequence_7_and_its_converse(lag):
    """runs all shorter than L, the leading one included, and a trailing run of any length: every row equals the whole call, none
    left out.  A run of 2 L: the frames more than L before its far end hold, and differ from the whole call -- the stream does not
    look ahead"""
    rng = np.random.default_rng(lag)
    lengths = [g for g in (lag - 1, 1, lag - 1, max(lag // 2, 1)) if 0 < g < lag]
    v = fs.runs(sum(lengths) + 2 * len(lengths) + 4 * lag + 12, lengths, first=lag + 1)
    v[:lag - 1] = False            # the leading run counts: L - 1 rows
    v[len(v) - 2 * lag - 3:] = False   # the trailing run does not
    assert v[lag - 1] and v.any()
    n = len(v)
    f0, logs = fs.f0_of(v, rng), rng.uniform(4.0, 6.5, n)
    sp, ap = rng.standard_normal((n, ND)), rng.standard_normal((n, N_AP))
    for orders in (1, 2, 3):
        got, tail = fs.stream(ND, N_AP, orders, lag, FILL, f0, sp, ap, random_cuts(n, rng, 8), logs, 8, lag)
        rows = np.concatenate(got + [tail])
        assert len(rows) == n and _same(rows, whole_call(orders, f0, logs, sp, ap)), orders
    # the converse
    a = 4
    v = fs.runs(2 * lag + 12, [2 * lag], first=a)
    b = a + 2 * lag + 1            # the far end
    assert v[a] and v[b] and not v[a + 1:b].any()
    n = len(v)
    f0, logs = fs.f0_of(v, rng, odd=False), rng.uniform(4.0, 6.5, n)
    sp, ap = rng.standard_normal((n, ND)), rng.standard_normal((n, N_AP))
    got, tail = fs.stream(ND, N_AP, 3, lag, FILL, f0, sp, ap, random_cuts(n, rng, 8), logs, 8, lag)
    rows, whole = np.concatenate(got + [tail]), whole_call(3, f0, logs, sp, ap)
    lf0 = 3 * ND
    early = np.arange(a + 1, b - lag)          # more than L before the far end
    assert len(early) == lag and np.array_equal(rows[early, lf0], np.full(lag, logs[a]))
    assert (rows[early, lf0] != whole[early, lf0]).all()
    late = np.arange(b - lag, n)
    assert np.array_equal(rows[late, lf0], whole[late, lf0])


@pytest.mark.parametrize("lag", [1, 2, 5, 64])
def test_point_8_the_step_of_a_long_run(lag):
    """a run whose far end lies g > L frames behind its last voiced frame: the step falls at the frame L before the far end, its
    size is (g - L) / g of the difference of the two logs, and that frame's deltas are the deltas of its own prefix"""
    rng = np.random.default_rng(100 + lag)
    for g in (lag + 1, lag + 2, 2 * lag + 7):
        a = 3
        b = a + g
        v = fs.runs(b + lag + 6, [g - 1], first=a)
        n = len(v)
        f0, logs = fs.f0_of(v, rng, odd=False), rng.uniform(4.0, 6.5, n)
        sp, ap = rng.standard_normal((n, ND)), rng.standard_normal((n, N_AP))
        got, tail = fs.stream(ND, N_AP, 3, lag, FILL, f0, sp, ap, random_cuts(n, rng, 8), logs, 8, lag)
        rows, whole = np.concatenate(got + [tail]), whole_call(3, f0, logs, sp, ap)
        lf0, s = 3 * ND, b - lag
        assert a < s
        held = rows[a + 1:s, lf0]
        assert np.array_equal(held, np.full(s - a - 1, logs[a]))                    # before the step: the last voiced log
        assert np.array_equal(rows[s:, lf0], whole[s:, lf0])                        # from the step on: the whole call's
        step = rows[s, lf0] - (rows[s - 1, lf0] if s - 1 > a else logs[a])
        want = (g - lag) / g * (logs[b] - logs[a])
        assert abs(step - want) <= 1e-12 * max(abs(logs[a]), abs(logs[b]))
        # the deltas of frame s read the interpolated neighbour of its own prefix, not the held value emitted one frame earlier
        assert rows[s, lf0 + 1] == 0.5 * (whole[s + 1, lf0] - whole[s - 1, lf0])
        assert rows[s, lf0 + 2] == (whole[s - 1, lf0] + whole[s + 1, lf0]) - 2.0 * whole[s, lf0]
        assert _same(rows[s], whole[s])
