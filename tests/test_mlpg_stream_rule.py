"""CPU tests of the MLPG stream's rule (tests/mlpg_stream_rule.py): the bounded-state recursion the kernels implement equals the
definition -- tests/features_rule.py's mlpg on every prefix -- bit for bit, whatever the cut into pushes; bad and infinite variances
behave as include/world_class_mlpg_stream.h states; the count E matches the library's; the lag / accuracy table of DESIGN.md."""
import numpy as np
import pytest

import features_rule as fr
import mlpg_stream_rule as ms

SHAPE = (5, 2)   # nd, n_ap: 8 static columns, lf0 and two bands among them
NS = [1, 2, 3, 4, 7, 40]
LAGS = [0, 1, 2, 3, 8, 64]


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def case(n, orders, seed):
    """means of unit scale, variances over four decades, 1e-2 .. 1e2"""
    rng = np.random.default_rng(seed)
    W = fr.width(*SHAPE, orders)
    return rng.standard_normal((n, W)), 10.0 ** rng.uniform(-2.0, 2.0, (n, W))


def cuts_of(n, rng, most):
    """a random cut of n rows into pushes of 0 .. most rows"""
    cuts = []
    while sum(cuts) < n:
        cuts.append(int(min(rng.integers(0, most + 1), n - sum(cuts))))
    return cuts + [0]


@pytest.mark.parametrize("orders", [2, 3])
@pytest.mark.parametrize("n", NS)
def test_the_recursion_is_the_definition_bit_for_bit(n, orders):
    nd, n_ap = SHAPE
    mean, var = case(n, orders, 100 * n + orders)
    rng = np.random.default_rng(n)
    for lag in LAGS:
        for per_frame, v in ((True, var), (False, var[0])):
            pushed, flushed = ms.by_prefixes(nd, n_ap, orders, lag, mean, v, per_frame)
            assert len(pushed) == ms.emitted(n, lag) and len(flushed) == min(lag, n)
            outs = None
            for cuts in ([1] * n, [n], [0, n, 0], cuts_of(n, rng, 3), cuts_of(n, rng, 8)):
                got, tail = ms.stream(nd, n_ap, orders, lag, mean, v, per_frame, cuts)
                o = 0
                for k, g in zip(cuts, got):   # every push writes E(T1) - E(T0) rows
                    assert len(g) == ms.emitted(o + k, lag) - ms.emitted(o, lag)
                    o += k
                got = np.concatenate(got)
                assert _same(got, pushed) and _same(tail, flushed), (lag, per_frame, cuts)
                assert outs is None or (_same(got, outs[0]) and _same(tail, outs[1]))   # invariant under the cut
                outs = (got, tail)
            assert np.isfinite(pushed).all() and np.isfinite(flushed).all()
            assert np.array_equal(np.concatenate([pushed, flushed])[:, nd + 1], mean[:, orders * (nd + 1)])   # vuv: the frame's own
            if lag >= n:   # nothing before the flush, and the flush is the whole call
                assert len(pushed) == 0
                assert _same(flushed, fr.mlpg([n], nd, n_ap, orders, mean, v, per_frame))


def test_the_ring_wraps():
    """a ring of 3 + 5 + 1 rows under 200 rows: slots are reused dozens of times"""
    nd, n_ap = SHAPE
    mean, var = case(200, 3, 7)
    want = ms.by_prefixes(nd, n_ap, 3, 5, mean, var, True)
    got, tail = ms.stream(nd, n_ap, 3, 5, mean, var, True, [3] * 66 + [2], max_rows_per_push=3, max_lag=5)
    assert _same(np.concatenate(got), want[0]) and _same(tail, want[1])


@pytest.mark.parametrize("orders", [2, 3])
def test_bad_and_infinite_variances(orders):
    """NaN, 0, -1, -inf in row j of a static column: every frame of that column emitted by rows >= j is NaN, the flush included,
    and nothing else moves; +inf drops the observation (its mean is not looked at); the vuv column's variance is not read"""
    nd, n_ap = SHAPE
    n, lag = 40, 3
    mean, var = case(n, orders, 11 + orders)
    cols, vuv_col = fr.columns(nd, n_ap, orders)
    ocols, S = ms.out_columns(nd, n_ap)
    clean, clean_tail = ms.stream(nd, n_ap, orders, lag, mean, var, True, [4] * 10)
    clean = np.concatenate(clean)
    spots = [(2, orders - 1, 30), (nd, 1, 0), (nd + 2, 0, n - 1)]   # (static column, its order, row)
    for bad in (np.nan, 0.0, -1.0, -np.inf):
        for c, k, j in spots:
            v = var.copy()
            v[j, cols[c][k]] = bad
            v[5, vuv_col] = bad
            got, tail = ms.stream(nd, n_ap, orders, lag, mean, v, True, [4] * 10)
            got = np.concatenate(got)
            want = ms.by_prefixes(nd, n_ap, orders, lag, mean, v, True)
            assert _same(got, want[0]) and _same(tail, want[1])
            hit = np.zeros(got.shape, dtype=bool)
            hit[max(j - lag, 0):, ocols[c]] = True   # row i emits frame i - lag
            assert np.isnan(got[hit]).all() and np.array_equal(got[~hit], clean[~hit])
            assert np.isnan(tail[:, ocols[c]]).all() and np.array_equal(np.delete(tail, ocols[c], axis=1), np.delete(clean_tail, ocols[c], axis=1))
    v, m2 = var.copy(), mean.copy()
    for c, k, j in spots:
        v[j, cols[c][k]] = np.inf
        m2[j, cols[c][k]] = np.nan
    got, tail = ms.stream(nd, n_ap, orders, lag, mean, v, True, [4] * 10)
    want = ms.by_prefixes(nd, n_ap, orders, lag, mean, v, True)
    assert _same(np.concatenate(got), want[0]) and _same(tail, want[1]) and np.isfinite(want[0]).all() and np.isfinite(tail).all()
    got2, tail2 = ms.stream(nd, n_ap, orders, lag, m2, v, True, [4] * 10)
    assert _same(np.concatenate(got2), np.concatenate(got)) and _same(tail2, tail)


def test_one_row_of_variances_may_change_from_push_to_push():
    """var_per_frame == 0 is the per-frame rule on that row repeated: a different row at every push is the per-frame call on the
    rows so repeated"""
    nd, n_ap = SHAPE
    mean, var = case(12, 3, 5)
    s = ms.Stream(nd, n_ap, 3, 2, max_rows_per_push=4)
    got = [s.push(mean[o:o + 4], var[o], False) for o in (0, 4, 8)]
    tail = s.flush()
    want = ms.by_prefixes(nd, n_ap, 3, 2, mean, np.repeat(var[[0, 4, 8]], 4, axis=0), True)
    assert _same(np.concatenate(got), want[0]) and _same(tail, want[1])


def test_emitted_matches_the_library():
    """the library builds on a machine without a GPU; the count is host arithmetic"""
    from world_class_amd import build
    build.build()
    from world_class_amd import mlpg_stream
    for rows in (0, 1, 2, 7, 64, 65, 2 ** 40):
        for lag in (0, 1, 5, 64, 2 ** 31 - 1):
            assert mlpg_stream.emitted(rows, lag) == ms.emitted(rows, lag) == max(rows - lag, 0)
    L = mlpg_stream._L()
    assert L.wc_mlpg_stream_emitted(-1, 0) == -1 == ms.emitted(-1, 0) and L.wc_mlpg_stream_emitted(3, -1) == -1 == ms.emitted(3, -1)
    with pytest.raises(ValueError):
        mlpg_stream.emitted(-1, 2)


def lag_table(lags=(4, 8, 16, 32, 64)):
    """400 frames, unit-scale means, variances (1, 0.1, 0.05) for static / delta / delta-delta, orders 3: the greatest difference
    between frame t from the prefix through t + L and the whole solve, as a share of max|c|"""
    nd, n_ap, n = 4, 0, 400
    rng = np.random.default_rng(2024)
    W = fr.width(nd, n_ap, 3)
    cols, vuv_col = fr.columns(nd, n_ap, 3)
    mean = rng.standard_normal((n, W))
    var = np.ones(W)
    for ks in cols:
        var[ks[1]], var[ks[2]] = 0.1, 0.05
    whole = fr.mlpg([n], nd, n_ap, 3, mean, var, False)
    out = {}
    for lag in lags:
        got, _ = ms.stream(nd, n_ap, 3, lag, mean, var, False, [8] * 50)
        got = np.concatenate(got)
        out[lag] = np.abs(got - whole[:len(got)]).max() / np.abs(whole).max()
    return out


def test_lag_accuracy_table():
    table = lag_table()
    for lag, err in table.items():
        print("mlpg stream, lag %3d: %.1e of max|c|" % (lag, err))
    assert table[64] < table[8] and table[64] < 1e-6
