"""CPU tests of the model-feature rule (tests/features_rule.py, the numpy statement of include/world_class_features.h): the
interpolation on hand-written contours, the deltas against np.correlate, MLPG against a dense solve of W^T P W, and MLPG of the
pack's own statics and deltas."""
import numpy as np
import pytest

import features_rule as fr

EPS = np.finfo(np.float64).eps
SIZES = [1, 2, 3, 4, 5, 64, 65, 257]


def test_interpolation_on_hand_written_contours():
    e = np.e
    lf0 = fr.continuous_lf0([0, 0, e, 0, 0, 0, e ** 3, 0], -7.0)
    want = np.array([1.0, 1.0, 1.0, (1 - 0.25) * 1.0 + 0.25 * np.log(e ** 3), 0.5 * 1.0 + 0.5 * np.log(e ** 3),
                     (1 - 0.75) * 1.0 + 0.75 * np.log(e ** 3), np.log(e ** 3), np.log(e ** 3)])
    assert np.array_equal(lf0, want)
    assert np.array_equal(fr.continuous_lf0([0.0, -1.0, np.nan, np.inf], -7.0), np.full(4, -7.0))   # nothing voiced: the fill
    assert np.array_equal(fr.voiced([0.0, -1.0, np.nan, np.inf, fr.DBL_MAX, 5e-324]), [False, False, False, False, True, True])
    assert np.array_equal(fr.continuous_lf0([100.0], 0.0), np.log([100.0]))
    assert np.array_equal(fr.continuous_lf0([0, 0, 200.0], 0.0), np.full(3, np.log(200.0)))         # one voiced frame, at the end
    assert np.array_equal(fr.continuous_lf0([200.0, 0, 0], 0.0), np.full(3, np.log(200.0)))         # at the start
    assert np.array_equal(fr.continuous_lf0([np.nan, 200.0, np.inf], 0.0), np.full(3, np.log(200.0)))
    # voiced frames are the logs bit for bit, and a gap between equal ends is flat to an ulp of (1 - a) l + a l
    f0 = np.array([110.0, 0, 0, 0, 0, 0, 0, 110.0, 220.0])
    lf0 = fr.continuous_lf0(f0, 0.0)
    assert lf0[0] == np.log(110.0) and lf0[7] == np.log(110.0) and lf0[8] == np.log(220.0)
    assert np.abs(lf0[1:7] - np.log(110.0)).max() <= 2 * EPS * np.log(110.0)
    # logs handed in (another library's) are used as they are
    assert np.array_equal(fr.continuous_lf0([3.0, 0, 5.0], 0.0, logs=[1.0, 99.0, 2.0]), [1.0, 1.5, 2.0])


@pytest.mark.parametrize("n", [1, 2, 3, 64, 257])
def test_deltas_equal_np_correlate(n):
    """D x: to the last bit -- np.correlate adds 0.5 x(t+1) and -0.5 x(t-1) and a zero, halving is exact and so the one rounding
    of the difference is the same.  np.correlate does not reverse its window: the one that gives 0.5 (x(t+1) - x(t-1)) is
    [-0.5, 0, 0.5]; with [0.5, 0, -0.5] it gives the negative, which is exact, so both are held to the last bit.
    DD x: within 1 ulp of the result's terms, because np.correlate sums x(t-1) - 2 x(t) + x(t+1) from the left where the rule adds
    the neighbours first: two roundings either way, of sums of magnitude <= 4 max|x|."""
    x = np.random.default_rng(100 + n).standard_normal(n) * 3.0
    d1, d2 = fr.deltas(x)
    # np.correlate's "same" is as long as the LONGER argument, the window's 3 for n < 3: there the zero padding "same" stands for
    # is written out, x padded by one zero either side and correlated in "valid" mode
    same = (lambda w: np.correlate(x, w, "same")) if n >= 3 else (lambda w: np.correlate(np.pad(x, 1), w, "valid"))
    assert np.array_equal(d1, same([-0.5, 0.0, 0.5]))
    assert np.array_equal(d1, -same([0.5, 0.0, -0.5]))
    assert np.abs(d2 - same([1.0, -2.0, 1.0])).max() <= 4.0 * np.abs(x).max() * EPS
    if n == 1:
        assert d1[0] == 0.0 and d2[0] == -2.0 * x[0]
    # columns are independent
    m = np.stack([x, -x, 2.0 * x], axis=1)
    e1, e2 = fr.deltas(m)
    assert np.array_equal(e1[:, 0], d1) and np.array_equal(e2[:, 2], 2.0 * d2)


def test_np_correlate_same_is_the_zero_padded_window():
    """the sign and centring the rule takes from np.correlate(mode="same")"""
    x = np.array([1.0, 4.0, 9.0, 16.0])
    assert np.array_equal(fr.deltas(x)[0], [2.0, 4.0, 6.0, -4.5])      # 0.5 (x(t+1) - x(t-1)), x outside as 0
    assert np.array_equal(np.correlate(x, [-0.5, 0.0, 0.5], "same"), [2.0, 4.0, 6.0, -4.5])
    assert np.array_equal(fr.deltas(x)[1], [2.0, 2.0, 2.0, -23.0])
    assert np.array_equal(np.correlate(x, [1.0, -2.0, 1.0], "same"), [2.0, 2.0, 2.0, -23.0])


def _case(n, orders, seed, cols=3):
    rng = np.random.default_rng(seed)
    mean = rng.standard_normal((n, orders, cols))
    var = 10.0 ** rng.uniform(-2.0, 2.0, (n, orders, cols))
    return mean, var


@pytest.mark.parametrize("orders", [2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_mlpg_against_a_dense_solve(n, orders):
    """variances over 1e-2 .. 1e2.  Normalised residual |R c - r| / (|R| |c| + |r|) <= 16 eps (infinity norms): the backward error
    of a banded SPD factorisation of half-bandwidth 2, with a constant to spare.  Against np.linalg.solve: 1e-11 of max|c|, the
    dense solve's own conditioning being the margin."""
    mean, var = _case(n, orders, 7 * n + orders)
    a0, a1, a2, r = fr.mlpg_system(mean, var)
    c = fr.mlpg_solve(a0, a1, a2, r)
    worst_res = worst_dense = 0.0
    for k in range(mean.shape[2]):
        R, rhs = fr.dense_system(mean[:, :, k], var[:, :, k])
        # the banded entries are the dense matrix's, to rounding
        band = np.diag(a0[:, k])
        for off, a in ((1, a1), (2, a2)):
            for t in range(n - off):
                band[t, t + off] = band[t + off, t] = a[t, k]
        assert np.abs(band - R).max() <= 8 * EPS * np.abs(R).max()
        assert np.abs(rhs - r[:, k]).max() <= 8 * EPS * (np.abs(rhs).max() + np.abs(1.0 / var[:, :, k]).max() * np.abs(mean[:, :, k]).max())
        res = np.abs(band @ c[:, k] - r[:, k]).max() / (np.abs(band).sum(1).max() * np.abs(c[:, k]).max() + np.abs(r[:, k]).max())
        dense = np.abs(c[:, k] - np.linalg.solve(R, rhs)).max() / np.abs(c[:, k]).max()
        worst_res, worst_dense = max(worst_res, res), max(worst_dense, dense)
    print("mlpg n %d orders %d: residual %.2f eps, against the dense solve %.2e" % (n, orders, worst_res / EPS, worst_dense))
    assert worst_res <= 16 * EPS
    assert worst_dense <= 1e-11


@pytest.mark.parametrize("orders", [2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_mlpg_of_its_own_pack_returns_the_statics(n, orders):
    """means = the pack's own statics and deltas, all variances equal: W c = mu has the statics as its exact solution up to the
    deltas' rounding, so MLPG returns them within cond(R) <= 1 + |D|^2 + |DD|^2 <= 18 times the residual bound: 1e-12 of max|x|"""
    nd, n_ap = 4, 2
    rng = np.random.default_rng(50 + n)
    f0 = np.where(rng.uniform(size=n) < 0.6, rng.uniform(80.0, 400.0, n), 0.0)
    sp, ap = rng.standard_normal((n, nd)) * 2.0, -rng.uniform(0.0, 30.0, (n, n_ap))
    rows = fr.pack([n], nd, n_ap, orders, f0, sp, ap, 5.0)
    for var in (np.full(rows.shape[1], 0.37), None):
        v = np.full(rows.shape, 2.5) if var is None else var
        st = fr.mlpg([n], nd, n_ap, orders, rows, v, var is None)
        f0_, sp_, ap_ = fr.unpack(nd, n_ap, 1, st, 0.5)
        x = fr.pack([n], nd, n_ap, 1, f0, sp, ap, 5.0)
        err = np.abs(st - x).max() / np.abs(x).max()
        print("mlpg of its own pack, n %d orders %d: %.2e" % (n, orders, err))
        assert err <= 1e-12
        assert np.array_equal(st[:, nd + 1], fr.voiced(f0).astype(float))
        assert np.array_equal(f0_ == 0.0, ~fr.voiced(f0)) and np.abs(sp_ - sp).max() <= 1e-12 * np.abs(x).max() and ap_.shape == (n, n_ap)


def test_variances_that_drop_an_observation_or_a_column():
    n, nd, n_ap, orders = 9, 2, 1, 3
    rng = np.random.default_rng(3)
    W = fr.width(nd, n_ap, orders)
    mean, var = rng.standard_normal((n, W)), 10.0 ** rng.uniform(-1, 1, (n, W))
    base = fr.mlpg([n], nd, n_ap, orders, mean, var, True)
    cols, vuv_col = fr.columns(nd, n_ap, orders)
    for bad in (np.nan, 0.0, -1.0):
        v = var.copy()
        v[4, cols[1][2]] = bad     # the delta-delta of mgc coefficient 1
        v[2, vuv_col] = bad        # the vuv column's variance is not read
        out = fr.mlpg([n], nd, n_ap, orders, mean, v, True)
        assert np.isnan(out[:, 1]).all()
        keep = [c for c in range(nd + 2 + n_ap) if c != 1]
        assert np.array_equal(out[:, keep], base[:, keep])
    # +inf: the observation is dropped -- the same as any mean there
    v = var.copy()
    v[4, cols[0][1]] = np.inf
    m2 = mean.copy()
    m2[4, cols[0][1]] = 1e30
    assert np.array_equal(fr.mlpg([n], nd, n_ap, orders, mean, v, True), fr.mlpg([n], nd, n_ap, orders, m2, v, True))
    assert not np.array_equal(fr.mlpg([n], nd, n_ap, orders, mean, v, True)[:, 0], base[:, 0])


def test_layout_and_batches():
    assert fr.width(25, 1, 3) == 82 and fr.width(24, 0, 1) == 26
    cols, vuv_col = fr.columns(2, 2, 3)
    assert cols == [[0, 2, 4], [1, 3, 5], [6, 7, 8], [10, 12, 14], [11, 13, 15]] and vuv_col == 9
    # nothing crosses an utterance boundary: a batch is its utterances one by one
    lengths, nd, n_ap = [0, 3, 1, 5], 3, 1
    rng = np.random.default_rng(9)
    t = sum(lengths)
    f0, sp, ap = np.where(np.arange(t) % 3 == 0, 0.0, 150.0 + np.arange(t)), rng.standard_normal((t, nd)), rng.standard_normal((t, n_ap))
    rows = fr.pack(lengths, nd, n_ap, 3, f0, sp, ap, 1.0)
    o = 0
    for n in lengths:
        assert np.array_equal(rows[o:o + n], fr.pack([n], nd, n_ap, 3, f0[o:o + n], sp[o:o + n], ap[o:o + n], 1.0))
        o += n
    var = np.full(rows.shape[1], 1.0)
    st = fr.mlpg(lengths, nd, n_ap, 3, rows, var, False)
    assert np.array_equal(st[:3], fr.mlpg([3], nd, n_ap, 3, rows[:3], var, False))
