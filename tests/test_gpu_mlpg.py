"""-m gpu: wc_mlpg_device against tests/features_rule.py, bit for bit: the batch and shapes of tests/test_gpu_features.py, orders 2 and
3, one row of variances for the batch and one per frame, rows of doubles and of floats."""
import numpy as np
import pytest

import features_rule as fr
from test_gpu_features import LENGTHS, SHAPES, _dev, _guarded, _rows, _same, batch, device_pack, env  # noqa: F401

pytestmark = pytest.mark.gpu


def device_mlpg(env, lengths, nd, n_ap, orders, mean, var, per_frame, fmt="f64"):
    w, ft, torch = env
    t = int(sum(lengths))
    dt = np.float64 if fmt == "f64" else np.float32
    d_static = _guarded(torch, t, nd + 2 + n_ap)
    torch.cuda.synchronize()
    ft.mlpg(lengths, nd, n_ap, orders, _dev(torch, mean, dt), _dev(torch, var, dt), d_static, per_frame, fmt)
    w.lib().wc_synchronize()
    return _rows(d_static, t, nd + 2 + n_ap)


def case(nd, n_ap, orders, seed, dt=np.float64):
    """means of unit scale and variances over four decades, 1e-2 .. 1e2, per frame and as one row"""
    rng = np.random.default_rng(seed)
    t, W = sum(LENGTHS), fr.width(nd, n_ap, orders)
    mean = rng.standard_normal((t, W)).astype(dt)
    var = (10.0 ** rng.uniform(-2.0, 2.0, (t, W))).astype(dt)
    return mean, var, var[7].copy()


@pytest.mark.parametrize("orders", [2, 3])
@pytest.mark.parametrize("nd,n_ap", SHAPES)
def test_mlpg_equals_the_rule_bit_for_bit(env, nd, n_ap, orders):
    """no tolerance: division is correctly rounded and the build keeps every product and sum apart (-ffp-contract=off), so the rule's
    order of operations gives the kernel's bits"""
    for fmt, dt in (("f64", np.float64), ("f32", np.float32)):
        mean, var, var_row = case(nd, n_ap, orders, 31 * nd + orders, dt)
        for per_frame, v in ((True, var), (False, var_row)):
            got = device_mlpg(env, LENGTHS, nd, n_ap, orders, mean, v, per_frame, fmt)
            want = fr.mlpg(LENGTHS, nd, n_ap, orders, mean.astype(np.float64), v.astype(np.float64), per_frame)
            assert np.isfinite(got).all()
            assert _same(got, want), (fmt, per_frame)
            assert np.array_equal(got[:, nd + 1], mean[:, orders * (nd + 1)].astype(np.float64))   # vuv is copied through


@pytest.mark.parametrize("orders", [2, 3])
def test_variances_that_drop_a_column_or_an_observation(env, orders):
    """a NaN, a 0 and a negative variance each make exactly their own (utterance, static column) NaN; +inf drops the observation;
    the vuv column's variance is not read"""
    nd, n_ap = 60, 5
    mean, var, var_row = case(nd, n_ap, orders, 99 + orders)
    cols, vuv_col = fr.columns(nd, n_ap, orders)
    offs = np.concatenate([[0], np.cumsum(LENGTHS)])
    base = device_mlpg(env, LENGTHS, nd, n_ap, orders, mean, var, True)
    # (static column, its order, utterance, frame in it): an mgc coefficient of the second wavefront, lf0, a band; utterances of 600, 65, 1
    spots = [(63, orders - 1, 7, 300), (nd, 1, 5, 64), (nd + 2, 0, 1, 0)]
    for bad in (np.nan, 0.0, -1.0, -np.inf):
        v = var.copy()
        for c, k, u, t in spots:
            v[offs[u] + t, cols[c][k]] = bad
        v[offs[6] + 5, vuv_col] = bad
        got = device_mlpg(env, LENGTHS, nd, n_ap, orders, mean, v, True)
        assert _same(got, fr.mlpg(LENGTHS, nd, n_ap, orders, mean, v, True))
        hit = np.zeros(got.shape, dtype=bool)
        for c, k, u, t in spots:
            hit[offs[u]:offs[u + 1], c if c <= nd else c + 1] = True
        assert np.isnan(got[hit]).all() and np.array_equal(got[~hit], base[~hit])
        # one row of variances for the batch: that static column in every utterance
        vr = var_row.copy()
        vr[cols[nd + 1][0]] = bad
        vr[vuv_col] = bad
        got = device_mlpg(env, LENGTHS, nd, n_ap, orders, mean, vr, False)
        assert _same(got, fr.mlpg(LENGTHS, nd, n_ap, orders, mean, vr, False))
        assert np.isnan(got[:, nd + 2]).all() and np.isfinite(np.delete(got, nd + 2, axis=1)).all()
    v, m2 = var.copy(), mean.copy()
    for c, k, u, t in spots[:2]:
        v[offs[u] + t, cols[c][k]] = np.inf
        m2[offs[u] + t, cols[c][k]] = np.nan    # a dropped observation's mean is not looked at
    got = device_mlpg(env, LENGTHS, nd, n_ap, orders, mean, v, True)
    assert np.isfinite(got).all() and _same(got, fr.mlpg(LENGTHS, nd, n_ap, orders, mean, v, True))
    assert _same(got, device_mlpg(env, LENGTHS, nd, n_ap, orders, m2, v, True))
    changed = np.abs(got - base).max(axis=0) > 0
    assert np.array_equal(np.flatnonzero(changed), [60, 64])   # (static column 63 stands behind vuv: output column 64)


@pytest.mark.parametrize("nd,n_ap", SHAPES)
def test_an_utterance_does_not_depend_on_its_neighbours(env, nd, n_ap):
    mean, var, var_row = case(nd, n_ap, 3, 400 + nd)
    whole = device_mlpg(env, LENGTHS, nd, n_ap, 3, mean, var, True)
    whole_row = device_mlpg(env, LENGTHS, nd, n_ap, 3, mean, var_row, False)
    o = 0
    for n in LENGTHS:
        assert _same(device_mlpg(env, [n], nd, n_ap, 3, mean[o:o + n], var[o:o + n], True), whole[o:o + n]), n
        assert _same(device_mlpg(env, [n], nd, n_ap, 3, mean[o:o + n], var_row, False), whole_row[o:o + n]), n
        o += n
    # and not on the order either: the batch reversed
    rev = LENGTHS[::-1]
    offs = np.concatenate([[0], np.cumsum(LENGTHS)])
    idx = np.concatenate([np.arange(offs[u], offs[u + 1]) for u in range(len(LENGTHS) - 1, -1, -1)]).astype(int)
    assert _same(device_mlpg(env, rev, nd, n_ap, 3, mean[idx], var[idx], True), whole[idx])


@pytest.mark.parametrize("orders", [2, 3])
@pytest.mark.parametrize("nd,n_ap", SHAPES)
def test_mlpg_of_the_devices_own_pack_returns_the_statics(env, nd, n_ap, orders):
    """means = the device's pack of finite rows, all variances equal: the statics come back within the CPU test's bound, 1e-12 of
    max|x| (cond(R) <= 1 + |D|^2 + |DD|^2 <= 18 times the residual bound of the banded factorisation)"""
    f0, sp, ap = batch(nd, n_ap, 1)   # (variant 1 holds no values that are not finite in the coded rows)
    rows = device_pack(env, LENGTHS, nd, n_ap, orders, f0, sp, ap)
    statics = device_pack(env, LENGTHS, nd, n_ap, 1, f0, sp, ap)
    for per_frame, var in ((False, np.full(rows.shape[1], 0.04)), (True, np.full(rows.shape, 7.0))):
        got = device_mlpg(env, LENGTHS, nd, n_ap, orders, rows, var, per_frame)
        err = np.abs(got - statics).max() / np.abs(statics).max()
        print("mlpg of the device's own pack, nd %d n_ap %d orders %d: %.3e of max|x|" % (nd, n_ap, orders, err))
        assert err <= 1e-12
        assert np.array_equal(got[:, nd + 1], statics[:, nd + 1])
