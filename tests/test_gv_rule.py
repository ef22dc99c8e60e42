"""CPU tests that hold tests/gv_rule.py (THE rule of include/world_class_gv.h) to the mathematics: the ascent direction and the Hessian
diagonal against finite differences of J through features_rule.dense_system, the banded product against the dense one, THE sum, J over
the iterations, both branches of the step, the variance-scaling start, the mask and every exit."""
import math

import numpy as np
import pytest

import features_rule as fr
import gv_rule as gr


def blurred(n, S, orders, seed, blur=5):
    """an over-smoothed model of one utterance: natural trajectories x [n, S] (a slow wave and noise, a scale per column), the model's
    means the statics and deltas of their moving average, variances over two decades below a tenth of the column's scale squared
    -> mean, var [n, orders, S], gv_mean, gv_var [S]: the variance of x and a tenth of its square.
    Why the variances are small against the global variance, as a trained model's are: h(t) of the rule is positive at a frame with
    d(t) = 0 only while (N - 1) * pv * |e| < omega * a0(t) * N * N / (2 * w_gv), that is about |e| < gv_var / (2 * orders * var_0(t))
    at equal weights.  With gv_var = 0.1 * gv_mean^2 and a v that strays a tenth of gv_mean from it, that asks var_0 < gv_mean / 6;
    gv_mean is about 0.76 of the scale squared here.  Beyond it h changes sign, the step is no ascent step, and the halving of the
    step is the rule's only answer (test_a_trace_takes_both_branches_of_the_step walks that branch)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)[:, None]
    scale = np.linspace(2.0, 0.2, S)
    x = scale * (np.sin(2.0 * np.pi * t / rng.uniform(7.0, 40.0, S) + rng.uniform(0.0, 6.0, S)) + 0.5 * rng.standard_normal((n, S))) + rng.standard_normal(S)
    k = min(blur, n)
    pad = np.concatenate([np.repeat(x[:1], k // 2, axis=0), x, np.repeat(x[-1:], k - 1 - k // 2, axis=0)])
    y = np.stack([pad[i:i + n] for i in range(k)]).mean(axis=0)
    mean = np.stack((y,) + fr.deltas(y), axis=1)[:, :orders]
    var = 10.0 ** rng.uniform(-3.0, -1.0, (n, orders, S)) * (scale * scale)
    gv_mean = x.var(axis=0) + 0.01 * scale * scale
    return mean, var, gv_mean, 0.1 * gv_mean * gv_mean


def solved(mean, var):
    system = fr.mlpg_system(mean, var)
    return system, fr.mlpg_solve(*system)


def dense_J(mean, var, c, m, gv_mean, gv_var, w_ml, w_gv):
    """J of one column through the dense W^T P W and W^T P mu, plain numpy sums"""
    R, rr = fr.dense_system(mean, var)
    omega = w_ml / (mean.shape[1] * len(c))
    v = np.var(c[m])
    return omega * (c @ rr - 0.5 * c @ R @ c) - 0.5 * w_gv * (v - gv_mean) ** 2 / gv_var


@pytest.mark.parametrize("orders", [2, 3])
def test_g_and_h_are_the_gradient_and_the_hessian_diagonal_of_J(orders):
    n, S = 23, 3
    mean, var, gv_mean, gv_var = blurred(n, S, orders, 5 + orders)
    system, c = solved(mean, var)
    m = np.ones(n, dtype=bool)
    m[[0, 1, 11, 22]] = False
    w_ml, w_gv = 1.5, 0.75
    trace = []
    gr.refine(system, c, m, orders, gv_mean, gv_var, w_ml, w_gv, 0.1, 1, trace=trace)
    h, g = trace[0]["h"], trace[0]["g"]
    # the c the step was taken from: the variance-scaled start
    c0 = gr.refine(None, c, m, orders, gv_mean, gv_var, max_iter=0)
    for col in range(S):
        J = lambda x: dense_J(mean[:, :, col], var[:, :, col], x, m, gv_mean[col], gv_var[col], w_ml, w_gv)
        eps = 1e-4 * np.abs(c0[:, col]).max()
        for t in np.flatnonzero(m):
            up, dn = c0[:, col].copy(), c0[:, col].copy()
            up[t] += eps
            dn[t] -= eps
            grad = (J(up) - J(dn)) / (2.0 * eps)
            hess = (J(up) - 2.0 * J(c0[:, col]) + J(dn)) / (eps * eps)
            # J is a quartic in c(t): the central differences are exact to O(eps^2) of its higher derivatives
            assert abs(grad - g[t, col] * h[t, col]) <= 1e-6 * max(abs(grad), np.abs(g[:, col] * h[:, col]).max())
            assert abs(-hess - h[t, col]) <= 1e-5 * abs(h[t, col])
        assert abs(trace[0]["J"][col] - J(c0[:, col])) <= 1e-12 * max(1.0, abs(J(c0[:, col])))


@pytest.mark.parametrize("orders", [2, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 65])
def test_the_banded_product_is_the_dense_one(n, orders):
    mean, var, _, _ = blurred(n, 4, orders, 100 + n)
    a0, a1, a2, r = fr.mlpg_system(mean, var)
    c = np.random.default_rng(n).standard_normal((n, 4))
    got = gr.banded(a0, a1, a2, c)
    for col in range(4):
        R, _ = fr.dense_system(mean[:, :, col], var[:, :, col])
        want = R @ c[:, col]
        assert np.abs(got[:, col] - want).max() <= 1e-13 * (np.abs(R) @ np.abs(c[:, col])).max()


def test_the_sum_has_its_order():
    rng = np.random.default_rng(7)
    for n in (0, 1, 63, 64, 65, 200, 1000):
        x = rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)
        # pairwise and lane sums are within n eps sum|x| of the exact sum
        assert abs(gr.gv_sum(x) - math.fsum(x)) <= (n + 6) * 2.0 ** -53 * np.abs(x).sum()
    assert gr.gv_sum(np.zeros(0)) == 0.0 and not np.signbit(gr.gv_sum(np.array([-0.0])))
    # an order that matters: lane 0 holds 1e16 then 1.0 (lost), lane 1 holds -1e16; a left-to-right sum would give 1.0
    x = np.zeros(130)
    x[0], x[1], x[64] = 1e16, -1e16, 1.0
    assert gr.gv_sum(x) == 0.0 and np.sum(x[[0, 1, 64]]) == 1.0
    # the butterfly pairs lane l with l ^ 32 first: (1e16 + -1e16) + 1.0 in lanes 0, 32, 1
    x = np.zeros(64)
    x[0], x[32], x[1] = 1e16, -1e16, 1.0
    assert gr.gv_sum(x) == 1.0
    x[32], x[1] = 1.0, -1e16    # (1e16 + 1.0) + -1e16
    assert gr.gv_sum(x) == 0.0
    cols = rng.standard_normal((300, 5))
    assert np.array_equal(gr.gv_sum(cols), [gr.gv_sum(cols[:, k]) for k in range(5)])


@pytest.mark.parametrize("orders", [2, 3])
@pytest.mark.parametrize("n", [2, 3, 65, 600])
def test_J_rises_over_the_iterations(n, orders):
    S = 6
    mean, var, gv_mean, gv_var = blurred(n, S, orders, 40 + n)
    system, c = solved(mean, var)
    trace = []
    out = gr.refine(system, c, None, orders, gv_mean, gv_var, step_init=0.1, max_iter=5, trace=trace)
    J = np.array([s["J"] for s in trace[:-1]])
    assert np.isfinite(J).all() and np.isfinite(out).all()
    assert (np.diff(J, axis=0) >= 0.0).all()
    # and the last step rose as well: J of the result
    a0, a1, a2, r = system
    assert (gr.objective(a0, a1, a2, r, out, np.ones(n, dtype=bool), orders, gv_mean, gv_var, 1.0, 1.0) >= J[-1]).all()


STEP_BOTH = 2.0   # a step_init whose trace halves and grows (tests/test_gpu_gv.py runs the same case on the device)


def both_branches_case(orders=3):
    n, S = 191, 6
    mean, var, gv_mean, gv_var = blurred(n, S, orders, 77)
    return n, S, mean, var, gv_mean, gv_var


def test_a_trace_takes_both_branches_of_the_step():
    n, S, mean, var, gv_mean, gv_var = both_branches_case()
    system, c = solved(mean, var)
    trace = []
    gr.refine(system, c, None, 3, gv_mean, gv_var, step_init=STEP_BOTH, max_iter=5, trace=trace)
    steps = np.array([s["step"] for s in trace[:-1]])
    ratio = steps[1:] / steps[:-1]
    assert (ratio == 0.5).any() and (ratio == 1.2).any()
    assert set(np.unique(ratio)) <= {0.5, 1.2, 1.0}
    J = np.array([s["J"] for s in trace[:-1]])
    assert np.array_equal(ratio == 0.5, np.diff(J, axis=0) < 0.0) and np.array_equal(ratio == 1.2, np.diff(J, axis=0) > 0.0)


def test_five_steps_bring_the_variance_towards_the_global_one():
    n, S = 600, 6
    mean, var, gv_mean, gv_var = blurred(n, S, 3, 11)
    system, c = solved(mean, var)
    trace = []
    gr.refine(system, c, None, 3, gv_mean, gv_var, trace=trace)
    v_ml = gr.stat(c, np.ones(n, dtype=bool))[2]
    assert (v_ml < 0.9 * gv_mean).all()                               # over-smoothed
    assert (np.abs(trace[-1]["v"] - gv_mean) < np.abs(v_ml - gv_mean)).all()


def masks(n):
    m = np.ones(n, dtype=bool)
    m[:n // 7], m[n // 2:n // 2 + n // 9], m[n - n // 5:] = False, False, False
    return m


def test_the_start_alone_gives_the_global_variance_and_leaves_unmasked_frames():
    n, S = 300, 5
    mean, var, gv_mean, gv_var = blurred(n, S, 3, 3)
    system, c = solved(mean, var)
    for m in (np.ones(n, dtype=bool), masks(n)):
        out = gr.refine(None, c, m, 3, gv_mean, gv_var, max_iter=0)
        assert np.abs(out[m].var(axis=0) / gv_mean - 1.0).max() <= 1e-12
        assert np.abs(out[m].mean(axis=0) - c[m].mean(axis=0)).max() <= 1e-12 * np.abs(c).max()
        assert np.array_equal(out[~m], c[~m]) and not np.array_equal(out[m], c[m])
        full = gr.refine(system, c, m, 3, gv_mean, gv_var, max_iter=5)
        assert np.array_equal(full[~m].view(np.int64), c[~m].view(np.int64))    # bitwise
        assert not np.array_equal(full[m], out[m])


def test_every_exit():
    n, S = 40, 8
    mean, var, gv_mean, gv_var = blurred(n, S, 3, 9)
    system, c = solved(mean, var)
    c[:, 5] = 1.25                                # a constant column: the first v is 0
    m = masks(n)
    gm, gv = gv_mean.copy(), gv_var.copy()
    gv[0] = np.inf                                # switched off; its mean is not looked at
    gm[0] = np.nan
    gv[1], gv[2], gm[3], gm[4] = np.nan, 0.0, -1.0, np.inf
    gv[6] = -np.inf
    out = gr.refine(system, c, m, 3, gm, gv)
    bits = lambda a: np.ascontiguousarray(a).view(np.int64)
    assert np.array_equal(bits(out[:, [0, 5]]), bits(c[:, [0, 5]]))
    for col in (1, 2, 3, 4, 6):
        assert np.isnan(out[m, col]).all() and np.array_equal(bits(out[~m, col]), bits(c[~m, col]))
    assert np.isfinite(out[:, 7]).all() and not np.array_equal(out[m, 7], c[m, 7])
    ref = gr.refine(system, c, m, 3, gv_mean, gv_var)
    assert np.array_equal(out[:, 7], ref[:, 7])   # the bad columns touch nothing else
    for bad in (np.nan, 0.0, -2.0):               # gv_mean: NaN, 0, negative
        gm2 = gv_mean.copy()
        gm2[7] = bad
        assert np.isnan(gr.refine(system, c, m, 3, gm2, gv_var)[m, 7]).all()
    # N < 2: as it is, but a bad value still marks the masked frame
    for count in (0, 1):
        few = np.zeros(n, dtype=bool)
        few[:count] = True
        out = gr.refine(system, c, few, 3, gv_mean, gv_var)
        assert np.array_equal(bits(out), bits(c))
        out = gr.refine(system, c, few, 3, gm, gv)
        assert np.isnan(out[few][:, [1, 2, 3, 4, 6]]).all() and np.array_equal(bits(out[~few]), bits(c[~few]))
    two = np.zeros(n, dtype=bool)
    two[[3, 30]] = True
    out = gr.refine(system, c, two, 3, gv_mean, gv_var)
    assert not np.array_equal(out[two, 7], c[two, 7]) and np.array_equal(bits(out[~two]), bits(c[~two]))
    # values that are not finite travel: a NaN in the trajectory gives a NaN v, and the column stays as it is
    c2 = c.copy()
    c2[7, 2] = np.nan
    assert np.array_equal(bits(gr.refine(system, c2, m, 3, gv_mean, gv_var)[:, 2]), bits(c2[:, 2]))


def test_stats_are_the_masked_mean_and_variance():
    lengths, nd, n_ap = [0, 1, 2, 70, 200], 4, 2
    rng = np.random.default_rng(12)
    static = rng.standard_normal((sum(lengths), nd + 2 + n_ap)) * 3.0 + 1.0
    mask = rng.uniform(size=sum(lengths)) < 0.7
    mask[1] = True
    for mk in (None, mask):
        mean, var = gr.stats(lengths, nd, n_ap, static, mk)
        assert mean.shape == var.shape == (5, nd + 1 + n_ap)
        assert np.isnan(mean[0]).all() and np.isnan(var[0]).all()
        o = 0
        for u, n in enumerate(lengths):
            rows = static[o:o + n][(np.ones(n, dtype=bool) if mk is None else mk[o:o + n])]
            o += n
            if len(rows) == 0:
                assert np.isnan(mean[u]).all()
                continue
            x = np.delete(rows, nd + 1, axis=1)
            assert np.abs(mean[u] - x.mean(axis=0)).max() <= 1e-14 * np.abs(x).max()
            assert np.abs(var[u] - x.var(axis=0)).max() <= 1e-13 * max(x.var(axis=0).max(), 1e-300)
    none = gr.stats([3], nd, n_ap, static[:3], np.zeros(3))
    assert np.isnan(none[0]).all() and np.isnan(none[1]).all()


def test_mlpg_gv_runs_the_batch_utterance_by_utterance():
    lengths, nd, n_ap, orders = [0, 5, 70], 3, 1, 3
    S, W = nd + 1 + n_ap, fr.width(nd, n_ap, orders)
    rng = np.random.default_rng(4)
    cols, vuv = fr.columns(nd, n_ap, orders)
    mean, var = np.zeros((75, W)), np.ones((75, W))
    gvm = None
    o = 0
    for n in lengths[1:]:
        mu, vr, gvm, gvv = blurred(n, S, orders, 60 + n)
        mean[o:o + n][:, np.array(cols).T] = mu
        var[o:o + n][:, np.array(cols).T] = vr
        o += n
    mean[:, vuv] = rng.uniform(size=75)
    static = fr.mlpg(lengths, nd, n_ap, orders, mean, var, True)
    out = gr.mlpg_gv(lengths, nd, n_ap, orders, mean, var, True, gvm, gvv, None, static)
    assert np.array_equal(out[:, nd + 1], static[:, nd + 1])      # vuv is never touched
    stat_cols = [c if c <= nd else c + 1 for c in range(S)]
    take = np.array(cols).T
    for a, b in ((0, 5), (5, 75)):
        sys_ = fr.mlpg_system(mean[a:b][:, take], var[a:b][:, take])
        assert np.array_equal(out[a:b][:, stat_cols], gr.refine(sys_, static[a:b][:, stat_cols], None, orders, gvm, gvv))
