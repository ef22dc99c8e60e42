"""CPU tests of THE rule of include/world_class_gmm.h as tests/gmm_rule.py states it: against the mathematics in exact rational
arithmetic on fixtures where every operation of the rule is exact, against a dense evaluation on random well-conditioned models, and
through its branches (ties, frames that are not finite, refusals, unnormalised weights, one mixture)."""
import itertools
import math
from fractions import Fraction as Fr

import numpy as np
import pytest

import gmm_rule as gm


# ---- exact fixtures --------------------------------------------------------------------------------------------------------------------
def exact_model(n_mix, dx, dy, seed):
    """integer lower-triangular factors with power-of-two diagonals, Sxx = L L^T in integers, small integer Syx, Syy diagonal and large
    enough for a positive cvar; means in quarters -> weight, mean, cov"""
    rng = np.random.default_rng(seed)
    D = dx + dy
    weight = rng.integers(1, 5, size=n_mix).astype(np.float64)
    mean = rng.integers(-8, 9, size=(n_mix, D)) / 4.0
    cov = np.zeros((n_mix, D, D))
    for m in range(n_mix):
        L = np.tril(rng.integers(-3, 4, size=(dx, dx)), -1).astype(np.float64)
        L[np.arange(dx), np.arange(dx)] = 2.0 ** rng.integers(0, 2, size=dx)
        Sxx = L @ L.T                                   # integers: exact
        Syx = rng.integers(-2, 3, size=(dy, dx)).astype(np.float64)
        inv = inverse([[Fr(v) for v in row] for row in Sxx.tolist()])
        for j in range(dy):
            sub = sum(Fr(Syx[j, a]) * inv[a][b] * Fr(Syx[j, b]) for a in range(dx) for b in range(dx))
            cov[m, dx + j, dx + j] = float(math.floor(sub) + 1 + int(rng.integers(0, 4)))
        cov[m, :dx, :dx], cov[m, dx:, :dx], cov[m, :dx, dx:] = Sxx, Syx, Syx.T
    return weight, mean, cov


def inverse(a):
    """the inverse of a matrix of Fractions by exact Gauss-Jordan elimination"""
    n = len(a)
    a = [list(row) + [Fr(int(i == j)) for j in range(n)] for i, row in enumerate(a)]
    for col in range(n):
        piv = next(r for r in range(col, n) if a[r][col] != 0)
        a[col], a[piv] = a[piv], a[col]
        p = a[col][col]
        a[col] = [v / p for v in a[col]]
        for r in range(n):
            if r != col and a[r][col] != 0:
                f = a[r][col]
                a[r] = [v - f * w for v, w in zip(a[r], a[col])]
    return [row[n:] for row in a]


def fr(a):
    return [Fr(float(v)) for v in a]


EXACT = list(itertools.product((1, 2, 5), (1, 3), (1, 4)))


@pytest.mark.parametrize("dx,dy,n_mix", EXACT)
def test_exact_fixtures_equal_the_definitions_in_rational_arithmetic(dx, dy, n_mix):
    """no tolerance: every operation of the rule is exact on these fixtures, so every intermediate the rule hands out (d, z, q, W, B,
    cvar, mean), read as a Fraction, equals the definition evaluated in Fractions from Sxx^-1 by exact elimination"""
    weight, mean, cov = exact_model(n_mix, dx, dy, 100 * dx + 10 * dy + n_mix)
    p = gm.prepare(weight, mean, cov, dx, dy)
    rng = np.random.default_rng(dx + dy)
    x = rng.integers(-64, 65, size=(9, dx)) / 8.0     # dyadic rationals of a few bits
    got_mean, got_var, best, ll = gm.convert(p, x)
    _, z, q = gm.loglik(p, x)
    assert p["W"].shape == (n_mix, dx, dx) and p["B"].shape == (n_mix, dy, dx) and p["cvar"].shape == (n_mix, dy) and p["c"].shape == (n_mix,)
    for m in range(n_mix):
        Sxx = [[Fr(float(cov[m, i, j])) for j in range(dx)] for i in range(dx)]
        Syx = [[Fr(float(cov[m, dx + j, i])) for i in range(dx)] for j in range(dy)]
        inv = inverse(Sxx)
        W = [fr(p["W"][m, i]) for i in range(dx)]
        assert all(W[i][k] == 0 for i in range(dx) for k in range(i + 1, dx)) and all(W[i][i] > 0 for i in range(dx))
        # W^T W = Sxx^-1 with W lower triangular and a positive diagonal: W is L^-1 itself
        assert [[sum(W[k][i] * W[k][j] for k in range(dx)) for j in range(dx)] for i in range(dx)] == inv
        B = [fr(p["B"][m, j]) for j in range(dy)]
        assert B == [[sum(Syx[j][i] * W[k][i] for i in range(dx)) for k in range(dx)] for j in range(dy)]
        gain = [[sum(Syx[j][a] * inv[a][b] for a in range(dx)) for b in range(dx)] for j in range(dy)]   # Syx Sxx^-1
        assert fr(p["cvar"][m]) == [Fr(float(cov[m, dx + j, dx + j])) - sum(gain[j][b] * Syx[j][b] for b in range(dx)) for j in range(dy)]
        assert (p["cvar"][m] > 0).all()
        diag = [1.0 / float(p["W"][m, i, i]) for i in range(dx)]      # powers of two: L(i,i) itself
        assert all(Fr(v) * W[i][i] == 1 for i, v in enumerate(diag))
        ld = math.log(diag[0])
        for i in range(1, dx):
            ld = ld + math.log(diag[i])
        assert p["c"][m] == (math.log(float(weight[m])) - ld) - (0.5 * float(dx)) * 1.8378770664093453
        for t in range(len(x)):
            d = [Fr(float(x[t, k])) - Fr(float(mean[m, k])) for k in range(dx)]
            assert fr(z[t, m]) == [sum(W[i][k] * d[k] for k in range(dx)) for i in range(dx)]
            q_exact = sum(d[a] * inv[a][b] * d[b] for a in range(dx) for b in range(dx))
            assert Fr(float(q[t, m])) == q_exact
            assert ll[t, m] == p["c"][m] - 0.5 * q[t, m]
            if best[t] == m:
                assert fr(got_mean[t]) == [Fr(float(mean[m, dx + j])) + sum(gain[j][b] * d[b] for b in range(dx)) for j in range(dy)]
                assert np.array_equal(got_var[t], p["cvar"][m])
    assert ((best >= 0) & (best < n_mix)).all()
    assert np.array_equal(best, np.argmax(ll, axis=1))


# ---- random well-conditioned models ----------------------------------------------------------------------------------------------------
def random_model(n_mix, dx, dy, seed):
    """Sxx = I + G G^T / dx with a standard-normal G; Syx small against it; -> weight, mean, cov and cond(Sxx) of the worst mixture"""
    rng = np.random.default_rng(seed)
    D = dx + dy
    weight = rng.uniform(0.5, 1.5, size=n_mix)
    weight /= weight.sum()
    mean = rng.normal(size=(n_mix, D))
    cov = np.zeros((n_mix, D, D))
    cond = 0.0
    for m in range(n_mix):
        G = rng.normal(size=(dx, dx))
        Sxx = np.eye(dx) + G @ G.T / dx
        Sxx = 0.5 * (Sxx + Sxx.T)
        Syx = 0.1 * rng.normal(size=(dy, dx))
        cov[m, :dx, :dx], cov[m, dx:, :dx], cov[m, :dx, dx:] = Sxx, Syx, Syx.T
        cov[m, dx:, dx:] = np.eye(dy) * (1.0 + float(np.max(np.sum(Syx * np.linalg.solve(Sxx, Syx.T).T, axis=1))))
        cond = max(cond, float(np.linalg.cond(Sxx)))
    return weight, mean, cov, cond


RANDOM_SEED = 2007
RATIO_MEASURED = 0.012   # measured: see the docstring below


def test_random_models_against_the_dense_evaluation():
    """dx = 50, n_mix = 8, 200 frames drawn around the mixtures' means.  ll against log w - (dx log 2 pi + slogdet + d^T solve(Sxx, d))
    / 2, the error relative to |c_m| + q, the bound a multiple of dx * cond(Sxx) * 2^-53.  Measured on the rule alone against the
    dense evaluation (numpy with OpenBLAS, glibc): cond(Sxx) = 5.11 and a worst ratio of 0.012 of dx * cond * 2^-53 -- the triangular
    sums of a well-conditioned factor lose far less than the bound allows.  RATIO_MEASURED is that figure; four times it is asserted,
    to allow for other libm / BLAS builds.  This checks the rule, not the device.  best equals the dense argmax on every frame
    whose dense margin between its best two exceeds twice that bound on the frame's largest |c_m| + q; the seed leaves no frame out
    (measured: the least margin is 1.06 against a bound near 1e-14), and at most 2 % may be"""
    dx, dy, n_mix, n = 50, 3, 8, 200
    weight, mean, cov, cond = random_model(n_mix, dx, dy, RANDOM_SEED)
    assert cond < 20.0
    rng = np.random.default_rng(RANDOM_SEED + 1)
    of = rng.integers(0, n_mix, size=n)
    x = np.stack([mean[m, :dx] + np.linalg.cholesky(cov[m, :dx, :dx]) @ rng.normal(size=dx) for m in of])
    p = gm.prepare(weight, mean, cov, dx, dy)
    got_mean, got_var, best, ll = gm.convert(p, x)
    _, _, q = gm.loglik(p, x)
    dense = np.zeros((n, n_mix))
    for m in range(n_mix):
        Sxx = cov[m, :dx, :dx]
        d = x - mean[m, :dx]
        sign, logdet = np.linalg.slogdet(Sxx)
        assert sign > 0
        dense[:, m] = math.log(weight[m]) - 0.5 * (dx * gm.LOG_2PI + logdet + np.sum(d * np.linalg.solve(Sxx, d.T).T, axis=1))
    scale = np.abs(p["c"])[None, :] + q
    unit = dx * cond * 2.0 ** -53
    ratio = float(np.max(np.abs(ll - dense) / scale)) / unit
    print("gmm rule against dense: cond %.2f, worst error %.3f of dx * cond * 2^-53" % (cond, ratio))
    bound = 4.0 * RATIO_MEASURED * unit
    assert ratio <= 4.0 * RATIO_MEASURED
    top2 = np.sort(dense, axis=1)[:, -2:]
    margin = top2[:, 1] - top2[:, 0]
    clear = margin > 2.0 * bound * scale.max(axis=1)
    print("gmm rule against dense: least margin %.3g, %d of %d frames left out" % (margin.min(), int((~clear).sum()), n))
    assert int((~clear).sum()) <= 0.02 * n          # the dense evaluation alone stays within the cap
    assert np.array_equal(best[clear], np.argmax(dense, axis=1)[clear])
    # the conditional mean and variance against the dense definitions, to the same kind of bound on their own scale
    for t in range(0, n, 17):
        m = int(best[t])
        Sxx, Syx = cov[m, :dx, :dx], cov[m, dx:, :dx]
        want = mean[m, dx:] + Syx @ np.linalg.solve(Sxx, x[t] - mean[m, :dx])
        assert np.allclose(got_mean[t], want, rtol=0, atol=1e-11 * (1.0 + np.abs(want).max()))
        assert np.allclose(got_var[t], np.diag(cov[m, dx:, dx:] - Syx @ np.linalg.solve(Sxx, Syx.T)), rtol=1e-11, atol=0)


# ---- branches --------------------------------------------------------------------------------------------------------------------------
def small_model(n_mix=8, dx=3, dy=2, seed=5):
    weight, mean, cov, _ = random_model(n_mix, dx, dy, seed)
    return weight, mean, cov


def test_an_exact_tie_goes_to_the_least_index():
    weight, mean, cov = small_model()
    weight[7], mean[7], cov[7] = weight[3], mean[3], cov[3]
    p = gm.prepare(weight, mean, cov, 3, 2)
    x = mean[3, :3] + np.array([[0.0, 0.0, 0.0], [0.01, -0.02, 0.005]])
    _, _, best, ll = gm.convert(p, x)
    assert np.array_equal(ll[:, 3], ll[:, 7]) and (best == 3).all()
    assert (ll[:, 3][:, None] >= ll).all()


def test_frames_that_are_not_finite_drop_out_and_leave_their_neighbours_alone():
    """a NaN makes every ll NaN; so does an infinity that meets a zero of W (a diagonal Sxx has W(i,k) = -0.0 below its diagonal) or
    an infinity of the other sign in the same sum: best = -1, mean = 0.0, var = +inf.  The finite frame between them is what it is alone"""
    weight, mean, cov = small_model()
    for m in range(8):   # diagonal source covariances: W's off-diagonal entries are zeros
        cov[m, :3, :3] = np.diag(np.diag(cov[m, :3, :3]))
        cov[m, 3:, :3] *= 0.1
        cov[m, :3, 3:] = cov[m, 3:, :3].T
    p = gm.prepare(weight, mean, cov, 3, 2)
    assert (p["W"][:, 1, 0] == 0.0).all()
    fine = mean[2, :3] + 0.1
    x = np.stack([np.array([np.nan, 0.0, 0.0]), fine, np.array([np.inf, 0.0, 0.0]), np.array([0.0, -np.inf, 1.0])])
    got_mean, got_var, best, ll = gm.convert(p, x)
    alone = gm.convert(p, fine[None, :])
    assert best.tolist() == [-1, int(alone[2][0]), -1, -1] and best[1] >= 0
    for t in (0, 2, 3):
        assert np.isnan(ll[t]).all() and (got_mean[t] == 0.0).all() and not np.signbit(got_mean[t]).any() and (got_var[t] == np.inf).all()
    for a, b in zip((got_mean[1], got_var[1], ll[1]), (alone[0][0], alone[1][0], alone[3][0])):
        assert np.array_equal(a, b) and np.isfinite(a).all()
    # opposite infinities in one sum, on a full W
    weight, mean, cov = small_model(8, 2, 2)
    p = gm.prepare(weight, mean, cov, 2, 2)
    s = np.sign(p["W"][:, 1, 0])
    assert (s != 0).all() and len(set(s.tolist())) == 2
    _, _, best, ll = gm.convert(p, np.array([[np.inf, np.inf], [np.inf, -np.inf]]))
    # W(1,1) > 0: z(1) = W(1,0) * inf + W(1,1) * (+-inf) is NaN in the mixtures where the two terms differ in sign; a mixture where
    # they agree carries -inf and is judged as the rule says
    for t, sgn in ((0, 1.0), (1, -1.0)):
        assert np.array_equal(np.isnan(ll[t]), s * sgn < 0)
        rest = np.flatnonzero(~np.isnan(ll[t]))
        assert best[t] == (rest[0] if len(rest) else -1) and (ll[t, rest] == -np.inf).all()


def test_every_refusal_of_prepare_names_its_mixture_and_row():
    weight, mean, cov = small_model()
    ok = lambda **kw: gm.prepare(kw.get("weight", weight), kw.get("mean", mean), kw.get("cov", cov), kw.get("dx", 3), kw.get("dy", 2))
    ok()
    with pytest.raises(ValueError, match="n_mix"):
        gm.prepare(np.zeros(0), np.zeros((0, 5)), np.zeros((0, 5, 5)), 3, 2)
    with pytest.raises(ValueError, match="n_mix"):
        gm.prepare(np.ones(1025), np.zeros((1025, 2)), np.tile(np.eye(2), (1025, 1, 1)), 1, 1)
    for dx, dy in ((0, 5), (5, 0), (193, 1), (1, 193)):
        with pytest.raises(ValueError, match="dx and dy"):
            gm.prepare(np.ones(1), np.zeros((1, dx + dy)), np.eye(dx + dy)[None], dx, dy)
    for which in ("weight", "mean", "cov"):
        with pytest.raises(ValueError, match="null"):
            ok(**{which: None})
    for bad in (0.0, -1.0, np.nan, np.inf):
        w2 = weight.copy()
        w2[5] = bad
        with pytest.raises(ValueError, match="mixture 5: a weight"):
            ok(weight=w2)
    m2 = mean.copy()
    m2[4, 3] = np.inf
    with pytest.raises(ValueError, match="mixture 4, row 3: a mean"):
        ok(mean=m2)
    c2 = cov.copy()
    c2[6, 4, 1] = np.nan
    with pytest.raises(ValueError, match="mixture 6, row 4: a covariance"):
        ok(cov=c2)
    c2 = cov.copy()
    c2[6, 1, 4] = np.nan       # above the diagonal: never read
    c2[0, 0, 2] = np.inf
    for a, b in zip(ok(cov=c2).values(), ok().values()):
        assert np.array_equal(a, b)
    c2 = cov.copy()
    c2[2, 1, 1] = c2[2, 1, 0] ** 2 / c2[2, 0, 0] - 1e-3     # the second pivot goes negative
    with pytest.raises(ValueError, match="mixture 2, row 1: the source covariance is not positive definite"):
        ok(cov=c2)
    c2 = cov.copy()
    c2[1, 0, 0] = 0.0
    with pytest.raises(ValueError, match="mixture 1, row 0: "):
        ok(cov=c2)
    c2 = cov.copy()
    c2[3, 4, 4] = 0.0          # Syy(1,1) = 0: cvar(1) = -sum B^2 <= 0, row dx + 1 of the joint covariance
    with pytest.raises(ValueError, match="mixture 3, row 4: a conditional variance"):
        ok(cov=c2)
    c2[1, 0, 0] = -1.0         # the earlier mixture is named first
    with pytest.raises(ValueError, match="mixture 1, row 0: "):
        ok(cov=c2)


def test_unnormalised_weights_move_every_ll_by_one_log_and_leave_best_alone():
    weight, mean, cov = small_model()
    rng = np.random.default_rng(9)
    x = mean[rng.integers(0, 8, size=40), :3] + 0.3 * rng.normal(size=(40, 3))
    a = gm.convert(gm.prepare(weight, mean, cov, 3, 2), x)
    b = gm.convert(gm.prepare(16.0 * weight, mean, cov, 3, 2), x)
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    shift = b[3] - a[3]
    assert np.allclose(shift, math.log(16.0), rtol=0, atol=64 * 2.0 ** -52 * np.abs(a[3]).max())
    assert abs(sum(weight) - 1.0) < 1e-12 and sum(16.0 * weight) > 15.0


def test_one_mixture():
    weight, mean, cov = small_model(1)
    p = gm.prepare(weight, mean, cov, 3, 2)
    x = np.array([[0.0, 1.0, -1.0], [np.nan, 0.0, 0.0], [2.0, 2.0, 2.0]])
    got_mean, got_var, best, ll = gm.convert(p, x)
    assert best.tolist() == [0, -1, 0] and ll.shape == (3, 1)
    assert np.array_equal(got_var[0], p["cvar"][0]) and np.array_equal(got_var[2], p["cvar"][0]) and (got_var[1] == np.inf).all()
    Sxx, Syx = cov[0, :3, :3], cov[0, 3:, :3]
    assert np.allclose(got_mean[0], mean[0, 3:] + Syx @ np.linalg.solve(Sxx, x[0] - mean[0, :3]), rtol=0, atol=1e-13)


def test_float_rows_widen_exactly_and_float_outputs_are_the_cast():
    weight, mean, cov = small_model()
    p = gm.prepare(weight, mean, cov, 3, 2)
    x32 = (mean[:, :3] + 0.25).astype(np.float32)
    a = gm.convert(p, x32, np.float32)
    b = gm.convert(p, x32.astype(np.float64))
    assert a[0].dtype == np.float32 and a[1].dtype == np.float32
    assert np.array_equal(a[0], b[0].astype(np.float32)) and np.array_equal(a[1], b[1].astype(np.float32))
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
