"""CPU tests of tests/gmm_train_rule.py, THE rule of include/world_class_gmm_train.h, against the mathematics: a fixture in exact
arithmetic, the statistics against a dense einsum, centred against raw second moments, the fold's order at the segment's edge, the
starved, kept and floored branches of the update, the joint preparation against gmm_rule.prepare, and the two conditions the GPU
tests assert without a margin: the planted fixture's loglik rises strictly over five iterations, and eight iterations on the planted
pair lower the conversion's error."""
import math
from fractions import Fraction

import numpy as np
import pytest

import gmm_rule as gm
import gmm_train_rule as tr


def unpack(S2, D):
    n_mix = S2.shape[0]
    full = np.zeros((n_mix, D, D))
    ii, jj = tr.tri(D)
    full[:, ii, jj] = S2
    full[:, jj, ii] = S2
    return full


def exact_fixture():
    """three clusters of integer rows 1000 apart under unit covariances: every posterior is exactly 0 or 1"""
    centres = np.array([[0.0, 0.0, 0.0], [1000.0, 0.0, -1000.0], [0.0, 2000.0, 1000.0]])
    offs = np.array([[1, 0, -1], [0, 2, 1], [-1, -2, 0], [2, 1, 1], [0, 0, 3], [-2, 1, 0], [1, 1, 1], [-1, -3, -3]], dtype=np.float64)
    which = np.array([0, 1, 2, 0, 0, 1, 2, 2, 1, 0, 0, 2, 1, 0, 2, 0])
    rows = centres[which] + offs[np.arange(16) % 8]
    model = (np.array([0.5, 0.25, 0.25]), centres + np.array([1.0, -1.0, 2.0]), np.tile(np.eye(3), (3, 1, 1)))
    return rows, which, model


def test_exact_fixture_posteriors_are_zero_or_one_and_the_statistics_are_integers():
    rows, which, (w, mean, cov) = exact_fixture()
    gamma, fll, state, _ = tr.posteriors(tr.prepare(w, mean, cov), rows)
    assert (state == 1).all() and np.array_equal(gamma, np.eye(3)[which])      # exp underflowed to exactly 0.0
    tot = tr.statistics(rows, mean, gamma, fll, state == 1)
    d = rows[:, None, :] - mean[None]
    onehot = np.eye(3)[which]
    assert np.array_equal(tot["N"], np.bincount(which, minlength=3).astype(float)) and tot["n_live"] == 16
    assert np.array_equal(tot["S1"], np.einsum("tm,tmi->mi", onehot, d))       # (sums of small integers are exact in any order)
    assert np.array_equal(unpack(tot["S2"], 3), np.einsum("tm,tmi,tmj->mij", onehot, d, d))
    ll = gm.loglik(tr.prepare(w, mean, cov), rows)[0]
    assert tot["LL"] == pytest.approx(float(ll[np.arange(16), which].sum()), rel=1e-15)
    # the update in rationals
    nw, nmean, ncov, starved, kept = tr.update(w, mean, cov, tot)
    assert starved == 0 and kept == 0
    for m in range(3):
        sel = rows[which == m]
        n = len(sel)
        assert nw[m] == n / 16.0
        for i in range(3):
            mu_i = Fraction(int(sel[:, i].sum()), n)
            assert abs(Fraction(nmean[m, i]) - mu_i) <= abs(mu_i) * Fraction(1, 2 ** 51)
            for j in range(3):
                c = Fraction(int((sel[:, i] * sel[:, j]).sum()), n) - mu_i * Fraction(int(sel[:, j].sum()), n)
                assert abs(Fraction(ncov[m, i, j]) - c) <= Fraction(1, 2 ** 40)
        assert np.array_equal(ncov[m], ncov[m].T)


def random_joint(n_mix, D, seed):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(n_mix, D, D))
    cov = a @ a.transpose(0, 2, 1) / D + 0.5 * np.eye(D)
    return rng.uniform(0.2, 1.0, size=n_mix), 2.0 * rng.normal(size=(n_mix, D)), cov


def test_statistics_equal_a_dense_einsum_and_skip_frames_that_are_not_live():
    w, mean, cov = random_joint(5, 6, 3)
    rng = np.random.default_rng(8)
    rows = mean[rng.integers(0, 5, size=300)] + rng.normal(size=(300, 6))
    mask = (np.arange(300) % 3 != 1).astype(np.uint8)
    rows[8] = np.nan                # a dropped frame
    rows[11, 2] = np.inf            # another
    rows[4] = np.nan                # masked as well: masked, not dropped
    gamma, fll, state, _ = tr.posteriors(tr.prepare(w, mean, cov), rows, mask)
    assert state[8] == 2 and state[11] == 2 and state[4] == 0 and (state[mask == 0] == 0).all()
    assert (gamma[state != 1] == 0.0).all() and (fll[state != 1] == 0.0).all()
    live = state == 1
    assert np.allclose(gamma[live].sum(axis=1), 1.0, rtol=0, atol=1e-14)
    tot = tr.statistics(rows, mean, gamma, fll, live)
    clean = np.where(live[:, None], rows, 0.0)
    d = clean[:, None, :] - mean[None]
    g = np.where(live[:, None], gamma, 0.0)
    assert np.allclose(tot["N"], g.sum(axis=0), rtol=1e-13) and tot["n_live"] == int(live.sum())
    assert np.allclose(tot["S1"], np.einsum("tm,tmi->mi", g, d), rtol=1e-11, atol=1e-11)
    assert np.allclose(unpack(tot["S2"], 6), np.einsum("tm,tmi,tmj->mij", g, d, d), rtol=1e-11, atol=1e-11)
    assert np.isfinite(tot["S2"]).all() and tot["LL"] == pytest.approx(float(fll[live].sum()), rel=1e-13)


def test_centred_second_moments_keep_what_raw_ones_cancel():
    """one mixture, all gamma 1, rows 1e8 away from 0 with unit spread: the update's covariance from statistics centred on a mean
    near the data is right to 1e-9; the textbook raw moments E[zz'] - mu mu' lose it entirely"""
    rng = np.random.default_rng(2)
    rows = 1e8 + rng.normal(size=(500, 2))
    mean0 = np.array([[1e8 + 0.3, 1e8 - 0.2]])
    gamma, fll = np.ones((500, 1)), np.zeros(500)
    tot = tr.statistics(rows, mean0, gamma, fll, np.ones(500, dtype=bool))
    _, nmean, ncov, _, kept = tr.update(np.ones(1), mean0, np.eye(2)[None], tot)
    want = np.cov(rows.T - 1e8, bias=True)
    assert kept == 0 and np.abs(ncov[0] - want).max() < 1e-9 and np.abs(nmean[0] - rows.mean(axis=0)).max() < 1e-7
    raw = (rows[:, :, None] * rows[:, None, :]).mean(axis=0) - np.outer(rows.mean(axis=0), rows.mean(axis=0))
    assert np.abs(raw - want).max() > 1e-3


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049])
def test_the_fold_takes_segments_of_1024_ascending(n):
    rng = np.random.default_rng(n)
    rows, mean = rng.normal(size=(n, 2)), rng.normal(size=(2, 2))
    gamma = rng.random(size=(n, 2))
    fll = rng.normal(size=n)
    live = rng.random(size=n) > 0.1
    tot = tr.statistics(rows, mean, gamma, fll, live)
    # LL and N by hand, frame by frame
    LL, N = 0.0, np.zeros(2)
    for a in range(0, n, 1024):
        part, pn = None, None
        for t in range(a, min(a + 1024, n)):
            if live[t]:
                part = float(fll[t]) if part is None else part + float(fll[t])
                pn = gamma[t].copy() if pn is None else pn + gamma[t]
        LL, N = LL + part, N + pn
    assert tot["LL"] == LL and np.array_equal(tot["N"], N)
    # a cut at a multiple of 1024 is the one call; any other cut is another rule
    if n > 1024:
        two = tr.statistics(rows, mean, gamma, fll, live, cuts=[1024, n - 1024])
        assert all(np.array_equal(two[k], tot[k]) for k in ("N", "S1", "S2")) and two["LL"] == tot["LL"]
        other = tr.statistics(rows, mean, gamma, fll, live, cuts=[1000, n - 1000])
        assert not np.array_equal(other["S2"], tot["S2"]) and np.allclose(other["S2"], tot["S2"], rtol=1e-9, atol=1e-9)
    # a segment without a live frame adds +0.0
    none = tr.statistics(rows, mean, gamma, fll, np.zeros(n, dtype=bool))
    assert none["LL"] == 0.0 and not np.signbit(none["S1"]).any() and (none["S2"] == 0.0).all() and none["n_live"] == 0


def test_the_first_term_keeps_its_sign():
    """gamma = 0 and a negative d give g = -0.0: a sum of such terms is -0.0 within the segment, and +0.0 + -0.0 = +0.0 in the total"""
    rows, mean = np.array([[-1.0, 1.0], [-2.0, 3.0]]), np.zeros((1, 2))
    tot = tr.statistics(rows, mean, np.zeros((2, 1)), np.zeros(2), np.ones(2, dtype=bool))
    assert (tot["S1"] == 0.0).all() and not np.signbit(tot["S1"]).any()
    again = tr.statistics(rows, mean, np.zeros((2, 1)), np.zeros(2), np.ones(2, dtype=bool), start=dict(tot, S1=-tot["S1"]))
    assert np.signbit(again["S1"][0, 0]) and not np.signbit(again["S1"][0, 1])     # -0.0 + -0.0 = -0.0: the partial was -0.0


def test_update_starved_kept_and_floored():
    w, mean, cov = random_joint(4, 3, 5)
    rng = np.random.default_rng(6)
    rows = np.concatenate([mean[0] + rng.normal(size=(40, 3)), mean[1] + rng.normal(size=(2, 3)),
                           mean[2] + np.outer(rng.normal(size=30), [1.0, 2.0, -1.0]), mean[3] + 0.01 * rng.normal(size=(30, 3))])
    gamma = np.zeros((102, 4))
    gamma[:40, 0], gamma[40:42, 1], gamma[42:72, 2], gamma[72:, 3] = 1.0, 1.0, 1.0, 1.0
    tot = tr.statistics(rows, mean, gamma, np.zeros(102), np.ones(102, dtype=bool))
    floor = np.array([0.5, 0.5, 0.5])
    nw, nmean, ncov, starved, kept = tr.update(w, mean, cov, tot, min_occupancy=3.0)
    assert (starved, kept) == (1, 1)                   # mixture 1 has N = 2 < 3; mixture 2's frames lie on a line: no Cholesky
    for m in (1, 2):
        assert nw[m] == w[m] and np.array_equal(nmean[m], mean[m]) and np.array_equal(ncov[m], cov[m])
    assert nw[0] == 40.0 / 102.0 and not np.array_equal(nmean[0], mean[0]) and (np.diag(ncov[3]) < 1e-3).all()
    fw, fmean, fcov, starved, kept = tr.update(w, mean, cov, tot, min_occupancy=3.0, floor=floor)
    assert (starved, kept) == (1, 1)                   # the line's variances lie above this floor: it is kept still
    assert (np.diag(fcov[3]) == 0.5).all() and np.array_equal(np.tril(fcov[3], -1), np.tril(ncov[3], -1)) and np.array_equal(fcov[3], fcov[3].T)
    assert np.array_equal(fcov[0], ncov[0]) or (np.diag(ncov[0]) < 0.5).any()
    high = tr.update(w, mean, cov, tot, min_occupancy=3.0, floor=np.full(3, 8.0))
    assert high[3:] == (1, 0) and (np.diag(high[2][2]) == 8.0).all()       # a floor above them makes it positive definite
    # NaN occupancies starve: !(N >= min_occupancy)
    bad = dict(tot, N=np.array([np.nan, 2.0, 30.0, 30.0]))
    assert tr.update(w, mean, cov, bad, min_occupancy=1.0)[3] == 1


@pytest.mark.parametrize("n_mix,D", [(1, 2), (3, 5), (2, 17)])
def test_the_joint_preparation_is_creates_rule_on_the_whole_matrix(n_mix, D):
    """gmm_rule.prepare with the joint matrix taken as Sxx (dx := D) next to one more dimension of its own"""
    w, mean, cov = random_joint(n_mix, D, 10 * D + n_mix)
    big = np.zeros((n_mix, D + 1, D + 1))
    big[:, :D, :D], big[:, D, D] = cov, 1.0
    want = gm.prepare(w, np.concatenate([mean, np.zeros((n_mix, 1))], axis=1), big, D, 1)
    got = tr.prepare(w, mean, cov)
    assert np.array_equal(got["W"], want["W"]) and np.array_equal(got["c"], want["c"]) and np.array_equal(got["mux"], want["mux"])
    broken = cov.copy()
    broken[n_mix - 1, 1, 1] = broken[n_mix - 1, 1, 0] ** 2 / broken[n_mix - 1, 0, 0] - 1e-3
    with pytest.raises(ValueError, match="mixture %d, row 1: the joint covariance is not positive definite" % (n_mix - 1)):
        tr.prepare(w, mean, broken)
    assert tr.factor(broken)[2].tolist() == [-1] * (n_mix - 1) + [1]


def test_loglik_rises_strictly_over_five_iterations_on_the_planted_fixture():
    rows, (w, mean, cov) = tr.planted()
    assert rows.shape == (3000, 4) and mean.shape == (3, 4)
    _, ll = tr.iterate(w, mean, cov, rows, 5)
    assert all(b > a for a, b in zip(ll, ll[1:])), ll
    # by far more than the device's exp and log can move a total: the GPU test asserts strict increase without a margin
    assert min(b - a for a, b in zip(ll, ll[1:])) > 1e-6 * abs(ll[0])


def conversion_error(model, joint, dx):
    """the mean squared error of the converted rows against the target, and of MLPG's statics (the target's first three columns as
    statics, the next three as deltas whose variances are +inf: the planted deltas are not the statics' deltas)"""
    import features_rule as fr
    w, mean, cov = model
    n = len(joint)
    got, var, _, _ = gm.convert(gm.prepare(w, mean, cov, dx, joint.shape[1] - dx), joint[:, :dx])
    rows_mean, rows_var = np.zeros((n, fr.width(3, 0, 2))), np.ones((n, fr.width(3, 0, 2)))
    rows_mean[:, :6], rows_var[:, :6] = got, var
    rows_var[:, 3:6] = np.inf
    static = fr.mlpg([n], 3, 0, 2, rows_mean, rows_var, True)
    return float(((got - joint[:, dx:]) ** 2).mean()), float(((static[:, :3] - joint[:, dx:dx + 3]) ** 2).mean())


def test_eight_iterations_lower_the_conversion_error_on_the_planted_pair():
    from world_class_amd.gmm_train import initial_model
    joint = tr.planted_pair()
    assert joint.shape == (2000, 12)
    start = initial_model(joint, 4, 1)
    trained, ll = tr.iterate(*start, joint, 8)
    before, after = conversion_error(start, joint, 6), conversion_error(trained, joint, 6)
    assert after[0] < 0.5 * before[0] and after[1] < 0.5 * before[1], (before, after)
    assert all(b >= a for a, b in zip(ll, ll[1:]))
