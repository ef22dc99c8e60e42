"""-m gpu: the trainer of include/world_class_gmm_train.h against tests/gmm_train_rule.py.

Posteriors and frame_ll against the rule with libm inside the bounds of the device's exp and log.  U, their error in ulp: the ROCm
tree carries no accuracy table, so U was measured on this file's own arguments (tools/gmm_train_probe.py --ulp: exp 1 ulp, log 1 ulp
at the most against libm) and is twice that.  Everything behind the posteriors bit for bit: the statistics against the rule fed with
the device's own gamma and frame_ll, the update against the rule's update on the device's own statistics."""
import threading

import numpy as np
import pytest

import gmm_rule as gm
import gmm_train_rule as tr
from test_gmm_train_rule import random_joint
from test_gpu_gmm import DT, bits, nan_filled, same, untouched

pytestmark = pytest.mark.gpu

U = 2.0
EPS = 2.0 ** -53
SHAPES = [(2, 1), (5, 3), (17, 70), (65, 9), (192, 8)]            # (D, n_mix)
LENGTHS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 3073)
LONG = {(2, 1): LENGTHS, (5, 3): LENGTHS, (17, 70): (65, 1025, 3073), (65, 9): (64, 2049), (192, 8): (1, 1025)}


@pytest.fixture(scope="module")
def env():
    import torch
    import world_class_amd as w
    from world_class_amd import gmm_train
    w.lib().wc_set_device(0)
    return w, gmm_train, torch


_TRAINERS = {}


def trainer(env, D, n_mix):
    """one trainer and model per shape for the whole module; every test leaves its statistics cleared"""
    if (D, n_mix) not in _TRAINERS:
        w, gt, torch = env
        weight, mean, cov = random_joint(n_mix, D, 100 * D + n_mix)
        mean = mean * (0.5 if D <= 17 else 1.0)      # the small shapes' mixtures overlap
        t = gt.GmmTrainer(n_mix, max(1, D // 2), D - max(1, D // 2))
        t.set_model(weight, mean, cov)
        _TRAINERS[(D, n_mix)] = dict(t=t, weight=weight, mean=mean, cov=cov)
    return _TRAINERS[(D, n_mix)]


def frames(mdl, n, seed, fmt="f64", bad=True):
    """n joint rows around the mixtures' means; where bad, a few that are not finite"""
    mean = mdl["mean"]
    rng = np.random.default_rng(seed)
    x = mean[rng.integers(0, mean.shape[0], size=n)] + 0.8 * rng.normal(size=(n, mean.shape[1]))
    if bad and n >= 63:
        x[5, 0], x[17, -1], x[40, 0], x[n - 1, 0] = np.nan, np.inf, -np.inf, np.nan
    return x.astype(DT[fmt])


def masks(n):
    off = np.ones(n, dtype=np.uint8)
    off[1024:2048] = 0
    if n <= 1024:
        off[:] = 0
    return {"none": None, "every other": (np.arange(n) % 2).astype(np.uint8) * 7, "a segment off": off}


def on_device(env, x, pad=(2, 1), mask=None):
    """x [n, D] inside rows of width D + sum(pad) whose other columns are NaN, with a guard row -> d_rows, ld, col, d_mask"""
    w, gt, torch = env
    n, D = x.shape
    rows = np.full((n + 1, D + sum(pad)), np.nan, dtype=x.dtype)
    rows[:n, pad[0]:pad[0] + D] = x
    d_mask = None if mask is None else torch.from_numpy(np.concatenate([mask, [1]]).astype(np.uint8)).cuda()
    return torch.from_numpy(rows.ravel().copy()).cuda(), D + sum(pad), pad[0], d_mask


def device_posterior(env, mdl, x, mask=None, pad=(2, 1)):
    w, gt, torch = env
    t = mdl["t"]
    n = len(x)
    d_rows, ld, col, d_mask = on_device(env, x, pad, mask)
    d_post, d_fll = nan_filled(torch, (n + 1) * t.n_mix, np.float64), nan_filled(torch, n + 1, np.float64)
    torch.cuda.synchronize()
    t.posterior(n, d_rows, ld, d_post, d_fll, col, d_mask, "f32" if x.dtype == np.float32 else "f64")
    w.lib().wc_synchronize()
    post, fll = d_post.cpu().numpy().reshape(n + 1, t.n_mix), d_fll.cpu().numpy()
    assert untouched(post[n]) and untouched(fll[n:])
    return post[:n].copy(), fll[:n].copy()


def device_stats(env, mdl, x, mask=None, cuts=None, pad=(2, 1), between=None):
    """accumulate in calls of the lengths cuts, then the totals; the statistics are cleared behind them"""
    w, gt, torch = env
    t = mdl["t"]
    n = len(x)
    d_rows, ld, col, d_mask = on_device(env, x, pad, mask)
    torch.cuda.synchronize()
    o = 0
    for k in (cuts or [n]):
        t.accumulate(k, d_rows[o * ld:], ld, col, None if d_mask is None else d_mask[o:], "f32" if x.dtype == np.float32 else "f64")
        o += k
        if between:
            between()
    assert o == n
    out = t.stats()
    t.reset_stats()
    return out


def assert_stats(got, want, n_dropped, what=""):
    N, S1, S2, info = got
    assert same(N, want["N"]), (what, "N")
    assert same(S1, want["S1"]), (what, "S1")
    assert same(S2, want["S2"]), (what, "S2")
    assert bits(np.array([info["loglik"]]))[0] == bits(np.array([want["LL"]]))[0], (what, "LL", info["loglik"], want["LL"])
    assert info["n_live"] == want["n_live"] and info["n_dropped"] == n_dropped, (what, info)


def live_of(gamma):
    return gamma.sum(axis=1) > 0.0


# ---- posteriors ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,n_mix,n", [(2, 1, 65), (5, 3, 1025), (17, 70, 130), (65, 9, 64), (192, 8, 3)])
def test_posteriors_and_frame_ll_lie_inside_the_bounds_of_exp_and_log(env, D, n_mix, n):
    mdl = trainer(env, D, n_mix)
    prep = tr.prepare(mdl["weight"], mdl["mean"], mdl["cov"])
    for fmt in ("f64", "f32"):
        x = frames(mdl, n, seed=n + D, fmt=fmt)
        for name, mask in masks(n).items():
            got_g, got_f = device_posterior(env, mdl, x, mask)
            want_g, want_f, state, (top, logs) = tr.posteriors(prep, x, mask)
            off = state != 1
            assert (got_g[off] == 0.0).all() and not np.signbit(got_g[off]).any() and (got_f[off] == 0.0).all(), (fmt, name)
            if n >= 63 and mask is None:
                assert state[5] == 2 and state[17] == 2 and state[40] == 2 and state[n - 1] == 2
            big = want_g >= 2.0 ** -1000
            err = np.abs(got_g - want_g)
            print("gamma: max err / bound", float((err[big] / (want_g[big] * (2 * U + n_mix + 2) * EPS)).max()) if big.any() else 0.0)
            assert (err[big] <= want_g[big] * (2 * U + n_mix + 2) * EPS).all(), (fmt, name)
            assert (err[~big] <= 2.0 ** -1000).all(), (fmt, name)
            bound = (np.abs(top) + np.abs(logs)) * (U + n_mix + 2) * EPS
            assert (np.abs(got_f - want_f) <= bound).all(), (fmt, name)
            assert np.array_equal(live_of(got_g), state == 1)


# ---- statistics ------------------------------------------------------------------------------------------------------------------------
CASES = [(D, m, n) for D, m in SHAPES for n in LONG[(D, m)]]


@pytest.mark.parametrize("D,n_mix,n", CASES)
def test_statistics_equal_the_rule_on_the_devices_own_posteriors_bit_for_bit(env, D, n_mix, n):
    """both formats, rows inside wider rows whose other columns are NaN, three masks, frames that are not finite dropped and counted"""
    mdl = trainer(env, D, n_mix)
    kinds = ("f64", "f32") if D <= 5 or n in (1, 64, 65) else ("f64",)
    for fmt in kinds:
        x = frames(mdl, n, seed=3 * n + D, fmt=fmt)
        for name, mask in masks(n).items():
            if n == 0:
                got = device_stats(env, mdl, x, mask)
                assert (got[0] == 0.0).all() and (got[2] == 0.0).all() and got[3] == dict(loglik=0.0, n_live=0, n_dropped=0, n_starved=0, n_kept=0)
                continue
            gamma, fll = device_posterior(env, mdl, x, mask)
            live = live_of(gamma)
            counted = np.ones(n, dtype=bool) if mask is None else mask != 0
            want = tr.statistics(x.astype(np.float64), mdl["mean"], gamma, fll, live)
            assert_stats(device_stats(env, mdl, x, mask), want, int((counted & ~live).sum()), (fmt, name))
            if n >= 63 and mask is None:
                assert not live[[5, 17, 40, n - 1]].any() and int((counted & ~live).sum()) == 4


def test_launch_shape_cuts_and_posterior_calls_change_nothing(env):
    """3073 frames at (17, 70): 1, 2 and 0 segments per launch are bit-equal; calls cut at multiples of 1024 equal the one call; a cut
    at 1000 equals the rule for that cut; a posterior call between two accumulates leaves the statistics alone"""
    w, gt, torch = env
    D, n_mix, n = 17, 70, 3073
    mdl = trainer(env, D, n_mix)
    t = mdl["t"]
    x = frames(mdl, n, seed=99)
    mask = masks(n)["every other"]
    gamma, fll = device_posterior(env, mdl, x, mask)
    live = live_of(gamma)
    dropped = int(((mask != 0) & ~live).sum())
    want = tr.statistics(x, mdl["mean"], gamma, fll, live)
    for g in (1, 2, 0):
        t.set_segments_per_launch(g)
        assert_stats(device_stats(env, mdl, x, mask), want, dropped, g)
        g1, f1 = device_posterior(env, mdl, x, mask)
        assert same(g1, gamma) and same(f1, fll)
    t.set_segments_per_launch(2)
    assert_stats(device_stats(env, mdl, x, mask, cuts=[1024, 2048, 1]), want, dropped, "cuts at multiples of 1024")
    t.set_segments_per_launch(0)
    assert_stats(device_stats(env, mdl, x, mask, cuts=[2048, 1025]), want, dropped, "cuts at multiples of 1024")
    want_cut = tr.statistics(x, mdl["mean"], gamma, fll, live, cuts=[1000, n - 1000])
    assert not np.array_equal(want_cut["S2"], want["S2"])
    assert_stats(device_stats(env, mdl, x, mask, cuts=[1000, n - 1000]), want_cut, dropped, "a cut at 1000")
    d_rows, ld, col, d_mask = on_device(env, x, (0, 0), mask)
    d_post = nan_filled(torch, n * n_mix, np.float64)
    between = lambda: t.posterior(n, d_rows, ld, d_post, None, col, d_mask)
    assert_stats(device_stats(env, mdl, x, mask, cuts=[1024, 2048, 1], between=between), want, dropped, "posterior between")
    w.lib().wc_synchronize()
    assert same(d_post.cpu().numpy().reshape(n, n_mix), gamma)


# ---- update ----------------------------------------------------------------------------------------------------------------------------
def test_update_equals_the_rule_on_the_devices_own_statistics(env):
    """five mixtures over integer clusters far apart: 0 and 1 ordinary; 2 far from every frame (starved); 3 over twelve identical frames
    (its covariance is exactly 0: kept without a floor, floored with one); 4 over six frames, starved at min_occupancy 8"""
    w, gt, torch = env
    D, n_mix = 4, 5
    rng = np.random.default_rng(31)
    centres = 500.0 * np.array([[0, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64)
    x = np.concatenate([centres[0] + rng.integers(-3, 4, size=(40, D)), centres[1] + rng.integers(-3, 4, size=(30, D)),
                        np.tile(centres[3] + 1.0, (12, 1)), centres[4] + rng.integers(-3, 4, size=(6, D))]).astype(np.float64)
    x = x[rng.permutation(len(x))]
    model = (np.full(n_mix, 0.2), centres + 0.5, np.tile(np.eye(D), (n_mix, 1, 1)))
    t = gt.GmmTrainer(n_mix, 2, 2)
    mdl = dict(t=t, mean=model[1])
    for floor, min_occ, expect in ((None, 8.0, (2, 1)), (np.full(D, 0.25), 8.0, (2, 0)), (np.full(D, 0.25), 1.0, (1, 0))):
        t.set_model(*model)
        d_rows, ld, col, _ = on_device(env, x, (0, 0))
        t.accumulate(len(x), d_rows, ld, col)
        N, S1, S2, info = t.stats()
        assert N.tolist() == [40.0, 30.0, 0.0, 12.0, 6.0] and info["n_live"] == 88 and info["n_dropped"] == 0
        got_info = t.update(min_occ, floor)
        tot = dict(N=N, S1=S1, S2=S2, LL=info["loglik"], n_live=info["n_live"])
        ww, wm, wc, starved, kept = tr.update(*model, tot, min_occ, floor)
        assert (starved, kept) == expect == (got_info["n_starved"], got_info["n_kept"])
        assert got_info["loglik"] == info["loglik"] and got_info["n_live"] == 88
        gw, gm_, gc = t.model()
        assert same(gw, ww) and same(gm_, wm) and same(gc, wc)
        assert np.array_equal(gc, gc.transpose(0, 2, 1)) and np.array_equal(gm_[2], model[1][2])
        after = t.stats()
        assert (after[0] == 0.0).all() and (after[2] == 0.0).all() and after[3]["n_live"] == 0 and after[3]["loglik"] == 0.0   # cleared
        if floor is not None:
            assert (np.diag(gc[3]) == 0.25).all() and (gc[3][~np.eye(D, dtype=bool)] == 0.0).all()
        else:
            assert np.array_equal(gc[3], np.eye(D)) and gw[3] == 0.2
        # the model in force on the device is the updated one: its posteriors follow the rule on it
        g2, _ = device_posterior(env, mdl, x[:8])
        want_g = tr.posteriors(tr.prepare(gw, gm_, gc), x[:8])[0]
        assert np.abs(g2 - want_g).max() <= (2 * U + n_mix + 2) * EPS
    t.close()


def test_five_fit_iterations_on_the_planted_fixture(env):
    """loglik rises strictly (test_gmm_train_rule.py shows the rule's does, by a margin far above the bound below), and every total
    lies within the frame_ll bound, summed over the frames, of the rule run on the device's own successive models"""
    w, gt, torch = env
    rows, start = tr.planted()
    n, D = rows.shape
    t = gt.GmmTrainer(3, 2, 2)
    t.set_model(*start)
    d_rows = torch.from_numpy(rows.ravel().copy()).cuda()
    torch.cuda.synchronize()
    totals = []
    for k in range(5):
        model = t.model()
        info, = t.fit(d_rows, n, D, 1)
        want_g, want_f, state, (top, logs) = tr.posteriors(tr.prepare(*model), rows)
        want = tr.statistics(rows, model[1], want_g, want_f, state == 1)["LL"]
        bound = float(((np.abs(top) + np.abs(logs)) * (U + 3 + 2) * EPS).sum())
        print("iteration", k, "loglik", info["loglik"], "rule", want, "difference", abs(info["loglik"] - want), "bound", bound)
        assert abs(info["loglik"] - want) <= bound
        assert info["n_live"] == n and info["n_starved"] == 0 and info["n_kept"] == 0
        totals.append(info["loglik"])
    assert all(b > a for a, b in zip(totals, totals[1:])), totals
    t2 = gt.GmmTrainer(3, 2, 2)
    t2.set_model(*start)
    again = [i["loglik"] for i in t2.fit(d_rows, n, D, 5)]
    assert again == totals and all(same(a, b) for a, b in zip(t.model(), t2.model()))      # fit is the loop
    t.close()
    t2.close()


# ---- refusals and threads --------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_statistics_model_and_outputs_untouched(env):
    w, gt, torch = env
    L = gt._L()
    for args in ((0, 1, 1), (1025, 1, 1), (1, 0, 2), (1, 2, 0), (1, 100, 93), (1, -1, 5)):
        assert not L.wc_gmm_trainer_create(*args) and "gmm trainer create" in w.last_error()
    D, n_mix, n = 5, 3, 100
    mdl = trainer(env, D, n_mix)
    x = frames(mdl, n, seed=1, bad=False)
    d_rows, ld, col, d_mask = on_device(env, x, (2, 1), np.ones(n, dtype=np.uint8))
    fresh = gt.GmmTrainer(n_mix, 2, 3)
    big = nan_filled(torch, 2 * n * n_mix + 2 * n, np.float64)
    post, fll = big[:n * n_mix], big[n * n_mix:n * n_mix + n]
    torch.cuda.synchronize()
    h = fresh._h
    acc = lambda h=h, nf=n, f=0, rows=d_rows, ld=ld, col=col, mask=d_mask: L.wc_gmm_trainer_accumulate_device(h, nf, f, w._opt(rows), ld, col, w._opt(mask))
    pos = lambda h=h, nf=n, f=0, rows=d_rows, ld=ld, col=col, mask=d_mask, p=post, l=fll: L.wc_gmm_trainer_posterior_device(
        h, nf, f, w._opt(rows), ld, col, w._opt(mask), w._opt(p), w._opt(l))

    def refused(rc, text):
        assert rc == -1 and text in w.last_error(), (rc, text, w.last_error())

    # before a model is set
    refused(acc(), "no model is set")
    refused(pos(), "no model is set")
    refused(L.wc_gmm_trainer_update(h, 1.0, None, None), "no model is set")
    refused(L.wc_gmm_trainer_model_host(h, None, None, None), "no model is set")
    # set_model refuses what create refuses, on the joint matrix, and keeps no part of a refused model
    weight, mean, cov = mdl["weight"], mdl["mean"], mdl["cov"]
    hp = gt._host

    def set_model(weight=weight, mean=mean, cov=cov):
        a, b, c = (None if v is None else np.ascontiguousarray(v, dtype=np.float64) for v in (weight, mean, cov))
        return L.wc_gmm_trainer_set_model(h, hp(a), hp(b), hp(c))

    def edited(a, at, v):
        a = a.copy()
        a[at] = v
        return a

    refused(set_model(weight=None), "null array")
    refused(set_model(weight=edited(weight, 1, 0.0)), "mixture 1: a weight")
    refused(set_model(mean=edited(mean, (2, 4), np.inf)), "mixture 2, row 4: a mean")
    refused(set_model(cov=edited(cov, (0, 3, 1), np.nan)), "mixture 0, row 3: a covariance")
    refused(set_model(cov=edited(cov, (1, 4, 4), 0.0)), "mixture 1, row 4: the joint covariance is not positive definite")
    refused(acc(), "no model is set")
    assert set_model(cov=edited(cov, (0, 1, 3), np.nan)) == 0          # entries above the diagonal are never read
    assert all(same(a, b) for a, b in zip(fresh.model(), (weight, mean, cov)))
    refused(set_model(cov=edited(cov, (1, 4, 4), 0.0)), "not positive definite")
    assert all(same(a, b) for a, b in zip(fresh.model(), (weight, mean, cov)))     # the model in force stays
    # accumulate and posterior
    for call in (acc, pos):
        refused(call(h=None), "null handle")
        refused(call(nf=-1), "n_frames")
        refused(call(nf=2 ** 32), "n_frames")
        refused(call(f=2), "format")
        refused(call(f=-1), "format")
        refused(call(col=-1), "negative column")
        refused(call(ld=col + D - 1), "ld < col + D")
        refused(call(col=col + 2), "ld < col + D")
        refused(call(rows=None), "null d_rows")
        assert call(nf=0, rows=None) == 0
    refused(pos(p=None, l=None), "both outputs are NULL")
    refused(pos(l=big[n * n_mix - 1:]), "the two outputs overlap")
    refused(pos(p=d_rows), "overlaps the rows")
    refused(pos(l=d_rows[ld:]), "overlaps the rows")
    # update and the launch setting
    assert acc() == 0
    before = fresh.stats()
    refused(L.wc_gmm_trainer_update(h, 0.5, None, None), "min_occupancy")
    refused(L.wc_gmm_trainer_update(h, float("nan"), None, None), "min_occupancy")
    refused(L.wc_gmm_trainer_update(h, float("inf"), None, None), "min_occupancy")
    refused(L.wc_gmm_trainer_update(h, 1.0, hp(np.array([0.1, 0.1, -0.1, 0.1, 0.1])), None), "a floor")
    refused(L.wc_gmm_trainer_update(h, 1.0, hp(np.array([0.1, np.nan, 0.1, 0.1, 0.1])), None), "a floor")
    refused(L.wc_gmm_trainer_set_segments_per_launch(h, -1), "g < 0")
    refused(L.wc_gmm_trainer_update(None, 1.0, None, None), "null handle")
    after = fresh.stats()
    assert all(same(a, b) for a, b in zip(before[:3], after[:3])) and before[3] == after[3] and before[3]["n_live"] == n
    assert all(same(a, b) for a, b in zip(fresh.model(), (weight, mean, cov)))
    fresh.reset_stats()
    refused(L.wc_gmm_trainer_update(h, 1.0, None, None), "n_live == 0")
    none = np.zeros(n, dtype=np.uint8)
    assert acc(mask=torch.from_numpy(none).cuda()) == 0
    refused(L.wc_gmm_trainer_update(h, 1.0, None, None), "n_live == 0")
    assert all(same(a, b) for a, b in zip(fresh.model(), (weight, mean, cov)))
    w.lib().wc_synchronize()
    assert untouched(big.cpu().numpy())
    # and the calls that follow the refusals work
    assert pos() == 0
    w.lib().wc_synchronize()
    got = big.cpu().numpy()
    want_g, want_f = device_posterior(env, mdl, x, None)
    assert same(got[:n * n_mix].reshape(n, n_mix), want_g) and same(got[n * n_mix:n * n_mix + n], want_f) and untouched(got[n * n_mix + n:])
    fresh.close()


def test_two_trainers_on_two_host_threads_reproduce_the_single_thread(env):
    w, gt, torch = env
    shapes = [(5, 3, 2049), (17, 70, 1025)]
    single, work_items = [], []
    for D, n_mix, n in shapes:
        mdl = trainer(env, D, n_mix)
        x = frames(mdl, n, seed=D)
        single.append(device_stats(env, mdl, x))
        t = gt.GmmTrainer(n_mix, mdl["t"].dx, mdl["t"].dy)
        t.set_model(mdl["weight"], mdl["mean"], mdl["cov"])
        d_rows, ld, col, _ = on_device(env, x, (1, 0))
        work_items.append((t, n, d_rows, ld, col))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    results, errors = [None, None], []

    def work(i):
        try:
            t, n, d_rows, ld, col = work_items[i]
            assert w.lib().wc_set_stream(streams[i].cuda_stream) == 0
            for rep in range(3):
                t.reset_stats()
                t.accumulate(n, d_rows, ld, col)
                results[i] = t.stats()
            assert w.lib().wc_set_stream(None) == 0
        except Exception as e:      # noqa: BLE001 -- handed to the main thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for got, want, item in zip(results, single, work_items):
        assert all(same(a, b) for a, b in zip(got[:3], want[:3])) and got[3] == want[3]
        item[0].close()
