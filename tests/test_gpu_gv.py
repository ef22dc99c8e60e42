"""-m gpu: wc_mlpg_gv_device and wc_gv_stats_device (include/world_class_gv.h) against tests/gv_rule.py, bit for bit, on
wc_mlpg_device's own output.  One batch of lengths [0, 1, 2, 3, 63, 64, 65, 128, 129, 191, 600] plus one utterance on each side of the
LDS threshold (2048 frames), three shapes, orders 2 and 3, rows of doubles and of floats, one row of variances and one per frame, three
masks, max_iter 0, 1 and 5; every output with a guard row of NaN behind it."""
import ctypes as C
import itertools

import numpy as np
import pytest

import features_rule as fr
import gv_rule as gr
from test_gpu_features import _dev, _guarded, _rows, _same
from test_gv_rule import STEP_BOTH, blurred, both_branches_case, masks

pytestmark = pytest.mark.gpu

LDS_FRAMES = 2048   # kGvLdsFrames of wc_gv.hip: the trajectory stands in LDS up to this length and in scratch beyond it
LENGTHS = [0, 1, 2, 3, 63, 64, 65, 128, 129, 191, 600, LDS_FRAMES, LDS_FRAMES + 1]
SHAPES = [(25, 1), (60, 5), (24, 0)]   # (60, 5): 66 static columns


@pytest.fixture(scope="module")
def env():
    import torch
    import world_class_amd as w
    from world_class_amd import features as ft, gv
    w.lib().wc_set_device(0)
    return w, ft, torch, gv


def model(lengths, nd, n_ap, orders, seed, dt=np.float64):
    """the over-smoothed model of tests/test_gv_rule.py for every utterance of a batch, as rows -> mean, var [frames, width], the row of
    variances of one frame, gv_mean, gv_var [S]"""
    S, W = nd + 1 + n_ap, fr.width(nd, n_ap, orders)
    cols, vuv = fr.columns(nd, n_ap, orders)
    take = np.array(cols).T
    t = sum(lengths)
    mean, var = np.zeros((t, W)), np.ones((t, W))
    o = 0
    for u, n in enumerate(lengths):
        if n:
            mu, vr, _, _ = blurred(n, S, orders, seed + u)
            mean[o:o + n][:, take], var[o:o + n][:, take] = mu, vr
        o += n
    mean[:, vuv] = np.random.default_rng(seed).uniform(size=t)
    scale = np.linspace(2.0, 0.2, S)
    gv_mean = 0.76 * scale * scale
    mean, var = mean.astype(dt), var.astype(dt)
    return mean, var, var[min(7, t - 1)].copy(), gv_mean, 0.1 * gv_mean * gv_mean


def batch_masks(lengths):
    """None; silence at both ends and in the middle of every utterance; 0, 1 and 2 frames left in turn.  A mask byte counts where it
    is not 0: 1, 2 and 255 stand for it"""
    t = sum(lengths)
    sil, few = np.zeros(t, dtype=np.uint8), np.zeros(t, dtype=np.uint8)
    o = 0
    for u, n in enumerate(lengths):
        sil[o:o + n] = np.where(masks(n), (1, 2, 255)[u % 3], 0)
        left = np.arange(n)[::max(1, n // 2)][:u % 3]
        few[o + left] = 255
        o += n
    return {"none": None, "silence": sil, "few": few}


def device_mlpg(env, lengths, nd, n_ap, orders, mean, var, per_frame, fmt="f64"):
    """-> the device array of static rows with its guard row, and the means and variances on the device"""
    w, ft, torch, gv = env
    dt = np.float64 if fmt == "f64" else np.float32
    d_static = _guarded(torch, int(sum(lengths)), nd + 2 + n_ap)
    d_mean, d_var = _dev(torch, mean, dt), _dev(torch, var, dt)
    torch.cuda.synchronize()
    ft.mlpg(lengths, nd, n_ap, orders, d_mean, d_var, d_static, per_frame, fmt)
    w.lib().wc_synchronize()
    return d_static, d_mean, d_var


def device_gv(env, lengths, nd, n_ap, orders, d_mean, d_var, per_frame, fmt, gv_mean, gv_var, mask, d_static, **kw):
    """refines a copy of d_static -> the rows"""
    w, ft, torch, gv = env
    d_out = d_static.clone()
    d_mask = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8)).cuda()
    d_gm, d_gvv = _dev(torch, gv_mean), _dev(torch, gv_var)
    torch.cuda.synchronize()
    gv.mlpg_gv(lengths, nd, n_ap, orders, d_mean, d_var, d_gm, d_gvv, d_out, d_mask, per_frame, fmt, **kw)
    w.lib().wc_synchronize()
    return _rows(d_out, int(sum(lengths)), nd + 2 + n_ap)


@pytest.mark.parametrize("orders", [2, 3])
@pytest.mark.parametrize("nd,n_ap", SHAPES)
def test_mlpg_gv_equals_the_rule_bit_for_bit(env, nd, n_ap, orders):
    """no tolerance: division and the square root are correctly rounded, the build keeps every product and sum apart, and the kernel
    adds in THE sum's order"""
    t = sum(LENGTHS)
    mks = batch_masks(LENGTHS)
    moved = 0
    for fmt, dt in (("f64", np.float64), ("f32", np.float32)):
        mean, var, var_row, gv_mean, gv_var = model(LENGTHS, nd, n_ap, orders, 17 * nd + orders, dt)
        for per_frame, v in ((True, var), (False, var_row)):
            d_static, d_mean, d_var = device_mlpg(env, LENGTHS, nd, n_ap, orders, mean, v, per_frame, fmt)
            static = _rows(d_static, t, nd + 2 + n_ap)
            assert np.isfinite(static).all()
            for (name, mask), max_iter in itertools.product(mks.items(), (0, 1, 5)):
                got = device_gv(env, LENGTHS, nd, n_ap, orders, d_mean, d_var, per_frame, fmt, gv_mean, gv_var, mask, d_static, max_iter=max_iter)
                want = gr.mlpg_gv(LENGTHS, nd, n_ap, orders, mean.astype(np.float64), v.astype(np.float64), per_frame, gv_mean, gv_var, mask,
                                  static, max_iter=max_iter)
                assert _same(got, want), (fmt, per_frame, name, max_iter)
                assert np.isfinite(got).all()
                assert np.array_equal(got[:, nd + 1], static[:, nd + 1])           # vuv is never touched
                if mask is not None:                                                # unmasked frames are never written
                    assert np.array_equal(got[mask == 0].view(np.int64), static[mask == 0].view(np.int64))
                moved += int((got != static).any())
    assert moved == 2 * 2 * 9


def test_a_step_that_halves_and_grows(env):
    """tests/test_gv_rule.py proves that this case's trace takes both branches of the step; here bit equality is all it takes"""
    n, S, mu, vr, gv_mean, gv_var = both_branches_case()
    nd, n_ap, orders = S - 2, 1, 3
    cols, vuv = fr.columns(nd, n_ap, orders)
    mean, var = np.zeros((n, fr.width(nd, n_ap, orders))), np.ones((n, fr.width(nd, n_ap, orders)))
    mean[:, np.array(cols).T], var[:, np.array(cols).T] = mu, vr
    d_static, d_mean, d_var = device_mlpg(env, [n], nd, n_ap, orders, mean, var, True)
    static = _rows(d_static, n, S + 1)
    assert _same(static, fr.mlpg([n], nd, n_ap, orders, mean, var, True))
    got = device_gv(env, [n], nd, n_ap, orders, d_mean, d_var, True, "f64", gv_mean, gv_var, None, d_static, step_init=STEP_BOTH, max_iter=5)
    traces = []
    want = gr.mlpg_gv([n], nd, n_ap, orders, mean, var, True, gv_mean, gv_var, None, static, step_init=STEP_BOTH, max_iter=5, traces=traces)
    steps = np.array([s["step"] for s in traces[0][:-1]])
    assert (steps[1:] < steps[:-1]).any() and (steps[1:] > steps[:-1]).any()
    assert _same(got, want)
    # the weights reach the kernel: other weights, other bits, and the rule's
    got2 = device_gv(env, [n], nd, n_ap, orders, d_mean, d_var, True, "f64", gv_mean, gv_var, None, d_static, w_ml=1.5, w_gv=0.25, max_iter=3)
    assert _same(got2, gr.mlpg_gv([n], nd, n_ap, orders, mean, var, True, gv_mean, gv_var, None, static, w_ml=1.5, w_gv=0.25, max_iter=3))
    assert not _same(got2, got)


@pytest.mark.parametrize("nd,n_ap", SHAPES)
def test_stats_equal_the_rule(env, nd, n_ap):
    w, ft, torch, gv = env
    S, t = nd + 1 + n_ap, sum(LENGTHS)
    rng = np.random.default_rng(nd)
    static = rng.standard_normal((t, S + 1)) * np.linspace(3.0, 0.1, S + 1) + rng.standard_normal(S + 1)
    d_static = _dev(torch, static)
    for name, mask in batch_masks(LENGTHS).items():
        d_m, d_v = _guarded(torch, len(LENGTHS), S), _guarded(torch, len(LENGTHS), S)
        d_mask = None if mask is None else torch.from_numpy(mask).cuda()
        torch.cuda.synchronize()
        gv.stats(LENGTHS, nd, n_ap, d_static, d_m, d_v, d_mask)
        w.lib().wc_synchronize()
        mean, var = gr.stats(LENGTHS, nd, n_ap, static, mask)
        assert _same(_rows(d_m, len(LENGTHS), S), mean) and _same(_rows(d_v, len(LENGTHS), S), var), name
        assert np.isnan(mean[0]).all() and (name == "few" or np.isfinite(mean[-1]).all())      # length 0, or no frame left: 0.0 / 0.0
        if name == "none":   # the rule's sum against numpy's
            x = np.delete(static[-(LDS_FRAMES + 1):], nd + 1, axis=1)
            assert np.abs(var[-1] - x.var(axis=0)).max() <= 1e-12 * x.var(axis=0).max()
    assert bool((d_static == _dev(torch, static)).all())
    # utterances and no frames at all: NaN for each, from NULL rows
    d_m, d_v = _guarded(torch, 2, S), _guarded(torch, 2, S)
    torch.cuda.synchronize()
    gv.stats([0, 0], nd, n_ap, None, d_m, d_v)
    w.lib().wc_synchronize()
    assert np.isnan(_rows(d_m, 2, S)).all() and np.isnan(_rows(d_v, 2, S)).all()


def test_bad_global_variances_and_the_switch(env):
    """each bad GV value makes exactly its static column NaN in every utterance and touches nothing else; +inf leaves the column
    bitwise as MLPG wrote it, its gv_mean unread"""
    nd, n_ap, orders = 60, 5, 3
    lengths = [n for n in LENGTHS if n <= 600]
    mean, var, var_row, gv_mean, gv_var = model(lengths, nd, n_ap, orders, 3)
    d_static, d_mean, d_var = device_mlpg(env, lengths, nd, n_ap, orders, mean, var, True)
    static = _rows(d_static, sum(lengths), nd + 2 + n_ap)
    base = device_gv(env, lengths, nd, n_ap, orders, d_mean, d_var, True, "f64", gv_mean, gv_var, None, d_static)
    gm, gv_ = gv_mean.copy(), gv_var.copy()
    # static columns 0, 63 (behind vuv: output column 64), lf0 (60), a band (62 -> 63) ...
    bad = {0: ("var", np.nan), 63: ("var", 0.0), 60: ("var", -1.0), 62: ("mean", np.nan), 5: ("mean", 0.0), 6: ("mean", -3.0), 7: ("mean", np.inf),
           8: ("var", -np.inf)}
    for c, (which, value) in bad.items():
        (gm if which == "mean" else gv_)[c] = value
    off = [9, 61]
    gv_[off], gm[9] = np.inf, np.nan
    for mask in (None, batch_masks(lengths)["silence"]):
        got = device_gv(env, lengths, nd, n_ap, orders, d_mean, d_var, True, "f64", gm, gv_, mask, d_static)
        assert _same(got, gr.mlpg_gv(lengths, nd, n_ap, orders, mean, var, True, gm, gv_, mask, static))
        ref = base if mask is None else device_gv(env, lengths, nd, n_ap, orders, d_mean, d_var, True, "f64", gv_mean, gv_var, mask, d_static)
        on = np.ones(len(got), dtype=bool) if mask is None else mask != 0
        out_col = lambda c: c if c <= nd else c + 1
        hit = np.zeros(got.shape, dtype=bool)
        for c in bad:
            hit[on, out_col(c)] = True
        assert np.isnan(got[hit]).all() and np.array_equal(got[~hit & ~np.isin(np.arange(got.shape[1]), [out_col(c) for c in off])],
                                                           ref[~hit & ~np.isin(np.arange(got.shape[1]), [out_col(c) for c in off])])
        for c in off:
            assert np.array_equal(got[:, out_col(c)].view(np.int64), static[:, out_col(c)].view(np.int64))
        assert not np.array_equal(ref[:, 9], static[:, 9])


@pytest.mark.parametrize("nd,n_ap", SHAPES[:2])
def test_an_utterance_does_not_depend_on_its_neighbours(env, nd, n_ap):
    orders = 3
    mean, var, var_row, gv_mean, gv_var = model(LENGTHS, nd, n_ap, orders, 50 + nd)
    mask = batch_masks(LENGTHS)["silence"]
    d_static, d_mean, d_var = device_mlpg(env, LENGTHS, nd, n_ap, orders, mean, var, True)
    whole = device_gv(env, LENGTHS, nd, n_ap, orders, d_mean, d_var, True, "f64", gv_mean, gv_var, mask, d_static)
    o = 0
    for n in LENGTHS:
        s = slice(o, o + n)
        d_s, d_m, d_v = device_mlpg(env, [n], nd, n_ap, orders, mean[s], var[s], True)
        assert _same(device_gv(env, [n], nd, n_ap, orders, d_m, d_v, True, "f64", gv_mean, gv_var, mask[s], d_s), whole[s]), n
        o += n
    # and not on the order either: the batch reversed (the long utterances first: the scratch planes of the others move)
    offs = np.concatenate([[0], np.cumsum(LENGTHS)])
    idx = np.concatenate([np.arange(offs[u], offs[u + 1]) for u in range(len(LENGTHS) - 1, -1, -1)]).astype(int)
    d_s, d_m, d_v = device_mlpg(env, LENGTHS[::-1], nd, n_ap, orders, mean[idx], var[idx], True)
    assert _same(device_gv(env, LENGTHS[::-1], nd, n_ap, orders, d_m, d_v, True, "f64", gv_mean, gv_var, mask[idx], d_s), whole[idx])


def test_refused_calls_leave_the_outputs_untouched(env):
    """every refusal of the header, for both calls: WC_ERR_INVALID with a text, the outputs still NaN and the rows as they were"""
    w, ft, torch, gv = env
    nd, n_ap, lengths = 25, 1, [3, 64]
    t, S = sum(lengths), nd + 1 + n_ap
    L = gv._L()
    ints = lambda v: (C.c_int * len(v))(*v)
    W = fr.width(nd, n_ap, 3)
    mean, var = _dev(torch, np.ones(t * W)), _dev(torch, np.ones(W))
    static = _dev(torch, np.tile(np.arange(S + 1.0), t))
    gm, gvv = _dev(torch, np.ones(S)), _dev(torch, np.ones(S))
    mask = torch.ones(t, dtype=torch.uint8, device="cuda")
    o_m, o_v = _guarded(torch, 2, S), _guarded(torch, 2, S)
    p = lambda x: None if x is None else x.data_ptr()
    huge = [2 ** 31 - 1, 2 ** 31 - 1, 2]   # 2^32 frames
    nan, inf = float("nan"), float("inf")
    torch.cuda.synchronize()

    def refine(n_utt=2, ln=ints(lengths), nd_=nd, n_ap_=n_ap, orders=3, fmt=0, m=mean, v=var, per_frame=0, a=gm, b=gvv, k=mask, w_ml=1.0, w_gv=1.0,
               step=0.1, it=5, out=static):
        return L.wc_mlpg_gv_device(n_utt, ln, nd_, n_ap_, orders, fmt, p(m), p(v), per_frame, p(a), p(b), p(k), w_ml, w_gv, step, it, p(out))

    def stats(n_utt=2, ln=ints(lengths), nd_=nd, n_ap_=n_ap, rows=static, k=mask, a=o_m, b=o_v):
        return L.wc_gv_stats_device(n_utt, ln, nd_, n_ap_, p(rows), p(k), p(a), p(b))

    refused = [
        refine(nd_=0), refine(n_ap_=-1), refine(orders=1), refine(orders=4), refine(fmt=2), refine(fmt=-1), refine(per_frame=2),
        refine(ln=ints([-3, 64])), refine(n_utt=-1), refine(n_utt=3, ln=ints(huge)), refine(ln=None),
        refine(it=-1), refine(it=65), refine(w_ml=nan), refine(w_ml=-1.0), refine(w_ml=inf), refine(w_ml=0.0), refine(w_gv=nan), refine(w_gv=-0.5),
        refine(w_gv=inf), refine(step=nan), refine(step=-0.1), refine(step=inf),
        refine(m=None), refine(v=None), refine(a=None), refine(b=None), refine(out=None), refine(a=None, it=0),
        refine(out=mean), refine(out=var), refine(a=static), refine(b=static), refine(k=static),
        stats(nd_=0), stats(n_ap_=-1), stats(ln=ints([3, -1])), stats(n_utt=-1), stats(n_utt=3, ln=ints(huge)), stats(ln=None),
        stats(rows=None), stats(a=None), stats(b=None), stats(a=o_m, b=o_m), stats(a=static), stats(b=static),
    ]
    w.lib().wc_synchronize()
    assert all(rc < 0 for rc in refused), refused
    assert "gv" in w.last_error()
    assert bool(torch.isnan(o_m).all()) and bool(torch.isnan(o_v).all())
    assert bool((static == _dev(torch, np.tile(np.arange(S + 1.0), t))).all())
    for kept in (mean, var, gm, gvv):
        assert bool((kept == 1.0).all())
    # the same arguments, not refused; max_iter == 0 reads no means and no variances; a w_gv and a step of 0 are weights like others
    assert stats() == 0 and refine(m=None, v=None, it=0) == 0 and refine(w_gv=0.0, step=0.0) == 0 and refine() == 0 and refine(k=None) == 0
    assert refine(n_utt=0, ln=None, out=None) == 0 and stats(n_utt=0, ln=None, a=None, b=None) == 0
    w.lib().wc_synchronize()
    assert not bool(torch.isnan(o_m[:2 * S]).any()) and bool(torch.isnan(o_m[2 * S:]).all())


def test_numpy_front_end(env):
    w, ft, torch, gv = env
    nd, n_ap, orders, lengths = 6, 2, 3, [70, 5]
    S = nd + 1 + n_ap
    mean, var, var_row, gv_mean, gv_var = model(lengths, nd, n_ap, orders, 8)
    means, variances = [mean[:70], mean[70:]], [var[:70], var[70:]]
    mks = [masks(70), np.ones(5, dtype=bool)]
    st = ft.mlpg_host(means, variances, nd, n_ap, orders)
    out = gv.mlpg_gv_host(means, variances, st, gv_mean, gv_var, nd, n_ap, orders, masks=mks)
    want = gr.mlpg_gv(lengths, nd, n_ap, orders, mean, var, True, gv_mean, gv_var, np.concatenate(mks), np.concatenate(st))
    assert _same(np.concatenate(out), want)
    sc = gv.scale_host(st, gv_mean, gv_var, nd, n_ap)
    assert _same(np.concatenate(sc), gr.mlpg_gv(lengths, nd, n_ap, orders, None, None, False, gv_mean, gv_var, None, np.concatenate(st), max_iter=0))
    m, v = gv.stats_host(sc, nd, n_ap)
    assert m.shape == v.shape == (2, S) and np.abs(v / gv_mean - 1.0).max() <= 1e-12
    m2, v2 = gv.stats_host(out, nd, n_ap, masks=mks)
    rm, rv = gr.stats(lengths, nd, n_ap, np.concatenate(out), np.concatenate(mks))
    assert _same(m2, rm) and _same(v2, rv)
    one = gv.mlpg_gv_host(means, var_row, ft.mlpg_host(means, var_row, nd, n_ap, orders), gv_mean, gv_var, nd, n_ap, orders, max_iter=2, step_init=0.2)
    assert one[0].shape == (70, S + 1) and np.isfinite(np.concatenate(one)).all()
