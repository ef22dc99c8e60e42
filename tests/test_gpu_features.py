"""-m gpu: model features on the device (include/world_class_features.h): wc_pack_model_features_device and
wc_unpack_model_features_device against tests/features_rule.py.  One batch of lengths [0, 1, 2, 3, 64, 65, 191, 600] at three
shapes, three sets of contours over it; every output with a guard row of NaN behind it."""
import ctypes as C

import numpy as np
import pytest

import features_rule as fr

pytestmark = pytest.mark.gpu

LOG_EXP_REL = 1e-12   # log / exp of two math libraries: the project's bound (tests/test_gpu_morph.py)
LENGTHS = [0, 1, 2, 3, 64, 65, 191, 600]
SHAPES = [(25, 1), (60, 5), (24, 0)]   # (60, 5): 66 static columns, more than one wavefront; (24, 0): no bands, a NULL d_coded_ap
FILL = -3.25


@pytest.fixture(scope="module")
def env():
    import torch
    import world_class_amd as w
    from world_class_amd import features as ft
    w.lib().wc_set_device(0)
    return w, ft, torch


def _dev(torch, a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype).ravel().copy()).cuda()


def _guarded(torch, n, width, dtype=np.float64):
    """n rows of NaN with a guard row of NaN behind them"""
    return torch.full(((n + 1) * width,), np.nan, dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda")


def _rows(t, n, width):
    a = t.cpu().numpy().reshape(n + 1, width)
    assert np.isnan(a[n]).all(), "the guard row was written"
    return a[:n]


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def _gaps(n, gaps, first=5):
    """voiced everywhere but in runs of the given lengths, each between two voiced frames, the first behind frame `first`"""
    v = np.ones(n, dtype=bool)
    i = first + 1
    for g in gaps:
        v[i:i + g] = False
        i += g + 2
    assert i <= n
    return v


def contours(variant, rng):
    """F0 of the batch.  Over the three variants: all unvoiced (the fill), all voiced, one voiced frame at the first, a middle and the
    last index, unvoiced runs at both ends, gaps of 63, 64, 65 and 300 frames (they cross the scan's carries), NaN, -1 and +inf"""
    out = []
    for n in LENGTHS:
        f = rng.uniform(70.0, 500.0, n)
        v = np.ones(n, dtype=bool)
        one = lambda i: np.arange(n) == i
        if variant == 0:
            v = {1: v, 2: ~v, 3: one(1), 64: v, 65: one(0), 191: v, 600: _gaps(600, [63, 64, 65, 300])}.get(n, v)
            if n == 191:
                v[:17], v[150:] = False, False   # unvoiced runs at both ends
        elif variant == 1:
            v = {1: ~v, 2: one(1), 3: v, 64: one(63), 65: ~v, 191: one(95), 600: rng.uniform(size=n) < 0.4}.get(n, v)
            if n == 600:
                v[:70], v[-131:] = False, False
        else:
            v = {1: v, 2: one(0), 3: one(2), 64: one(0), 65: one(64), 191: _gaps(191, [63, 64], first=0), 600: ~v}.get(n, v)
        f = np.where(v, f, 0.0)
        if n >= 64:   # unvoiced values that are not 0
            for i, bad in zip(np.flatnonzero(~v)[:3], (np.nan, -1.0, np.inf)):
                f[i] = bad
        if n == 191 and variant == 0:
            f[40], f[41], f[90] = np.nan, -1.0, np.inf   # inside the voiced stretch: they open gaps of their own
        out.append(f)
    return np.concatenate(out)


def batch(nd, n_ap, variant):
    rng = np.random.default_rng(1000 * nd + 10 * n_ap + variant)
    t = sum(LENGTHS)
    f0 = contours(variant, rng)
    sp = rng.standard_normal((t, nd)) * np.linspace(3.0, 0.05, nd)
    ap = -rng.uniform(0.0, 40.0, (t, n_ap))
    if variant == 0:   # values that are not finite travel through as they are
        sp[300, 3], sp[301, 3], sp[500, nd - 1] = np.nan, np.inf, -np.inf
    return f0, sp, ap


def device_pack(env, lengths, nd, n_ap, orders, f0, sp, ap, fmt="f64", fill=FILL):
    w, ft, torch = env
    t, W = int(sum(lengths)), fr.width(nd, n_ap, orders)
    dt = np.float64 if fmt == "f64" else np.float32
    d_rows = _guarded(torch, t, W, dt)
    torch.cuda.synchronize()
    ft.pack(lengths, nd, n_ap, orders, _dev(torch, f0), _dev(torch, sp), _dev(torch, ap) if n_ap else None, d_rows, fill, fmt)
    w.lib().wc_synchronize()
    return _rows(d_rows, t, W)


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("nd,n_ap", SHAPES)
def test_pack_equals_the_rule(env, nd, n_ap, variant):
    """the voiced lf0 within LOG_EXP_REL of np.log; everything else -- the interpolated lf0, every delta, vuv, the float rows -- the
    rule on the device's own voiced logs, bit for bit"""
    f0, sp, ap = batch(nd, n_ap, variant)
    v = fr.voiced(f0)
    logs = None
    for orders in (3, 1, 2):
        got = device_pack(env, LENGTHS, nd, n_ap, orders, f0, sp, ap)
        lf0 = got[:, orders * nd]
        if logs is None:
            logs = lf0.copy()
            rel = (np.abs(logs[v] - np.log(f0[v])) / np.abs(np.log(f0[v]))).max() if v.any() else 0.0
            print("pack nd %d n_ap %d variant %d: voiced log against numpy %.3e (relative)" % (nd, n_ap, variant, rel))
            assert rel < LOG_EXP_REL
        assert np.array_equal(lf0[v], logs[v])   # (the same logs at every order)
        want = fr.pack(LENGTHS, nd, n_ap, orders, f0, sp, ap, FILL, logs=logs)
        assert _same(got, want), orders
        assert np.array_equal(got[:, orders * (nd + 1)], v.astype(np.float64))
        got32 = device_pack(env, LENGTHS, nd, n_ap, orders, f0, sp, ap, "f32")
        with np.errstate(over="ignore"):
            assert _same(got32, want.astype(np.float32)), orders
    if variant == 0:
        assert np.isnan(got[300, 3]) and np.isinf(got[301, 3]) and np.isfinite(got[:, 4:nd - 1]).all()   # they touch their own column only


def test_pack_fill_and_single_utterances(env):
    """an utterance does not depend on its neighbours in the batch; with nothing voiced every frame holds lf0_fill, +-inf and -0.0
    included; empty calls write nothing"""
    w, ft, torch = env
    nd, n_ap = 25, 1
    f0, sp, ap = batch(nd, n_ap, 0)
    whole = device_pack(env, LENGTHS, nd, n_ap, 3, f0, sp, ap)
    o = 0
    for n in LENGTHS:
        one = device_pack(env, [n], nd, n_ap, 3, f0[o:o + n], sp[o:o + n], ap[o:o + n])
        assert _same(one, whole[o:o + n]), n
        o += n
    for fill in (np.inf, -np.inf, -0.0, 1e300):
        got = device_pack(env, [65, 3], nd, n_ap, 3, np.zeros(68), sp[:68], ap[:68], fill=fill)
        assert _same(got, fr.pack([65, 3], nd, n_ap, 3, np.zeros(68), sp[:68], ap[:68], fill))
        assert np.array_equal(got[:, 3 * nd], np.full(68, fill)) and np.signbit(got[0, 3 * nd]) == np.signbit(fill)
    # nothing to do: no array is needed
    ft.pack([], nd, 0, 3, None, None, None, None)
    ft.pack([0, 0], nd, n_ap, 3, None, None, _dev(torch, ap[:1]), None)
    ft.unpack(0, nd, n_ap, 3, None, None, None, None)
    w.lib().wc_synchronize()


@pytest.mark.parametrize("nd,n_ap", SHAPES)
def test_unpack(env, nd, n_ap):
    """statics bit for bit, F0 within LOG_EXP_REL of np.exp, the gate at and beside the threshold, a NaN vuv unvoiced, NULL outputs,
    float rows widened exactly"""
    w, ft, torch = env
    rng = np.random.default_rng(77 + nd)
    n, thr = 333, 0.5
    for orders in (1, 3):
        W = fr.width(nd, n_ap, orders)
        cols, vuv_col = fr.columns(nd, n_ap, orders)
        rows = rng.standard_normal((n, W)) * 4.0
        rows[:, orders * nd] = rng.uniform(np.log(60.0), np.log(800.0), n)
        for fmt, dt in (("f64", np.float64), ("f32", np.float32)):
            # the threshold, its neighbours in the rows' own format, NaN, and values far from it
            gate = np.array([thr, np.nextafter(dt(thr), dt(1.0)), np.nextafter(dt(thr), dt(0.0)), np.nan, 1.0, 0.0, np.inf, -np.inf], dtype=dt)
            r = rows.astype(dt)
            r[:, vuv_col] = gate[np.arange(n) % len(gate)]
            d_rows = _dev(torch, r, dt)
            outs = [_guarded(torch, n, 1), _guarded(torch, n, nd), _guarded(torch, n, max(n_ap, 1))]
            torch.cuda.synchronize()
            ft.unpack(n, nd, n_ap, orders, d_rows, outs[0], outs[1], outs[2] if n_ap else None, thr, fmt)
            w.lib().wc_synchronize()
            f0, csp = _rows(outs[0], n, 1)[:, 0], _rows(outs[1], n, nd)
            wide = r.astype(np.float64)
            want_f0, want_sp, want_ap = fr.unpack(nd, n_ap, orders, wide, thr)
            on = wide[:, vuv_col] > thr
            assert np.array_equal(on, np.isin(np.arange(n) % len(gate), [1, 4, 6]))   # above the threshold only; NaN is unvoiced
            assert np.array_equal(f0 == 0.0, ~on) and np.array_equal(f0[~on], np.zeros((~on).sum()))
            rel = (np.abs(f0[on] - want_f0[on]) / want_f0[on]).max()
            print("unpack nd %d n_ap %d orders %d %s: exp against numpy %.3e (relative)" % (nd, n_ap, orders, fmt, rel))
            assert rel < LOG_EXP_REL
            assert _same(csp, want_sp)
            if n_ap:
                assert _same(_rows(outs[2], n, n_ap), want_ap)
            else:
                assert bool(torch.isnan(outs[2]).all())
            # each output alone: the others are NULL and nothing else is written
            for keep in range(3 if n_ap else 2):
                solo = [_guarded(torch, n, 1), _guarded(torch, n, nd), _guarded(torch, n, max(n_ap, 1))]
                torch.cuda.synchronize()
                ft.unpack(n, nd, n_ap, orders, d_rows, *[s if k == keep else None for k, s in enumerate(solo)], thr, fmt)
                w.lib().wc_synchronize()
                assert _same(solo[keep].cpu().numpy(), outs[keep].cpu().numpy())
                assert all(bool(torch.isnan(s).all()) for k, s in enumerate(solo) if k != keep)
    # an infinite threshold gates everything off, -inf lets every vuv but NaN and -inf through
    d_rows, d_f0 = _dev(torch, r.astype(np.float64)), _guarded(torch, n, 1)
    ft.unpack(n, nd, n_ap, 3, d_rows, d_f0, None, None, np.inf)
    w.lib().wc_synchronize()
    assert np.array_equal(_rows(d_f0, n, 1), np.zeros((n, 1)))
    ft.unpack(n, nd, n_ap, 3, d_rows, d_f0, None, None, -np.inf)
    w.lib().wc_synchronize()
    assert np.array_equal(_rows(d_f0, n, 1)[:, 0] == 0.0, np.isin(np.arange(n) % len(gate), [3, 7]))


def test_refused_calls_leave_the_outputs_untouched(env):
    """every refusal of the header, for the three calls: WC_ERR_INVALID before anything is enqueued, the outputs still NaN"""
    w, ft, torch = env
    nd, n_ap, lengths = 25, 1, [3, 64]
    t = sum(lengths)
    L = ft._L()
    ints = lambda v: (C.c_int * len(v))(*v)
    f0, sp, ap = _dev(torch, np.full(t, 100.0)), _dev(torch, np.ones(t * nd)), _dev(torch, np.ones(t * n_ap))
    W = fr.width(nd, n_ap, 3)
    rows = _guarded(torch, t, W)
    mean, var, static = _dev(torch, np.ones(t * W)), _dev(torch, np.ones(W)), _guarded(torch, t, nd + 2 + n_ap)
    o_f0, o_sp, o_ap = _guarded(torch, t, 1), _guarded(torch, t, nd), _guarded(torch, t, n_ap)
    p = lambda x: None if x is None else x.data_ptr()
    huge = [2 ** 31 - 1, 2 ** 31 - 1, 2]   # 2^32 frames
    nan = float("nan")
    torch.cuda.synchronize()

    def pack(n_utt=2, ln=ints(lengths), nd_=nd, n_ap_=n_ap, orders=3, a=f0, b=sp, c=ap, fill=0.0, fmt=0, out=rows):
        return L.wc_pack_model_features_device(n_utt, ln, nd_, n_ap_, orders, p(a), p(b), p(c), fill, fmt, p(out))

    def mlpg(n_utt=2, ln=ints(lengths), nd_=nd, n_ap_=n_ap, orders=3, fmt=0, m=mean, v=var, per_frame=0, out=static):
        return L.wc_mlpg_device(n_utt, ln, nd_, n_ap_, orders, fmt, p(m), p(v), per_frame, p(out))

    def unpack(n=t, nd_=nd, n_ap_=n_ap, orders=3, fmt=0, r=mean, thr=0.5, a=o_f0, b=o_sp, c=o_ap):
        return L.wc_unpack_model_features_device(n, nd_, n_ap_, orders, fmt, p(r), thr, p(a), p(b), p(c))

    refused = [
        pack(nd_=0), pack(n_ap_=-1), pack(orders=0), pack(orders=4), pack(fmt=2), pack(fmt=-1), pack(ln=ints([3, -1])), pack(n_utt=-1),
        pack(n_utt=3, ln=ints(huge)), pack(ln=None), pack(a=None), pack(b=None), pack(out=None), pack(c=None), pack(n_ap_=0), pack(fill=nan),
        pack(out=sp), pack(out=f0), pack(out=ap),
        mlpg(nd_=0), mlpg(n_ap_=-1), mlpg(orders=1), mlpg(orders=4), mlpg(fmt=2), mlpg(ln=ints([-3, 64])), mlpg(n_utt=-1), mlpg(n_utt=3, ln=ints(huge)),
        mlpg(ln=None), mlpg(m=None), mlpg(v=None), mlpg(out=None), mlpg(per_frame=2), mlpg(out=mean), mlpg(out=var),
        unpack(nd_=0), unpack(n_ap_=-1), unpack(orders=0), unpack(orders=4), unpack(fmt=2), unpack(n=-1), unpack(n=2 ** 32), unpack(r=None),
        unpack(thr=nan), unpack(n_ap_=0), unpack(a=mean, b=None, c=None), unpack(b=mean), unpack(c=mean),
    ]
    w.lib().wc_synchronize()
    assert all(rc < 0 for rc in refused), refused
    assert "model features" in w.last_error() or "mlpg" in w.last_error()
    for out in (rows, static, o_f0, o_sp, o_ap):
        assert bool(torch.isnan(out).all())
    for kept, value in ((f0, 100.0), (sp, 1.0), (ap, 1.0), (mean, 1.0), (var, 1.0)):
        assert bool((kept == value).all())
    assert ft.width(25, 1, 3) == 82
    with pytest.raises(ValueError):
        ft.width(0, 1, 3)
    # the same arguments, not refused
    assert pack() == 0 and mlpg() == 0 and unpack() == 0
    w.lib().wc_synchronize()
    assert not bool(torch.isnan(rows[:t * W]).any()) and bool(torch.isnan(rows[t * W:]).all())


def test_numpy_front_end(env):
    w, ft, torch = env
    nd, n_ap = 6, 2
    rng = np.random.default_rng(5)
    lengths = [70, 5]
    f0s = [np.where(rng.uniform(size=n) < 0.5, rng.uniform(80, 300, n), 0.0) for n in lengths]
    sps, aps = [rng.standard_normal((n, nd)) for n in lengths], [-rng.uniform(0, 9, (n, n_ap)) for n in lengths]
    rows = ft.pack_host(f0s, sps, aps, orders=3, lf0_fill=1.0)
    logs = np.concatenate([r[:, 3 * nd] for r in rows])
    want = fr.pack(lengths, nd, n_ap, 3, np.concatenate(f0s), np.concatenate(sps), np.concatenate(aps), 1.0, logs=logs)
    assert _same(np.concatenate(rows), want)
    st = ft.mlpg_host(rows, np.full(fr.width(nd, n_ap, 3), 0.5), nd, n_ap, 3)
    assert _same(np.concatenate(st), fr.mlpg(lengths, nd, n_ap, 3, want, np.full(want.shape[1], 0.5), False))
    st2 = ft.mlpg_host(rows, [np.full(r.shape, 0.5) for r in rows], nd, n_ap, 3)
    assert _same(np.concatenate(st2), np.concatenate(st))
    f0, csp, cap = ft.unpack_host(st[0], nd, n_ap)
    assert np.array_equal(f0 > 0, f0s[0] > 0) and np.abs(csp - sps[0]).max() < 1e-12 * 4 and cap.shape == (70, n_ap)
    rows32 = ft.pack_host(f0s, sps, None, orders=2, out_format="f32")
    assert rows32[0].dtype == np.float32 and rows32[0].shape == (70, fr.width(nd, 0, 2))
