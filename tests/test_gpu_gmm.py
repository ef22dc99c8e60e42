"""-m gpu: wc_gmm_create, wc_gmm_prepared_host and wc_gmm_convert_device (include/world_class_gmm.h) against tests/gmm_rule.py, bit for
bit: what create prepared, then mean, variance, best mixture and log-likelihoods on the library's own prepared arrays, for rows of doubles
and of floats in both directions, inside wider rows whose other columns and a guard row behind the last carry a NaN of a recognisable
payload, with each output NULL in turn, cut into pushes, with ties and frames that are not finite, through every refusal, and from two
host threads."""
import threading

import numpy as np
import pytest

import gmm_rule as gm
from test_gmm_rule import random_model

pytestmark = pytest.mark.gpu

SMALL = [(1, 1, 1), (2, 3, 5), (7, 1, 2), (50, 50, 64)]     # (dx, dy, n_mix)
WIDE = [(64, 65, 3), (65, 64, 2), (192, 192, 2)]            # a dimension at or above the 64 lanes of a wavefront; the widest tile
PAYLOAD64, PAYLOAD32, PAYLOAD_INT = 0x7FF8DEAD0000BEEF, 0x7FC0BEEF, -559038737
DT = {"f64": np.float64, "f32": np.float32}


@pytest.fixture(scope="module")
def env():
    import torch
    import world_class_amd as w
    from world_class_amd import gmm
    w.lib().wc_set_device(0)
    return w, gmm, torch


_MODELS = {}


def model(env, dx, dy, n_mix, tie=False):
    """one model per shape for the whole module: the host arrays, the handle, and the library's own prepared arrays with the means"""
    key = (dx, dy, n_mix, tie)
    if key not in _MODELS:
        w, gmm, torch = env
        weight, mean, cov, _ = random_model(n_mix, dx, dy, 1000 * dx + 10 * dy + n_mix)
        if tie:
            weight[7], mean[7], cov[7] = weight[3], mean[3], cov[3]
        g = gmm.Gmm(weight, mean, cov, dx)
        c, W, B, cvar = g.prepared()
        _MODELS[key] = dict(weight=weight, mean=mean, cov=cov, g=g,
                            own=dict(c=c, W=W, B=B, cvar=cvar, mux=mean[:, :dx].copy(), muy=mean[:, dx:].copy()))
    return _MODELS[key]


def frames(mdl, n, seed=1):
    """n source vectors around the mixtures' means"""
    mean = mdl["mean"]
    dx = mdl["own"]["mux"].shape[1]
    rng = np.random.default_rng(seed)
    return mean[rng.integers(0, mean.shape[0], size=n), :dx] + 0.7 * rng.normal(size=(n, dx))


def nan_filled(torch, count, dtype):
    """count elements of a NaN with a recognisable payload (ints: a recognisable value) on the device"""
    if dtype == np.int32:
        a = np.full(count, PAYLOAD_INT, dtype=np.int32)
    elif dtype == np.float32:
        a = np.full(count, PAYLOAD32, dtype=np.uint32).view(np.float32)
    else:
        a = np.full(count, PAYLOAD64, dtype=np.uint64).view(np.float64)
    return torch.from_numpy(a).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def untouched(a):
    if a.dtype == np.int32:
        return bool((a == PAYLOAD_INT).all())
    return bool((bits(a) == (PAYLOAD32 if a.dtype == np.float32 else PAYLOAD64)).all())


def device_convert(env, mdl, x, fmt_in="f64", fmt_out="f64", pad_in=(0, 0), pad_out=(0, 0), skip=()):
    """x [n, dx] into rows of width dx + sum(pad_in) at column pad_in[0], the outputs into rows of width dy + sum(pad_out) at column
    pad_out[0]; every buffer carries one guard row; the outputs named in skip are NULL -> dict of the host arrays (None where skipped),
    after asserting that every element outside the written columns, and the guard rows, kept their bits"""
    w, gmm, torch = env
    g = mdl["g"]
    n, dx, dy, n_mix = len(x), g.dx, g.dy, g.n_mix
    ld_in, col_in, ld_out, col_out = dx + sum(pad_in), pad_in[0], dy + sum(pad_out), pad_out[0]
    rows = np.full((n + 1, ld_in), 123.0, dtype=DT[fmt_in])
    rows[:n, col_in:col_in + dx] = x
    d_rows = torch.from_numpy(rows.ravel().copy()).cuda()
    d = dict(mean=nan_filled(torch, (n + 1) * ld_out, DT[fmt_out]), var=nan_filled(torch, (n + 1) * ld_out, DT[fmt_out]),
             best=nan_filled(torch, n + 1, np.int32), loglik=nan_filled(torch, (n + 1) * n_mix, np.float64))
    arg = {k: (None if k in skip else v) for k, v in d.items()}
    torch.cuda.synchronize()
    g.convert(n, d_rows, ld_in, arg["mean"], arg["var"], ld_out, col_in, col_out, arg["best"], arg["loglik"], fmt_in, fmt_out)
    w.lib().wc_synchronize()
    assert np.array_equal(bits(d_rows.cpu().numpy()), bits(rows.ravel()))       # the input is read only
    out = {}
    for k in ("mean", "var"):
        a = d[k].cpu().numpy().reshape(n + 1, ld_out)
        if k in skip:
            assert untouched(a)
            out[k] = None
            continue
        assert untouched(a[n]) and untouched(a[:n, :col_out]) and untouched(a[:n, col_out + dy:]), k
        out[k] = a[:n, col_out:col_out + dy].copy()
    b, ll = d["best"].cpu().numpy(), d["loglik"].cpu().numpy().reshape(n + 1, n_mix)
    assert untouched(b[n:]) and untouched(ll[n])
    out["best"] = None if "best" in skip else b[:n].copy()
    out["loglik"] = None if "loglik" in skip else ll[:n].copy()
    if "best" in skip:
        assert untouched(b)
    if "loglik" in skip:
        assert untouched(ll)
    return out


def same(got, want):
    """the same bits, signed zeros included; a NaN stands where a NaN stands (its sign and payload are no part of the rule: the host's
    and the device's invalid operations make different ones)"""
    if got.shape != want.shape or got.dtype != want.dtype or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    return np.array_equal(bits(got)[~np.isnan(got)], bits(want)[~np.isnan(want)])


def assert_equals_rule(got, want, what):
    for k, v in zip(("mean", "var", "best", "loglik"), want):
        if got[k] is not None:
            if k == "best":
                assert got[k].dtype == np.int32 and np.array_equal(got[k], v), (what, k)
            else:
                assert same(got[k], v), (what, k)


# ---- create ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dx,dy,n_mix", SMALL + WIDE)
def test_prepared_equals_the_rule_bit_for_bit(env, dx, dy, n_mix):
    """no tolerance: division and the square root are correctly rounded, the build keeps every product and sum apart, and log is the
    same libm function on both sides"""
    mdl = model(env, dx, dy, n_mix)
    want = gm.prepare(mdl["weight"], mdl["mean"], mdl["cov"], dx, dy)
    for k in ("c", "W", "B", "cvar"):
        assert same(mdl["own"][k], want[k]), k
    assert np.isfinite(mdl["own"]["c"]).all() and (mdl["own"]["cvar"] > 0).all()
    assert (np.triu(mdl["own"]["W"], 1) == 0.0).all() and not np.signbit(np.triu(mdl["own"]["W"], 1)).any()
    g = mdl["g"]
    from world_class_amd.gmm import _L, _host
    c_only = np.empty(n_mix)
    assert _L().wc_gmm_prepared_host(g._h, _host(c_only), None, None, None) == 0 and same(c_only, want["c"])   # each pointer may be NULL


def test_every_refusal_of_create_allocates_nothing_and_names_what_the_rule_names(env):
    w, gmm, torch = env
    weight, mean, cov, _ = random_model(8, 3, 2, 5)
    gmm.Gmm(weight, mean, cov, 3).close()
    torch.cuda.synchronize()

    def refused(text, weight=weight, mean=mean, cov=cov, dx=3):
        free = torch.cuda.mem_get_info()[0]
        with pytest.raises(w.WorldClassError) as e:
            gmm.Gmm(weight, mean, cov, dx)
        assert text in str(e.value), str(e.value)
        assert torch.cuda.mem_get_info()[0] >= free         # nothing of the refused model stays on the device
        try:
            gm.prepare(weight, mean, cov, dx, np.asarray(mean).shape[1] - dx)
        except ValueError as r:
            assert text in str(r), str(r)      # the rule refuses the same thing under the same name
        else:
            raise AssertionError("the rule takes what the library refuses")

    def edited(a, at, v):
        a = a.copy()
        a[at] = v
        return a

    for bad in (0.0, -1.0, np.nan, np.inf):
        refused("mixture 5: a weight", weight=edited(weight, 5, bad))
    refused("mixture 4, row 3: a mean", mean=edited(mean, (4, 3), np.inf))
    refused("mixture 6, row 4: a covariance", cov=edited(cov, (6, 4, 1), np.nan))
    refused("mixture 2, row 1: the source covariance is not positive definite", cov=edited(cov, (2, 1, 1), cov[2, 1, 0] ** 2 / cov[2, 0, 0] - 1e-3))
    refused("mixture 1, row 0: the source covariance is not positive definite", cov=edited(cov, (1, 0, 0), 0.0))
    refused("mixture 3, row 4: a conditional variance", cov=edited(cov, (3, 4, 4), 0.0))
    refused("mixture 1, row 0: ", cov=edited(edited(cov, (3, 4, 4), 0.0), (1, 0, 0), -1.0))
    refused("dx and dy", mean=np.zeros((1, 194)), weight=np.ones(1), cov=np.eye(194)[None], dx=193)
    refused("dx and dy", mean=np.zeros((1, 194)), weight=np.ones(1), cov=np.eye(194)[None], dx=1)
    refused("n_mix", weight=np.ones(1025), mean=np.zeros((1025, 2)), cov=np.tile(np.eye(2), (1025, 1, 1)), dx=1)
    from world_class_amd.gmm import _L, _host
    one, eye = np.ones(1), np.eye(2).ravel().copy()
    for args in ((0, 1, 1, _host(one), _host(eye), _host(eye)), (1, 0, 1, _host(one), _host(eye), _host(eye)), (1, 1, 0, _host(one), _host(eye), _host(eye)),
                 (1, 1, 1, None, _host(eye), _host(eye)), (1, 1, 1, _host(one), None, _host(eye)), (1, 1, 1, _host(one), _host(eye), None)):
        assert not _L().wc_gmm_create(*args) and "gmm create" in w.last_error()
    # entries above the diagonal are never read; and a create that follows the refusals succeeds
    g = gmm.Gmm(weight, mean, edited(edited(cov, (6, 1, 4), np.nan), (0, 0, 2), np.inf), 3)
    want = gm.prepare(weight, mean, cov, 3, 2)
    for a, k in zip(g.prepared(), ("c", "W", "B", "cvar")):
        assert same(a, want[k])
    g.close()


# ---- convert ---------------------------------------------------------------------------------------------------------------------------
CASES = [(s, n) for s in SMALL for n in (0, 1, 63, 64, 65, 130, 1000)] + [(s, n) for s in WIDE for n in (1, 65)]


@pytest.mark.parametrize("shape,n", CASES)
def test_convert_equals_the_rule_bit_for_bit(env, shape, n):
    """both input formats and both output formats inside wider rows (ld_in > dx with col_in > 0, ld_out > dy with col_out > 0) and
    in rows of their own; each output NULL in turn"""
    dx, dy, n_mix = shape
    mdl = model(env, dx, dy, n_mix)
    x = frames(mdl, n, seed=n + dx)
    for fmt_in in ("f64", "f32"):
        xi = x.astype(DT[fmt_in])
        want64 = gm.convert(mdl["own"], xi)
        for fmt_out in ("f64", "f32"):
            want = (want64[0].astype(DT[fmt_out]), want64[1].astype(DT[fmt_out]), want64[2], want64[3])
            got = device_convert(env, mdl, xi, fmt_in, fmt_out, pad_in=(2, 1), pad_out=(1, 4))
            assert_equals_rule(got, want, (fmt_in, fmt_out))
            if n:
                assert (got["best"] >= 0).all() and np.isfinite(got["loglik"]).all() and np.isfinite(got["mean"]).all()
        if fmt_in == "f64":
            assert_equals_rule(device_convert(env, mdl, xi), want64, "rows of their own")
            for skip in ("mean", "var", "best", "loglik"):
                assert_equals_rule(device_convert(env, mdl, xi, pad_out=(0, 2), skip=(skip,)), want64, "without " + skip)
            assert_equals_rule(device_convert(env, mdl, xi, skip=("mean", "var", "best")), want64, "the table alone")
            assert_equals_rule(device_convert(env, mdl, xi, skip=("mean", "var", "loglik")), want64, "best alone")


def test_the_result_does_not_depend_on_the_launch_shape(env):
    """1000 frames at (50, 50, 64) in one call and in pushes of 1, 7, 64, 65 and the rest -- 512 frames and more take the mixtures whole,
    the short pushes cut them into shares -- give identical bits in all four outputs; 3 frames at 1024 mixtures equal the rule"""
    w, gmm, torch = env
    dx, dy, n_mix, n = 50, 50, 64, 1000
    mdl = model(env, dx, dy, n_mix)
    g = mdl["g"]
    x = frames(mdl, n, seed=77)
    whole = device_convert(env, mdl, x)
    d_rows = torch.from_numpy(x.ravel().copy()).cuda()
    d_mean, d_var = nan_filled(torch, n * dy, np.float64), nan_filled(torch, n * dy, np.float64)
    d_best, d_ll = nan_filled(torch, n, np.int32), nan_filled(torch, n * n_mix, np.float64)
    torch.cuda.synchronize()
    o = 0
    for k in (1, 7, 64, 65, n - 137):
        g.convert(k, d_rows[o * dx:], dx, d_mean[o * dy:], d_var[o * dy:], dy, 0, 0, d_best[o:], d_ll[o * n_mix:])
        o += k
    assert o == n
    w.lib().wc_synchronize()
    assert same(d_mean.cpu().numpy().reshape(n, dy), whole["mean"]) and same(d_var.cpu().numpy().reshape(n, dy), whole["var"])
    assert np.array_equal(d_best.cpu().numpy(), whole["best"]) and same(d_ll.cpu().numpy().reshape(n, n_mix), whole["loglik"])
    many = model(env, 2, 1, 1024)
    x3 = frames(many, 3, seed=5)
    assert_equals_rule(device_convert(env, many, x3, pad_in=(1, 0), pad_out=(0, 1)), gm.convert(many["own"], x3), "1024 mixtures")


def test_ties_frames_that_are_not_finite_and_floats_that_widen(env):
    """two identical mixtures at 3 and 7: best is 3.  A NaN, and an infinity that the arithmetic turns into NaN (diagonal source
    covariances: W's entries below the diagonal are zeros): best = -1, mean = 0.0, var = +inf, the finite frames next to them
    untouched.  Infinities that travel through as ll = -inf are judged as the rule judges them.  A float input converts as its
    exact double"""
    w, gmm, torch = env
    tied = model(env, 3, 2, 8, tie=True)
    x = tied["mean"][3, :3] + np.array([[0.0, 0.0, 0.0], [0.01, -0.02, 0.005], [np.inf, np.inf, -np.inf], [-np.inf, 1.0, np.inf]])
    got = device_convert(env, tied, x)
    assert_equals_rule(got, gm.convert(tied["own"], x), "tie")
    assert (got["best"][:2] == 3).all() and same(got["loglik"][:2, 3], got["loglik"][:2, 7])
    weight, mean, cov, _ = random_model(8, 3, 2, 5)
    for m in range(8):
        cov[m, :3, :3] = np.diag(np.diag(cov[m, :3, :3]))
        cov[m, 3:, :3] *= 0.1
        cov[m, :3, 3:] = cov[m, 3:, :3].T
    g = gmm.Gmm(weight, mean, cov, 3)
    c, W, B, cvar = g.prepared()
    mdl = dict(g=g, mean=mean, own=dict(c=c, W=W, B=B, cvar=cvar, mux=mean[:, :3].copy(), muy=mean[:, 3:].copy()))
    fine = mean[2, :3] + 0.1
    x = np.stack([fine, [np.nan, 0.0, 0.0], fine, [np.inf, 0.0, 0.0], fine, [0.0, -np.inf, 1.0], fine] + [fine] * 60 + [[0.0, 0.0, np.nan]])
    for fmt in ("f64", "f32"):
        xi = x.astype(DT[fmt])
        got = device_convert(env, mdl, xi, fmt, fmt, pad_in=(1, 1), pad_out=(2, 0))
        want = gm.convert(mdl["own"], xi, DT[fmt])
        assert_equals_rule(got, want, fmt)
        out = [1, 3, 5, 67]
        assert (got["best"][out] == -1).all() and np.isnan(got["loglik"][out]).all()
        assert (got["mean"][out] == 0.0).all() and not np.signbit(got["mean"][out]).any() and (got["var"][out] == np.inf).all()
        keep = np.setdiff1d(np.arange(len(x)), out)
        assert (got["best"][keep] == got["best"][0]).all() and got["best"][0] >= 0
        assert same(got["mean"][keep], np.tile(got["mean"][0], (len(keep), 1))) and np.isfinite(got["mean"][keep]).all()
    x32 = (mean[:, :3] + 0.3).astype(np.float32)
    a, b = device_convert(env, mdl, x32, "f32", "f64"), device_convert(env, mdl, x32.astype(np.float64), "f64", "f64")
    assert all(same(a[k], b[k]) for k in a) and not np.array_equal(x32.astype(np.float64), mean[:, :3] + 0.3)
    g.close()


def test_every_refusal_of_convert_leaves_the_outputs_untouched(env):
    w, gmm, torch = env
    mdl = model(env, 2, 3, 5)
    g = mdl["g"]
    n, dx, dy, n_mix = 10, 2, 3, 5
    d_rows = torch.from_numpy(frames(mdl, n).ravel().copy()).cuda()
    f32_rows = torch.zeros(n * dx, dtype=torch.float32, device="cuda")
    big = nan_filled(torch, 4 * n * n_mix, np.float64)       # every output is cut from this one array
    d_best = nan_filled(torch, n, np.int32)
    mean, var, ll = big[:n * dy], big[n * dy:2 * n * dy], big[2 * n * dy:2 * n * dy + n * n_mix]
    from world_class_amd.gmm import _L
    raw = lambda h, nf, fi, rows, ldi, ci, fo, m, v, ldo, co, b, l: _L().wc_gmm_convert_device(
        h, nf, fi, w._opt(rows), ldi, ci, fo, w._opt(m), w._opt(v), ldo, co, w._opt(b), w._opt(l))
    ok = dict(h=g._h, nf=n, fi=0, rows=d_rows, ldi=dx, ci=0, fo=0, m=mean, v=var, ldo=dy, co=0, b=d_best, l=ll)
    torch.cuda.synchronize()
    refusals = [
        (dict(h=None), "null handle"), (dict(nf=-1), "n_frames"), (dict(nf=2 ** 32), "n_frames"), (dict(fi=2), "format"), (dict(fi=-1), "format"),
        (dict(fo=2), "format"), (dict(ci=-1, ldi=dx + 5), "negative column"), (dict(co=-1, ldo=dy + 5), "negative column"),
        (dict(ldi=dx - 1), "ld_in < col_in + dx"), (dict(ci=1), "ld_in < col_in + dx"), (dict(ldo=dy - 1), "ld_out < col_out + dy"),
        (dict(co=1), "ld_out < col_out + dy"), (dict(rows=None), "null d_rows_in"), (dict(m=None, v=None, b=None, l=None), "all four outputs"),
        (dict(m=d_rows), "overlaps the input"), (dict(l=d_rows[2:]), "overlaps the input"), (dict(fi=1, rows=f32_rows, b=f32_rows[3:]), "overlaps the input"),
        (dict(v=mean), "two outputs overlap"), (dict(v=big[n * dy - 1:]), "two outputs overlap"), (dict(l=big[2 * n * dy - 1:]), "two outputs overlap"),
        (dict(m=None, v=None, l=big, b=big[n * n_mix - 1:]), "two outputs overlap"),
        (dict(ldo=2 * dy, v=big[dy:]), "two outputs overlap"),      # interleaved rows: the ranges from first to last element overlap
    ]
    for change, text in refusals:
        assert raw(**{**ok, **change}) == -1, change      # WC_ERR_INVALID
        assert text in w.last_error(), (change, w.last_error())
    w.lib().wc_synchronize()
    assert untouched(big.cpu().numpy()) and untouched(d_best.cpu().numpy())
    # nothing to do writes nothing and asks for nothing
    assert raw(**{**ok, **dict(nf=0, rows=None, m=None, v=None, b=None, l=None)}) == 0
    assert raw(**{**ok, **dict(nf=0)}) == 0
    w.lib().wc_synchronize()
    assert untouched(big.cpu().numpy()) and untouched(d_best.cpu().numpy())
    assert raw(**ok) == 0
    w.lib().wc_synchronize()
    want = gm.convert(mdl["own"], d_rows.cpu().numpy().reshape(n, dx))
    assert same(mean.cpu().numpy().reshape(n, dy), want[0]) and np.array_equal(d_best.cpu().numpy(), want[2])
    assert untouched(big[2 * n * dy + n * n_mix:].cpu().numpy())


def test_two_host_threads_on_their_own_streams_share_one_handle(env):
    """the handle is read-only: two threads, each on a stream of its own (wc_set_stream is per thread), convert halves of their own
    and each the whole; all results equal the single thread's"""
    w, gmm, torch = env
    dx, dy, n_mix, n = 50, 50, 64, 700
    mdl = model(env, dx, dy, n_mix)
    g = mdl["g"]
    x = frames(mdl, n, seed=3)
    single = device_convert(env, mdl, x)
    d_rows = torch.from_numpy(x.ravel().copy()).cuda()
    outs = [dict(mean=nan_filled(torch, n * dy, np.float64), var=nan_filled(torch, n * dy, np.float64), best=nan_filled(torch, n, np.int32),
                 ll=nan_filled(torch, n * n_mix, np.float64)) for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    errors = []

    def work(i):
        try:
            assert w.lib().wc_set_stream(streams[i].cuda_stream) == 0
            o = outs[i]
            for rep in range(3):
                for a, b in ((0, 300), (300, n)):    # the second of the pair without a table of its own: through the shared scratch
                    g.convert(b - a, d_rows[a * dx:], dx, o["mean"][a * dy:], o["var"][a * dy:], dy, 0, 0, o["best"][a:],
                              o["ll"][a * n_mix:] if a == 0 else None)
            assert w.lib().wc_synchronize() == 0
            assert w.lib().wc_set_stream(None) == 0
        except Exception as e:      # noqa: BLE001 -- handed to the main thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    torch.cuda.synchronize()
    for o in outs:
        assert same(o["mean"].cpu().numpy().reshape(n, dy), single["mean"]) and same(o["var"].cpu().numpy().reshape(n, dy), single["var"])
        assert np.array_equal(o["best"].cpu().numpy(), single["best"])
        assert same(o["ll"].cpu().numpy().reshape(n, n_mix)[:300], single["loglik"][:300])
        assert untouched(o["ll"].cpu().numpy().reshape(n, n_mix)[300:])
