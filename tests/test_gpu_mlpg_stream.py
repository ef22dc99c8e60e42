"""-m gpu: MLPG streams (include/world_class_mlpg_stream.h) against tests/mlpg_stream_rule.py and against wc_mlpg_device itself, bit
for bit.  One handle per shape with seven streams of 0, 1, 2, 3, 7, 65 and 200 rows, at most 8 rows per push and a lag of at most
64; every output buffer with a guard row of NaN behind what frames_out promises."""
import ctypes as C
import functools

import numpy as np
import pytest

import features_rule as fr
import mlpg_stream_rule as ms
from test_gpu_features import SHAPES, _dev, _guarded, _rows, _same, env  # noqa: F401
from test_gpu_mlpg import device_mlpg

pytestmark = pytest.mark.gpu

ROWS = [0, 1, 2, 3, 7, 65, 200]
OFFS = np.concatenate([[0], np.cumsum(ROWS)])
MAX_ROWS, MAX_LAG = 8, 64
LAGS = [0, 1, 2, 5, 64]


@pytest.fixture(scope="module")
def handles(env):
    """one handle per (shape, orders, streams, bounds), made on first use and closed behind the module's last test"""
    from world_class_amd import mlpg_stream
    made = {}

    def get(nd, n_ap, orders, n_streams=len(ROWS), max_rows=MAX_ROWS, max_lag=MAX_LAG):
        key = (nd, n_ap, orders, n_streams, max_rows, max_lag)
        if key not in made:
            made[key] = mlpg_stream.MlpgStream(n_streams, nd, n_ap, orders, max_rows, max_lag)
        return made[key]

    yield get
    for h in made.values():
        h.close()


@functools.lru_cache(maxsize=None)
def case(nd, n_ap, orders, fmt="f64"):
    """means of unit scale and variances over four decades for the seven streams, as values of the format; one row of variances"""
    rng = np.random.default_rng(17 * nd + orders)
    dt = np.float64 if fmt == "f64" else np.float32
    t, W = sum(ROWS), fr.width(nd, n_ap, orders)
    mean = rng.standard_normal((t, W)).astype(dt)
    var = (10.0 ** rng.uniform(-2.0, 2.0, (t, W))).astype(dt)
    for a in (mean, var):
        a.setflags(write=False)
    return mean, var, var[9]


@functools.lru_cache(maxsize=None)
def rule(nd, n_ap, orders, fmt, per_frame, u, lag):
    """the rule's outputs of stream u at a lag, computed once: (the pushes' rows, the flush's rows)"""
    mean, var, var_row = case(nd, n_ap, orders, fmt)
    s = slice(OFFS[u], OFFS[u + 1])
    got, tail = ms.stream(nd, n_ap, orders, lag, mean[s].astype(np.float64), (var[s] if per_frame else var_row).astype(np.float64), per_frame,
                          eights(ROWS[u]) + [0])
    return np.concatenate(got), tail


def eights(n, k=MAX_ROWS):
    return [k] * (n // k) + ([n % k] if n % k else [])


def drive(env, h, lags, means, variances, per_frame, fmt, cuts, reset=True, flush=True):
    """Resets the streams to their lags, pushes stream u's rows means[u] in pushes of cuts[u][0], cuts[u][1], ... rows (push p of
    every stream in call p) with variances[u] per frame, or the one row `variances`; then flushes all.  frames_out and the getters
    are held against E at every call.  Returns per stream (the pushes' rows, the flush's rows)"""
    w, ft, torch = env
    n, nd, n_ap = h.n_streams, h.nd, h.n_ap
    S1, W = nd + 2 + n_ap, fr.width(nd, n_ap, h.orders)
    dt = np.float64 if fmt == "f64" else np.float32
    if reset:
        for u in range(n):
            h.reset(u, lags[u])
    done = [h.rows_received(u) for u in range(n)]
    first = list(done)
    outs = [[np.zeros((0, S1))] for _ in range(n)]
    for p in range(max(len(c) for c in cuts)):
        k = [c[p] if p < len(c) else 0 for c in cuts]
        expect = [ms.emitted(done[u] + k[u], lags[u]) - ms.emitted(done[u], lags[u]) for u in range(n)]
        take = [slice(done[u] - first[u], done[u] - first[u] + k[u]) for u in range(n)]
        d_mean = d_var = None
        if sum(k):
            d_mean = _dev(torch, np.concatenate([np.asarray(means[u], dtype=dt).reshape(-1, W)[take[u]] for u in range(n)]), dt)
            d_var = _dev(torch, np.concatenate([np.asarray(variances[u], dtype=dt).reshape(-1, W)[take[u]] for u in range(n)]) if per_frame
                         else variances, dt)
        d_static = _guarded(torch, sum(expect), S1)
        torch.cuda.synchronize()
        got = h.push_device(k, d_mean, d_var, d_static, per_frame, fmt)
        w.lib().wc_synchronize()
        assert got == expect, (p, got, expect)
        rows = _rows(d_static, sum(expect), S1)
        o = 0
        for u in range(n):
            outs[u].append(rows[o:o + expect[u]])
            o += expect[u]
            done[u] += k[u]
            assert h.rows_received(u) == done[u] and h.frames_emitted(u) == ms.emitted(done[u], lags[u]) and h.get_lag(u) == lags[u]
    pushed = [np.concatenate(o) for o in outs]
    if not flush:
        return [(a, None) for a in pushed]
    expect = [min(lags[u], done[u]) for u in range(n)]
    d_static = _guarded(torch, sum(expect), S1)
    torch.cuda.synchronize()
    got = h.flush_device([1] * n, d_static)
    w.lib().wc_synchronize()
    assert got == expect
    rows = _rows(d_static, sum(expect), S1)
    cuts_at = np.cumsum(expect)[:-1]
    for u in range(n):
        assert h.frames_emitted(u) == done[u] and h.rows_received(u) == done[u]
    return list(zip(pushed, np.split(rows, cuts_at)))


def per_stream(a):
    return [a[OFFS[u]:OFFS[u + 1]] for u in range(len(ROWS))]


@pytest.mark.parametrize("orders", [2, 3])
@pytest.mark.parametrize("nd,n_ap", SHAPES)
def test_streams_equal_the_rule_bit_for_bit(env, handles, nd, n_ap, orders):
    """no tolerance (a NaN is a NaN): the kernels follow the rule operation for operation.  Lags 0, 1, 2, 5 and 64 rotate over the
    seven streams, so that every stream runs at every lag and one push holds streams of different lags; rows of doubles and of
    floats; variances per frame and as one row"""
    h = handles(nd, n_ap, orders)
    assert h.max_frames_per_push == MAX_ROWS and h.max_frames_per_flush == MAX_LAG
    for fmt in ("f64", "f32"):
        mean, var, var_row = case(nd, n_ap, orders, fmt)
        for per_frame in (True, False):
            for turn in range(len(LAGS)):
                lags = [LAGS[(u + turn) % len(LAGS)] for u in range(len(ROWS))]
                got = drive(env, h, lags, per_stream(mean), per_stream(var) if per_frame else var_row, per_frame, fmt, [eights(n) for n in ROWS])
                for u, (pushed, tail) in enumerate(got):
                    want = rule(nd, n_ap, orders, fmt, per_frame, u, lags[u])
                    assert _same(pushed, want[0]) and _same(tail, want[1]), (fmt, per_frame, u, lags[u])
                    assert np.isfinite(pushed).all() and np.isfinite(tail).all()
                    vuv = mean[OFFS[u]:OFFS[u + 1], orders * (nd + 1)].astype(np.float64)
                    assert np.array_equal(np.concatenate([pushed, tail])[:, nd + 1], vuv)


@pytest.mark.parametrize("orders", [2, 3])
def test_streams_equal_the_whole_call_on_every_prefix(env, handles, orders):
    """wc_mlpg_device itself: all prefixes of a 40-row stream in one ragged batch of lengths 1 .. 40; pushed row i emits row i - L of
    utterance i, the flush is the last rows of utterance 39.  At L = 64 the flush of every stream is the whole call's last 64 rows:
    the whole call where the stream has no more rows than that"""
    nd, n_ap, n = 60, 5, 40
    mean, var, var_row = case(nd, n_ap, orders)
    mean, var = mean[-n:], var[-n:]
    lengths = list(range(1, n + 1))
    starts = np.concatenate([[0], np.cumsum(lengths)])
    idx = np.concatenate([np.arange(i) for i in lengths])
    h1 = handles(nd, n_ap, orders, 1)
    for per_frame, v, v_batch in ((True, var, var[idx]), (False, var_row, var_row)):
        batch = device_mlpg(env, lengths, nd, n_ap, orders, mean[idx], v_batch, per_frame)
        for lag in (3, 0):
            (pushed, tail), = drive(env, h1, [lag], [mean], [v] if per_frame else v, per_frame, "f64", [[3] * 13 + [1]])
            want = np.array([batch[starts[i] + i - lag] for i in range(lag, n)])
            assert _same(pushed, want), (per_frame, lag)
            assert _same(tail, batch[starts[n - 1] + n - lag:starts[n]]), (per_frame, lag)
    mean, var, var_row = case(nd, n_ap, orders)
    whole = device_mlpg(env, ROWS, nd, n_ap, orders, mean, var, True)
    got = drive(env, handles(nd, n_ap, orders), [64] * len(ROWS), per_stream(mean), per_stream(var), True, "f64", [eights(n) for n in ROWS])
    for u, (pushed, tail) in enumerate(got):
        assert len(pushed) == max(ROWS[u] - 64, 0)
        assert _same(tail, whole[OFFS[u] + max(ROWS[u] - 64, 0):OFFS[u + 1]]), u


def random_cuts(n, rng, most=MAX_ROWS):
    """a cut of n rows into pushes of 0 .. most rows, zeros among them"""
    cuts = [0]
    while sum(cuts) < n:
        cuts.append(int(min(rng.integers(0, most + 1), n - sum(cuts))))
    return cuts + [0]


def test_every_cut_gives_the_same_rows(env, handles):
    """one row per push, eights, three seeded random cuts that contain zeros: identical bit for bit.  And the 200-row stream in a
    handle of 3 rows per push and a lag of 5 at most, whose ring of 9 rows wraps dozens of times"""
    nd, n_ap, orders = 60, 5, 3
    mean, var, _ = case(nd, n_ap, orders)
    h = handles(nd, n_ap, orders)
    lags = [5, 64, 0, 1, 2, 5, 5]
    run = lambda cuts: drive(env, h, lags, per_stream(mean), per_stream(var), True, "f64", cuts)
    base = run([eights(n) for n in ROWS])
    for u, (pushed, tail) in enumerate(base):
        want = rule(nd, n_ap, orders, "f64", True, u, lags[u])
        assert _same(pushed, want[0]) and _same(tail, want[1])
    rng = np.random.default_rng(3)
    for cuts in [[[1] * n for n in ROWS]] + [[random_cuts(n, rng) for n in ROWS] for _ in range(3)]:
        for (pushed, tail), (p0, t0) in zip(run(cuts), base):
            assert _same(pushed, p0) and _same(tail, t0)
    small = handles(nd, n_ap, orders, 1, 3, 5)
    (pushed, tail), = drive(env, small, [5], per_stream(mean)[6:], per_stream(var)[6:], True, "f64", [eights(200, 3)])
    assert _same(pushed, base[6][0]) and _same(tail, base[6][1])


def test_streams_are_independent_and_a_reset_forgets(env, handles):
    nd, n_ap, orders = 60, 5, 3
    mean, var, _ = case(nd, n_ap, orders)
    lags = [2, 0, 1, 2, 5, 64, 5]
    h, h1 = handles(nd, n_ap, orders), handles(nd, n_ap, orders, 1)
    means, variances = per_stream(mean), per_stream(var)
    base = drive(env, h, lags, means, variances, True, "f64", [eights(n) for n in ROWS])
    for u in range(len(ROWS)):   # each stream alone in a one-stream handle
        (pushed, tail), = drive(env, h1, [lags[u]], means[u:u + 1], variances[u:u + 1], True, "f64", [eights(ROWS[u])])
        assert _same(pushed, base[u][0]) and _same(tail, base[u][1]), u
    # 100 rows of other data and no flush, a reset to another lag, 9 more rows (flushed or not), a reset again: a fresh stream
    want = rule(nd, n_ap, orders, "f64", True, 5, 5)
    for first_lag, flush_between in ((64, True), (5, False)):
        drive(env, h1, [first_lag], [means[6][100:]], [variances[6][100:]], True, "f64", [eights(100)], flush=False)
        drive(env, h1, [3], [means[6][:9]], [variances[6][:9]], True, "f64", [[8, 1]], flush=flush_between)
        (pushed, tail), = drive(env, h1, [5], means[5:6], variances[5:6], True, "f64", [eights(65)])
        assert _same(pushed, want[0]) and _same(tail, want[1]), first_lag


@pytest.mark.parametrize("orders", [2, 3])
def test_variances_that_drop_a_column_or_an_observation(env, handles, orders):
    """NaN, 0, -1 and -inf at (static column 63, row 30), (lf0, row 0) and (the last band, in the second wavefront beside the vuv
    lane; the last row before the flush) of the 65-row stream at lag 5: the frames emitted from that row on are NaN in exactly that
    column; everything emitted before it, every other column and every other stream equal the clean run.  +inf with a NaN mean is
    dropped; a bad variance in the vuv column is not read"""
    nd, n_ap = 60, 5
    mean, var, _ = case(nd, n_ap, orders)
    cols, vuv_col = fr.columns(nd, n_ap, orders)
    h = handles(nd, n_ap, orders)
    lags, u, lag = [5] * len(ROWS), 5, 5
    cuts = [eights(n) for n in ROWS]
    clean = drive(env, h, lags, per_stream(mean), per_stream(var), True, "f64", cuts)
    spots = [(63, orders - 1, 30), (nd, 1, 0), (nd + n_ap, 0, ROWS[u] - 1)]   # (static column, its order, row of stream u)
    ocol = lambda c: c if c <= nd else c + 1
    for bad in (np.nan, 0.0, -1.0, -np.inf):
        v = var.copy()
        for c, k, j in spots:
            v[OFFS[u] + j, cols[c][k]] = bad
        v[OFFS[6] + 5, vuv_col] = bad
        got = drive(env, h, lags, per_stream(mean), per_stream(v), True, "f64", cuts)
        for s in range(len(ROWS)):
            if s != u:
                assert _same(got[s][0], clean[s][0]) and _same(got[s][1], clean[s][1]), (bad, s)
        pushed, tail = got[u]
        want = ms.stream(nd, n_ap, orders, lag, mean[OFFS[u]:OFFS[u + 1]], v[OFFS[u]:OFFS[u + 1]], True, cuts[u])
        assert _same(pushed, np.concatenate(want[0])) and _same(tail, want[1])
        hit, hit_tail = np.zeros(pushed.shape, dtype=bool), np.zeros(tail.shape, dtype=bool)
        for c, k, j in spots:
            hit[max(j - lag, 0):, ocol(c)] = True   # pushed row i emits frame i - lag
            hit_tail[:, ocol(c)] = True
        assert np.isnan(pushed[hit]).all() and np.array_equal(pushed[~hit], clean[u][0][~hit])
        assert np.isnan(tail[hit_tail]).all() and np.array_equal(tail[~hit_tail], clean[u][1][~hit_tail])
    v, m2 = var.copy(), mean.copy()
    for c, k, j in spots:
        v[OFFS[u] + j, cols[c][k]] = np.inf
        m2[OFFS[u] + j, cols[c][k]] = np.nan   # a dropped observation's mean is not looked at
    got = drive(env, h, lags, per_stream(mean), per_stream(v), True, "f64", cuts)
    want = ms.stream(nd, n_ap, orders, lag, mean[OFFS[u]:OFFS[u + 1]], v[OFFS[u]:OFFS[u + 1]], True, cuts[u])
    assert _same(got[u][0], np.concatenate(want[0])) and _same(got[u][1], want[1])
    assert np.isfinite(got[u][0]).all() and np.isfinite(got[u][1]).all()
    got2 = drive(env, h, lags, per_stream(m2), per_stream(v), True, "f64", cuts)
    for s in range(len(ROWS)):
        assert _same(got2[s][0], got[s][0]) and _same(got2[s][1], got[s][1])
    # one row of variances that is bad from the third push on: the frames of rows >= 16
    vr = np.array(case(nd, n_ap, orders)[2])
    bad_row = vr.copy()
    bad_row[cols[nd + 1][0]] = 0.0
    h1 = handles(nd, n_ap, orders, 1)
    h1.reset(0, lag)
    m = per_stream(mean)[u]
    parts = [drive(env, h1, [lag], [m[o:o + 8]], vr if o < 16 else bad_row, False, "f64", [[8]], reset=False, flush=o == 24)[0] for o in (0, 8, 16, 24)]
    pushed, tail = np.concatenate([p[0] for p in parts]), parts[-1][1]
    s = ms.Stream(nd, n_ap, orders, lag)
    want = np.concatenate([s.push(m[o:o + 8], vr if o < 16 else bad_row, False) for o in (0, 8, 16, 24)])
    assert _same(pushed, want) and _same(tail, s.flush())
    assert np.isnan(pushed[16 - lag:, nd + 2]).all() and np.isnan(tail[:, nd + 2]).all()
    assert np.isfinite(pushed[:16 - lag]).all() and np.isfinite(np.delete(pushed, nd + 2, axis=1)).all()


def test_refused_calls_change_nothing(env):
    """every refusal of the header: WC_ERR_INVALID (NULL from create) on the host; after each one a push that continues gives the
    rows it would have given had the refused call never been made"""
    w, ft, torch = env
    from world_class_amd import mlpg_stream
    nd, n_ap, orders, lag = 25, 1, 3, 2
    L = mlpg_stream._L()
    W, S1 = fr.width(nd, n_ap, orders), nd + 2 + n_ap
    mean, var, var_row = case(nd, n_ap, orders)
    for args in ((3, 0, n_ap, 3, 8, 8), (3, nd, -1, 3, 8, 8), (3, nd, n_ap, 1, 8, 8), (3, nd, n_ap, 4, 8, 8), (0, nd, n_ap, 3, 8, 8),
                 (3, nd, n_ap, 3, 0, 8), (3, nd, n_ap, 3, 8, -1), (3, 2 ** 30, 2 ** 30, 3, 8, 8), (2 ** 20, 60, 5, 3, 8, 64),
                 (1, 60, 5, 3, 2 ** 31 - 1, 2 ** 31 - 1)):
        assert not L.wc_mlpg_stream_create(*args), args
        assert "mlpg stream" in w.last_error()
    h = mlpg_stream.MlpgStream(3, nd, n_ap, orders, 8, 8)
    raw = h._h
    ints = lambda v: (C.c_int * len(v))(*v)
    p = lambda x: None if x is None else x.data_ptr()
    # stream 0 runs at lag 2; stream 1 was never reset; stream 2 has ended
    h.reset(0, lag)
    h.reset(2, 1)
    d_m, d_v, d_row = _dev(torch, mean[:16]), _dev(torch, var[:16]), _dev(torch, var_row)
    d_out = _guarded(torch, 3 * 8, S1)
    torch.cuda.synchronize()
    assert h.push_device([0, 0, 1], d_m, d_v, d_out, True) == [0, 0, 0] and h.flush_device([0, 0, 1], d_out) == [0, 0, 1]
    w.lib().wc_synchronize()
    assert h.get_lag(1) == -1 and h.get_lag(2) == 1 and h.rows_received(2) == 1 and h.frames_emitted(2) == 1
    rows_m, rows_v = mean[100:140], var[100:140]
    got, taken = [], [0]

    def go_on(k):
        """k more rows to stream 0"""
        o = taken[0]
        out = _guarded(torch, 8, S1)
        dm, dv = _dev(torch, rows_m[o:o + k]), _dev(torch, rows_v[o:o + k])
        torch.cuda.synchronize()
        n = h.push_device([k, 0, 0], dm, dv, out, True)
        w.lib().wc_synchronize()
        assert n == [ms.emitted(o + k, lag) - ms.emitted(o, lag), 0, 0]
        got.append(out.cpu().numpy().reshape(9, S1)[:n[0]])
        taken[0] += k

    go_on(4)
    out3 = (C.c_int * 3)()

    def push(n_rows=ints([1, 0, 0]), fmt=0, m=d_m, v=d_v, per_frame=1, out=d_out, fo=out3, hh=raw):
        return L.wc_mlpg_stream_push_device(hh, n_rows, fmt, p(m), p(v), per_frame, p(out), fo)

    def flush(want=ints([1, 0, 0]), out=d_out, fo=out3, hh=raw):
        return L.wc_mlpg_stream_flush_device(hh, want, p(out), fo)

    refusals = [
        lambda: L.wc_mlpg_stream_reset(raw, -1, 0), lambda: L.wc_mlpg_stream_reset(raw, 3, 0), lambda: L.wc_mlpg_stream_reset(None, 0, 0),
        lambda: L.wc_mlpg_stream_reset(raw, 0, -1), lambda: L.wc_mlpg_stream_reset(raw, 0, 9),
        lambda: push(n_rows=ints([-1, 0, 0])), lambda: push(n_rows=ints([9, 0, 0])), lambda: push(n_rows=ints([1, 1, 0])),
        lambda: push(n_rows=ints([1, 0, 1])), lambda: push(n_rows=None), lambda: push(fo=None), lambda: push(hh=None),
        lambda: push(m=None), lambda: push(v=None), lambda: push(out=None), lambda: push(fmt=2), lambda: push(fmt=-1),
        lambda: push(per_frame=2), lambda: push(per_frame=-1), lambda: push(out=d_m), lambda: push(out=d_v),
        lambda: push(v=d_row, per_frame=0, out=d_row),
        lambda: flush(want=None), lambda: flush(fo=None), lambda: flush(hh=None), lambda: flush(want=ints([1, 1, 0])),
        lambda: flush(want=ints([1, 0, 1])), lambda: flush(out=None),
    ]
    for i, call in enumerate(refusals):
        rc = call()
        assert rc < 0 and "mlpg stream" in w.last_error(), i
        assert h.rows_received(0) == taken[0] and h.frames_emitted(0) == ms.emitted(taken[0], lag) and h.get_lag(0) == lag
        assert h.get_lag(1) == -1 and h.rows_received(2) == 1 and h.frames_emitted(2) == 1
        go_on(1)
    for name in ("rows_received", "frames_emitted", "get_lag"):
        assert getattr(h, name)(-1) == -1 and getattr(h, name)(3) == -1
    w.lib().wc_synchronize()
    assert bool(torch.isnan(d_out[S1:]).all())   # (the one row stream 2 flushed stands at its head)
    assert bool((d_m == _dev(torch, mean[:16])).all())
    d_tail = _guarded(torch, lag, S1)
    torch.cuda.synchronize()
    assert h.flush_device([1, 0, 0], d_tail) == [lag, 0, 0]
    w.lib().wc_synchronize()
    n = taken[0]
    want = ms.stream(nd, n_ap, orders, lag, rows_m[:n], rows_v[:n], True, [n])
    assert _same(np.concatenate(got), want[0][0]) and _same(_rows(d_tail, lag, S1), want[1])
    # an ended stream refuses rows until it is reset; a wanted stream with no rows flushes nothing and ends
    assert push() < 0
    h.reset(0, 8)
    assert h.flush_device([1, 0, 0], None) == [0, 0, 0] and push() < 0
    h.reset(0, 0)
    d_one = _guarded(torch, 1, S1)
    torch.cuda.synchronize()
    assert push(out=d_one) == 0 and list(out3) == [1, 0, 0]
    w.lib().wc_synchronize()
    assert _same(_rows(d_one, 1, S1), ms.stream(nd, n_ap, orders, 0, mean[:1], var[:1], True, [1])[0][0])
    h.close()
