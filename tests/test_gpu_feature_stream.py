"""-m gpu: feature streams (include/world_class_feature_stream.h) against tests/feature_stream_rule.py and against
wc_pack_model_features_device itself, bit for bit.  One handle per shape and order with seven streams of 0, 1, 2, 3, 7, 65 and 200
rows, at most 8 rows per push and a lag of at most 64, so that a ring of 73 rows wraps on the 200-row stream; every output buffer
with a guard row of NaN behind what frames_out promises.  (The rings and the scratch of a handle are out of a test's reach: create
fills them with NaN itself, so that a row read before a push took it would show in the outputs, which the tests hold finite.)"""
import ctypes as C
import functools

import numpy as np
import pytest

import feature_stream_rule as fs
import features_rule as fr
from test_gpu_features import SHAPES, _dev, _guarded, _rows, _same, device_pack, env  # noqa: F401

pytestmark = pytest.mark.gpu

ROWS = [0, 1, 2, 3, 7, 65, 200]
OFFS = np.concatenate([[0], np.cumsum(ROWS)])
MAX_ROWS, MAX_LAG = 8, 64
LAGS = [0, 1, 2, 5, 64]
FILL = -3.25
WC_ERR_INVALID = -1   # include/world_class_c.h


@pytest.fixture(scope="module")
def handles(env):
    """one handle per (shape, orders, streams, bounds), made on first use and closed behind the module's last test"""
    from world_class_amd import feature_stream
    made = {}

    def get(nd, n_ap, orders, n_streams=len(ROWS), max_rows=MAX_ROWS, max_lag=MAX_LAG):
        key = (nd, n_ap, orders, n_streams, max_rows, max_lag)
        if key not in made:
            made[key] = feature_stream.FeatureStream(n_streams, nd, n_ap, orders, max_rows, max_lag)
        return made[key]

    yield get
    for h in made.values():
        h.close()


@functools.lru_cache(maxsize=None)
def contour():
    """F0 of the seven streams, the contours of tests/test_feature_stream_rule.py: one voiced row; a leading run; all unvoiced; two
    runs inside one push; a leading run, runs of 1 .. 6 rows (L - 1, L and L + 1 of the lags 2 and 5) and a trailing run; a run of
    100 rows, whose left end has left the ring of 73 when its far end arrives, a run of 63 (L - 1 at lag 64), short runs and a
    trailing run; NaN, -1 and +inf among the unvoiced values"""
    rng = np.random.default_rng(4)
    v65 = fs.runs(65, [1, 2, 3, 4, 5, 6], first=3)
    v65[:3], v65[55:] = False, False
    v200 = fs.runs(200, [100, 63, 5, 4], first=2)
    v200[190:] = False
    masks = [np.zeros(0, dtype=bool), np.ones(1, dtype=bool), np.array([False, True]), np.zeros(3, dtype=bool),
             np.array([True, False, True, False, False, True, True]), v65, v200]
    assert [len(m) for m in masks] == ROWS
    f0 = np.concatenate([fs.f0_of(m, rng) for m in masks])
    assert np.isnan(f0).any() and (f0 < 0).any() and np.isinf(f0).any()
    f0.setflags(write=False)
    return f0


@functools.lru_cache(maxsize=None)
def case(nd, n_ap):
    rng = np.random.default_rng(31 * nd + n_ap)
    t = sum(ROWS)
    sp = rng.standard_normal((t, nd)) * np.linspace(3.0, 0.05, nd)
    ap = -rng.uniform(0.0, 40.0, (t, n_ap))
    for a in (sp, ap):
        a.setflags(write=False)
    return contour(), sp, ap


_LOGS = {}


def device_logs(env):
    """log(f0) of the voiced rows as the device takes it: the lf0 column of wc_pack_model_features_device (tests/test_gpu_features.py)"""
    if "logs" not in _LOGS:
        f0 = contour()
        got = device_pack(env, ROWS, 1, 0, 1, f0, np.zeros((len(f0), 1)), np.zeros((len(f0), 0)))
        v = fr.voiced(f0)
        logs = np.where(v, got[:, 1], 0.0)
        assert (np.abs(logs[v] - np.log(f0[v])) / np.abs(np.log(f0[v]))).max() < 1e-12
        _LOGS["logs"] = logs
    return _LOGS["logs"]


def per_stream(a):
    return [a[OFFS[u]:OFFS[u + 1]] for u in range(len(ROWS))]


def eights(n, k=MAX_ROWS):
    return [k] * (n // k) + ([n % k] if n % k else [])


_RULE = {}


def rule(env, nd, n_ap, orders, u, lag, fill=FILL):
    """the rule's outputs of stream u at a lag on the device's own logs, computed once: (the pushes' rows, the flush's rows)"""
    key = (nd, n_ap, orders, u, lag, fill)
    if key not in _RULE:
        f0, sp, ap = (per_stream(a)[u] for a in case(nd, n_ap))
        got, tail = fs.stream(nd, n_ap, orders, lag, fill, f0, sp, ap, eights(ROWS[u]) + [0], per_stream(device_logs(env))[u], MAX_ROWS, MAX_LAG)
        _RULE[key] = (np.concatenate(got), tail)
    return _RULE[key]


def drive(env, h, lags, data, fmt, cuts, fills=None, reset=True, flush=True):
    """Resets the streams to their lags, pushes stream u's rows data[u] = (f0, sp, ap) in pushes of cuts[u][0], cuts[u][1], ... rows
    (push p of every stream in call p); then flushes all.  frames_out and the getters are held against E at every call.  Returns per
    stream (the pushes' rows, the flush's rows)"""
    w, ft, torch = env
    n, nd, n_ap = h.n_streams, h.nd, h.n_ap
    W = fr.width(nd, n_ap, h.orders)
    dt = np.float64 if fmt == "f64" else np.float32
    if reset:
        for u in range(n):
            h.reset(u, lags[u], FILL if fills is None else fills[u])
    done = [h.rows_received(u) for u in range(n)]
    first = list(done)
    outs = [[np.zeros((0, W), dtype=dt)] for _ in range(n)]
    for p in range(max(len(c) for c in cuts)):
        k = [c[p] if p < len(c) else 0 for c in cuts]
        expect = [fs.emitted(done[u] + k[u], lags[u]) - fs.emitted(done[u], lags[u]) for u in range(n)]
        take = [slice(done[u] - first[u], done[u] - first[u] + k[u]) for u in range(n)]
        d_f0 = d_sp = d_ap = None
        if sum(k):
            d_f0 = _dev(torch, np.concatenate([np.asarray(data[u][0])[take[u]] for u in range(n)]))
            d_sp = _dev(torch, np.concatenate([np.asarray(data[u][1]).reshape(-1, nd)[take[u]] for u in range(n)]))
            d_ap = _dev(torch, np.concatenate([np.asarray(data[u][2]).reshape(-1, n_ap)[take[u]] for u in range(n)])) if n_ap else None
        d_rows = _guarded(torch, sum(expect), W, dt)
        torch.cuda.synchronize()
        got = h.push_device(k, d_f0, d_sp, d_ap, d_rows, fmt)
        w.lib().wc_synchronize()
        assert got == expect, (p, got, expect)
        rows = _rows(d_rows, sum(expect), W)
        o = 0
        for u in range(n):
            outs[u].append(rows[o:o + expect[u]])
            o += expect[u]
            done[u] += k[u]
            assert h.rows_received(u) == done[u] and h.frames_emitted(u) == fs.emitted(done[u], lags[u]) and h.get_lag(u) == lags[u]
    pushed = [np.concatenate(o) for o in outs]
    if not flush:
        return [(a, None) for a in pushed]
    expect = [min(lags[u], done[u]) for u in range(n)]
    d_rows = _guarded(torch, sum(expect), W, dt)
    torch.cuda.synchronize()
    got = h.flush_device([1] * n, d_rows, fmt)
    w.lib().wc_synchronize()
    assert got == expect
    rows = _rows(d_rows, sum(expect), W)
    for u in range(n):
        assert h.frames_emitted(u) == done[u] and h.rows_received(u) == done[u]
    return list(zip(pushed, np.split(rows, np.cumsum(expect)[:-1])))


def data_of(nd, n_ap):
    return list(zip(*(per_stream(a) for a in case(nd, n_ap))))


@pytest.mark.parametrize("orders", [1, 2, 3])
@pytest.mark.parametrize("nd,n_ap", SHAPES)
def test_streams_equal_the_rule_bit_for_bit(env, handles, nd, n_ap, orders):
    """no tolerance: the kernels follow the rule operation for operation, on the device's own voiced logs.  Lags 0, 1, 2, 5 and 64
    rotate over the seven streams, so that every stream runs at every lag and one push holds streams of different lags; rows of
    doubles and of floats"""
    h = handles(nd, n_ap, orders)
    assert h.max_frames_per_push == MAX_ROWS and h.max_frames_per_flush == MAX_LAG
    f0 = contour()
    for fmt in ("f64", "f32"):
        for turn in range(len(LAGS)):
            lags = [LAGS[(u + turn) % len(LAGS)] for u in range(len(ROWS))]
            got = drive(env, h, lags, data_of(nd, n_ap), fmt, [eights(n) for n in ROWS])
            for u, (pushed, tail) in enumerate(got):
                want = rule(env, nd, n_ap, orders, u, lags[u])
                if fmt == "f32":
                    want = tuple(a.astype(np.float32) for a in want)
                assert _same(pushed, want[0]) and _same(tail, want[1]), (fmt, u, lags[u])
                assert np.isfinite(pushed).all() and np.isfinite(tail).all()
                vuv = fr.voiced(f0[OFFS[u]:OFFS[u + 1]]).astype(pushed.dtype)
                assert np.array_equal(np.concatenate([pushed, tail])[:, orders * (nd + 1)], vuv)


@pytest.mark.parametrize("orders", [1, 2, 3])
def test_streams_equal_the_whole_call_on_every_prefix(env, handles, orders):
    """wc_pack_model_features_device itself, no numpy log: all prefixes of the 65-row stream in one ragged batch of lengths 1 .. 65;
    pushed row i emits row i - L of utterance i, the flush is the last rows of utterance 64.  At L = 64 the flush of every stream
    is the whole call's last 64 rows: the whole call where the stream has no more rows than that"""
    nd, n_ap, n = 60, 5, 65
    f0, sp, ap = data_of(nd, n_ap)[5]
    lengths = list(range(1, n + 1))
    starts = np.concatenate([[0], np.cumsum(lengths)])
    idx = np.concatenate([np.arange(i) for i in lengths])
    batch = device_pack(env, lengths, nd, n_ap, orders, f0[idx], sp[idx], ap[idx])
    h1 = handles(nd, n_ap, orders, 1)
    for lag in (5, 2, 0):
        (pushed, tail), = drive(env, h1, [lag], [(f0, sp, ap)], "f64", [[3] * 21 + [2]])
        want = np.array([batch[starts[i] + i - lag] for i in range(lag, n)])
        assert _same(pushed, want), lag
        assert _same(tail, batch[starts[n - 1] + n - lag:starts[n]]), lag
    whole = device_pack(env, ROWS, nd, n_ap, orders, *case(nd, n_ap))
    got = drive(env, handles(nd, n_ap, orders), [64] * len(ROWS), data_of(nd, n_ap), "f64", [eights(n) for n in ROWS])
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
    h = handles(nd, n_ap, orders)
    lags = [5, 64, 0, 1, 2, 5, 5]
    data = data_of(nd, n_ap)
    run = lambda cuts: drive(env, h, lags, data, "f64", cuts)
    base = run([eights(n) for n in ROWS])
    for u, (pushed, tail) in enumerate(base):
        want = rule(env, nd, n_ap, orders, u, lags[u])
        assert _same(pushed, want[0]) and _same(tail, want[1])
    rng = np.random.default_rng(3)
    for cuts in [[[1] * n for n in ROWS]] + [[random_cuts(n, rng) for n in ROWS] for _ in range(3)]:
        for (pushed, tail), (p0, t0) in zip(run(cuts), base):
            assert _same(pushed, p0) and _same(tail, t0)
    small = handles(nd, n_ap, orders, 1, 3, 5)
    (pushed, tail), = drive(env, small, [5], data[6:], "f64", [eights(200, 3)])
    assert _same(pushed, base[6][0]) and _same(tail, base[6][1])


def test_streams_are_independent_and_a_reset_forgets(env, handles):
    nd, n_ap, orders = 60, 5, 3
    lags = [2, 0, 1, 2, 5, 64, 5]
    h, h1 = handles(nd, n_ap, orders), handles(nd, n_ap, orders, 1)
    data = data_of(nd, n_ap)
    base = drive(env, h, lags, data, "f64", [eights(n) for n in ROWS])
    for u in range(len(ROWS)):   # each stream alone in a one-stream handle
        (pushed, tail), = drive(env, h1, [lags[u]], data[u:u + 1], "f64", [eights(ROWS[u])])
        assert _same(pushed, base[u][0]) and _same(tail, base[u][1]), u
    # 100 rows of other data (the end of the long run and what follows it: the carried record is in use) and no flush, a reset to
    # another lag and another lf0_fill, 9 more rows (flushed or not), a reset again: a fresh stream
    want = rule(env, nd, n_ap, orders, 5, 5)
    tail_of = lambda d, a, b: tuple(x[a:b] for x in d)
    for first_lag, flush_between in ((64, True), (5, False)):
        drive(env, h1, [first_lag], [tail_of(data[6], 100, 200)], "f64", [eights(100)], flush=False)
        drive(env, h1, [3], [tail_of(data[6], 0, 9)], "f64", [[8, 1]], fills=[7.5], flush=flush_between)
        (pushed, tail), = drive(env, h1, [5], data[5:6], "f64", [eights(65)])
        assert _same(pushed, want[0]) and _same(tail, want[1]), first_lag
    # lf0_fill belongs to the stream: the all-unvoiced stream and the leading runs show another one, nothing else changes
    for u in (3, 5):
        (pushed, tail), = drive(env, h1, [2], data[u:u + 1], "f64", [eights(ROWS[u])], fills=[np.inf])
        want = rule(env, nd, n_ap, orders, u, 2, np.inf)
        assert _same(pushed, want[0]) and _same(tail, want[1]) and np.isinf(np.concatenate([pushed, tail])[0, orders * nd])


def test_values_that_are_not_finite_travel_through(env, handles):
    """NaN, +inf and -inf in coded columns of the 65-row stream: they show in their own static column, in the rows of the frame and
    of its two neighbours, and nowhere else"""
    nd, n_ap, orders, u, lag = 60, 5, 3, 5, 5
    f0, sp, ap = (np.array(a) for a in data_of(nd, n_ap)[u])
    spots = [(3, 10, np.nan), (nd - 1, 30, np.inf), (nd + 1 + 4, 64, -np.inf), (0, 0, np.nan)]   # (static column, row, value)
    for c, t, bad in spots:
        (sp if c < nd else ap)[t, c if c < nd else c - nd - 1] = bad
    h1 = handles(nd, n_ap, orders, 1)
    (clean_p, clean_t), = drive(env, h1, [lag], data_of(nd, n_ap)[u:u + 1], "f64", [eights(65)])
    (pushed, tail), = drive(env, h1, [lag], [(f0, sp, ap)], "f64", [eights(65)])
    got, clean = np.concatenate([pushed, tail]), np.concatenate([clean_p, clean_t])
    want, want_tail = fs.stream(nd, n_ap, orders, lag, FILL, f0, sp, ap, eights(65), per_stream(device_logs(env))[u], MAX_ROWS, MAX_LAG)
    assert _same(pushed, np.concatenate(want)) and _same(tail, want_tail)
    cols, _ = fr.columns(nd, n_ap, orders)
    hit = np.zeros(got.shape, dtype=bool)
    for c, t, bad in spots:
        hit[t, cols[c][0]] = True
        for k in (1, 2):
            hit[max(t - 1, 0):t + 2, cols[c][k]] = True
        hit[t, cols[c][1]] = False   # (the delta of the frame itself reads its neighbours alone)
    assert not np.isfinite(got[hit]).any() and np.array_equal(got[~hit], clean[~hit])


def test_refused_calls_change_nothing(env):
    """every refusal of the header: WC_ERR_INVALID (NULL from create) on the host with a text; after each one a push that continues
    gives the rows it would have given had the refused call never been made"""
    w, ft, torch = env
    from world_class_amd import feature_stream
    nd, n_ap, orders, lag = 25, 1, 3, 2
    L = feature_stream._L()
    W = fr.width(nd, n_ap, orders)
    for args in ((3, 0, n_ap, 3, 8, 8), (3, nd, -1, 3, 8, 8), (3, nd, n_ap, 0, 8, 8), (3, nd, n_ap, 4, 8, 8), (0, nd, n_ap, 3, 8, 8),
                 (3, nd, n_ap, 3, 0, 8), (3, nd, n_ap, 3, 8, -1), (3, 2 ** 30, 2 ** 30, 3, 8, 8), (2 ** 20, 60, 5, 3, 8, 64),
                 (1, 60, 5, 3, 2 ** 31 - 1, 2 ** 31 - 1)):
        assert not L.wc_feature_stream_create(*args), args
        assert "feature stream" in w.last_error()
    h = feature_stream.FeatureStream(3, nd, n_ap, orders, 8, 8)
    h0 = feature_stream.FeatureStream(1, nd, 0, orders, 8, 8)   # no bands: d_coded_ap is NULL
    raw = h._h
    ints = lambda v: (C.c_int * len(v))(*v)
    p = lambda x: None if x is None else x.data_ptr()
    rng = np.random.default_rng(8)
    n_all = 60
    f0_h, sp_h, ap_h = rng.uniform(70.0, 500.0, n_all), rng.standard_normal((n_all, nd)), -rng.uniform(0.0, 40.0, (n_all, n_ap))
    # stream 0 runs at lag 2; stream 1 was never reset; stream 2 has ended
    h.reset(0, lag, FILL)
    h.reset(2, 1, FILL)
    h0.reset(0, 0, FILL)
    d_f0, d_sp, d_ap = _dev(torch, f0_h[:16]), _dev(torch, sp_h[:16]), _dev(torch, ap_h[:16])
    d_out = _guarded(torch, 3 * 8, W)
    torch.cuda.synchronize()
    assert h.push_device([0, 0, 1], d_f0, d_sp, d_ap, d_out) == [0, 0, 0] and h.flush_device([0, 0, 1], d_out) == [0, 0, 1]
    w.lib().wc_synchronize()
    assert h.get_lag(1) == -1 and h.get_lag(2) == 1 and h.rows_received(2) == 1 and h.frames_emitted(2) == 1
    got, taken = [], [0]

    def go_on(k):
        """k more rows to stream 0"""
        o = taken[0]
        out = _guarded(torch, 8, W)
        a, b, c = _dev(torch, f0_h[o:o + k]), _dev(torch, sp_h[o:o + k]), _dev(torch, ap_h[o:o + k])
        torch.cuda.synchronize()
        n = h.push_device([k, 0, 0], a, b, c, out)
        w.lib().wc_synchronize()
        assert n == [fs.emitted(o + k, lag) - fs.emitted(o, lag), 0, 0]
        got.append(out.cpu().numpy().reshape(9, W)[:n[0]])
        taken[0] += k

    go_on(4)
    out3, out1 = (C.c_int * 3)(), (C.c_int * 1)()

    def push(n_rows=ints([1, 0, 0]), a=d_f0, b=d_sp, c=d_ap, fmt=0, out=d_out, fo=out3, hh=raw):
        return L.wc_feature_stream_push_device(hh, n_rows, p(a), p(b), p(c), fmt, p(out), fo)

    def flush(want=ints([1, 0, 0]), fmt=0, out=d_out, fo=out3, hh=raw):
        return L.wc_feature_stream_flush_device(hh, want, fmt, p(out), fo)

    nan = float("nan")
    refusals = [
        lambda: L.wc_feature_stream_reset(raw, -1, 0, 0.0), lambda: L.wc_feature_stream_reset(raw, 3, 0, 0.0),
        lambda: L.wc_feature_stream_reset(None, 0, 0, 0.0), lambda: L.wc_feature_stream_reset(raw, 0, -1, 0.0),
        lambda: L.wc_feature_stream_reset(raw, 0, 9, 0.0), lambda: L.wc_feature_stream_reset(raw, 0, 1, nan),
        lambda: push(n_rows=ints([-1, 0, 0])), lambda: push(n_rows=ints([9, 0, 0])), lambda: push(n_rows=ints([1, 1, 0])),
        lambda: push(n_rows=ints([1, 0, 1])), lambda: push(n_rows=None), lambda: push(fo=None), lambda: push(hh=None),
        lambda: push(a=None), lambda: push(b=None), lambda: push(c=None), lambda: push(out=None), lambda: push(fmt=2), lambda: push(fmt=-1),
        lambda: push(out=d_f0), lambda: push(out=d_sp), lambda: push(out=d_ap),
        lambda: L.wc_feature_stream_push_device(h0._h, ints([1]), p(d_f0), p(d_sp), p(d_ap), 0, p(d_out), out1),   # bands where n_ap is 0
        lambda: flush(want=None), lambda: flush(fo=None), lambda: flush(hh=None), lambda: flush(want=ints([1, 1, 0])),
        lambda: flush(want=ints([1, 0, 1])), lambda: flush(out=None), lambda: flush(fmt=2), lambda: flush(fmt=-1),
    ]
    for i, call in enumerate(refusals):
        rc = call()
        assert rc == WC_ERR_INVALID and "feature stream" in w.last_error(), i
        assert h.rows_received(0) == taken[0] and h.frames_emitted(0) == fs.emitted(taken[0], lag) and h.get_lag(0) == lag
        assert h.get_lag(1) == -1 and h.rows_received(2) == 1 and h.frames_emitted(2) == 1
        assert h0.rows_received(0) == 0 and h0.frames_emitted(0) == 0
        go_on(1)
    for name in ("rows_received", "frames_emitted", "get_lag"):
        assert getattr(h, name)(-1) == -1 and getattr(h, name)(3) == -1
        assert getattr(L, "wc_feature_stream_" + name)(None, 0) == -1   # a NULL handle
    assert L.wc_feature_stream_max_frames_per_push(None) == WC_ERR_INVALID == L.wc_feature_stream_max_frames_per_flush(None)
    L.wc_feature_stream_destroy(None)
    w.lib().wc_synchronize()
    assert bool(torch.isnan(d_out[W:]).all())   # (the one row stream 2 flushed stands at its head)
    assert bool((d_f0 == _dev(torch, f0_h[:16])).all()) and bool((d_sp == _dev(torch, sp_h[:16])).all())
    d_tail = _guarded(torch, lag, W)
    torch.cuda.synchronize()
    assert h.flush_device([1, 0, 0], d_tail) == [lag, 0, 0]
    w.lib().wc_synchronize()
    # every row voiced: no run at all, so the pushes and the flush are the whole call on the rows taken (consequence 7)
    n = taken[0]
    assert n == 4 + len(refusals) <= n_all
    whole = device_pack(env, [n], nd, n_ap, orders, f0_h[:n], sp_h[:n], ap_h[:n])
    assert _same(np.concatenate(got + [_rows(d_tail, lag, W)]), whole)
    # an ended stream refuses rows until it is reset; a wanted stream with no rows flushes nothing and ends
    assert push() == WC_ERR_INVALID
    h.reset(0, 8, FILL)
    assert h.flush_device([1, 0, 0], None) == [0, 0, 0] and push() == WC_ERR_INVALID
    h.reset(0, 0, FILL)
    d_one = _guarded(torch, 1, W)
    torch.cuda.synchronize()
    assert push(out=d_one) == 0 and list(out3) == [1, 0, 0]
    w.lib().wc_synchronize()
    assert _same(_rows(d_one, 1, W), device_pack(env, [1], nd, n_ap, orders, f0_h[:1], sp_h[:1], ap_h[:1]))
    # a stream without bands takes its rows with d_coded_ap NULL
    W0 = fr.width(nd, 0, orders)
    d_one = _guarded(torch, 1, W0)
    torch.cuda.synchronize()
    assert h0.push_device([1], d_f0, d_sp, None, d_one) == [1]
    w.lib().wc_synchronize()
    assert _same(_rows(d_one, 1, W0), device_pack(env, [1], nd, 0, orders, f0_h[:1], sp_h[:1], np.zeros((1, 0))))
    h.close()
    h0.close()
