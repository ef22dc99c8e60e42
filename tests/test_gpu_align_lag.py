"""-m gpu: the settled positions of alignment streams (wc_align_stream_reserve_lag, _set_lag, _push_settled_device, _tail_device)
against the plain restatement of their rule (tests/align_lag_rule.py), bit for bit (NaN equal to NaN), and for unwindowed streams
against the device's own wc_align_features_ex_device run as one batch of all prefixes of the voice: track lengths around the
eight-cell rounds and the 64 lanes crossed with lags around 64 and beyond the voice, push sizes around the settle kernel's 64
lanes, rings that wrap many times, stale rings behind a reset, windows with and without the monotone flag, a mixed push, a NaN
row, the tail behind every push, wc_align_stream_push_device interleaved, every refusal, and followable voices.

Many cases share one push: a handle's streams do not depend on each other (test_a_mixed_push holds that), so a test gives every
case its own stream on the same track and pushes the same rows to all of them."""
import ctypes as C

import numpy as np
import pytest

import align_lag_rule as alr
import align_stream_rule as asr
import align_window_rule as awr

pytestmark = pytest.mark.gpu
DIMS = 8
SENT = -12345.5
HOPS = [1, 2, 8, 63, 64]
LAGS = [1, 2, 7, 63, 64, 65, 200]  # (200: beyond every voice here but one)
_refs, _whole = {}, {}


@pytest.fixture(scope="module")
def env():
    import world_class_amd as w
    from world_class_amd import io as wio, stream
    w.lib().wc_set_device(0)
    return w, wio, stream


def _rows(n, seed, dims=DIMS):
    return np.random.default_rng(seed).standard_normal((n, dims))


VOICE = _rows(200, 31200)  # made once and left unchanged
OTHER = _rows(200, 31202)
TRACK = _rows(300, 31201)


def _ref(name, a, b, open_begin, lag, win):
    """the rule's (position, cost, settled, tail behind the last row) for all rows of a on the track b with the lag, under win =
    (width, back, hop, monotone) or no window: computed once per name (the rule does not depend on the pushes,
    tests/test_align_lag_rule.py)"""
    key = (name, bool(open_begin), lag, win)
    if key not in _refs:
        f = alr.follower(b, 1, DIMS, open_begin, lag, win)
        _refs[key] = f.push(a) + ((f.tail() if lag > 0 else None),)
    return _refs[key]


def _whole_call(env, name, a, b, open_begin):
    """d_cost and d_b_on_a of wc_align_features_ex_device (pattern 0, band 0, open end) for every prefix of a against b, as ONE
    batch on the device: (cost (n), b_on_a per prefix); once per name"""
    key = (name, bool(open_begin))
    if key not in _whole:
        w, wio, stream = env
        n, m = len(a), len(b)
        a_lens, b_lens = list(range(1, n + 1)), [m] * n
        held = [w.DeviceArray.from_host(np.concatenate([a[:i] for i in a_lens])), w.DeviceArray.from_host(np.concatenate([b] * n)),
                w.DeviceArray(n), w.DeviceArray(n, np.int32), w.DeviceArray(sum(a_lens))]
        wio.align_features_ex_device(a_lens, held[0], b_lens, held[1], DIMS, 1, DIMS, 0, 0, (1 if open_begin else 0) | 2, held[2], held[3],
                                     d_b_on_a=held[4])
        w.lib().wc_synchronize()
        cost, packed = held[2].to_host(), held[4].to_host()
        ends = np.cumsum(a_lens)
        _whole[key] = (cost, [packed[e - i:e].copy() for i, e in zip(a_lens, ends)])
        for x in held:
            x.free()
    return _whole[key]


def _bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.array_equal(got, want, equal_nan=True), (what, got, want)
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok].view(np.uint64), want[ok].view(np.uint64)), what


def _same(got, want, what=None):
    for k, part in enumerate(("position", "cost", "settled")):
        _bits(got[k], want[k], (what, part))


def _against_the_whole_call(got, tail, whole, lag, what=None):
    """consequence 3 on the device: settled and the tail from d_b_on_a of the prefixes"""
    cost, maps = whole
    n = len(got[0])
    assert got[1].tobytes() == cost[:n].tobytes() and np.isfinite(cost[:n]).all(), what
    want = np.array([maps[i][max(i - lag, 0)] for i in range(n)])
    assert got[2].tobytes() == want.tobytes(), (what, got[2], want)
    if tail is not None:
        assert tail.tobytes() == maps[n - 1][-min(lag + 1, n):].tobytes(), (what, tail)


def _attach(h, u, open_begin, lag, win, track=0):
    h.reset(u, track, open_begin=open_begin)
    assert h.get_lag(u) == 0
    if win is not None:
        h.set_window(u, win[0], win[1], win[2], monotone=win[3])
    h.set_lag(u, lag)
    assert h.get_lag(u) == lag and h.get_window(u) == ((0, 0, 1, False) if win is None else tuple(win))


def _run_all(h, a, cuts, tails=None, plain_pushes=()):
    """the rows of a through EVERY stream of the handle in pushes of the sizes in cuts: per stream (position, cost, settled);
    tails, if a list, receives h.tail() behind every push; the pushes whose index is in plain_pushes go through
    wc_align_stream_push_device and their settled values are NaN here"""
    out, o = [([], [], []) for _ in range(h.n_streams)], 0
    for k, c in enumerate(cuts):
        rows = [a[o:o + c]] * h.n_streams
        res = [r + (np.full(c, np.nan),) for r in h.push(rows)] if k in plain_pushes else h.push_settled(rows)
        for u, r in enumerate(res):
            assert [len(x) for x in r] == [c] * 3
            for x, y in zip(out[u], r):
                x.append(y)
        o += c
        if tails is not None:
            tails.append(h.tail())
    assert o == len(a)
    return [tuple(np.concatenate(x) for x in s) for s in out]


def _cuts(n, k):
    return [k] * (n // k) + ([n % k] if n % k else [])


@pytest.mark.parametrize("m", [1, 2, 7, 8, 9, 64, 65, 130])
def test_track_lengths_and_lags(env, m):
    """voices of 70 and of 140 rows in one push each, every lag with and without an open beginning: the rule, and the device's
    whole call on every prefix"""
    w, wio, stream = env
    cases = [(ob, lag) for ob in (False, True) for lag in LAGS]
    h = stream.AlignStream(DIMS, len(cases), 1, 130, 140)
    h.reserve_lag(200)
    h.set_track(0, TRACK[:m])
    for n in (70, 140):
        for u, (ob, lag) in enumerate(cases):
            _attach(h, u, ob, lag, None)
        tails = []
        got = _run_all(h, VOICE[:n], [n], tails)
        for u, (ob, lag) in enumerate(cases):
            want = _ref("v%d_t%d" % (n, m), VOICE[:n], TRACK[:m], ob, lag, None)
            _same(got[u], want, (m, n, ob, lag))
            _bits(tails[0][u], want[3], (m, n, ob, lag, "tail"))
            _against_the_whole_call(got[u], tails[0][u], _whole_call(env, "v140_t%d" % m, VOICE[:140], TRACK[:m], ob), lag, (m, n, ob, lag))
            assert h.rows_received(u) == n
    h.close()


PUSH_CASES = [(False, 1, None), (True, 7, None), (False, 63, None), (True, 64, None), (False, 65, None), (True, 200, None),
              (False, 64, (17, 5, 1, False)), (True, 7, (17, 5, 8, True)), (False, 65, (64, 16, 63, True)), (True, 2, (65, 1, 64, False))]


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 130, "ragged"])
def test_push_sizes(env, k):
    """140 rows in pushes of k and in ragged cuts: lane l of the settle kernel takes pushed rows l, l + 64, l + 128"""
    w, wio, stream = env
    cuts = [5, 64, 1, 65, 3, 2] if k == "ragged" else _cuts(140, k)
    h = stream.AlignStream(DIMS, len(PUSH_CASES), 1, 130, 130)
    h.reserve_lag(200)
    h.set_track(0, TRACK[:130])
    for u, (ob, lag, win) in enumerate(PUSH_CASES):
        _attach(h, u, ob, lag, win)
    got = _run_all(h, VOICE[:140], cuts)
    tail = h.tail()
    for u, (ob, lag, win) in enumerate(PUSH_CASES):
        want = _ref("v140_t130", VOICE[:140], TRACK[:130], ob, lag, win)
        _same(got[u], want, (k, ob, lag, win))
        _bits(tail[u], want[3], (k, ob, lag, win, "tail"))
        if win is None:
            _against_the_whole_call(got[u], tail[u], _whole_call(env, "v140_t130", VOICE[:140], TRACK[:130], ob), lag, (k, ob, lag))
    h.close()


@pytest.mark.parametrize("max_lag,max_rows,lag,n,m,cuts", [
    (3, 2, 3, 41, 65, [1] * 41), (3, 2, 3, 41, 65, [2] * 20 + [1]), (3, 2, 3, 41, 65, [1, 2] * 13 + [2]), (3, 2, 2, 41, 65, [2, 1] * 13 + [2]),
    (64, 65, 64, 200, 130, [65, 65, 65, 5]), (64, 65, 64, 200, 130, [64, 1, 65, 5, 65]), (64, 65, 64, 200, 130, [1] * 7 + [63, 65, 65])])
def test_the_ring_wraps(env, max_lag, max_rows, lag, n, m, cuts):
    """a ring of max_lag + max_rows_per_push rows under a voice many times as long: no row that a walk needs has been overwritten"""
    w, wio, stream = env
    cases = [(False, None), (True, None), (False, (17, 5, 8, True)), (True, (33, 9, 1, False))]
    h = stream.AlignStream(DIMS, len(cases), 1, m, max_rows)
    h.reserve_lag(max_lag)
    h.set_track(0, TRACK[:m])
    for u, (ob, win) in enumerate(cases):
        _attach(h, u, ob, lag, win)
    tails = []
    got = _run_all(h, VOICE[:n], cuts, tails)
    for u, (ob, win) in enumerate(cases):
        want = _ref("v%d_t%d" % (n, m), VOICE[:n], TRACK[:m], ob, lag, win)
        _same(got[u], want, (cuts[:3], ob, win))
        _bits(tails[-1][u], want[3], (cuts[:3], ob, win, "tail"))
        if win is None:
            _against_the_whole_call(got[u], tails[-1][u], _whole_call(env, "v%d_t%d" % (n, m), VOICE[:n], TRACK[:m], ob), lag, (cuts[:3], ob))
    h.close()


def test_a_stale_ring_never_shows(env):
    """voice X to its end, then a reset, the lag again and voice Y on the same streams, windowed and unwindowed: Y's rule result,
    though the ring holds X's choices in every row that Y has not reached and outside Y's windows.  Stream 4 follows a track of 9
    rows in a handle whose rows are 300 wide, beside a stream on the track of 300"""
    w, wio, stream = env
    cases = [(0, False, 7, None), (0, True, 64, None), (0, False, 20, (17, 5, 8, True)), (0, True, 65, (33, 32, 2, False)), (1, True, 30, None),
             (0, True, 100, (64, 20, 64, False))]
    tracks = [TRACK, TRACK[100:109]]
    h = stream.AlignStream(DIMS, len(cases), 2, 300, 64)
    h.reserve_lag(100)
    for t, b in enumerate(tracks):
        h.set_track(t, b)
    for a, name, cuts in ((OTHER[:140], "x", [64, 64, 12]), (VOICE[:100], "y", [30, 64, 6]), (OTHER[:70], "z", [1, 5, 64])):
        for u, (t, ob, lag, win) in enumerate(cases):
            _attach(h, u, ob, lag, win, t)
        got = _run_all(h, a, cuts)
        tail = h.tail()
        for u, (t, ob, lag, win) in enumerate(cases):
            want = _ref("stale_%s_%d" % (name, t), a, tracks[t], ob, lag, win)
            _same(got[u], want, (name, u))
            _bits(tail[u], want[3], (name, u, "tail"))
    h.close()


def _windows(m):
    """(open_begin, lag, (width, back, hop, monotone)) for a track of m rows: every width with back 0, 1 and width - 1, the hops,
    the two flags and the lags in rotation (the pattern of tests/test_gpu_align_window.py)"""
    cases = []
    for width in (1, 2, 7, 8, 9, 17, 63, 64, 65, m, m + 3):
        for back in sorted({0, min(1, width - 1), width - 1}):
            k = len(cases)
            cases.append((k % 2 == 1, LAGS[k % 7], (width, back, HOPS[k % 5], k % 3 == 2)))
    return cases


@pytest.mark.parametrize("m", [65, 130])
def test_windows(env, m):
    """140 rows in three pushes under about thirty windows, with the acquisition epoch of an open beginning; and consequence 4 on
    the device: a window over the whole track without the monotone flag gives the same handle's unwindowed settled values"""
    w, wio, stream = env
    cases = _windows(m)
    whole = [(ob, lag, win) for ob in (False, True) for lag in (7, 64) for win in (None, (m, 0, 1, False), (m + 7, 3, 63, False), (1 << 30, m - 1, 8, False))]
    cases = cases + whole
    h = stream.AlignStream(DIMS, len(cases), 1, 130, 70)
    h.reserve_lag(200)
    h.set_track(0, TRACK[:m])
    for u, (ob, lag, win) in enumerate(cases):
        _attach(h, u, ob, lag, win)
    got = _run_all(h, VOICE[:140], [5, 70, 65])
    tail = h.tail()
    for u, (ob, lag, win) in enumerate(cases):
        want = _ref("v140_t%d" % m, VOICE[:140], TRACK[:m], ob, lag, win)
        _same(got[u], want, (m, ob, lag, win))
        _bits(tail[u], want[3], (m, ob, lag, win, "tail"))
    first = len(cases) - len(whole)
    for u in range(first, len(cases)):
        plain = first + 4 * ((u - first) // 4)
        assert cases[plain][2] is None and cases[plain][:2] == cases[u][:2]
        for x, y in zip(got[u], got[plain]):
            assert x.tobytes() == y.tobytes(), cases[u]
        assert tail[u].tobytes() == tail[plain].tobytes()
    h.close()


# (track, open_begin, lag, window): lag only, window only, both, neither
MIXED = [(0, False, 20, None), (1, True, 0, (40, 10, 1, False)), (0, True, 64, (24, 6, 8, True)), (2, False, 0, None), (0, True, 3, None),
         (2, False, 9, (16, 15, 64, False))]


def _mixed(env, counts_per_round, settled=True):
    """six streams on three tracks pushed through the device form into sentinel-filled outputs, stream u taking
    counts_per_round[r][u] rows of its voice in round r.  Returns per stream (position, cost, settled) over all its rows"""
    w, wio, stream = env
    tracks = [TRACK[:130], TRACK[140:149], TRACK[160:224]]
    voices = [VOICE[:140], VOICE[:140][::-1].copy(), OTHER[:140], OTHER[5:145], VOICE[17:157], OTHER[30:170]]
    h = stream.AlignStream(DIMS, 6, 3, 130, 64)
    h.reserve_lag(64)
    for t, b in enumerate(tracks):
        h.set_track(t, b)
    for u, (t, ob, lag, win) in enumerate(MIXED):
        _attach(h, u, ob, lag, win, t)
    taken = [0] * 6
    res = [([], [], []) for _ in range(6)]
    cap = 6 * 64
    for counts in counts_per_round:
        rows = np.concatenate([voices[u][taken[u]:taken[u] + c] for u, c in enumerate(counts)] + [np.zeros((0, DIMS))])
        held = [w.DeviceArray.from_host(rows if len(rows) else np.zeros((1, DIMS)))] + [w.DeviceArray.from_host(np.full(cap + 2, SENT)) for _ in range(3)]
        if settled:
            h.push_settled_device(counts, *held)
        else:
            h.push_device(counts, *held[:3])
        outs = [x.to_host() for x in held[1:]]
        for x in held:
            x.free()
        tot = sum(counts)
        for k, o in enumerate(outs):
            assert (o[tot:] == SENT).all(), "a result behind the pushed rows was written"
            assert settled or k < 2 or (o == SENT).all(), "wc_align_stream_push_device wrote a settled value"
        o = 0
        for u, c in enumerate(counts):
            for k in range(3):
                res[u][k].append(outs[k][o:o + c])
            taken[u] += c
            o += c
    assert [h.rows_received(u) for u in range(6)] == taken
    tail = h.tail()
    assert [x is not None for x in tail] == [lag > 0 and taken[u] > 0 for u, (t, ob, lag, win) in enumerate(MIXED)]
    h.close()
    out = [tuple(np.concatenate(x) for x in r) for r in res]
    if settled:
        for u, (t, ob, lag, win) in enumerate(MIXED):
            f = alr.follower(tracks[t], 1, DIMS, ob, lag, win)
            _same(out[u], f.push(voices[u][:taken[u]]), u)
            if tail[u] is not None:
                _bits(tail[u], f.tail(), (u, "tail"))
    return out, tail


def test_a_mixed_push(env):
    """streams with a lag only, a window only, both, neither and no rows in the same pushes: each equals the rule, each equals the
    same stream pushed alone with its neighbours idle, and the streams without a lag get from both entry points the same
    positions and costs, with their position as the settled value"""
    rounds = [[3, 64, 0, 7, 1, 0], [0, 0, 64, 7, 1, 64], [64, 1, 64, 0, 1, 35], [1, 0, 0, 64, 1, 0], [0, 2, 0, 35, 1, 0], [62, 63, 1, 0, 1, 41]]
    together, tails = _mixed(env, rounds)
    for u in range(6):
        alone, tail = _mixed(env, [[c if v == u else 0 for v, c in enumerate(r)] for r in rounds])
        for x, y in zip(alone[u], together[u]):
            assert x.tobytes() == y.tobytes(), u
        assert (tail[u] is None and tails[u] is None) or tail[u].tobytes() == tails[u].tobytes()
    plain, _ = _mixed(env, rounds, settled=False)
    for u, (t, ob, lag, win) in enumerate(MIXED):
        assert plain[u][0].tobytes() == together[u][0].tobytes() and plain[u][1].tobytes() == together[u][1].tobytes(), u
        if lag == 0:
            assert together[u][2].tobytes() == together[u][0].tobytes()


def test_a_nan_row_in_the_middle_of_a_voice(env):
    """a NaN row of the voice: no cell wins in or behind it, so settled is NaN from there on and the tail behind it is all NaN, K
    entries of it; the rows before it are untouched.  A NaN row of the track leaves the columns in front of it alone: the
    settled values go on, per the rule"""
    w, wio, stream = env
    voice = VOICE[:100].copy()
    voice[37, 5] = np.nan
    track = TRACK[:65].copy()
    track[50, 3] = np.nan
    cases = [(0, False, 5, None), (0, True, 64, None), (0, False, 20, (17, 5, 1, False)), (0, True, 7, (17, 5, 8, True)), (1, False, 5, None),
             (1, True, 64, (33, 8, 8, True))]
    tracks = [TRACK[:65], track]
    h = stream.AlignStream(DIMS, len(cases), 2, 65, 64)
    h.reserve_lag(64)
    for t, b in enumerate(tracks):
        h.set_track(t, b)
    for a, name in ((voice, "nan_voice"), (VOICE[:100], "nan_track")):
        for u, (t, ob, lag, win) in enumerate(cases):
            _attach(h, u, ob, lag, win, t)
        tails = []
        got = _run_all(h, a, [30, 8, 62], tails)  # (the NaN row is the last of the second push)
        for u, (t, ob, lag, win) in enumerate(cases):
            f = alr.follower(tracks[t], 1, DIMS, ob, lag, win)
            want = f.push(a)
            _same(got[u], want, (name, u))
            _bits(tails[-1][u], f.tail(), (name, u, "tail"))
            if name == "nan_voice":
                assert np.isnan(got[u][2][37:]).all() and np.isnan(tails[1][u]).all() and len(tails[1][u]) == min(lag + 1, 38)
                if win is None:
                    assert not np.isnan(got[u][2][:37]).any() and not np.isnan(tails[0][u]).any()
            elif t == 1 and win is None:
                assert not np.isnan(got[u][2][1:]).any() and (got[u][0][1:] < 50).all()
    h.close()


def test_the_tail_behind_every_push(env):
    """the tail behind every push of a cut sequence: the whole call's last K entries (unwindowed) and the rule's; a tail changes
    nothing, so the pushes behind it give the same bits as without it, and two tails in a row are the same"""
    w, wio, stream = env
    cases = [(False, 1, None), (True, 7, None), (False, 64, None), (True, 140, None), (False, 20, (17, 5, 8, True)), (True, 65, (40, 10, 1, False))]
    cuts = [1, 1, 5, 64, 1, 63, 5]
    h = stream.AlignStream(DIMS, len(cases), 1, 130, 64)
    h.reserve_lag(140)
    h.set_track(0, TRACK[:130])
    for u, (ob, lag, win) in enumerate(cases):
        _attach(h, u, ob, lag, win)
    tails = []
    got = _run_all(h, VOICE[:140], cuts, tails)
    again = h.tail()
    for u, (ob, lag, win) in enumerate(cases):
        f = alr.follower(TRACK[:130], 1, DIMS, ob, lag, win)
        o = 0
        for k, c in enumerate(cuts):
            f.push(VOICE[o:o + c])
            o += c
            _bits(tails[k][u], f.tail(), (u, k))
            if win is None:
                maps = _whole_call(env, "v140_t130", VOICE[:140], TRACK[:130], ob)[1]
                assert tails[k][u].tobytes() == maps[o - 1][-min(lag + 1, o):].tobytes(), (u, k)
        _same(got[u], _ref("v140_t130", VOICE[:140], TRACK[:130], ob, lag, win), u)
        assert again[u].tobytes() == tails[-1][u].tobytes()
    only = h.tail([1, 4])  # packed stream by stream: the two that were asked for
    assert [x is not None for x in only] == [False, True, False, False, True, False]
    assert only[1].tobytes() == again[1].tobytes() and only[4].tobytes() == again[4].tobytes()
    h.close()


def test_push_device_on_a_stream_with_a_lag(env):
    """wc_align_stream_push_device records the choices and writes no settled value: interleaved with the settled push, the settled
    values of the later rows are the rule's"""
    w, wio, stream = env
    cases = [(False, 7, None), (True, 64, None), (False, 20, (17, 5, 8, True)), (True, 100, (40, 10, 1, False))]
    cuts, plain_pushes = [10, 30, 1, 64, 5, 20, 10], (0, 1, 3, 5)
    h = stream.AlignStream(DIMS, len(cases), 1, 130, 64)
    h.reserve_lag(100)
    h.set_track(0, TRACK[:130])
    for u, (ob, lag, win) in enumerate(cases):
        _attach(h, u, ob, lag, win)
    got = _run_all(h, VOICE[:140], cuts, plain_pushes=plain_pushes)
    tail = h.tail()
    written = np.concatenate([np.full(c, k not in plain_pushes) for k, c in enumerate(cuts)])
    for u, (ob, lag, win) in enumerate(cases):
        want = _ref("v140_t130", VOICE[:140], TRACK[:130], ob, lag, win)
        _same((got[u][0], got[u][1], got[u][2][written]), (want[0], want[1], want[2][written]), u)
        _bits(tail[u], want[3], (u, "tail"))
    h.close()


def test_refusals_leave_everything_as_it_was(env):
    w, wio, stream = env
    L = stream._lib()
    h = stream.AlignStream(DIMS, 4, 2, 130, 16)
    h.set_track(0, TRACK[:130])
    for u in range(3):
        h.reset(u, 0)
    state = lambda: ([h.get_lag(u) for u in range(4)], [h.rows_received(u) for u in range(4)])
    assert h.get_lag(-1) == -1 and h.get_lag(4) == -1
    d_rows, d_out = w.DeviceArray.from_host(VOICE[:16]), [w.DeviceArray.from_host(np.full(20, SENT)) for _ in range(3)]
    d_tail = w.DeviceArray.from_host(np.full(20, SENT))

    def refused(calls, want):
        for k, call in enumerate(calls):
            with pytest.raises(w.WorldClassError):
                call()
            assert state() == want, k
        assert all((x.to_host() == SENT).all() for x in d_out + [d_tail]), "a refused call wrote"

    # before the reservation: no lag but 0, no tail, no reservation that is too small or too large
    refused([lambda: h.set_lag(0, 1), lambda: h.reserve_lag(0), lambda: h.reserve_lag(-1), lambda: h.reserve_lag(1 << 30),
             lambda: h.reserve_lag((1 << 30) // (4 * 130) - 15),  # (4 streams x (max_lag + 16) rows x 130 bytes: one row of rings above 2^30)
             lambda: h.reserve_lag((1 << 31) - 1), lambda: h.tail([0])], ([0] * 4, [0] * 4))
    h.set_lag(0, 0)
    h.reserve_lag(8)
    h.set_lag(0, 8)
    h.set_lag(1, 3)
    h.set_lag(1, 0)  # removed again
    h.set_lag(2, 5)
    first = h.push_settled([VOICE[:3], None, None, None])[0]  # stream 0 has rows now
    want = ([8, 0, 5, 0], [3, 0, 0, 0])
    refused([lambda: h.reserve_lag(8), lambda: h.reserve_lag(1),  # twice
             lambda: h.set_lag(-1, 1), lambda: h.set_lag(4, 1),  # a bad index
             lambda: h.set_lag(3, 1), lambda: h.set_lag(3, 0),  # never reset
             lambda: h.set_lag(0, 2), lambda: h.set_lag(0, 0),  # a stream with rows
             lambda: h.set_lag(1, 9), lambda: h.set_lag(1, -1),  # above max_lag, negative
             lambda: h.push_settled_device([1, 0, 2, 0], d_rows, d_out[0], d_out[1], None),  # no d_settled
             lambda: h.push_settled_device([1, 0, 2, 0], d_rows, None, d_out[1], d_out[2]),
             lambda: h.push_settled_device([1, 0, 0, 1], d_rows, *d_out),  # rows for a stream that was never reset
             lambda: h.push_settled_device([1, 17, 0, 0], d_rows, *d_out), lambda: h.push_settled_device([1, -1, 0, 0], d_rows, *d_out),
             lambda: h.tail([1]), lambda: h.tail([0, 1]),  # a stream without a lag
             lambda: h.tail([2]), lambda: h.tail([0, 2]),  # a stream without rows
             lambda: w._check(L.wc_align_stream_tail_device(h._h, None, d_tail.ptr)),
             lambda: w._check(L.wc_align_stream_tail_device(h._h, (C.c_int * 4)(1, 0, 0, 0), None))], want)
    h.push_settled_device([0, 0, 0, 0], None, None, None, None)  # no rows: nothing to read or to write
    assert state() == want
    rest = h.push_settled([VOICE[3:16], VOICE[:16], VOICE[:16], None])
    got = tuple(np.concatenate([first[k], rest[0][k]]) for k in range(3))
    _same(got, _ref("v16_t130", VOICE[:16], TRACK[:130], False, 8, None), "refused in between")
    _same(rest[1], _ref("v16_t130", VOICE[:16], TRACK[:130], False, 0, None), "set_lag(0)")
    _same(rest[2], _ref("v16_t130", VOICE[:16], TRACK[:130], False, 5, None), "refused throughout")
    plain = asr.follow(VOICE[:16], TRACK[:130], 1, DIMS)
    _bits(rest[1][0], plain[0], "position")
    _bits(rest[1][2], plain[0], "settled at lag 0")
    h.reset(0, 0)  # a reset removes the lag
    assert state() == ([0, 0, 5, 0], [0, 16, 16, 0])
    _same(h.push_settled([VOICE[:16], None, None, None])[0], _ref("v16_t130", VOICE[:16], TRACK[:130], False, 0, None), "after the reset")
    for x in [d_rows, d_tail] + d_out:
        x.free()
    h.close()


@pytest.mark.parametrize("s", [0, 3, 7])
def test_a_followable_voice(env, s):
    """a followable voice of tests/align_window_rule.py (dims 8, every coefficient compared) at lag 20 under the window (60, 20, 8,
    monotone) and without a window: the rule bit for bit.  Prints the two quality figures of tools/align_lag_probe.py; nothing is
    asserted on them"""
    w, wio, stream = env
    voice, track, _ = awr.followable(s)
    win = (60, 20, 8, True)
    h = stream.AlignStream(8, 2, 1, 300, 64, dim_begin=0)
    h.reserve_lag(20)
    h.set_track(0, track)
    _attach(h, 0, False, 20, win)
    _attach(h, 1, False, 20, None)
    got = _run_all(h, voice, [64, 64, 22])
    tail = h.tail()
    for u, wn in enumerate((win, None)):
        f = alr.follower(track, 0, 8, False, 20, wn)
        _same(got[u], f.push(voice), (s, wn))
        _bits(tail[u], f.tail(), (s, wn, "tail"))
        # rows 0..n-1 on the newest path: the settled values of rows 20.. stand for rows 0..n-21, the tail for the rest
        settled = np.concatenate([got[u][2][20:], tail[u][1:]])
        true = alr.true_positions(s)
        falls = float((np.diff(got[u][2]) < 0).mean())
        print("followable(%d) %s: settled falls in %.3f of the rows; mean |settled - true| %.3f, mean |position - true| %.3f"
              % (s, "windowed" if wn else "unwindowed", falls, np.abs(settled - true).mean(), np.abs(got[u][0] - true).mean()))
    h.close()
