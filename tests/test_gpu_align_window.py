"""-m gpu: alignment streams with a search window (wc_align_stream_set_window) against the plain restatement of their rule
(tests/align_window_rule.py), bit for bit (NaN equal to NaN): track lengths and widths around the eight-cell rounds and the 64
lanes, every back and hop at its ends, push sizes around an epoch, the same rows cut three ways from either state-row parity, the
acquisition epoch of an open beginning, a window over the whole track beside the same handle's unwindowed stream, windowed and
unwindowed streams in one push, poisoned state rows and local costs, the monotone flag on a phrase that stands twice, a NaN row,
the window removed again, every refusal, and one of the followable voices of tests/test_align_window_rule.py.

Many cases share one push: a handle's streams do not depend on each other (test_a_mixed_push holds that), so a test gives every
window its own stream on the same track and pushes the same rows to all of them."""
import ctypes as C

import numpy as np
import pytest

import align_stream_rule as asr
import align_window_rule as awr

pytestmark = pytest.mark.gpu
DIMS = 60
SENT = -12345.5
HOPS = [1, 2, 8, 63, 64]
_refs = {}


@pytest.fixture(scope="module")
def env():
    import world_class_amd as w
    from world_class_amd import io as wio, stream
    w.lib().wc_set_device(0)
    return w, wio, stream


def _rows(n, seed, dims=DIMS):
    return np.random.default_rng(seed).standard_normal((n, dims))


VOICE = _rows(130, 30200)  # made once and left unchanged
TRACK = _rows(300, 30201)


def _ref(name, a, b, open_begin, win):
    """the rule's (position, cost) for all rows of a on the track b under win = (width, back, hop, monotone), or under no window
    for win = None: computed once per name (the rule does not depend on the pushes, tests/test_align_window_rule.py)"""
    key = (name, bool(open_begin), win)
    if key not in _refs:
        _refs[key] = asr.follow(a, b, 1, DIMS, open_begin) if win is None else awr.follow(a, b, 1, DIMS, open_begin, *win)
    return _refs[key]


def _same(got, want, what=None):
    assert np.array_equal(got[0], want[0], equal_nan=True), (what, "position", got[0], want[0])
    assert np.array_equal(got[1], want[1], equal_nan=True), (what, "cost", got[1], want[1])
    finite = ~np.isnan(want[1])
    assert np.array_equal(np.asarray(got[1])[finite].view(np.uint64), np.asarray(want[1])[finite].view(np.uint64)), what


def _attach(h, u, open_begin, win, track=0):
    h.reset(u, track, open_begin=open_begin)
    if win is not None:
        h.set_window(u, win[0], win[1], win[2], monotone=win[3])
        assert h.get_window(u) == tuple(win)
    else:
        assert h.get_window(u) == (0, 0, 1, False)


def _run_all(h, a, cuts):
    """the rows of a through EVERY stream of the handle in pushes of the sizes in cuts: per stream (position, cost)"""
    out, o = [([], []) for _ in range(h.n_streams)], 0
    for c in cuts:
        for u, (p, q) in enumerate(h.push([a[o:o + c]] * h.n_streams)):
            assert len(p) == c and len(q) == c
            out[u][0].append(p)
            out[u][1].append(q)
        o += c
    assert o == len(a)
    return [(np.concatenate(p), np.concatenate(q)) for p, q in out]


def _cuts(n, k):
    return [k] * (n // k) + ([n % k] if n % k else [])


def _poison(h, cases, track=0):
    """130 rows of NaN through every stream, unwindowed (all m columns of both state rows and of d become NaN), then the cases are
    attached again"""
    for u in range(h.n_streams):
        h.reset(u, track)
    for p, c in h.push([np.full((130, h.dims), np.nan)] * h.n_streams):
        assert np.isnan(p).all() and np.isnan(c).all() and len(p) == 130
    for u, (ob, win) in enumerate(cases):
        _attach(h, u, ob, win, track)


def _windows(m):
    """(open_begin, (width, back, hop, monotone)) for a track of m rows: every width with back 0, 1 and width - 1, the hops and the
    two flags in rotation"""
    cases = []
    for width in (1, 2, 7, 8, 9, 17, 63, 64, 65, m, m + 3):
        for back in sorted({0, min(1, width - 1), width - 1}):
            k = len(cases)
            cases.append((k % 2 == 1, (width, back, HOPS[k % 5], k % 3 == 2)))
    return cases


@pytest.mark.parametrize("m", [1, 2, 7, 8, 9, 17, 64, 65, 130, 300])
def test_track_lengths_widths_backs_and_hops(env, m):
    """70 rows in one push on tracks around the eight-cell rounds and the 64 lanes: about thirty windows, one stream each"""
    w, wio, stream = env
    cases = _windows(m)
    h = stream.AlignStream(DIMS, len(cases), 1, 300, 130)
    h.set_track(0, TRACK[:m])
    _poison(h, cases)
    got = _run_all(h, VOICE[:70], [70])
    for u, (ob, win) in enumerate(cases):
        _same(got[u], _ref("v70_t%d" % m, VOICE[:70], TRACK[:m], ob, win), (m, ob, win))
        assert h.rows_received(u) == 70
    h.close()


PUSH_CASES = [(False, (17, 5, 1, False)), (True, (17, 5, 8, False)), (False, (64, 16, 63, True)), (True, (65, 1, 64, False)),
              (False, (9, 8, 2, True)), (True, (130, 0, 8, True)), (False, (1, 0, 1, False)), (False, (63, 62, 64, False))]


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 130])
def test_push_sizes(env, k):
    """130 rows in pushes of k: passes end with the push or with the epoch, whichever comes first"""
    w, wio, stream = env
    h = stream.AlignStream(DIMS, len(PUSH_CASES), 1, 130, 130)
    h.set_track(0, TRACK[:130])
    for u, (ob, win) in enumerate(PUSH_CASES):
        _attach(h, u, ob, win)
    got = _run_all(h, VOICE, _cuts(130, k))
    for u, (ob, win) in enumerate(PUSH_CASES):
        _same(got[u], _ref("v130_t130", VOICE, TRACK[:130], ob, win), (k, ob, win))
        assert h.rows_received(u) == 130
    h.close()


def test_split_invariance_and_state_parity(env):
    """the same 130 rows as 130 x 1, as (64, 1, 65) and as one push, then again as (64, 1, 65) and as 130 x 1, on the same streams
    with a reset in between.  Under hop 8 one push of 130 rows is 17 passes and under hop 64 three: the parity of the state rows
    flips, under hop 3 (44 passes) it does not; epoch boundaries fall inside the pushes and between them"""
    w, wio, stream = env
    cases = [(False, (17, 5, 8, False)), (True, (17, 5, 8, True)), (False, (33, 9, 64, False)), (True, (24, 23, 3, True)), (False, (40, 0, 1, False))]
    h = stream.AlignStream(DIMS, len(cases), 1, 130, 130)
    h.set_track(0, TRACK[:130])
    outs = []
    for cuts in ([1] * 130, [64, 1, 65], [130], [64, 1, 65], [1] * 130):
        for u, (ob, win) in enumerate(cases):
            _attach(h, u, ob, win)
        outs.append(_run_all(h, VOICE, cuts))
        for u, (ob, win) in enumerate(cases):
            _same(outs[-1][u], _ref("v130_t130", VOICE, TRACK[:130], ob, win), (cuts[:3], ob, win))
    for o in outs[1:]:
        for u in range(len(cases)):
            assert o[u][0].tobytes() == outs[0][u][0].tobytes() and o[u][1].tobytes() == outs[0][u][1].tobytes()
    h.close()


def test_acquisition_under_an_open_beginning(env):
    """a 40-row phrase that starts at column 150 of 300: under an open beginning the first hop rows search the whole track and find
    it (cost 0.0, position 150 + i), then 32 columns follow it; without the flag the window starts at column 0"""
    w, wio, stream = env
    track = TRACK.copy()
    phrase = _rows(40, 30202)
    track[150:190] = phrase
    cases = [(True, (32, 8, 1, False)), (True, (32, 8, 8, False)), (True, (32, 8, 8, True)), (False, (32, 8, 1, False)), (False, (32, 8, 8, False))]
    h = stream.AlignStream(DIMS, len(cases), 1, 300, 130)
    h.set_track(0, track)
    for cuts in ([40], [13, 27], [1] * 40):
        _poison(h, cases)
        got = _run_all(h, phrase, cuts)
        for u, (ob, win) in enumerate(cases):
            _same(got[u], _ref("phrase150", phrase, track, ob, win), (cuts[:2], ob, win))
            if ob:
                assert (got[u][1] == 0.0).all() and got[u][0].tolist() == [150.0 + i for i in range(40)]
            else:
                assert (got[u][0] < 150).all() and (got[u][1] > 0.0).all()
    h.close()


@pytest.mark.parametrize("m", [9, 65, 130])
def test_a_window_over_the_whole_track_is_the_same_handles_unwindowed_stream(env, m):
    w, wio, stream = env
    cases = [(ob, win) for ob in (False, True) for win in (None, (m, 0, 1, False), (m, m - 1, 8, False), (m + 7, 3, 63, False), (1 << 30, 1, 64, False))]
    h = stream.AlignStream(DIMS, len(cases), 1, 130, 130)
    h.set_track(0, TRACK[:m])
    _poison(h, cases)
    got = _run_all(h, VOICE, [5, 64, 61])
    for u, (ob, win) in enumerate(cases):
        plain = got[0 if not ob else 5]
        assert got[u][0].tobytes() == plain[0].tobytes() and got[u][1].tobytes() == plain[1].tobytes(), (m, ob, win)
        _same(got[u], _ref("v130_t%d" % m, VOICE, TRACK[:m], ob, None), (m, ob, win))
    h.close()


def _mixed(env, counts_of_others):
    """five streams on three tracks of 130, 9 and 64 rows, pushed through the device form into sentinel-filled outputs: streams 0, 2
    and 3 with a window, 1 and 4 without.  Stream 0 always takes (3, 0, 64, 1, 0, 62) rows; the others take what
    counts_of_others(u, round) says.  Returns per stream (position, cost) over all its rows and the rows it took"""
    w, wio, stream = env
    tracks = [TRACK[:130], TRACK[140:149], TRACK[160:224]]
    attach = [(0, False, (24, 6, 8, True)), (1, True, None), (0, True, (40, 10, 1, False)), (2, False, (16, 15, 64, False)), (0, False, None)]
    voices = [VOICE, VOICE[::-1].copy(), VOICE[5:], VOICE[17:], VOICE]
    h = stream.AlignStream(DIMS, 5, 3, 130, 64)
    for t, b in enumerate(tracks):
        h.set_track(t, b)
    for u, (t, ob, win) in enumerate(attach):
        _attach(h, u, ob, win, t)
    own = (3, 0, 64, 1, 0, 62)
    taken = [0] * 5
    res = [([], []) for _ in range(5)]
    cap = 5 * 64
    for r in range(len(own)):
        counts = [own[r]] + [min(counts_of_others(u, r), len(voices[u]) - taken[u]) for u in range(1, 5)]
        rows = np.concatenate([voices[u][taken[u]:taken[u] + c] for u, c in enumerate(counts)] + [np.zeros((0, DIMS))])
        d_rows = w.DeviceArray.from_host(rows if len(rows) else np.zeros((1, DIMS)))
        d_pos, d_cost = w.DeviceArray.from_host(np.full(cap + 2, SENT)), w.DeviceArray.from_host(np.full(cap + 2, SENT))
        h.push_device(counts, d_rows, d_pos, d_cost)
        pos, cost = d_pos.to_host(), d_cost.to_host()
        for x in (d_rows, d_pos, d_cost):
            x.free()
        tot = sum(counts)
        assert (pos[tot:] == SENT).all() and (cost[tot:] == SENT).all(), "a result behind the pushed rows was written"
        o = 0
        for u, c in enumerate(counts):
            res[u][0].append(pos[o:o + c])
            res[u][1].append(cost[o:o + c])
            taken[u] += c
            o += c
    assert [h.rows_received(u) for u in range(5)] == taken
    h.close()
    out = []
    for u, (t, ob, win) in enumerate(attach):
        got = (np.concatenate(res[u][0]), np.concatenate(res[u][1]))
        a = voices[u][:taken[u]]
        _same(got, asr.follow(a, tracks[t], 1, DIMS, ob) if win is None else awr.follow(a, tracks[t], 1, DIMS, ob, *win), u)
        out.append(got)
    return out, taken


def test_a_mixed_push(env):
    """three windowed and two unwindowed streams on three tracks in the same pushes, with idle streams; then with other
    neighbours: the unwindowed streams equal tests/align_stream_rule.py, the windowed the window's rule, and stream 0 does not change"""
    pattern = {1: (64, 0, 1, 0, 2, 63), 2: (0, 64, 64, 0, 0, 0), 3: (7, 7, 0, 64, 35, 0), 4: (1, 1, 1, 1, 1, 1)}
    a, taken_a = _mixed(env, lambda u, r: pattern[u][r])
    b, taken_b = _mixed(env, lambda u, r: pattern[5 - u][(r + 1) % 6])
    assert taken_a[0] == taken_b[0] == 130 and taken_a[1:] != taken_b[1:]
    assert a[0][0].tobytes() == b[0][0].tobytes() and a[0][1].tobytes() == b[0][1].tobytes()


def test_stale_state_rows_and_local_costs_never_show(env):
    """before every comparison the same streams take 130 rows of NaN without a window, so that both state rows and all of d are
    NaN in every column; then they are reset, get their windows and are pushed for real: what lies outside a window is +inf by the
    rule, never what memory holds"""
    w, wio, stream = env
    cases = [(False, (8, 3, 1, False)), (True, (8, 3, 1, True)), (False, (17, 0, 8, True)), (True, (33, 32, 2, False)), (False, (64, 20, 64, False)),
             (True, (5, 1, 63, False))]
    h = stream.AlignStream(DIMS, len(cases), 1, 130, 130)
    for m, cuts in ((130, [130]), (65, [64, 6]), (9, [1, 2]), (130, [1] * 5 + [65])):
        h.set_track(0, TRACK[:m])
        _poison(h, cases)
        n = sum(cuts)
        got = _run_all(h, VOICE[:n], cuts)
        for u, (ob, win) in enumerate(cases):
            _same(got[u], awr.follow(VOICE[:n], TRACK[:m], 1, DIMS, ob, *win), (m, cuts[:2], ob, win))
        for u in range(len(cases)):  # (set_track is refused while a stream with rows follows the slot)
            h.reset(u, 0)
    h.close()


def test_the_monotone_flag_on_a_phrase_that_stands_twice(env):
    """the track holds the phrase at column 50 and at column 120, each with a little noise whose size changes along the phrase: the
    first copy is the cheaper one up to row 11, the second up to row 25, then the first again.  The plain windowed position jumps
    forward and back (in the rule); the monotone one only forward"""
    w, wio, stream = env
    rng = np.random.default_rng(30203)
    phrase, track = rng.standard_normal((40, DIMS)), TRACK.copy()

    def unit(n):
        v = rng.standard_normal((n, DIMS))
        return v / np.linalg.norm(v[:, 1:], axis=1)[:, None]

    track[50:90] = phrase + np.r_[np.full(10, 0.01), np.full(10, 0.5), np.full(20, 0.01)][:, None] * unit(40)
    track[120:160] = phrase + np.r_[np.full(20, 0.1), np.full(20, 0.5)][:, None] * unit(40)
    cases = [(True, (192, 80, hop, mono)) for hop in (1, 8) for mono in (False, True)]
    h = stream.AlignStream(DIMS, len(cases), 1, 300, 130)
    h.set_track(0, track)
    for cuts in ([40], [13, 27]):
        _poison(h, cases)
        got = _run_all(h, phrase, cuts)
        for u, (ob, win) in enumerate(cases):
            want = _ref("twice", phrase, track, ob, win)
            _same(got[u], want, (cuts, win))
            assert not np.isnan(want[0]).any()
            assert (np.diff(want[0]) >= 0).all() == win[3] and want[0][11] < 120 <= want[0][12]
            assert (want[0][26:] >= 120).all() == win[3]
    h.close()


def test_a_nan_row_in_the_middle_of_a_voice(env):
    """no cell wins in or behind a NaN row: the position is NaN from there on and the window stays where it was; the cost is NaN at
    the row and +inf behind it"""
    w, wio, stream = env
    voice = VOICE[:100].copy()
    voice[37, 20] = np.nan
    cases = [(False, (17, 5, 1, False)), (True, (17, 5, 8, True)), (False, (65, 64, 2, True)), (True, (9, 0, 64, False))]
    h = stream.AlignStream(DIMS, len(cases), 1, 65, 64)
    h.set_track(0, TRACK[:65])
    for u, (ob, win) in enumerate(cases):
        _attach(h, u, ob, win)
    got = _run_all(h, voice, [30, 30, 40])
    for u, (ob, win) in enumerate(cases):
        los = []
        _same(got[u], awr.follow(voice, TRACK[:65], 1, DIMS, ob, *win, los=los), (ob, win))
        assert len(set(los[37:])) == 1
        assert not np.isnan(got[u][0][:37]).any() and np.isnan(got[u][0][37:]).all()
        assert np.isnan(got[u][1][37]) and (got[u][1][38:] == np.inf).all()
    h.close()


def test_refusals_and_the_window_removed_again(env):
    """every refused set_window leaves the settings and the stream's next results as they were; set_window(0) after a reset
    gives the unwindowed results; a reset removes the window"""
    w, wio, stream = env
    L = stream._lib()
    h = stream.AlignStream(DIMS, 4, 2, 130, 16)
    h.set_track(0, TRACK[:130])
    with pytest.raises(w.WorldClassError):  # never reset
        h.set_window(0, 8, 2)
    assert h.get_window(0) == (0, 0, 1, False)
    for u in range(3):
        h.reset(u, 0)
    h.set_window(0, 17, 5, 8, monotone=True)
    h.set_window(1, 17, 5, 8, monotone=True)
    h.set_window(1, 0, 0)  # removed again
    first = h.push([VOICE[:3], None, None, None])[0]  # stream 0 has rows now
    ok = [(17, 5, 8, True), (0, 0, 1, False), (0, 0, 1, False), (0, 0, 1, False)]
    i4 = [C.c_int(7) for _ in range(4)]
    refused = [
        lambda: h.set_window(-1, 8, 2), lambda: h.set_window(4, 8, 2),  # a bad index
        lambda: h.set_window(3, 8, 2),  # never reset
        lambda: h.set_window(0, 8, 2), lambda: h.set_window(0, 0, 0),  # a stream with rows
        lambda: h.set_window(2, -1, 0), lambda: h.set_window(2, 8, -1), lambda: h.set_window(2, 8, 8), lambda: h.set_window(2, 8, 9),
        lambda: h.set_window(2, 1, 1), lambda: h.set_window(2, 8, 2, 0), lambda: h.set_window(2, 8, 2, 65), lambda: h.set_window(2, 8, 2, -1),
        lambda: w._check(L.wc_align_stream_set_window(h._h, 2, 8, 2, 1, 2)), lambda: w._check(L.wc_align_stream_set_window(h._h, 2, 8, 2, 1, 3)),
        lambda: w._check(L.wc_align_stream_set_window(h._h, 2, 8, 2, 1, -1)),
        lambda: h.set_window(2, 0, 0, 1, monotone=True),  # the monotone flag without a window
        lambda: h.get_window(-1), lambda: h.get_window(4),
        lambda: w._check(L.wc_align_stream_get_window(h._h, 0, None, C.byref(i4[1]), C.byref(i4[2]), C.byref(i4[3]))),
        lambda: w._check(L.wc_align_stream_get_window(h._h, 0, C.byref(i4[0]), C.byref(i4[1]), C.byref(i4[2]), None)),
    ]
    for k, call in enumerate(refused):
        with pytest.raises(w.WorldClassError):
            call()
        assert [h.get_window(u) for u in range(4)] == ok and [h.rows_received(u) for u in range(4)] == [3, 0, 0, 0], k
    assert [x.value for x in i4] == [7] * 4
    rest = h.push([VOICE[3:16], VOICE[:16], VOICE[:16], None])
    want = awr.follow(VOICE[:16], TRACK[:130], 1, DIMS, False, 17, 5, 8, True)
    _same((np.concatenate([first[0], rest[0][0]]), np.concatenate([first[1], rest[0][1]])), want)
    plain = asr.follow(VOICE[:16], TRACK[:130], 1, DIMS)
    _same(rest[1], plain, "set_window(0)")
    _same(rest[2], plain, "refused throughout")
    h.reset(0, 0)  # a reset removes the window
    assert h.get_window(0) == (0, 0, 1, False)
    _same(h.push([VOICE[:16], None, None, None])[0], plain, "after the reset")
    h.close()


def test_a_followable_voice_on_the_device(env):
    """case 3 of tests/test_align_window_rule.py's hundred (dims 8, every coefficient compared) under each of its five windows: the
    unwindowed stream's positions and costs bit for bit, from the same handle's unwindowed stream as well"""
    w, wio, stream = env
    voice, track, want = awr.followable(3)
    wins = [(48, 16, 1), (48, 16, 8), (64, 16, 16), (32, 8, 8), (24, 8, 1)]
    h = stream.AlignStream(8, len(wins) + 1, 1, 300, 64, dim_begin=0)
    h.set_track(0, track)
    h.reset(0, 0)
    for u, (width, back, hop) in enumerate(wins):
        h.reset(u + 1, 0)
        h.set_window(u + 1, width, back, hop, monotone=u % 2 == 1)
    got = _run_all(h, voice, [64, 64, 22])
    for u in range(len(wins) + 1):
        _same(got[u], want, u)
    h.close()
