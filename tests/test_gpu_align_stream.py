"""-m gpu: alignment streams (wc_align_stream_*) against the plain restatement of their rule (tests/align_stream_rule.py), bit for
bit (NaN equal to NaN), and once against the device's own wc_align_features_ex_device run as one batch of all prefixes of a voice:
track lengths around the eight-cell rounds, push sizes around the 64-row passes, the same rows cut three ways, several streams on
several tracks in one push, both flags with a phrase that stands twice in the track, poisoned state rows and local costs, a NaN
row, a replaced track, two coefficient windows and every refusal."""
import numpy as np
import pytest

import align_stream_rule as asr

pytestmark = pytest.mark.gpu
DIMS = 60
SENT = -12345.5
_refs = {}


@pytest.fixture(scope="module")
def env():
    import world_class_amd as w
    from world_class_amd import io as wio, stream
    w.lib().wc_set_device(0)
    return w, wio, stream


def _rows(n, seed, dims=DIMS):
    return np.random.default_rng(seed).standard_normal((n, dims))


VOICE = _rows(130, 30100)  # the live voice of most tests: made once and left unchanged
TRACK = _rows(130, 30101)


def _ref(name, a, b, window, open_begin):
    """the rule's (position, cost) for all rows of a on the track b: computed once per name (the rule does not depend on the pushes,
    tests/test_align_stream_rule.py)"""
    key = (name, window, bool(open_begin))
    if key not in _refs:
        _refs[key] = asr.follow(a, b, window[0], window[1], open_begin)
    return _refs[key]


def _same(got, want, what=None):
    assert np.array_equal(got[0], want[0], equal_nan=True), (what, "position", got[0], want[0])
    assert np.array_equal(got[1], want[1], equal_nan=True), (what, "cost", got[1], want[1])
    finite = ~np.isnan(want[1])
    assert np.array_equal(np.asarray(got[1])[finite].view(np.uint64), np.asarray(want[1])[finite].view(np.uint64)), what


def _run(h, stream, a, cuts):
    """rows of a through one stream of the handle in pushes of the sizes in cuts (the other streams idle)"""
    pos, cost, o = [], [], 0
    for c in cuts:
        rows = [None] * h.n_streams
        rows[stream] = a[o:o + c]
        p, q = h.push(rows)[stream]
        assert len(p) == c and len(q) == c
        pos.append(p)
        cost.append(q)
        o += c
    assert o == len(a)
    return np.concatenate(pos), np.concatenate(cost)


def _cuts(n, k):
    return [k] * (n // k) + ([n % k] if n % k else [])


@pytest.mark.parametrize("m", [1, 2, 7, 8, 9, 17, 64, 65, 130])
def test_track_lengths(env, m):
    """70 rows in one push (a full pass and a pass of 6) on tracks around the eight-cell rounds, under both flags"""
    w, wio, stream = env
    h = stream.AlignStream(DIMS, 2, 1, 130, 130)
    h.set_track(0, TRACK[:m])
    assert h.track_length(0) == m
    h.reset(0, 0)
    h.reset(1, 0, open_begin=True)
    got = h.push([VOICE[:70], VOICE[:70]])
    for u in (0, 1):
        _same(got[u], _ref("v70_t%d" % m, VOICE[:70], TRACK[:m], (1, DIMS), u == 1), (m, u))
        assert h.rows_received(u) == 70
    assert not np.isnan(got[0][0]).any() and np.isfinite(got[0][1]).all()
    h.close()


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 130])
def test_push_sizes(env, k):
    """130 rows in pushes of k against max_rows_per_push = 130: one pass, a full pass, a pass plus one row, three passes"""
    w, wio, stream = env
    h = stream.AlignStream(DIMS, 2, 1, 65, 130)
    h.set_track(0, TRACK[:65])
    for u in (0, 1):
        h.reset(u, 0, open_begin=u == 1)
        _same(_run(h, u, VOICE, _cuts(130, k)), _ref("v130_t65", VOICE, TRACK[:65], (1, DIMS), u == 1), (k, u))
        assert h.rows_received(u) == 130
    h.close()


def test_split_invariance_and_state_parity(env):
    """the same 130 rows as 130 x 1 (130 passes), as (64, 1, 65) (four passes) and as one push (three passes: the parity of the
    state rows flips), then again as (64, 1, 65) and as 130 x 1 from the flipped parity, on one stream with a reset in between: all
    give the rule's bits"""
    w, wio, stream = env
    h = stream.AlignStream(DIMS, 1, 1, 130, 130)
    h.set_track(0, TRACK)
    want = _ref("v130_t130", VOICE, TRACK, (1, DIMS), False)
    outs = []
    for cuts in ([1] * 130, [64, 1, 65], [130], [64, 1, 65], [1] * 130):
        h.reset(0, 0)
        outs.append(_run(h, 0, VOICE, cuts))
        _same(outs[-1], want, cuts[:3])
    for o in outs[1:]:
        assert o[0].tobytes() == outs[0][0].tobytes() and o[1].tobytes() == outs[0][1].tobytes()
    h.close()


def _several(env, counts_of_others):
    """five streams on three tracks of 130, 9 and 64 rows, pushed through the device form into sentinel-filled outputs.  Stream 0
    always takes (3, 0, 64, 1, 0, 62) rows; the others take what counts_of_others(u, round) says.  Returns per stream (position,
    cost) over all its rows and the rows it took"""
    w, wio, stream = env
    tracks = [TRACK, TRACK[40:49], TRACK[60:124]]
    attach = [(0, False), (1, True), (0, True), (2, False), (0, False)]
    voices = [VOICE, VOICE[::-1].copy(), VOICE[5:], VOICE[17:], VOICE]
    h = stream.AlignStream(DIMS, 5, 3, 130, 64)
    for t, b in enumerate(tracks):
        h.set_track(t, b)
    for u, (t, ob) in enumerate(attach):
        h.reset(u, t, open_begin=ob)
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
    for u, (t, ob) in enumerate(attach):
        got = (np.concatenate(res[u][0]), np.concatenate(res[u][1]))
        _same(got, asr.follow(voices[u][:taken[u]], tracks[t], 1, DIMS, ob), u)
        out.append(got)
    return out, taken


def test_several_streams_in_one_push_and_their_independence(env):
    pattern = {1: (64, 0, 1, 0, 2, 63), 2: (0, 64, 64, 0, 0, 0), 3: (7, 7, 0, 64, 35, 0), 4: (1, 1, 1, 1, 1, 1)}
    a, taken_a = _several(env, lambda u, r: pattern[u][r])
    b, taken_b = _several(env, lambda u, r: pattern[5 - u][(r + 1) % 6])
    assert taken_a[0] == taken_b[0] == 130 and taken_a[1:] != taken_b[1:]
    assert a[0][0].tobytes() == b[0][0].tobytes() and a[0][1].tobytes() == b[0][1].tobytes()


@pytest.mark.parametrize("second", [50 + 3 * 64, 200])
def test_a_phrase_that_stands_twice_in_the_track(env, second):
    """a 40-row phrase at column 50 and again 3 * 64 columns further / at column 200 (a lower j % 64): pushed under an open
    beginning, both copies cost exactly 0.0 at every row, and the lower column must win"""
    w, wio, stream = env
    assert second % 64 <= 50 % 64 and second > 90
    phrase, track = _rows(40, 30102), _rows(300, 30103)
    track[50:90] = phrase
    track[second:second + 40] = phrase
    h = stream.AlignStream(DIMS, 2, 1, 300, 40)
    h.set_track(0, track)
    h.reset(0, 0, open_begin=True)
    h.reset(1, 0)
    for cuts in ([40], [13, 27]):
        got = _run(h, 0, phrase, cuts)
        assert (got[1] == 0.0).all() and got[0].tolist() == [50.0 + i for i in range(40)]
        _same(got, _ref("phrase%d" % second, phrase, track, (1, DIMS), True))
        h.reset(0, 0, open_begin=True)
    _same(_run(h, 1, phrase, [40]), _ref("phrase%d" % second, phrase, track, (1, DIMS), False))
    h.close()


def test_stale_state_rows_and_local_costs_never_show(env):
    """before every comparison the same streams take 130 rows of NaN (three passes: both state rows and all of d are NaN, and
    so is every result); then they are reset and pushed for real"""
    w, wio, stream = env
    h = stream.AlignStream(DIMS, 2, 1, 130, 130)
    h.set_track(0, TRACK)
    for u in (0, 1):
        h.reset(u, 0, open_begin=u == 1)
    poison = np.full((130, DIMS), np.nan)
    for m, cuts in ((130, [130]), (65, [64, 6]), (9, [1, 2]), (130, [1] * 5 + [65])):
        h.set_track(0, TRACK[:m])
        for p, c in h.push([poison, poison]):
            assert np.isnan(p).all() and np.isnan(c).all() and len(p) == 130
        for u in (0, 1):
            h.reset(u, 0, open_begin=u == 1)
        n = sum(cuts)
        for u in (0, 1):
            _same(_run(h, u, VOICE[:n], cuts), asr.follow(VOICE[:n], TRACK[:m], 1, DIMS, u == 1), (m, cuts, u))
        for u in (0, 1):
            h.reset(u, 0, open_begin=u == 1)
    h.close()


def test_a_nan_row_in_the_middle_of_a_voice(env):
    """no cell wins in or behind a NaN row: the position is NaN from there on; the cost is NaN at the row and, by the rule's
    comparisons, +inf behind it"""
    w, wio, stream = env
    voice = VOICE[:100].copy()
    voice[37, 20] = np.nan
    h = stream.AlignStream(DIMS, 2, 1, 65, 64)
    h.set_track(0, TRACK[:65])
    for u in (0, 1):
        h.reset(u, 0, open_begin=u == 1)
        got = _run(h, u, voice, [30, 30, 40])
        _same(got, asr.follow(voice, TRACK[:65], 1, DIMS, u == 1), u)
        assert not np.isnan(got[0][:37]).any() and np.isnan(got[0][37:]).all()
        assert np.isnan(got[1][37]) and (got[1][38:] == np.inf).all()
    h.close()


def test_track_replacement(env):
    w, wio, stream = env
    h = stream.AlignStream(DIMS, 2, 2, 130, 16)
    h.set_track(0, TRACK[:50])
    h.reset(0, 0)
    h.reset(1, 0, open_begin=True)
    _same(_run(h, 0, VOICE[:10], [10]), asr.follow(VOICE[:10], TRACK[:50], 1, DIMS))
    with pytest.raises(w.WorldClassError):  # stream 0 has rows on the slot
        h.set_track(0, TRACK[50:])
    assert h.track_length(0) == 50 and h.rows_received(0) == 10
    _same(_run(h, 0, VOICE[10:14], [4]), tuple(x[10:] for x in asr.follow(VOICE[:14], TRACK[:50], 1, DIMS)))
    h.reset(0, 0)
    h.set_track(0, TRACK[50:])  # (stream 1 is attached without rows: it follows the new track)
    assert h.track_length(0) == 80
    _same(_run(h, 0, VOICE[:16], [16]), asr.follow(VOICE[:16], TRACK[50:], 1, DIMS))
    _same(_run(h, 1, VOICE[:16], [16]), asr.follow(VOICE[:16], TRACK[50:], 1, DIMS, True))
    h.close()


@pytest.mark.parametrize("dims,window", [(60, (1, 60)), (40, (0, 33))])
def test_coefficient_windows(env, dims, window):
    w, wio, stream = env
    a, b = _rows(70, 30104, dims), _rows(33, 30105, dims)
    a[:, window[1]:], b[:, window[1]:] = np.nan, np.nan
    if window[0]:
        a[:, :window[0]], b[:, :window[0]] = np.nan, np.nan
    h = stream.AlignStream(dims, 1, 1, 33, 70, dim_begin=window[0], dim_end=window[1])
    h.set_track(0, b)
    h.reset(0, 0)
    got = _run(h, 0, a, [70])
    _same(got, asr.follow(a, b, window[0], window[1]))
    assert np.isfinite(got[1]).all()
    h.close()


def test_the_devices_own_whole_call_on_every_prefix(env):
    """all 70 prefixes of a voice against a 130-row track as ONE batch of wc_align_features_ex_device (pattern 0, band 0, open end):
    d_cost bit for bit, d_position = span[1]"""
    w, wio, stream = env
    n, m = 70, 130
    a_lens, b_lens = list(range(1, n + 1)), [m] * n
    d_a = w.DeviceArray.from_host(np.concatenate([VOICE[:i] for i in a_lens]))
    d_b = w.DeviceArray.from_host(np.concatenate([TRACK] * n))
    h = stream.AlignStream(DIMS, 1, 1, m, n)
    h.set_track(0, TRACK)
    for open_begin in (False, True):
        d_cost, d_len, d_span = w.DeviceArray(n), w.DeviceArray(n, np.int32), w.DeviceArray(2 * n, np.int32)
        wio.align_features_ex_device(a_lens, d_a, b_lens, d_b, DIMS, 1, DIMS, 0, 0, (1 if open_begin else 0) | 2, d_cost, d_len, d_span=d_span)
        w.lib().wc_synchronize()
        cost, span = d_cost.to_host(), d_span.to_host().reshape(n, 2)
        h.reset(0, 0, open_begin=open_begin)
        pos, got = _run(h, 0, VOICE[:n], [n])
        assert np.isfinite(cost).all() and got.tobytes() == cost.tobytes()
        assert np.array_equal(pos, span[:, 1].astype(np.float64))
        for x in (d_cost, d_len, d_span):
            x.free()
    d_a.free()
    d_b.free()
    h.close()


def test_refusals_leave_every_stream_as_it_was(env):
    w, wio, stream = env
    L = stream._lib()
    for bad in ((0, 0, 1, 1, 1, 4, 4), (4, -1, 4, 1, 1, 4, 4), (4, 0, 5, 1, 1, 4, 4), (4, 2, 2, 1, 1, 4, 4), (4, 3, 2, 1, 1, 4, 4),
                (4, 0, 4, 0, 1, 4, 4), (4, 0, 4, 1, 0, 4, 4), (4, 0, 4, 1, 1, 0, 4), (4, 0, 4, 1, 1, 4, 0),
                (4, 0, 4, 512, 1, 1 << 10, 1 << 10), (4, 0, 4, 1 << 20, 1, 1 << 20, 1 << 20)):
        assert not L.wc_align_stream_create(*bad), bad
    a, b = _rows(8, 30106, 4), _rows(20, 30107, 4)
    h = stream.AlignStream(4, 3, 2, 20, 8, dim_begin=0)
    assert [h.track_length(t) for t in (-1, 0, 1, 2)] == [-1, 0, 0, -1]
    assert [h.rows_received(u) for u in (-1, 0, 3)] == [-1, 0, -1]
    with pytest.raises(w.WorldClassError):  # a stream that was never reset takes no rows
        h.push([a[:1], None, None])
    with pytest.raises(w.WorldClassError):  # an empty slot
        h.reset(0, 0)
    h.set_track(0, b)
    h.reset(0, 0)
    h.reset(1, 0, open_begin=True)
    first = h.push([a[:3], None, None])[0]
    d_a, d_p, d_c = (w.DeviceArray.from_host(x) for x in (a, np.full(24, SENT), np.full(24, SENT)))
    refused = [
        lambda: h.push_device([-1, 0, 0], d_a, d_p, d_c),
        lambda: h.push_device([1, 9, 0], d_a, d_p, d_c),
        lambda: h.push_device([1, 1, 1], d_a, d_p, d_c),  # stream 2 is not attached
        lambda: h.push_device([1, 0, 0], None, d_p, d_c),
        lambda: h.push_device([1, 0, 0], d_a, None, d_c),
        lambda: h.push_device([1, 0, 0], d_a, d_p, None),
        lambda: h.reset(3, 0), lambda: h.reset(-1, 0), lambda: h.reset(0, 2), lambda: h.reset(0, -1),
        lambda: h.reset(0, 1),  # track 1 is empty
        lambda: w._check(L.wc_align_stream_reset(h._h, 0, 0, 2)), lambda: w._check(L.wc_align_stream_reset(h._h, 0, 0, 3)),
        lambda: w._check(L.wc_align_stream_reset(h._h, 0, 0, -1)),
        lambda: h.set_track_device(0, 0, d_a), lambda: h.set_track_device(1, 21, d_a), lambda: h.set_track_device(2, 4, d_a),
        lambda: h.set_track_device(-1, 4, d_a), lambda: h.set_track_device(1, 4, None),
        lambda: h.set_track_device(0, 4, d_a),  # stream 0 has rows on the slot
    ]
    for k, call in enumerate(refused):
        with pytest.raises(w.WorldClassError):
            call()
        assert [h.rows_received(u) for u in range(3)] == [3, 0, 0] and [h.track_length(t) for t in (0, 1)] == [20, 0], k
    with pytest.raises(ValueError):
        h.push_device([1, 0], d_a, d_p, d_c)
    h.push_device([0, 0, 0], None, None, None)  # nothing to read or write
    assert (d_p.to_host() == SENT).all() and (d_c.to_host() == SENT).all()
    for x in (d_a, d_p, d_c):
        x.free()
    rest = h.push([a[3:], a[:2], None])
    want = asr.follow(a, b, 0, 4)
    _same((np.concatenate([first[0], rest[0][0]]), np.concatenate([first[1], rest[0][1]])), want)
    _same(rest[1], asr.follow(a[:2], b, 0, 4, True))
    assert [h.rows_received(u) for u in range(3)] == [8, 2, 0]
    h.close()
