"""-m gpu: filter streams (include/world_class_filter_stream.h) against the batch call wc_frame_filter_run_device, bit for bit.  Seven
streams of 0 to about 3000 samples whose lengths lie on, one before and one behind a centre, with exact, held and surplus rows, at
settings that run all four segment-kernel forms, hop 1, hop 1.5, the tie hop and the largest hop, both kinds, under six kinds of cut.
Then a NaN row beside a border, a stream alone against the same stream among six others, reuse after a reset, windows filled to their
capacity exactly, every refusal with a following push that proves nothing moved, two host threads on two handles, and the block form
of the segment kernels against the wavefront form within filter_rule.K units.

A case packs every push's samples and rows into one upload each and reads the outputs of all pushes back with one copy."""
import os
import threading
from ctypes import c_double as C_double, c_int as C_int

import numpy as np
import pytest

import filter_rule as fr
import filter_stream_rule as fsr

pytestmark = pytest.mark.gpu

# (fs, fft_size, frame_period_ms, streams, longest): the block kernel at 512, the wavefront kernels at 1024 and 2048, the block kernel
# at 4096 (two streams); hop 1, where the tail is N deep; hop 1.5; the tie hop; the largest hop
SETTINGS = [(8000, 512, 5.0, 7, 3001), (16000, 1024, 5.0, 7, 3001), (48000, 2048, 5.0, 7, 3001), (96000, 4096, 5.0, 2, 3001),
            (8000, 512, 0.125, 7, 1500), (8000, 512, 0.1875, 7, 1500), (22050, 1024, 64.5 / 22.05, 7, 3001), (48000, 2048, 512 / 48.0, 7, 3001)]
IDS = ["512", "1024", "2048", "4096x2", "hop1", "hop1.5", "ties", "hop512"]
GUARD = 7.25
KIND_NAME = {fr.POWER: "power", fr.LOG: "log"}
_HANDLES, _CASES = {}, {}


@pytest.fixture(scope="module")
def env():
    import torch
    import world_class_amd as w
    from world_class_amd import filter as ff, filter_stream as fs_
    w.lib().wc_set_device(0)
    yield w, ff, torch, fs_
    for h in _HANDLES.values():
        h.close()
    _HANDLES.clear()
    _CASES.clear()


def batch_handle(env, fs, N, fp, block=False):
    key = ("batch", fs, N, fp, block)
    if key not in _HANDLES:
        if block:
            os.environ["WC_FILTER_KERNEL"] = "block"    # (read when the handle is created)
        try:
            _HANDLES[key] = env[1].FrameFilter(fs, N, fp)
        finally:
            os.environ.pop("WC_FILTER_KERNEL", None)
    return _HANDLES[key]


def stream_handle(env, fs, N, fp, kind, U, cap_s, cap_r, block=False, tag=0):
    key = ("stream", fs, N, fp, kind, U, cap_s, cap_r, block, tag)
    if key not in _HANDLES:
        if block:
            os.environ["WC_FILTER_KERNEL"] = "block"
        try:
            _HANDLES[key] = env[3].FilterStream(fs, N, fp, KIND_NAME[kind], U, cap_s, cap_r)
        finally:
            os.environ.pop("WC_FILTER_KERNEL", None)
    h = _HANDLES[key]
    for u in range(U):
        h.reset(u)
    return h


def up(env, a):
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    return env[2].from_numpy(a.copy() if a.size else np.zeros(1)).cuda()


def whole_call(env, fs, N, fp, kind, xs, rows, block=False):
    """the batch through wc_frame_filter_run_device -> the list of outputs"""
    h = batch_handle(env, fs, N, fp, block)
    lengths, f_lengths = [len(x) for x in xs], [len(r) for r in rows]
    d_x, d_rows = up(env, np.concatenate(xs)), up(env, np.concatenate([r.reshape(len(r), N // 2 + 1) for r in rows]))
    d_y = up(env, np.full(sum(lengths) + 8, GUARD))
    h.run(d_x, lengths, d_rows, f_lengths, d_y, KIND_NAME[kind])
    assert env[0].lib().wc_synchronize() == 0
    y = d_y.cpu().numpy()
    assert np.all(y[sum(lengths):] == GUARD)
    return [y[e - n:e].copy() for n, e in zip(lengths, np.cumsum(lengths))]


def lengths_of(fs, fp, U, longest):
    """0 to `longest` samples: n - 1 on a centre, one before it, one behind it; nothing; one sample; the longest; a few hops"""
    c, h = fr.centre(5, fp, fs), fr.hop(fp, fs)
    return ([c + 1, c, c + 2, 0, 1, longest, int(2.5 * h) + 2] if U == 7 else [longest, c + 1])[:U]


def case(env, setting, kind, nan=False):
    """(xs, rows, the whole call's outputs), once per setting and kind: rows exact, held (two), surplus, ... in turn"""
    key = (setting, kind, nan)
    if key not in _CASES:
        fs, N, fp, U, longest = setting
        rng = np.random.default_rng(900 + N + int(fp * 64))
        xs = [rng.normal(size=n) for n in lengths_of(fs, fp, U, longest)]
        rows = []
        for u, x in enumerate(xs):
            S = fr.segments(len(x), fp, fs)
            mode = fr.ROW_MODES[u % 3] if S else "surplus"
            rows.append(fr.mode_rows(("noise", "envelope")[u % 2], mode, S, N, kind, seed=u))
        if nan:
            rows[0][2, 3] = np.nan      # (stream 0 has a row per segment)
        _CASES[key] = (xs, rows, whole_call(env, fs, N, fp, kind, xs, rows))
    return _CASES[key]


def drive(env, st, xs, rows, schedules, extra=None):
    """the pushes schedules[u] = [(n_samples, n_rows, flush)] in lockstep (a stream whose schedule has ended is idle) -> the
    concatenated outputs per stream.  extra(st, p): called in front of push p (the refusal tests)"""
    U, width = len(xs), st.width
    P = max(len(s) for s in schedules)
    pos_x, pos_r, calls, x_parts, r_parts = [0] * U, [0] * U, [], [], []
    x_off = r_off = 0
    for p in range(P):
        ns, nr, fl = [0] * U, [0] * U, [0] * U
        for u in range(U):
            if p < len(schedules[u]):
                ns[u], nr[u], fl[u] = schedules[u][p]
                x_parts.append(xs[u][pos_x[u]:pos_x[u] + ns[u]])
                r_parts.append(rows[u][pos_r[u]:pos_r[u] + nr[u]].reshape(-1))
                pos_x[u] += ns[u]
                pos_r[u] += nr[u]
        calls.append((ns, nr, fl, x_off, r_off))
        x_off, r_off = x_off + sum(ns), r_off + sum(nr)
    assert pos_x == [len(x) for x in xs] and pos_r == [len(r) for r in rows]
    total = sum(pos_x)
    d_x, d_r = up(env, np.concatenate(x_parts + [np.zeros(1)])), up(env, np.concatenate(r_parts + [np.zeros(1)]))
    d_y = up(env, np.full(total + 8, GUARD))
    px, pr, py = d_x.data_ptr(), d_r.data_ptr(), d_y.data_ptr()
    yo, where = 0, [[] for _ in range(U)]
    for p, (ns, nr, fl, xo, ro) in enumerate(calls):
        if extra:
            extra(st, p)
        got = st.push(ns, px + 8 * xo, nr, pr + 8 * ro * width, py + 8 * yo, fl)
        for u in range(U):
            where[u].append((yo, got[u]))
            yo += got[u]
    assert env[0].lib().wc_synchronize() == 0
    y = d_y.cpu().numpy()
    assert yo == total and np.all(y[total:] == GUARD)
    return [np.concatenate([y[o:o + k] for o, k in w] + [np.zeros(0)]) for w in where]


def schedules_of(how, xs, rows, fp, fs, idle=False):
    out = []
    for u, (x, r) in enumerate(zip(xs, rows)):
        s = fsr.cut(how, len(x), len(r), fp, fs, seed=u)
        if idle:      # the stream sits out pushes here and there
            rng = np.random.default_rng(70 + u)
            s = [q for push in s for q in ([(0, 0, 0)] * int(rng.integers(0, 3)) + [push])]
        out.append(s)
    return out


def same_bits(got, want):
    for u, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, (u, g.shape, w.shape)
        assert np.array_equal(g, w, equal_nan=True), (u, int((g != w).sum()), float(np.nanmax(np.abs(g - w))))


@pytest.mark.parametrize("how", fsr.CUTS)
@pytest.mark.parametrize("kind", (fr.POWER, fr.LOG))
@pytest.mark.parametrize("setting", SETTINGS, ids=IDS)
def test_every_cut_is_the_whole_call_bit_for_bit(env, setting, kind, how):
    fs, N, fp, U, longest = setting
    xs, rows, want = case(env, setting, kind)
    st = stream_handle(env, fs, N, fp, kind, U, max(longest, fsr.min_pending_samples(fp, fs)), max(len(r) for r in rows))
    got = drive(env, st, xs, rows, schedules_of(how, xs, rows, fp, fs, idle=how == "random"))
    same_bits(got, want)
    for u, x in enumerate(xs):
        assert st.samples_received(u) == st.samples_committed(u) == len(x) and st.rows_received(u) == len(rows[u])
        assert st.segments_done(u) == fr.segments(len(x), fp, fs) and st.pending_samples(u) == 0 and st.pending_rows(u) == 0


@pytest.mark.parametrize("how", ("one_sample", "hop_and_row", "random"))
@pytest.mark.parametrize("setting", (SETTINGS[1], SETTINGS[4]), ids=("1024", "hop1"))
def test_a_nan_row_beside_a_border(env, setting, how):
    fs, N, fp, U, longest = setting
    xs, rows, want = case(env, setting, fr.LOG, nan=True)
    a2, n0 = fr.span(2, len(xs[0]), fp, fs)[0], len(xs[0])
    assert np.array_equal(np.isnan(want[0]), (np.arange(n0) >= a2) & (np.arange(n0) < a2 + N)) and np.isnan(want[0]).any()
    st = stream_handle(env, fs, N, fp, fr.LOG, U, longest, max(len(r) for r in rows))
    same_bits(drive(env, st, xs, rows, schedules_of(how, xs, rows, fp, fs)), want)


@pytest.mark.parametrize("setting", (SETTINGS[0], SETTINGS[2]), ids=("512", "2048"))
def test_a_stream_alone_and_among_six_others_and_after_a_reset(env, setting):
    fs, N, fp, U, longest = setting
    xs, rows, want = case(env, setting, fr.POWER)
    cap_s, cap_r = max(longest, fsr.min_pending_samples(fp, fs)), max(len(r) for r in rows)
    among = drive(env, stream_handle(env, fs, N, fp, fr.POWER, U, cap_s, cap_r), xs, rows, schedules_of("random", xs, rows, fp, fs))
    one = stream_handle(env, fs, N, fp, fr.POWER, 1, cap_s, cap_r)
    sched = fsr.cut("random", len(xs[5]), len(rows[5]), fp, fs, seed=5)
    alone = drive(env, one, [xs[5]], [rows[5]], [sched])
    same_bits(alone, [among[5]])
    same_bits(alone, [want[5]])
    # the handle again, in mid-stream: part of another signal, a reset, and the stream is a fresh one
    part = int(2.5 * fr.hop(fp, fs))
    one.reset(0)
    assert len(one.push_host([xs[2][::-1][:part]], [rows[2][:2]])[0]) > 0 and one.segments_done(0) > 0
    one.reset(0)
    assert (one.samples_received(0), one.rows_received(0), one.segments_done(0), one.samples_committed(0)) == (0, 0, 0, 0)
    same_bits(drive(env, one, [xs[5]], [rows[5]], [fsr.cut("hop_and_row", len(xs[5]), len(rows[5]), fp, fs)]), [want[5]])
    with pytest.raises(env[0].WorldClassError, match="has ended"):
        one.push_host([xs[5][:1]], [None])


@pytest.mark.parametrize("setting", (SETTINGS[0], SETTINGS[4], SETTINGS[6]), ids=("512", "hop1", "ties"))
def test_windows_filled_to_their_capacity_exactly(env, setting):
    """the least capacities create takes: samples until the window is full (a further sample is refused), then a row, and so on"""
    fs, N, fp, _, _ = setting
    cap_s = fsr.min_pending_samples(fp, fs)
    n = int(6.3 * fr.hop(fp, fs)) + 3
    x = np.random.default_rng(5).normal(size=n)
    S = fr.segments(n, fp, fs)
    rows = fr.mode_rows("envelope", "exact", S, N, fr.POWER, seed=1)
    c, sched, full = fsr.Counts(fs, fp, cap_s, 1), [], 0
    i = j = 0
    while i < n or (c.pending_rows == 0 and j < S):
        ns = min(cap_s - c.pending_samples, n - i)
        nr = 1 - c.pending_rows if ns == 0 else 0
        assert ns or nr
        c.step(ns, nr, 0)
        full += c.pending_samples == cap_s
        sched.append((ns, nr, 0))
        i, j = i + ns, j + nr
    rows = rows[:j]      # what one pending row lets in: the flush holds the last of them, as the whole call does
    want = whole_call(env, fs, N, fp, fr.POWER, [x], [rows])
    assert full >= 3
    st = stream_handle(env, fs, N, fp, fr.POWER, 1, cap_s, 1)

    def one_too_many(st, p):
        if st.pending_samples(0) == cap_s:
            with pytest.raises(env[0].WorldClassError, match="does not fit the windows"):
                st.push([1], None, [0], None, None)
    same_bits(drive(env, st, [x], [rows], [sched + [(0, 0, 1)]], extra=one_too_many), want)


def test_every_refusal_and_nothing_moves(env):
    w, _, torch, fs_ = env
    fs, N, fp = 16000, 1024, 5.0
    err = w.WorldClassError
    for args, text in (((fs, 1000, fp, "power", 1, 160, 1), "fft_size"), ((0, N, fp, "power", 1, 160, 1), "fs must be positive"),
                       ((fs, N, 0.01, "power", 1, 160, 1), "hop"), ((fs, N, 16.0625, "power", 1, 600, 1), "longest segment"),
                       ((fs, N, fp, "power", 0, 160, 1), "n_streams"), ((fs, N, fp, "power", 1, 159, 1), "max_pending_samples"),
                       ((fs, N, fp, "power", 1, 160, 0), "max_pending_rows"), ((fs, N, fp, "power", 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), "63 bits")):
        with pytest.raises(err, match=text):
            fs_.FilterStream(*args)
    assert not w.lib().wc_filter_stream_create(fs, N, C_double(fp), 2, 1, 160, 1) and "kind" in w.last_error()
    xs, rows, want = case(env, SETTINGS[1], fr.POWER)
    x, r = [xs[5], xs[0]], [rows[5], rows[0]]
    st = stream_handle(env, fs, N, fp, fr.POWER, 2, 400, 4)
    log = stream_handle(env, fs, N, fp, fr.LOG, 2, 400, 4)
    d = up(env, np.full(4096, GUARD))
    p = d.data_ptr()
    L = w.lib()
    out = (C_int * 2)()
    two = lambda a, b: (C_int * 2)(a, b)

    def refusals(st, push):
        h, state = st._h, [(st.samples_received(u), st.rows_received(u), st.segments_done(u), st.samples_committed(u)) for u in range(2)]
        for call, text in ((lambda: L.wc_filter_stream_push_device(None, two(0, 0), p, two(0, 0), p, None, p + 8192, out), "null handle"),
                           (lambda: L.wc_filter_stream_push_device(h, None, p, two(0, 0), p, None, p + 8192, out), "null n_samples"),
                           (lambda: L.wc_filter_stream_push_device(h, two(0, 0), p, None, p, None, p + 8192, out), "null n_samples"),
                           (lambda: L.wc_filter_stream_push_device(h, two(0, 0), p, two(0, 0), p, None, p + 8192, None), "null n_samples"),
                           (lambda: st.push([-1, 0], p, [0, 0], p, p + 8192), "negative count"),
                           (lambda: st.push([0, 0], p, [0, -2], p, p + 8192), "negative count"),
                           (lambda: st.push([401, 0], p, [0, 0], p, p + 8192), "does not fit the windows"),
                           (lambda: st.push([0, 0], p, [5, 0], p, p + 8192 * 3), "does not fit the windows"),
                           (lambda: st.push([1, 0], None, [0, 0], p, p + 8192), "null d_x"),
                           (lambda: st.push([0, 0], p, [1, 0], None, p + 8192), "null d_rows"),
                           (lambda: st.push([0, 0], None, [0, 0], None, None, [1, 1]), "null d_y") if push == 2 else (None, ""),
                           (lambda: st.push([100, 100], p, [1, 1], p + 8192, p + 8 * 199, [1, 1]), "d_y overlaps d_x") if push == 2 else (None, ""),
                           (lambda: st.push([100, 100], p, [1, 1], p + 8192, p + 8192 + 8 * 1025, [1, 1]), "d_y overlaps d_rows") if push == 2 else (None, ""),
                           (lambda: st.push_coded([0, 0], p, [0, 0], p, None, 0, p + 8192), "number_of_dimensions"),
                           (lambda: st.push_coded([0, 0], p, [0, 0], p, None, N // 2 + 1, p + 8192), "number_of_dimensions"),
                           (lambda: st.push_coded([0, 0], p, [1, 0], None, None, 24, p + 8192), "null d_coded_to"),
                           (lambda: log.push_coded([0, 0], p, [0, 0], p, None, 24, p + 8192), "WC_FILTER_POWER")):
            if call is None:
                continue
            if text.startswith("null handle") or text == "null n_samples":
                assert call() == -1 and text in w.last_error()
            else:
                with pytest.raises(err, match=text):
                    call()
        assert state == [(st.samples_received(u), st.rows_received(u), st.segments_done(u), st.samples_committed(u)) for u in range(2)]

    # a fresh stream: samples flushed without a row
    with pytest.raises(err, match="without a row"):
        st.push([5, 0], p, [0, 0], p, p + 8192, [1, 0])
    assert st.push([0, 0], None, [0, 0], None, None, [0, 1]) == [0, 0]          # a flush with n == 0 writes nothing and ends the stream
    with pytest.raises(err, match="has ended"):
        st.push([0, 1], p, [0, 0], p, p + 8192)
    with pytest.raises(err, match="has ended"):
        st.push([0, 0], p, [0, 1], p, p + 8192)
    with pytest.raises(err, match="bad stream index"):
        st.reset(2)
    assert L.wc_filter_stream_samples_received(st._h, 2) == -1
    assert L.wc_filter_stream_pending_rows(st._h, -1) == -1 and L.wc_filter_stream_segments_done(0, C_double(5.0), 1, 1) == -1
    st.reset(1)
    sched = [fsr.cut("hop_and_row", len(a), len(b), fp, fs) for a, b in zip(x, r)]
    got = drive(env, st, x, r, sched, extra=lambda st, k: refusals(st, k) if k in (0, 2, 7) else None)
    same_bits(got, [want[5], want[0]])
    assert np.all(d.cpu().numpy() == GUARD)      # no refused push wrote anything


def test_the_counts_follow_the_rule(env):
    w, _, _, fs_ = env
    for fs, N, fp, _, _ in SETTINGS:
        h = fr.hop(fp, fs)
        for n in (0, 1, int(h), int(3.5 * h), 3001):
            for F in (0, 1, 3, 5000):
                T = fs_.segments_done(fs, fp, n, F)
                assert T == fsr.segments_done(n, F, fp, fs) and fs_.committed(fs, fp, T) == fsr.committed(T, fp, fs)


def test_two_host_threads_on_two_handles(env):
    fs, N, fp, U, longest = SETTINGS[1]
    xs, rows, want = case(env, SETTINGS[1], fr.POWER)
    cap_s, cap_r = longest, max(len(r) for r in rows)
    hs = [stream_handle(env, fs, N, fp, fr.POWER, U, cap_s, cap_r, tag=t) for t in (1, 2)]
    got, errors = [None, None], []

    def work(i):
        try:
            for _ in range(3):
                for u in range(U):
                    hs[i].reset(u)
                got[i] = drive(env, hs[i], xs, rows, schedules_of(("hop_and_row", "random")[i], xs, rows, fp, fs))
        except Exception as e:      # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    same_bits(got[0], want)
    same_bits(got[1], want)


@pytest.mark.parametrize("setting", (SETTINGS[1], SETTINGS[2]), ids=("1024", "2048"))
def test_the_block_form_against_the_wavefront_form(env, setting):
    """a stream under WC_FILTER_KERNEL=block is the batch under it, bit for bit, and lies within K units of the wavefront form: the
    bound the batch's two forms are held to"""
    fs, N, fp, U, longest = setting
    xs, rows, wave = case(env, setting, fr.LOG)
    block = whole_call(env, fs, N, fp, fr.LOG, xs, rows, block=True)
    st = stream_handle(env, fs, N, fp, fr.LOG, U, longest, max(len(r) for r in rows), block=True)
    got = drive(env, st, xs, rows, schedules_of("hop_and_row", xs, rows, fp, fs))
    same_bits(got, block)
    worst = 0.0
    for g, v, x, r in zip(got, wave, xs, rows):
        if len(x):
            worst = max(worst, float(np.abs(g - v).max() / fr.unit(x, r, fr.LOG, fs, N, fp)))
    print("block stream against wavefront batch at %d: %.4f u (K = %s)" % (N, worst, fr.K))
    assert worst <= fr.K

