"""-m gpu: the frame filter (include/world_class_filter.h) against tests/filter_rule.py within K * u -- every size, rate and period
setting on ragged batches whose lengths sit on, before and behind a centre, with one row, exact, short (held) and surplus rows of
both kinds, at the largest hop each size accepts -- and bit for bit where the header promises the same bits: two runs, every
utterance alone, in place, outside a changed row's span, in front of a cut, and the coded call against the two public calls.  The
block form under WC_FILTER_KERNEL=block against the wavefront form, every refusal behind guard values, two host threads on two
handles.  Every test prints its largest |device - rule| / u: fr.K was set from those figures."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import filter_rule as fr

pytestmark = pytest.mark.gpu

# (fs, fft_size, frame_period_ms): 512 at 8 kHz; 1024 at 16 kHz / 5 ms and 24 kHz / 1 ms (hop 24: 43 rows would lie over a sample, but
# batch() gives it 111 samples, six segments; tests/test_gpu_filter_long.py runs that depth and hop 1); 2048 at 44.1 kHz / 5 ms (a
# fractional hop) and 48 kHz; 4096 at 96 kHz
SETTINGS = [(8000, 512, 5.0), (16000, 1024, 5.0), (24000, 1024, 1.0), (44100, 2048, 5.0), (48000, 2048, 5.0), (96000, 4096, 5.0)]
# the largest hop each size accepts and one step beyond it
EDGES = [(8000, 512, 16.0, 16.125), (16000, 1024, 16.0, 16.0625), (48000, 2048, 512 / 48.0, 513 / 48.0), (96000, 4096, 1024 / 96.0, 1025 / 96.0)]
GUARD = 7.25
BOUND = fr.K
_WORST = {}


@pytest.fixture(scope="module")
def env():
    import torch
    import world_class_amd as w
    from world_class_amd import filter as ff
    w.lib().wc_set_device(0)
    yield w, ff, torch
    for h in _HANDLES.values():
        h.close()
    _HANDLES.clear()


_HANDLES = {}


def handle(env, fs, N, fp, block=False):
    key = (fs, N, fp, block)
    if key not in _HANDLES:
        if block:
            os.environ["WC_FILTER_KERNEL"] = "block"    # (read when the handle is created)
        try:
            _HANDLES[key] = env[1].FrameFilter(fs, N, fp)
        finally:
            os.environ.pop("WC_FILTER_KERNEL", None)
    return _HANDLES[key]


def up(env, a, dtype=np.float64):
    a = np.ascontiguousarray(a, dtype=dtype).ravel()
    return env[2].from_numpy(a.copy() if a.size else np.zeros(1, dtype=dtype)).cuda()


def device(env, h, xs, rows, kind, inplace=False):
    """the batch through wc_frame_filter_run_device -> the list of outputs"""
    w, _, torch = env
    lengths, f_lengths = [len(x) for x in xs], [len(r) for r in rows]
    d_x = up(env, np.concatenate(xs))
    d_rows = up(env, np.concatenate([np.asarray(r, dtype=np.float64).reshape(len(r), h.fft_size // 2 + 1) for r in rows]))
    d_y = d_x if inplace else up(env, np.full(sum(lengths) + 8, GUARD))
    h.run(d_x, lengths, d_rows, f_lengths, d_y, "power" if kind == fr.POWER else "log")
    assert w.lib().wc_synchronize() == 0
    y = d_y.cpu().numpy()
    if not inplace:
        assert np.all(y[sum(lengths):] == GUARD)    # nothing behind the last sample
    return [y[e - n:e].copy() for n, e in zip(lengths, np.cumsum(lengths))]


def held_to_rule(name, ys, xs, rows, kind, fs, N, fp):
    worst = 0.0
    for y, x, r in zip(ys, xs, rows):
        if not len(x):
            assert len(y) == 0
            continue
        want = fr.frame_filter(x, r, kind, fs, N, fp)
        u = fr.unit(x, r, kind, fs, N, fp)
        assert np.array_equal(np.isnan(y), np.isnan(want))
        ok = ~np.isnan(want)
        if ok.any() and u > 0:
            worst = max(worst, float(np.abs(y[ok] - want[ok]).max() / u))
    _WORST[name] = max(_WORST.get(name, 0.0), worst)
    print("%s: max |device - rule| / u = %.4f (overall %.4f, K = %s)" % (name, worst, max(_WORST.values()), fr.K))
    assert worst <= BOUND
    return worst


def batch(fs, N, fp, kind, seed):
    """a ragged batch of 7: one sample; n - 1 one before the third centre, on it, one behind it; an empty utterance; a few hops; and
    rows that are one, exact, short (held), surplus, none (the empty one), exact, short"""
    rng = np.random.default_rng(seed)
    c3, h = fr.centre(3, fp, fs), fr.hop(fp, fs)
    lengths = [1, c3, c3 + 1, c3 + 2, 0, int(4.6 * h) + 1, int(2.5 * h) + 2]
    xs = [rng.normal(size=n) for n in lengths]
    S = [fr.segments(n, fp, fs) for n in lengths]
    f_lengths = [1, S[1], 2, S[3] + 2, 0, S[5], 1]
    whats = ["noise", "envelope", "notch", "noise", "zeros", "envelope", "zeros"]
    rows = [fr.as_kind(fr.case_rows(wh, f, N, seed + i), kind) for i, (wh, f) in enumerate(zip(whats, f_lengths))]
    return xs, rows


@pytest.mark.parametrize("kind", (fr.POWER, fr.LOG))
@pytest.mark.parametrize("fs,N,fp", SETTINGS)
def test_ragged_batches_against_the_rule(env, fs, N, fp, kind):
    h = handle(env, fs, N, fp)
    xs, rows = batch(fs, N, fp, kind, 3 + kind)
    assert [h.segments(len(x)) for x in xs] == [fr.segments(len(x), fp, fs) for x in xs]
    ys = device(env, h, xs, rows, kind)
    held_to_rule("ragged %d/%d/%g kind %d" % (fs, N, fp, kind), ys, xs, rows, kind, fs, N, fp)
    # LOG rows of zeros: M is exactly 1, what is left is the two transforms of the segment
    if kind == fr.LOG:
        assert np.abs(ys[6] - xs[6]).max() < 64 * 2.0 ** -52 * np.abs(xs[6]).sum()


@pytest.mark.parametrize("fs,N,fp,beyond", EDGES)
def test_the_largest_hop_runs_and_one_step_beyond_is_refused(env, fs, N, fp, beyond):
    w, ff, _ = env
    assert fr.accepts(fs, N, fp) and not fr.accepts(fs, N, beyond)
    with pytest.raises(w.WorldClassError):
        ff.FrameFilter(fs, N, beyond)
    h = handle(env, fs, N, fp)
    rng = np.random.default_rng(N)
    n = fr.centre(2, fp, fs) + 3                       # four segments, the middle ones N / 2 - 1 samples long
    xs = [rng.normal(size=n), rng.normal(size=fr.centre(1, fp, fs))]
    assert max(fr.span(t, n, fp, fs)[2] for t in range(fr.segments(n, fp, fs))) == N // 2 - 1
    rows = [fr.as_kind(fr.case_rows("noise", 4, N, 1), fr.POWER), fr.as_kind(fr.case_rows("envelope", 1, N, 2), fr.POWER)]
    held_to_rule("largest hop %d" % N, device(env, h, xs, rows, fr.POWER), xs, rows, fr.POWER, fs, N, fp)


@pytest.mark.parametrize("fs,N,fp", SETTINGS)
def test_the_same_bits(env, fs, N, fp):
    """two runs of one call; every utterance alone against its place in the batch; in place against a separate output; outside the span
    of a changed row; in front of a cut"""
    h = handle(env, fs, N, fp)
    kind = fr.POWER
    xs, rows = batch(fs, N, fp, kind, 11)
    ys = device(env, h, xs, rows, kind)
    again = device(env, h, xs, rows, kind)
    assert all(np.array_equal(a, b) for a, b in zip(ys, again))
    for u in range(len(xs)):
        if len(xs[u]):
            alone, = device(env, h, [xs[u]], [rows[u]], kind)
            assert np.array_equal(alone, ys[u]), u
    inplace = device(env, h, xs, rows, kind, inplace=True)
    assert all(np.array_equal(a, b) for a, b in zip(ys, inplace))
    # one row changed: the same bits outside [a_t, a_t + N)
    u, t = 5, 2
    changed = [r.copy() for r in rows]
    changed[u][t] = fr.as_kind(fr.case_rows("notch", 1, N, 5), kind)[0]
    other = device(env, h, xs, changed, kind)
    a = fr.span(t, len(xs[u]), fp, fs)[0]
    outside = np.ones(len(xs[u]), dtype=bool)
    outside[a:a + N] = False
    assert np.array_equal(other[u][outside], ys[u][outside]) and not np.array_equal(other[u], ys[u])
    assert all(np.array_equal(other[v], ys[v]) for v in range(len(xs)) if v != u)
    # the utterance cut short: the first segment the cut changes is the one that holds sample n_cut (its span or its end moves)
    n_cut = fr.centre(2, fp, fs) + 2
    cut, = device(env, h, [xs[u][:n_cut]], [rows[u]], kind)
    first = min(t for t in range(fr.segments(len(xs[u]), fp, fs)) if fr.span(t, len(xs[u]), fp, fs)[1] >= n_cut)
    a = fr.span(first, len(xs[u]), fp, fs)[0]
    assert a > 0 and np.array_equal(cut[:a], ys[u][:a])


@pytest.mark.parametrize("fs,N,fp", [(16000, 1024, 5.0), (48000, 2048, 5.0)])
def test_a_bad_row_poisons_its_span_and_nothing_else(env, fs, N, fp):
    h = handle(env, fs, N, fp)
    xs, rows = batch(fs, N, fp, fr.POWER, 21)
    ys = device(env, h, xs, rows, fr.POWER)
    for value in (0.0, -2.0, np.inf, np.nan):
        bad = [r.copy() for r in rows]
        bad[5][1, N // 2] = value                   # the last bin of a row
        bad[1][0, 3] = value
        zs = device(env, h, xs, bad, fr.POWER)
        held_to_rule("bad rows %d" % N, zs, xs, bad, fr.POWER, fs, N, fp)
        for u, t in ((5, 1), (1, 0)):
            a = fr.span(t, len(xs[u]), fp, fs)[0]
            hit = np.zeros(len(xs[u]), dtype=bool)
            hit[a:a + N] = True
            assert np.isnan(zs[u][hit]).all() and np.array_equal(zs[u][~hit], ys[u][~hit])
        assert all(np.array_equal(zs[v], ys[v]) for v in range(len(xs)) if v not in (1, 5))
    log_bad = [fr.case_rows("noise", len(r), N, 1) for r in rows]
    log_bad[3][2, 0] = -np.inf
    held_to_rule("bad log rows %d" % N, device(env, h, xs, log_bad, fr.LOG), xs, log_bad, fr.LOG, fs, N, fp)


@pytest.mark.parametrize("fs,N,fp", [(16000, 1024, 5.0), (24000, 1024, 1.0), (44100, 2048, 5.0), (48000, 2048, 5.0)])
def test_the_block_form_against_the_wavefront_form(env, fs, N, fp):
    wave, block = handle(env, fs, N, fp), handle(env, fs, N, fp, block=True)
    for kind in (fr.POWER, fr.LOG):
        xs, rows = batch(fs, N, fp, kind, 31)
        a, b = device(env, wave, xs, rows, kind), device(env, block, xs, rows, kind)
        held_to_rule("block form %d/%d/%g kind %d" % (fs, N, fp, kind), b, xs, rows, kind, fs, N, fp)
        worst = 0.0
        for ya, yb, x, r in zip(a, b, xs, rows):
            if len(x):
                worst = max(worst, float(np.abs(ya - yb).max() / fr.unit(x, r, kind, fs, N, fp)))
        print("block against wave %d/%d/%g kind %d: %.4f u" % (fs, N, fp, kind, worst))
        assert 0.0 < worst <= BOUND   # (two forms: not the same code, the same rule)


@pytest.mark.parametrize("fs,N,fp,nd", [(8000, 512, 5.0, 25), (16000, 1024, 5.0, 60), (48000, 2048, 5.0, 60), (96000, 4096, 5.0, 40)])
def test_the_coded_call_is_the_two_public_calls(env, fs, N, fp, nd):
    w, ff, torch = env
    from world_class_amd import codec
    h = handle(env, fs, N, fp)
    rng = np.random.default_rng(nd)
    hop = fr.hop(fp, fs)
    lengths = [int(3.3 * hop), 0, int(2.1 * hop)]
    f_lengths = [fr.segments(lengths[0], fp, fs), 0, 2]
    total = sum(f_lengths)
    xs = [rng.normal(size=n) for n in lengths]
    to, frm = 0.4 * rng.normal(size=(total, nd)), 0.4 * rng.normal(size=(total, nd))
    d_x, d_to, d_from = up(env, np.concatenate(xs)), up(env, to), up(env, frm)
    for given in (True, False):
        for skip in (False, True):
            d = to - frm if given else to.copy()
            if skip:
                d[:, 0] = 0.0
            d_d, d_sp = up(env, d), up(env, np.zeros(total * (N // 2 + 1)))
            codec.decode_spectral_envelope_device(fs, N, total, nd, d_d, d_sp)
            d_want, d_got = up(env, np.full(sum(lengths), GUARD)), up(env, np.full(sum(lengths), GUARD))
            h.run(d_x, lengths, d_sp, f_lengths, d_want, "power")
            h.run_coded(d_x, lengths, d_to, d_from if given else None, nd, f_lengths, d_got, skip_energy=skip)
            assert w.lib().wc_synchronize() == 0
            want, got = d_want.cpu().numpy(), d_got.cpu().numpy()
            assert np.array_equal(want, got) and not np.any(got == GUARD), (given, skip)
            # and the decoded rows are what the rule takes
            ys = [got[e - n:e] for n, e in zip(lengths, np.cumsum(lengths))]
            sp = d_sp.cpu().numpy().reshape(total, N // 2 + 1)
            rows = [sp[e - f:e] for f, e in zip(f_lengths, np.cumsum(f_lengths))]
            held_to_rule("coded %d" % N, ys, xs, rows, fr.POWER, fs, N, fp)


def test_every_refusal_leaves_the_outputs_untouched(env):
    w, ff, torch = env
    L = ff._L()
    fs, N, fp = 16000, 1024, 5.0
    for bad in ((fs, 1000, fp), (fs, 256, fp), (0, N, fp), (-1, N, fp), (fs, N, 0.05), (fs, N, float("nan")), (fs, N, float("inf")),
                (fs, N, -5.0), (fs, N, 16.0625)):
        assert not L.wc_frame_filter_create(*bad) and w.last_error()
    h = handle(env, fs, N, fp)
    n, f, nd = 300, 4, 30
    rng = np.random.default_rng(1)
    x = rng.normal(size=n)
    d_x, d_rows = up(env, x), up(env, np.ones((f, N // 2 + 1)))
    d_to, d_from = up(env, 0.1 * rng.normal(size=(f, nd))), up(env, 0.1 * rng.normal(size=(f, nd)))
    d_y = up(env, np.full(n + 16, GUARD))
    ints = lambda *v: (C.c_int * len(v))(*v)
    p = lambda t, off=0: None if t is None else t.data_ptr() + 8 * off

    def run(handle_=h._h, n_utt=1, x_=d_x, xl=ints(n), kind=0, rows=d_rows, fl=ints(f), y=d_y, y_off=0):
        return L.wc_frame_filter_run_device(handle_, n_utt, p(x_), xl, kind, p(rows), fl, p(y, y_off))

    def coded(handle_=h._h, n_utt=1, x_=d_x, xl=ints(n), to=d_to, frm=d_from, nd_=nd, fl=ints(f), y=d_y):
        return L.wc_frame_filter_run_coded_device(handle_, n_utt, p(x_), xl, p(to), p(frm), nd_, 0, fl, p(y))

    refused = [run(handle_=None), run(n_utt=-1), run(xl=ints(-1)), run(fl=ints(-1)), run(fl=ints(0)), run(kind=2), run(kind=-1),
               run(x_=None), run(rows=None), run(y=None), run(xl=None), run(fl=None),
               run(y=d_x, y_off=1), run(y=d_x, y_off=n - 1), run(y=d_rows), run(y=d_rows, y_off=f * (N // 2 + 1) - 1),
               coded(handle_=None), coded(nd_=0), coded(nd_=N // 2 + 1), coded(to=None), coded(y=d_to), coded(y=d_from), coded(n_utt=-1),
               coded(fl=ints(0)), coded(xl=ints(-3))]
    assert w.lib().wc_synchronize() == 0
    assert len(set(refused)) == 1 and refused[0] != 0 and refused[0] == run(kind=5), refused
    assert "frame filter" in w.last_error()
    assert np.all(d_y.cpu().numpy() == GUARD) and np.array_equal(d_x.cpu().numpy(), x)
    assert np.all(d_rows.cpu().numpy() == 1.0)
    assert L.wc_frame_filter_segments(None, 5) == refused[0] and L.wc_frame_filter_segments(h._h, -1) == refused[0]
    # what is not refused: nothing to do, an empty utterance, surplus rows, d_y == d_x
    assert run(n_utt=0, xl=None, fl=None, x_=None, rows=None, y=None) == 0
    assert run(xl=ints(0), fl=ints(0), x_=None, rows=None, y=None) == 0 and run(xl=ints(0), fl=ints(0)) == 0
    assert w.lib().wc_synchronize() == 0 and np.all(d_y.cpu().numpy() == GUARD)
    assert run() == 0 and coded() == 0 and run(y=d_x) == 0 and w.lib().wc_synchronize() == 0
    assert np.all(d_y.cpu().numpy()[n:] == GUARD) and not np.any(d_y.cpu().numpy()[:n] == GUARD)


def test_two_host_threads_on_two_handles(env):
    w, ff, torch = env
    settings = [(16000, 1024, 5.0), (48000, 2048, 5.0)]
    work_items = []
    for i, (fs, N, fp) in enumerate(settings):
        xs, rows = batch(fs, N, fp, fr.POWER, 41 + i)
        single = device(env, handle(env, fs, N, fp), xs, rows, fr.POWER)
        lengths, f_lengths = [len(x) for x in xs], [len(r) for r in rows]
        work_items.append(dict(h=ff.FrameFilter(fs, N, fp), lengths=lengths, f_lengths=f_lengths, d_x=up(env, np.concatenate(xs)),
                               d_rows=up(env, np.concatenate(rows)), d_y=up(env, np.full(sum(lengths), GUARD)), single=np.concatenate(single)))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    errors = []

    def work(i):
        try:
            it = work_items[i]
            assert w.lib().wc_set_stream(streams[i].cuda_stream) == 0
            for rep in range(3):
                it["h"].run(it["d_x"], it["lengths"], it["d_rows"], it["f_lengths"], it["d_y"], "power")
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
    for it in work_items:
        assert np.array_equal(it["d_y"].cpu().numpy(), it["single"])
        it["h"].close()
