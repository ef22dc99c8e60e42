"""-m gpu: the frame filter's overlap-add (filter_overlap_add_kernel) where tests/test_gpu_filter.py does not reach: utterances of
several tiles at every size, so that a tile's first segment comes from the estimate and the walk and the trips of four end inside
an utterance (a); N rows over every sample at hop 1, and a NaN row among them (b); a hop whose centres are rounding ties (c); the
partition of unity on all of these, which needs no rule (d); the same bits across tiles (e); 300 utterances with empty ones in
front, behind and side by side (f); one handle on two streams with nothing but its event between the calls (g).  The bound is per
sample, |device - rule|[k] <= fr.K_AT * u_at[k] (tests/filter_rule.py): every test prints its largest ratio, and the one in the
per-utterance u where that still says something."""
import hashlib

import numpy as np
import pytest

import filter_rule as fr
from test_gpu_filter import GUARD, device, env, handle, up  # noqa: F401 -- env is the module's fixture

pytestmark = pytest.mark.gpu

_RULE = {}
_GROUP, _SIZE = {}, {}


def rule(x, rows, kind, fs, N, fp):
    """(y, u, u_at) of the rule, once per input"""
    key = (hashlib.sha1(x.tobytes()).digest(), hashlib.sha1(np.ascontiguousarray(rows).tobytes()).digest(), kind, fs, N, fp)
    if key not in _RULE:
        a, r, size, bad = fr.parts(x, rows, kind, fs, N, fp)
        _RULE[key] = (fr.overlap_add(a, r, len(x)), fr.unit_of(size, bad), fr.unit_at_of(a, size, bad, len(x), N))
    return _RULE[key]


def held_at(group, name, ys, xs, rows, kind, fs, N, fp):
    worst, worst_u = 0.0, 0.0
    for y, x, r in zip(ys, xs, rows):
        if not len(x):
            assert len(y) == 0
            continue
        want, u, u_at = rule(x, r, kind, fs, N, fp)
        assert np.array_equal(np.isnan(y), np.isnan(want))
        ok = ~np.isnan(want)
        err = np.abs(y - want)
        assert np.all(err[ok & (u_at == 0.0)] == 0.0)
        ok &= u_at > 0.0
        if ok.any():
            worst = max(worst, float((err[ok] / u_at[ok]).max()))
            worst_u = max(worst_u, float(err[ok].max() / u))
    _GROUP[group] = max(_GROUP.get(group, 0.0), worst)
    _SIZE[N] = max(_SIZE.get(N, 0.0), worst)
    print("%s %s: max |device - rule| / u_at = %.4f (%.4f u); group %s %.4f, fft %d %.4f, K_AT = %s"
          % (group, name, worst, worst_u, group, _GROUP[group], N, _SIZE[N], fr.K_AT))
    assert worst <= fr.K_AT
    return worst


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(p, q) for p, q in zip(a, b))


# ---- a. the tile walk at every size ---------------------------------------------------------------------------------------------------
WALK_RUNS = [c + (False,) for c in fr.WALK] + [c + (True,) for c in fr.WALK if c[1] in (1024, 2048)]


@pytest.mark.parametrize("kind", (fr.POWER, fr.LOG))
@pytest.mark.parametrize("fs,N,fp,n,block", WALK_RUNS)
def test_the_tile_walk_at_every_size(env, fs, N, fp, n, block, kind):
    """the long utterance beside two short ones under a grid sized by the long one; exact, held and surplus rows on each in turn"""
    assert max(fr.estimates(n, fs, N, fp)) > 0.0 and 1 <= n % fr.OLA_TILE <= 8
    h = handle(env, fs, N, fp, block)
    for turn in range(3):
        modes = fr.ROW_MODES[turn:] + fr.ROW_MODES[:turn]
        xs, rows = fr.long_batch(fs, N, fp, n, kind, turn, modes)
        assert [h.segments(len(x)) for x in xs] == [fr.segments(len(x), fp, fs) for x in xs]
        ys = device(env, h, xs, rows, kind)
        held_at("a", "%d/%d/%g%s kind %d %s" % (fs, N, fp, " block" if block else "", kind, modes[0]), ys, xs, rows, kind, fs, N, fp)


# ---- b. deep overlap --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", (fr.POWER, fr.LOG))
@pytest.mark.parametrize("fs,N,fp,n", fr.DEEP)
def test_deep_overlap(env, fs, N, fp, n, kind):
    h = handle(env, fs, N, fp)
    x, rows = fr.deep_case(fs, N, fp, n, kind, 1)
    S = fr.segments(n, fp, fs)
    assert h.segments(n) == S and (fr.hop(fp, fs) != 1.0 or S == n)
    xs, rows = [x, x[:5].copy()], [rows, rows[:1].copy()]
    ys = device(env, h, xs, rows, kind)
    held_at("b", "%d/%d/%g kind %d, %d rows" % (fs, N, fp, kind, S), ys, xs, rows, kind, fs, N, fp)


@pytest.mark.parametrize("fs,N,fp,n", fr.DEEP[:2])
def test_a_nan_row_at_hop_one_poisons_its_span_and_nothing_else(env, fs, N, fp, n):
    h = handle(env, fs, N, fp)
    x, rows = fr.deep_case(fs, N, fp, n, fr.POWER, 2)
    clean, = device(env, h, [x], [rows], fr.POWER)
    t = 900                                           # a_t = t at hop 1: the span crosses from the first tile into the second
    a = fr.span(t, n, fp, fs)[0]
    assert a == t and a < fr.OLA_TILE < a + N <= n
    bad = rows.copy()
    bad[t, 3] = np.nan
    z, = device(env, h, [x], [bad], fr.POWER)
    hit = np.zeros(n, dtype=bool)
    hit[a:a + N] = True
    assert not np.isnan(clean).any() and np.isnan(z[hit]).all() and np.array_equal(z[~hit], clean[~hit])


# ---- c. a hop whose centres are ties ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", (fr.POWER, fr.LOG))
@pytest.mark.parametrize("fs,N,fp,n", fr.TIES)
def test_a_hop_whose_centres_are_ties(env, fs, N, fp, n, kind):
    h = handle(env, fs, N, fp)
    xs, rows = fr.long_batch(fs, N, fp, n, kind, 5)
    assert [h.segments(len(x)) for x in xs] == [fr.segments(len(x), fp, fs) for x in xs]
    ends = [fr.centre(t, fp, fs) + d for t in (3, 17, 19, 21, 25) for d in (0, 1, 2)]     # (n - 1 before, on and behind a centre that is a tie)
    assert [h.segments(m) for m in ends] == [fr.segments(m, fp, fs) for m in ends]
    ys = device(env, h, xs, rows, kind)
    held_at("c", "%d/%d/%.4f kind %d" % (fs, N, fp, kind), ys, xs, rows, kind, fs, N, fp)


# ---- d. the partition of unity: no rule behind it -------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs,N,fp,n", fr.WALK + fr.DEEP + fr.TIES)
def test_log_rows_of_zeros_return_x(env, fs, N, fp, n):
    h = handle(env, fs, N, fp)
    rng = np.random.default_rng(n + N)
    xs = [rng.normal(size=n), rng.normal(size=int(fr.hop(fp, fs)) + 1)]
    ys = device(env, h, xs, [np.zeros((1, N // 2 + 1)), np.zeros((3, N // 2 + 1))], fr.LOG)
    worst = max(float(np.abs(y - x).max() / (2.0 ** -52 * np.abs(x).sum())) for x, y in zip(xs, ys))
    print("d %d/%d/%g: max |y - x| = %.4f * 2^-52 |x|_1 (asked: 64)" % (fs, N, fp, worst))
    for x, y in zip(xs, ys):
        assert np.abs(y - x).max() < 64 * 2.0 ** -52 * np.abs(x).sum()


# ---- e. the same bits across tiles ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs,N,fp,n", [c for c in fr.WALK if c[1] in (1024, 2048)])
def test_the_same_bits_across_tiles(env, fs, N, fp, n):
    h = handle(env, fs, N, fp)
    kind = fr.POWER
    xs, rows = fr.long_batch(fs, N, fp, n, kind, 11)
    ys = device(env, h, xs, rows, kind)
    held_at("e", "%d/%d/%g" % (fs, N, fp), ys, xs, rows, kind, fs, N, fp)
    assert same(ys, device(env, h, xs, rows, kind))
    for u in range(len(xs)):
        alone, = device(env, h, [xs[u]], [rows[u]], kind)
        assert np.array_equal(alone, ys[u]), u
    assert same(ys, device(env, h, xs, rows, kind, inplace=True))
    # a row in the third tile changed: the same bits outside [a_t, a_t + N)
    t = min(t for t in range(len(rows[0])) if fr.centre(t, fp, fs) >= 2 * fr.OLA_TILE)
    assert fr.centre(t, fp, fs) < 3 * fr.OLA_TILE
    changed = [r.copy() for r in rows]
    changed[0][t] = fr.as_kind(fr.case_rows("notch", 1, N, 5), kind)[0]
    other = device(env, h, xs, changed, kind)
    a = fr.span(t, n, fp, fs)[0]
    outside = np.ones(n, dtype=bool)
    outside[a:a + N] = False
    assert a > fr.OLA_TILE and (N != 1024 or a + N < n)      # (at 2048 the span runs to the end: what lies in front of it is the claim)
    assert np.array_equal(other[0][outside], ys[0][outside]) and not np.array_equal(other[0], ys[0])
    assert same(other[1:], ys[1:])
    # cut inside the second tile: the first segment the cut changes is the one that holds sample n_cut
    n_cut = fr.OLA_TILE + 600
    cut, = device(env, h, [xs[0][:n_cut]], [rows[0]], kind)
    first = min(t for t in range(fr.segments(n, fp, fs)) if fr.span(t, n, fp, fs)[1] >= n_cut)
    a = fr.span(first, n, fp, fs)[0]
    assert fr.OLA_TILE < a < n_cut and np.array_equal(cut[:a], ys[0][:a])


# ---- f. many utterances -----------------------------------------------------------------------------------------------------------------
def test_three_hundred_utterances_with_empty_ones_at_both_ends(env):
    fs, N, fp = 16000, 1024, 5.0
    h = handle(env, fs, N, fp)
    cycle = (0, 0, 1, 79, 80, 81, 161)
    lengths = [cycle[i % 7] for i in range(298)] + [0, 0]
    assert len(lengths) == 300 and lengths[:2] == [0, 0] and lengths[-3:] == [79, 0, 0] and lengths[6:9] == [161, 0, 0]
    rng = np.random.default_rng(300)
    xs = [rng.normal(size=m) for m in lengths]
    S = [fr.segments(m, fp, fs) for m in lengths]
    assert sorted(set(S)) == [0, 1, 2, 3]
    f_lengths = [1 + i % s if s else 0 for i, s in enumerate(S)]
    assert all(set(f for f, s in zip(f_lengths, S) if s == k) == set(range(1, k + 1)) for k in (1, 2, 3))
    rows = [fr.as_kind(fr.case_rows(("noise", "notch", "envelope")[i % 3], f, N, i), fr.POWER) for i, f in enumerate(f_lengths)]
    assert [h.segments(m) for m in cycle] == [fr.segments(m, fp, fs) for m in cycle]
    ys = device(env, h, xs, rows, fr.POWER)          # (device() asserts that the guard behind d_y is untouched)
    held_at("f", "300 utterances", ys, xs, rows, fr.POWER, fs, N, fp)


# ---- g. one handle, two streams ---------------------------------------------------------------------------------------------------------
def test_one_handle_on_two_streams(env):
    """the handle's scratch goes from stream to stream behind its event: nothing else orders the calls"""
    w, _, torch = env
    fs, N, fp, n = fr.WALK[1]
    h = handle(env, fs, N, fp)
    work = []
    for kind, seed, modes in ((fr.POWER, 21, fr.ROW_MODES), (fr.LOG, 22, fr.ROW_MODES[::-1])):
        xs, rows = fr.long_batch(fs, N, fp, n, kind, seed, modes)
        alone = device(env, h, xs, rows, kind)            # on the default stream, behind a synchronisation
        held_at("g", "stream batch kind %d" % kind, alone, xs, rows, kind, fs, N, fp)
        lengths, f_lengths = [len(x) for x in xs], [len(r) for r in rows]
        work.append(dict(lengths=lengths, f_lengths=f_lengths, d_x=up(env, np.concatenate(xs)), d_rows=up(env, np.concatenate(rows)),
                         d_y=[up(env, np.full(sum(lengths) + 8, GUARD)) for _ in range(3)], alone=np.concatenate(alone),
                         kind="power" if kind == fr.POWER else "log"))
    assert not np.array_equal(work[0]["alone"], work[1]["alone"])
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    try:
        for rep in range(3):
            for it, s in zip(work, streams):
                assert w.lib().wc_set_stream(s.cuda_stream) == 0
                h.run(it["d_x"], it["lengths"], it["d_rows"], it["f_lengths"], it["d_y"][rep], it["kind"])
    finally:
        assert w.lib().wc_set_stream(None) == 0
    torch.cuda.synchronize()
    for it in work:
        for rep in range(3):
            y = it["d_y"][rep].cpu().numpy()
            total = sum(it["lengths"])
            assert np.all(y[total:] == GUARD) and np.array_equal(y[:total], it["alone"]), rep
