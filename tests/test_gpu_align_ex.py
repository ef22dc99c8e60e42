"""-m gpu: extended feature alignment (wc_align_features_ex_device) against the plain restatement of its rule
(tests/align_ex_rule.py), bit for bit and integer for integer: the plain call's bytes at pattern 0 without flags, the strip-width
edges of the slope-limited pattern in one ragged batch with and without a band, open ends under both patterns, ties everywhere,
totals that are not finite, a planted phrase that is known without the rule, NULL outputs, refusals, the chains into retime and
morph and ordering on the caller's stream.  Every output is filled with a sentinel before the call, with room behind its last
pair; what the call has no business writing must keep it."""
import ctypes as C

import numpy as np
import pytest

import align_ex_rule as ax

pytestmark = pytest.mark.gpu
SENT, ISENT = -12345.5, -99
OLD_EDGES = [(1, 1), (1, 5), (5, 1), (2, 2), (63, 64), (64, 65), (65, 129), (130, 97)]
# pattern 1: strips of two columns up to m = 128 and of three from m = 129, a last strip that is not full, n of 1 to 3, and
# infeasible pairs (max - 1 > 2 * (min - 1)) beside feasible ones
SLOPE_FINITE = [(1, 1), (2, 2), (2, 3), (3, 2), (33, 65), (63, 64), (64, 127), (64, 65), (65, 129), (130, 97)]
SLOPE_INFEASIBLE = [(1, 5), (5, 1), (10, 20)]
SLOPE_EDGES = SLOPE_FINITE[:4] + [SLOPE_INFEASIBLE[0]] + SLOPE_FINITE[4:7] + SLOPE_INFEASIBLE[1:] + SLOPE_FINITE[7:]
OPEN_SHAPES = [(1, 1), (1, 5), (5, 1), (2, 2), (50, 64), (50, 65), (7, 129), (64, 200), (130, 97)]


@pytest.fixture(scope="module")
def env():
    import torch
    import world_class_amd as w
    from world_class_amd import codec, io as wio
    w.lib().wc_set_device(0)
    return w, codec, wio, torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).ravel()).cuda()


def _outputs(torch, a_lens, b_lens):
    """sentinel-filled d_cost, d_path_length, d_path, d_b_on_a, d_a_on_b, d_span, d_timeline_a, d_timeline_b with room behind the
    last pair"""
    P, entries = len(a_lens), sum(n + m - 1 for n, m in zip(a_lens, b_lens))
    full = lambda n, v, dt: torch.full((n,), v, dtype=dt, device="cuda")
    return [full(P + 2, SENT, torch.float64), full(P + 2, ISENT, torch.int32), full(2 * (entries + 3), ISENT, torch.int32),
            full(sum(a_lens) + 2, SENT, torch.float64), full(sum(b_lens) + 2, SENT, torch.float64), full(2 * (P + 2), ISENT, torch.int32),
            full(entries + 3, SENT, torch.float64), full(entries + 3, SENT, torch.float64)]


def _align(env, a_lens, fa, b_lens, fb, dims, dim_begin, dim_end, band, step_pattern, flags):
    """the device call into sentinel-filled outputs: numpy copies of all eight"""
    w, codec, wio, torch = env
    outs = _outputs(torch, a_lens, b_lens)
    d_a, d_b = _dev(torch, fa), _dev(torch, fb)
    torch.cuda.synchronize()  # (torch's fills run on its own stream, the library's kernels on another)
    wio.align_features_ex_device(a_lens, d_a, b_lens, d_b, dims, dim_begin, dim_end, band, step_pattern, flags, *outs)
    w.lib().wc_synchronize()
    return [o.cpu().numpy() for o in outs]


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _assert_equals_rule(got, want, a_lens, b_lens):
    """got: the eight arrays of _align; want: align_ex_rule's dicts.  d_cost bitwise, the rest exactly, sentinels where nothing
    belongs"""
    cost, plen, path, boa, aob, span, tla, tlb = got
    P = len(a_lens)
    path, span = path.reshape(-1, 2), span.reshape(-1, 2)
    fa = fb = po = 0
    for u, (n, m, r) in enumerate(zip(a_lens, b_lens, want)):
        K = len(r["path"])
        if np.isnan(r["cost"]):
            assert np.isnan(cost[u]), u
        else:
            assert _bits(cost[u]) == _bits(r["cost"]), (u, cost[u], r["cost"])
        assert plen[u] == K, (u, plen[u], K)
        assert np.array_equal(path[po:po + K], r["path"]), u
        assert (path[po + K:po + n + m - 1] == ISENT).all(), "pair %d: path entries behind K were written" % u
        assert np.array_equal(boa[fa:fa + n], r["b_on_a"], equal_nan=True), u
        assert np.array_equal(aob[fb:fb + m], r["a_on_b"], equal_nan=True), u
        assert np.array_equal(span[u], r["span"]), (u, span[u], r["span"])
        assert np.array_equal(tla[po:po + K], r["timeline_a"]) and np.array_equal(tlb[po:po + K], r["timeline_b"]), u
        assert (tla[po + K:po + n + m - 1] == SENT).all() and (tlb[po + K:po + n + m - 1] == SENT).all(), "pair %d: timeline behind K" % u
        fa, fb, po = fa + n, fb + m, po + n + m - 1
    assert (cost[P:] == SENT).all() and (plen[P:] == ISENT).all() and (path[po:] == ISENT).all() and (span[P:] == ISENT).all()
    assert (boa[fa:] == SENT).all() and (aob[fb:] == SENT).all() and (tla[po:] == SENT).all() and (tlb[po:] == SENT).all()


def _random_batch(shapes, dims, seed):
    rng = np.random.default_rng(seed)
    a_lens, b_lens = [n for n, _ in shapes], [m for _, m in shapes]
    return a_lens, rng.standard_normal((sum(a_lens), dims)), b_lens, rng.standard_normal((sum(b_lens), dims))


_cases = {}


def _case(name, shapes, seed):
    """a ragged batch of random rows, made once and left unchanged"""
    if name not in _cases:
        _cases[name] = _random_batch(shapes, 60, seed)
    return _cases[name]


@pytest.mark.parametrize("band", [0, 5])
def test_pattern_0_without_flags_writes_the_bytes_of_the_plain_call(env, band):
    w, codec, wio, torch = env
    a_lens, fa, b_lens, fb = _case("old", OLD_EDGES, 20260)
    d_a, d_b = _dev(torch, fa), _dev(torch, fb)
    old, new = _outputs(torch, a_lens, b_lens), _outputs(torch, a_lens, b_lens)
    torch.cuda.synchronize()
    wio.align_features_device(a_lens, d_a, b_lens, d_b, 60, 1, 60, band, *old[:5])
    wio.align_features_ex_device(a_lens, d_a, b_lens, d_b, 60, 1, 60, band, 0, 0, *new[:5])
    w.lib().wc_synchronize()
    for k in range(5):
        assert old[k].cpu().numpy().tobytes() == new[k].cpu().numpy().tobytes(), k
    for k in range(5, 8):  # (not handed over: untouched)
        assert bool((new[k] == (ISENT if k == 5 else SENT)).all())
    want = ax.align_batch(a_lens, fa, b_lens, fb, 1, 60, band, 0, 0)
    _assert_equals_rule(_align(env, a_lens, fa, b_lens, fb, 60, 1, 60, band, 0, 0), want, a_lens, b_lens)
    assert all(np.isfinite(r["cost"]) for r in want)


@pytest.mark.parametrize("band", [0, 1, 4])
def test_pattern_1_boundary_shapes_in_one_ragged_batch_equal_the_rule(env, band):
    a_lens, fa, b_lens, fb = _case("slope", SLOPE_EDGES, 20261)
    want = ax.align_batch(a_lens, fa, b_lens, fb, 1, 60, band, 1, 0)
    got = _align(env, a_lens, fa, b_lens, fb, 60, 1, 60, band, 1, 0)
    _assert_equals_rule(got, want, a_lens, b_lens)
    for (n, m), r, c in zip(SLOPE_EDGES, want, got[0]):
        if (n, m) in SLOPE_INFEASIBLE:
            assert c == np.inf and len(r["path"]) == 0 and r["span"].tolist() == [-1, -1]
        elif band == 0:
            assert np.isfinite(c) and max(n, m) <= len(r["path"]) <= n + m - 1
            assert np.bincount(r["path"][:, 0]).max() <= 2 and np.bincount(r["path"][:, 1]).max() <= 2
    if band:  # a band can only cost: no finite total lies below the free one
        free = ax.align_batch(a_lens, fa, b_lens, fb, 1, 60, 0, 1, 0)
        assert all(r["cost"] >= f["cost"] for r, f in zip(want, free))


@pytest.mark.parametrize("step_pattern,flags", [(p, f) for p in (0, 1) for f in (1, 2, 3)])
def test_open_ends_in_one_ragged_batch_equal_the_rule(env, step_pattern, flags):
    a_lens, fa, b_lens, fb = _case("open", OPEN_SHAPES, 20262)
    want = ax.align_batch(a_lens, fa, b_lens, fb, 1, 60, 0, step_pattern, flags)
    got = _align(env, a_lens, fa, b_lens, fb, 60, 1, 60, 0, step_pattern, flags)
    _assert_equals_rule(got, want, a_lens, b_lens)
    fb0 = 0
    for (n, m), r in zip(OPEN_SHAPES, want):  # what the rule says about the span and the held ends, on the device's arrays
        aob = got[4][fb0:fb0 + m]
        fb0 += m
        if len(r["path"]) == 0:
            continue
        j0, j1 = r["span"]
        assert (j0 == 0 or flags & ax.OPEN_BEGIN) and (j1 == m - 1 or flags & ax.OPEN_END)
        assert (aob[:j0] == 0.0).all() and (aob[j1 + 1:] == n - 1).all()
    found = [(m, r["span"]) for (n, m), r in zip(OPEN_SHAPES, want) if len(r["path"])]
    assert any(j0 > 0 for _, (j0, _) in found) == bool(flags & ax.OPEN_BEGIN)
    assert any(j1 < m - 1 for m, (_, j1) in found) == bool(flags & ax.OPEN_END)


@pytest.mark.parametrize("step_pattern,flags", [(0, 3), (1, 0), (1, 3)])
@pytest.mark.parametrize("n,m", [(65, 129), (130, 97)])
def test_ties_everywhere(env, n, m, step_pattern, flags):
    """features from {0, 1, 2}: squared distances are small integers, their sums exact, and equal D meet at most cells and along the
    last row"""
    rng = np.random.default_rng(n)
    fa, fb = rng.integers(0, 3, (n, 3)).astype(np.float64), rng.integers(0, 3, (m, 3)).astype(np.float64)
    want = ax.align_batch([n], fa, [m], fb, 0, 3, 0, step_pattern, flags)
    _assert_equals_rule(_align(env, [n], fa, [m], fb, 3, 0, 3, 0, step_pattern, flags), want, [n], [m])
    assert np.isfinite(want[0]["cost"])


@pytest.mark.parametrize("step_pattern,flags", [(0, 2), (0, 3), (1, 3)])
def test_totals_that_are_not_finite_under_open_ends(env, step_pattern, flags):
    """four pairs: the second has a row of NaN in the middle of A (no cell of the last row wins: K = 0), the third in the middle of B
    (under pattern 0 with a closed beginning NaN spreads to the right of that column and the end is found left of it; an open
    beginning starts paths right of it too); the rule is the judge, and the neighbours are not affected"""
    shapes = [(40, 31), (50, 66), (35, 80), (20, 70)]
    a_lens, fa, b_lens, fb = _random_batch(shapes, 60, 99)
    fa[40 + 17] = np.nan
    fb[31 + 66 + 40] = np.nan
    want = ax.align_batch(a_lens, fa, b_lens, fb, 1, 60, 0, step_pattern, flags)
    got = _align(env, a_lens, fa, b_lens, fb, 60, 1, 60, 0, step_pattern, flags)
    _assert_equals_rule(got, want, a_lens, b_lens)
    cost, plen, _, boa, aob, span = got[:6]
    assert not np.isfinite(cost[1]) and plen[1] == 0 and span[2:4].tolist() == [-1, -1]
    assert np.isnan(boa[40:90]).all() and np.isnan(aob[31:97]).all()
    assert np.isfinite(cost[[0, 3]]).all() and plen[0] > 0 and plen[3] > 0
    if flags == 2:
        assert np.isfinite(cost[2]) and span[4] == 0 and 0 <= span[5] < 40


def _planted(n, dims, pre, total, max_hold, seed):
    """a query of n distinct rows and a track of `total` rows: pre random rows, the query with row r held h_r times (h_0 = h_last =
    1), random rows behind.  (query, track, g): g[k] is the query's row at track column pre + k"""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((n, dims))
    holds = 1 + (np.arange(n) * 7 + 3) % max_hold
    holds[[0, n - 1]] = 1
    g = np.repeat(np.arange(n), holds)
    post = total - pre - len(g)
    track = np.concatenate([rng.standard_normal((pre, dims)), q[g], rng.standard_normal((post, dims))])
    assert set(holds) == set(range(1, max_hold + 1))
    return q, track, g


@pytest.mark.parametrize("step_pattern,max_hold", [(0, 4), (1, 2)])
def test_a_planted_phrase_needs_no_rule(env, step_pattern, max_hold):
    total = 37 + int((1 + (np.arange(50) * 7 + 3) % max_hold).sum()) + 41  # (a little longer than the planted phrase needs)
    q, track, g = _planted(50, 60, 37, total, max_hold, 50 + step_pattern)
    m, post = len(track), len(track) - 37 - len(g)
    assert m == total and post >= 41
    cost, plen, path, boa, aob, span, tla, tlb = _align(env, [50], q, [m], track, 60, 1, 60, 0, step_pattern, 3)
    K = len(g)
    assert cost[0] == 0.0 and plen[0] == K and span[:2].tolist() == [37, 37 + K - 1]
    assert np.array_equal(path.reshape(-1, 2)[:K], np.stack([g, 37 + np.arange(K)], axis=1))
    assert np.array_equal(tla[:K], g.astype(np.float64)) and np.array_equal(tlb[:K], 37.0 + np.arange(K))
    assert np.array_equal(aob[:m], np.concatenate([np.zeros(37), g.astype(np.float64), np.full(post, 49.0)]))
    closed = _align(env, [50], q, [m], track, 60, 1, 60, 0, step_pattern, 0)
    assert closed[0][0] > 0 if step_pattern == 0 else closed[0][0] == np.inf


def test_a_planted_phrase_in_a_long_track(env):
    """200 x 5000 at pattern 0: a strip of 79 columns, ten rounds of eight cells with a last one that is not full"""
    pre = 2100
    q, track, g = _planted(200, 60, pre, 5000, 4, 200)
    m, K = len(track), len(g)
    assert m == 5000 and 400 <= K <= 600
    cost, plen, path, boa, aob, span, tla, tlb = _align(env, [200], q, [m], track, 60, 1, 60, 0, 0, 3)
    assert cost[0] == 0.0 and plen[0] == K and span[:2].tolist() == [pre, pre + K - 1]
    assert np.array_equal(path.reshape(-1, 2)[:K], np.stack([g, pre + np.arange(K)], axis=1))
    assert np.array_equal(tla[:K], g.astype(np.float64)) and np.array_equal(tlb[:K], pre + np.arange(K, dtype=np.float64))
    assert (tla[K:] == SENT).all() and (tlb[K:] == SENT).all() and (path.reshape(-1, 2)[K:] == ISENT).all()
    assert (aob[:pre] == 0.0).all() and np.array_equal(aob[pre:pre + K], g.astype(np.float64)) and (aob[pre + K:m] == 199.0).all()
    first = pre + np.concatenate([[0], np.cumsum(np.bincount(g))[:-1]])
    assert np.array_equal(boa[:200], (first + first + np.bincount(g) - 1) * 0.5)


def test_optional_outputs_may_be_null_one_at_a_time(env):
    w, codec, wio, torch = env
    a_lens, fa, b_lens, fb = _case("open", OPEN_SHAPES, 20262)
    full = _align(env, a_lens, fa, b_lens, fb, 60, 1, 60, 0, 1, 3)
    d_a, d_b = _dev(torch, fa), _dev(torch, fb)
    for drop in range(2, 8):
        outs = _outputs(torch, a_lens, b_lens)
        before = outs[drop].clone()
        args = [None if k == drop else o for k, o in enumerate(outs)]
        torch.cuda.synchronize()
        wio.align_features_ex_device(a_lens, d_a, b_lens, d_b, 60, 1, 60, 0, 1, 3, *args)
        w.lib().wc_synchronize()
        for k in range(8):
            if k != drop:
                assert outs[k].cpu().numpy().tobytes() == full[k].tobytes(), (drop, k)
        assert torch.equal(outs[drop], before)


def test_refused_calls_leave_the_outputs_untouched(env):
    w, codec, wio, torch = env
    L = w.lib()
    a_lens, fa, b_lens, fb = _random_batch([(9, 12), (6, 4)], 8, 5)
    d_a, d_b = _dev(torch, fa), _dev(torch, fb)
    outs = _outputs(torch, a_lens, b_lens)
    before = [o.clone() for o in outs]
    torch.cuda.synchronize()
    good = dict(n=2, al=a_lens, a=d_a, bl=b_lens, b=d_b, dims=8, lo=1, hi=8, band=0, pat=1, flags=3, cost=outs[0], plen=outs[1])
    ints = lambda v: None if v is None else (C.c_int * max(1, len(v)))(*v)
    ptr = lambda x: None if x is None else x.data_ptr()

    def call(**kw):
        g = dict(good, **kw)
        return wio._io().wc_align_features_ex_device(g["n"], ints(g["al"]), ptr(g["a"]), ints(g["bl"]), ptr(g["b"]), g["dims"], g["lo"], g["hi"],
                                                     g["band"], g["pat"], g["flags"], ptr(g["cost"]), ptr(g["plen"]), *[o.data_ptr() for o in outs[2:]])

    bad = [dict(pat=2), dict(pat=-1), dict(flags=4), dict(flags=-1), dict(flags=1, band=3), dict(flags=2, band=1), dict(flags=3, band=20),
           # 1.96e8 cells: above 2^27 and below 2^28, so only the cap of pattern 1 refuses it (from the lengths alone)
           dict(n=1, al=[14000], bl=[14000], flags=0), dict(n=1, al=[14000], bl=[14000]),
           # what the plain call refuses
           dict(n=-1), dict(al=[9, 0]), dict(bl=[0, 4]), dict(dims=0), dict(lo=-1), dict(hi=9), dict(lo=5, hi=5), dict(band=-1, flags=0),
           dict(al=None), dict(bl=None), dict(a=None), dict(b=None), dict(cost=None), dict(plen=None),
           dict(n=1, al=[20000], bl=[20000], pat=0)]
    assert 1 << 27 < 14000 * 14000 < 1 << 28
    for kw in bad:
        assert call(**kw) == -1, kw
        assert w.last_error(), kw
    assert call(n=0) == 0
    L.wc_synchronize()
    for o, b4 in zip(outs, before):
        assert torch.equal(o, b4)
    with pytest.raises(w.WorldClassError):
        wio.align_features_ex_device(a_lens, d_a, b_lens, d_b, 8, 1, 8, 0, 2, 0, *outs)
    with pytest.raises(ValueError):
        wio.align_features_ex_device(a_lens, d_a, b_lens[:1], d_b, 8, 1, 8, 0, 1, 0, *outs)
    assert call() == 0  # the arguments the bad ones were varied from are good
    L.wc_synchronize()
    _assert_equals_rule([o.cpu().numpy() for o in outs], ax.align_batch(a_lens, fa, b_lens, fb, 1, 8, 0, 1, 3), a_lens, b_lens)


def test_host_convenience_equals_the_device_call(env):
    w, codec, wio, torch = env
    a_lens, fa, b_lens, fb = _random_batch([(57, 83)], 60, 57)
    for band, pat, ob, oe in ((0, 1, True, True), (4, 1, False, False), (0, 0, False, True)):
        flags = (wio.ALIGN_OPEN_BEGIN if ob else 0) | (wio.ALIGN_OPEN_END if oe else 0)
        cost, plen, path, boa, aob, span, tla, tlb = _align(env, a_lens, fa, b_lens, fb, 60, 1, 60, band, pat, flags)
        r = wio.align_features_ex(fa, fb, band=band, step_pattern=pat, open_begin=ob, open_end=oe)
        K = plen[0]
        assert _bits(r["cost"]) == _bits(cost[0]) and r["path"].shape == (K, 2) and K > 0
        assert np.array_equal(r["path"], path.reshape(-1, 2)[:K]) and np.array_equal(r["span"], span[:2])
        assert np.array_equal(r["b_on_a"], boa[:57]) and np.array_equal(r["a_on_b"], aob[:83])
        assert np.array_equal(r["timeline_a"], tla[:K]) and np.array_equal(r["timeline_b"], tlb[:K])
    r = wio.align_features_ex(fa[:5], fb[:20], step_pattern=1)
    assert r["cost"] == np.inf and r["path"].shape == (0, 2) and r["span"].tolist() == [-1, -1] and len(r["timeline_a"]) == 0
    assert np.isnan(r["b_on_a"]).all() and np.isnan(r["a_on_b"]).all()


def _voices(torch, fs, fft, na, nb):
    from oracle.gen_golden import synth_params
    A, B = synth_params(fs, fft, na, 811), synth_params(fs, fft, nb, 812)
    return A, B, [_dev(torch, v) for v in A], [_dev(torch, v) for v in B]


def test_chain_code_align_retime(env):
    """two utterances coded on the device, the coded rows aligned with both ends open under pattern 1, d_a_on_b handed to
    wc_retime_parameters_device as it lies in HBM: A's parameters at B's timing, with A's end frames held outside the span, equal
    tests/retime_rule.py at the rule's map bit for bit"""
    w, codec, wio, torch = env
    import retime_rule as rr
    fs, fft, nd, na, nb = 16000, 1024, 60, 118, 127
    bins = fft // 2 + 1
    A, B, d_A, d_B = _voices(torch, fs, fft, na, nb)
    d_ca, d_cb = torch.zeros(na * nd, dtype=torch.float64, device="cuda"), torch.zeros(nb * nd, dtype=torch.float64, device="cuda")
    outs = _outputs(torch, [na], [nb])
    r_f0 = torch.full((nb + 1,), np.nan, dtype=torch.float64, device="cuda")
    r_sp, r_ap = (torch.full(((nb + 1) * bins,), np.nan, dtype=torch.float64, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    codec.code_features_device(fs, fft, na, nd, d_A[1], None, d_ca, None)
    codec.code_features_device(fs, fft, nb, nd, d_B[1], None, d_cb, None)
    wio.align_features_ex_device([na], d_ca, [nb], d_cb, nd, 1, nd, 0, 1, 3, *outs)
    wio.retime_parameters_device(fs, fft, [na], d_A[0], d_A[1], d_A[2], [nb], outs[4], None, None, r_f0, r_sp, r_ap)
    w.lib().wc_synchronize()
    ca, cb = d_ca.cpu().numpy().reshape(na, nd), d_cb.cpu().numpy().reshape(nb, nd)
    want = ax.align_batch([na], ca, [nb], cb, 1, nd, 0, 1, 3)
    _assert_equals_rule([o.cpu().numpy() for o in outs], want, [na], [nb])
    f0, sp, ap = rr.retime(A[0], A[1], A[2], want[0]["a_on_b"])
    assert np.array_equal(r_f0.cpu().numpy()[:nb], f0)
    assert np.array_equal(r_sp.cpu().numpy()[:nb * bins].reshape(nb, bins), sp)
    assert np.array_equal(r_ap.cpu().numpy()[:nb * bins].reshape(nb, bins), ap)
    assert np.isnan(r_f0.cpu().numpy()[nb]) and np.isnan(r_sp.cpu().numpy()[nb * bins:]).all()
    assert (np.diff(want[0]["a_on_b"]) > 0).any() and want[0]["cost"] > 0


LOG_EXP_REL = 1e-12  # tests/test_gpu_morph.py: what the device's log and exp may differ from numpy's by in a blended value


def test_chain_align_read_k_morph(env):
    """the coded rows aligned under pattern 1, K read back, the two timelines handed to wc_morph_parameters_device as they lie in HBM
    with weight 0.5 and out_length = K.  The blend is byte for byte the one the same call makes from the rule's timelines uploaded
    from the host, and it equals tests/morph_rule.py at the rule's timelines as far as that rule is exact: bit for bit in the ap
    rows, in F0 wherever not both frames are voiced and in what lies behind K; an sp bin or an F0 between two voiced frames at a
    weight of 0.5 goes through the device's log and exp, which morph_rule states to LOG_EXP_REL"""
    w, codec, wio, torch = env
    import morph_rule as mr
    import retime_rule as rr
    fs, fft, nd, na, nb = 16000, 1024, 60, 118, 127
    bins = fft // 2 + 1
    A, B, d_A, d_B = _voices(torch, fs, fft, na, nb)
    d_ca, d_cb = torch.zeros(na * nd, dtype=torch.float64, device="cuda"), torch.zeros(nb * nd, dtype=torch.float64, device="cuda")
    outs = _outputs(torch, [na], [nb])
    most = na + nb - 1
    d_w = _dev(torch, np.full(most, 0.5))
    blends = [[torch.full(((most + 1) * wd,), np.nan, dtype=torch.float64, device="cuda") for wd in (1, bins, bins)] for _ in range(2)]
    torch.cuda.synchronize()
    codec.code_features_device(fs, fft, na, nd, d_A[1], None, d_ca, None)
    codec.code_features_device(fs, fft, nb, nd, d_B[1], None, d_cb, None)
    wio.align_features_ex_device([na], d_ca, [nb], d_cb, nd, 1, nd, 0, 1, 0, *outs)
    w.lib().wc_synchronize()
    K = int(outs[1].cpu().numpy()[0])
    wio.morph_parameters_device(fs, fft, [na], *d_A, [nb], *d_B, [K], outs[6], outs[7], d_w, None, None, None, *blends[0])
    w.lib().wc_synchronize()
    ca, cb = d_ca.cpu().numpy().reshape(na, nd), d_cb.cpu().numpy().reshape(nb, nd)
    want = ax.align_batch([na], ca, [nb], cb, 1, nd, 0, 1, 0)
    _assert_equals_rule([o.cpu().numpy() for o in outs], want, [na], [nb])
    assert K == len(want[0]["path"]) and max(na, nb) <= K <= most
    ta, tb = want[0]["timeline_a"], want[0]["timeline_b"]
    d_ta, d_tb = _dev(torch, ta), _dev(torch, tb)
    torch.cuda.synchronize()
    wio.morph_parameters_device(fs, fft, [na], *d_A, [nb], *d_B, [K], d_ta, d_tb, d_w, None, None, None, *blends[1])
    w.lib().wc_synchronize()
    g_f0, g_sp, g_ap = (o.cpu().numpy() for o in blends[0])
    for o, g in zip(blends[1], (g_f0, g_sp, g_ap)):
        assert o.cpu().numpy().tobytes() == g.tobytes()
    f0, sp, ap = mr.morph(A, B, ta, tb, np.full(K, 0.5))
    glide = (rr.retime(A[0], A[1], A[2], ta)[0] != 0) & (rr.retime(B[0], B[1], B[2], tb)[0] != 0)
    rel = lambda g, x: float(np.abs(g / x - 1).max())
    e_sp, e_f0 = rel(g_sp[:K * bins].reshape(K, bins), sp), rel(g_f0[:K][glide], f0[glide])
    print("morph at the path's timelines against the numpy rule: K %d, %d of them between two voiced frames, sp %.3e, F0 %.3e (relative)" % (
        K, glide.sum(), e_sp, e_f0))
    assert np.array_equal(g_ap[:K * bins].reshape(K, bins), ap)
    assert glide.sum() > 20 and (~glide).sum() > 20 and np.array_equal(g_f0[:K][~glide], f0[:K][~glide])
    assert e_sp < LOG_EXP_REL and e_f0 < LOG_EXP_REL
    assert np.isnan(g_f0[K:]).all() and np.isnan(g_sp[K * bins:]).all() and np.isnan(g_ap[K * bins:]).all()


def test_ordered_on_the_callers_stream_behind_the_coder(env):
    """on a torch stream handed over by wc_set_stream: a long kernel, the uploads, the coder and the alignment behind each other with
    no synchronisation between them, twice (the second call reuses staging and scratch while the first may still run)"""
    w, codec, wio, torch = env
    from oracle.gen_golden import synth_params
    fs, fft, nd = 16000, 1024, 60
    lens = [(70, 90), (101, 64)]
    rows = [[np.ascontiguousarray(synth_params(fs, fft, n, 900 + 10 * k + q)[1]) for q, n in enumerate(p)] for k, p in enumerate(lens)]
    host = [[torch.from_numpy(r.ravel().copy()).pin_memory() for r in p] for p in rows]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert w.lib().wc_set_stream(s.cuda_stream) == 0
    try:
        kept = []
        with torch.cuda.stream(s):
            junk = torch.randn(2048, 2048, device="cuda")
            for _ in range(20):
                junk = junk @ junk * 1e-3
            for (na, nb), (h_a, h_b) in zip(lens, host):
                d_sa, d_sb = (torch.zeros(n * (fft // 2 + 1), dtype=torch.float64, device="cuda") for n in (na, nb))
                d_ca, d_cb = (torch.full((n * nd,), np.nan, dtype=torch.float64, device="cuda") for n in (na, nb))
                outs = _outputs(torch, [na], [nb])
                d_sa.copy_(h_a, non_blocking=True)
                d_sb.copy_(h_b, non_blocking=True)
                codec.code_features_device(fs, fft, na, nd, d_sa, None, d_ca, None)
                codec.code_features_device(fs, fft, nb, nd, d_sb, None, d_cb, None)
                wio.align_features_ex_device([na], d_ca, [nb], d_cb, nd, 1, nd, 0, 1, 3, *outs)
                kept.append((d_sa, d_sb, d_ca, d_cb, outs))
        s.synchronize()  # once
    finally:
        assert w.lib().wc_set_stream(None) == 0
    for (na, nb), (_, _, d_ca, d_cb, outs) in zip(lens, kept):
        ca, cb = d_ca.cpu().numpy().reshape(na, nd), d_cb.cpu().numpy().reshape(nb, nd)
        assert np.isfinite(ca).all() and np.isfinite(cb).all()
        _assert_equals_rule([o.cpu().numpy() for o in outs], ax.align_batch([na], ca, [nb], cb, 1, nd, 0, 1, 3), [na], [nb])
        again = _align(env, [na], ca, [nb], cb, nd, 1, nd, 0, 1, 3)  # the same on the library's own stream
        for o, g in zip(outs, again):
            assert o.cpu().numpy().tobytes() == g.tobytes()
