"""-m gpu: feature alignment (wc_align_features_device) against the plain restatement of its rule (tests/align_rule.py), bit for bit
and integer for integer: the strip-width and lane-count edges of a 64-lane design in one ragged batch, ties everywhere, the band,
the window of coefficients, totals that are not finite, a warp that is known without the rule, the chain code -> align -> retime,
refusals, the host convenience and ordering on the caller's stream.  Every output is filled with a sentinel before the call, with
room behind its last pair; what the call has no business writing must keep it."""
import ctypes as C

import numpy as np
import pytest

import align_rule as ar

pytestmark = pytest.mark.gpu
SENT, ISENT = -12345.5, -99
EDGES = [(1, 1), (1, 5), (5, 1), (2, 2), (63, 64), (64, 65), (65, 129), (130, 97)]


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
    """sentinel-filled d_cost, d_path_length, d_path, d_b_on_a, d_a_on_b with room behind the last pair"""
    P, entries = len(a_lens), sum(n + m - 1 for n, m in zip(a_lens, b_lens))
    full = lambda n, v, dt: torch.full((n,), v, dtype=dt, device="cuda")
    return [full(P + 2, SENT, torch.float64), full(P + 2, ISENT, torch.int32), full(2 * (entries + 3), ISENT, torch.int32),
            full(sum(a_lens) + 2, SENT, torch.float64), full(sum(b_lens) + 2, SENT, torch.float64)]


def _align(env, a_lens, fa, b_lens, fb, dims, dim_begin, dim_end, band):
    """the device call into sentinel-filled outputs: numpy copies of all five"""
    w, codec, wio, torch = env
    outs = _outputs(torch, a_lens, b_lens)
    d_a, d_b = _dev(torch, fa), _dev(torch, fb)
    torch.cuda.synchronize()  # (torch's fills run on its own stream, the library's kernels on another)
    wio.align_features_device(a_lens, d_a, b_lens, d_b, dims, dim_begin, dim_end, band, *outs)
    w.lib().wc_synchronize()
    return [o.cpu().numpy() for o in outs]


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _assert_equals_rule(got, want, a_lens, b_lens):
    """got: the five arrays of _align; want: align_rule's dicts.  d_cost bitwise, the rest exactly, sentinels where nothing belongs"""
    cost, plen, path, boa, aob = got
    P = len(a_lens)
    path = path.reshape(-1, 2)
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
        fa, fb, po = fa + n, fb + m, po + n + m - 1
    assert (cost[P:] == SENT).all() and (plen[P:] == ISENT).all() and (path[po:] == ISENT).all()
    assert (boa[fa:] == SENT).all() and (aob[fb:] == SENT).all()


def _random_batch(shapes, dims, seed):
    rng = np.random.default_rng(seed)
    a_lens, b_lens = [n for n, _ in shapes], [m for _, m in shapes]
    return a_lens, rng.standard_normal((sum(a_lens), dims)), b_lens, rng.standard_normal((sum(b_lens), dims))


_edge_case = {}


def _edges():
    """the ragged batch of the boundary shapes and the rule's answer, made once and left unchanged"""
    if not _edge_case:
        a_lens, fa, b_lens, fb = _random_batch(EDGES, 60, 20260)
        _edge_case["v"] = (a_lens, fa, b_lens, fb, ar.align_batch(a_lens, fa, b_lens, fb, 1, 60))
    return _edge_case["v"]


def test_boundary_shapes_in_one_ragged_batch_equal_the_rule(env):
    a_lens, fa, b_lens, fb, want = _edges()
    got = _align(env, a_lens, fa, b_lens, fb, 60, 1, 60, 0)
    _assert_equals_rule(got, want, a_lens, b_lens)
    for (n, m), r in zip(EDGES, want):
        assert max(n, m) <= len(r["path"]) <= n + m - 1 and np.isfinite(r["cost"])


def test_optional_outputs_may_be_null(env):
    w, codec, wio, torch = env
    a_lens, fa, b_lens, fb, want = _edges()
    full = _align(env, a_lens, fa, b_lens, fb, 60, 1, 60, 0)
    d_a, d_b = _dev(torch, fa), _dev(torch, fb)
    for keep in range(3):
        outs = _outputs(torch, a_lens, b_lens)
        args = [o if k < 2 or k - 2 == keep else None for k, o in enumerate(outs)]
        torch.cuda.synchronize()
        wio.align_features_device(a_lens, d_a, b_lens, d_b, 60, 1, 60, 0, *args)
        w.lib().wc_synchronize()
        for k in (0, 1, 2 + keep):
            assert np.array_equal(outs[k].cpu().numpy(), full[k]), (keep, k)


@pytest.mark.parametrize("n,m", [(65, 129), (130, 97)])
def test_ties_everywhere(env, n, m):
    """features from {0, 1, 2}: squared distances are small integers, their sums exact, and equal D meet at most cells"""
    rng = np.random.default_rng(n)
    fa, fb = rng.integers(0, 3, (n, 3)).astype(np.float64), rng.integers(0, 3, (m, 3)).astype(np.float64)
    want = ar.align_batch([n], fa, [m], fb, 0, 3)
    _assert_equals_rule(_align(env, [n], fa, [m], fb, 3, 0, 3, 0), want, [n], [m])


@pytest.mark.parametrize("n,m", [(130, 97), (7, 40)])
def test_band(env, n, m):
    a_lens, fa, b_lens, fb = _random_batch([(n, m)], 60, 7 * n + m)
    free = _align(env, a_lens, fa, b_lens, fb, 60, 1, 60, 0)
    costs = []
    for band in (0, 1, 3, max(n, m)):
        want = ar.align_batch(a_lens, fa, b_lens, fb, 1, 60, band)
        got = _align(env, a_lens, fa, b_lens, fb, 60, 1, 60, band)
        _assert_equals_rule(got, want, a_lens, b_lens)
        costs.append(got[0][0])
        if band == max(n, m):
            for g, f in zip(got, free):
                assert g.tobytes() == f.tobytes()
    assert costs[1] >= costs[2] >= costs[0] and costs[1] > costs[0]


def test_band_in_a_ragged_batch(env):
    """every pair of the boundary shapes under one band: each pair's own L, storage rows narrower than the matrix"""
    a_lens, fa, b_lens, fb, _ = _edges()
    for band in (1, 5):
        want = ar.align_batch(a_lens, fa, b_lens, fb, 1, 60, band)
        _assert_equals_rule(_align(env, a_lens, fa, b_lens, fb, 60, 1, 60, band), want, a_lens, b_lens)


@pytest.mark.parametrize("dims,lo,hi", [(1, 0, 1), (60, 1, 25), (70, 2, 69)])
def test_dimension_window(env, dims, lo, hi):
    """(70, 2, 69): more coefficients than one trip through the cost pass's LDS tile holds, and a last trip that is not full"""
    a_lens, fa, b_lens, fb = _random_batch([(33, 70), (41, 20)], dims, dims + hi)
    want = ar.align_batch(a_lens, fa, b_lens, fb, lo, hi)
    _assert_equals_rule(_align(env, a_lens, fa, b_lens, fb, dims, lo, hi, 0), want, a_lens, b_lens)


def test_totals_that_are_not_finite(env):
    """four pairs: the second has NaN in A's last row (the corner itself is NaN), the third in a row in the middle (the rule's
    comparisons leave +inf in the corner); both have K = 0 and NaN maps, their neighbours equal the rule"""
    shapes = [(40, 31), (50, 66), (35, 35), (20, 70)]
    a_lens, fa, b_lens, fb = _random_batch(shapes, 60, 99)
    fa[40 + 49] = np.nan
    fa[40 + 50 + 17] = np.nan
    want = ar.align_batch(a_lens, fa, b_lens, fb, 1, 60)
    got = _align(env, a_lens, fa, b_lens, fb, 60, 1, 60, 0)
    _assert_equals_rule(got, want, a_lens, b_lens)
    cost, plen, _, boa, aob = got
    assert np.isnan(cost[1]) and cost[2] == np.inf and plen[1] == 0 and plen[2] == 0
    assert np.isnan(boa[40:40 + 50 + 35]).all() and np.isnan(aob[31:31 + 66 + 35]).all()
    assert np.isfinite(cost[[0, 3]]).all() and np.isfinite(boa[:40]).all() and np.isfinite(boa[125:145]).all()


def test_a_known_warp_needs_no_rule(env):
    """B repeats each of A's 50 distinct rows 1 to 4 times: the cost is exactly 0, a_on_b is the warp itself and b_on_a the middle of
    each row's stretch"""
    rng = np.random.default_rng(50)
    a = rng.standard_normal((50, 60))
    holds = 1 + (np.arange(50) * 7 + 3) % 4
    holds[[0, 49]] = [3, 4]
    g = np.repeat(np.arange(50), holds)
    m = len(g)
    assert 110 <= m <= 130 and set(holds) == {1, 2, 3, 4}
    cost, plen, path, boa, aob = _align(env, [50], a, [m], a[g], 60, 1, 60, 0)
    assert cost[0] == 0.0 and plen[0] == m
    assert np.array_equal(aob[:m], g.astype(np.float64))
    first = np.concatenate([[0], np.cumsum(holds)[:-1]])
    assert np.array_equal(boa[:50], (first + first + holds - 1) * 0.5)
    assert np.array_equal(path.reshape(-1, 2)[:m], np.stack([g, np.arange(m)], axis=1))


def test_chain_code_align_retime(env):
    """two utterances coded on the device, the coded rows aligned, d_b_on_a handed to wc_retime_parameters_device as it lies in HBM: B's
    parameters at A's timing equal tests/retime_rule.py at the rule's map bit for bit"""
    w, codec, wio, torch = env
    import retime_rule as rr
    from oracle.gen_golden import synth_params
    fs, fft, nd, na, nb = 16000, 1024, 60, 118, 127
    bins = fft // 2 + 1
    A, B = synth_params(fs, fft, na, 811), synth_params(fs, fft, nb, 812)
    d_A, d_B = [_dev(torch, v) for v in A], [_dev(torch, v) for v in B]
    d_ca, d_cb = torch.zeros(na * nd, dtype=torch.float64, device="cuda"), torch.zeros(nb * nd, dtype=torch.float64, device="cuda")
    outs = _outputs(torch, [na], [nb])
    r_f0 = torch.full((na + 1,), np.nan, dtype=torch.float64, device="cuda")
    r_sp, r_ap = (torch.full(((na + 1) * bins,), np.nan, dtype=torch.float64, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    codec.code_features_device(fs, fft, na, nd, d_A[1], None, d_ca, None)
    codec.code_features_device(fs, fft, nb, nd, d_B[1], None, d_cb, None)
    wio.align_features_device([na], d_ca, [nb], d_cb, nd, 1, nd, 0, *outs)
    wio.retime_parameters_device(fs, fft, [nb], d_B[0], d_B[1], d_B[2], [na], outs[3], None, None, r_f0, r_sp, r_ap)
    w.lib().wc_synchronize()
    ca, cb = d_ca.cpu().numpy().reshape(na, nd), d_cb.cpu().numpy().reshape(nb, nd)
    want = ar.align_batch([na], ca, [nb], cb, 1, nd)
    _assert_equals_rule([o.cpu().numpy() for o in outs], want, [na], [nb])
    f0, sp, ap = rr.retime(B[0], B[1], B[2], want[0]["b_on_a"])
    assert np.array_equal(r_f0.cpu().numpy()[:na], f0)
    assert np.array_equal(r_sp.cpu().numpy()[:na * bins].reshape(na, bins), sp)
    assert np.array_equal(r_ap.cpu().numpy()[:na * bins].reshape(na, bins), ap)
    assert np.isnan(r_f0.cpu().numpy()[na]) and np.isnan(r_sp.cpu().numpy()[na * bins:]).all()
    assert (np.diff(want[0]["b_on_a"]) > 0).any() and want[0]["cost"] > 0


def test_refused_calls_leave_the_outputs_untouched(env):
    w, codec, wio, torch = env
    L = w.lib()
    a_lens, fa, b_lens, fb = _random_batch([(9, 12), (6, 4)], 8, 5)
    d_a, d_b = _dev(torch, fa), _dev(torch, fb)
    outs = _outputs(torch, a_lens, b_lens)
    before = [o.clone() for o in outs]
    torch.cuda.synchronize()
    good = dict(n=2, al=a_lens, a=d_a, bl=b_lens, b=d_b, dims=8, lo=1, hi=8, band=0, cost=outs[0], plen=outs[1])
    ints = lambda v: None if v is None else (C.c_int * max(1, len(v)))(*v)
    ptr = lambda x: None if x is None else x.data_ptr()

    def call(**kw):
        g = dict(good, **kw)
        return wio._io().wc_align_features_device(g["n"], ints(g["al"]), ptr(g["a"]), ints(g["bl"]), ptr(g["b"]), g["dims"], g["lo"], g["hi"], g["band"],
                                                  ptr(g["cost"]), ptr(g["plen"]), outs[2].data_ptr(), outs[3].data_ptr(), outs[4].data_ptr())

    bad = [dict(n=-1), dict(al=[9, 0]), dict(bl=[0, 4]), dict(al=[-3, 6]), dict(dims=0), dict(dims=-8), dict(lo=-1), dict(hi=9), dict(lo=8), dict(lo=5, hi=5),
           dict(lo=6, hi=3), dict(band=-1), dict(al=None), dict(bl=None), dict(a=None), dict(b=None), dict(cost=None), dict(plen=None),
           dict(al=[20000, 6], bl=[20000, 4]),            # 4e8 cells without a band: above the cap of 2^28
           dict(al=[0x7fffffff, 6], bl=[0x7fffffff, 4]),  # (what no scratch could hold is refused by the same count)
           dict(al=[0x7fffffff, 6], bl=[0x7fffffff, 4], band=0x7ffffff0)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert w.last_error(), kw
    assert call(n=0) == 0 and call(n=0, al=None, a=None, bl=None, b=None, cost=None, plen=None) == 0  # no pairs: nothing to do
    L.wc_synchronize()
    for o, b4 in zip(outs, before):
        assert torch.equal(o, b4)
    assert call() == 0  # the arguments the bad ones were varied from are good
    L.wc_synchronize()
    _assert_equals_rule([o.cpu().numpy() for o in outs], ar.align_batch(a_lens, fa, b_lens, fb, 1, 8), a_lens, b_lens)


def test_host_convenience_equals_the_device_call(env):
    w, codec, wio, torch = env
    a_lens, fa, b_lens, fb = _random_batch([(57, 83)], 60, 57)
    for band, lo, hi in ((0, 1, None), (4, 0, 30)):
        cost, plen, path, boa, aob = _align(env, a_lens, fa, b_lens, fb, 60, lo, 60 if hi is None else hi, band)
        r = wio.align_features(fa, fb, dim_begin=lo, dim_end=hi, band=band)
        assert _bits(r["cost"]) == _bits(cost[0]) and r["path"].shape == (plen[0], 2)
        assert np.array_equal(r["path"], path.reshape(-1, 2)[:plen[0]])
        assert np.array_equal(r["b_on_a"], boa[:57]) and np.array_equal(r["a_on_b"], aob[:83])
    bad = fa.copy()
    bad[56] = np.nan
    r = wio.align_features(bad, fb)
    assert np.isnan(r["cost"]) and r["path"].shape == (0, 2) and np.isnan(r["b_on_a"]).all() and np.isnan(r["a_on_b"]).all()


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
                wio.align_features_device([na], d_ca, [nb], d_cb, nd, 1, nd, 0, *outs)
                kept.append((d_sa, d_sb, d_ca, d_cb, outs))
        s.synchronize()  # once
    finally:
        assert w.lib().wc_set_stream(None) == 0
    for (na, nb), (_, _, d_ca, d_cb, outs) in zip(lens, kept):
        ca, cb = d_ca.cpu().numpy().reshape(na, nd), d_cb.cpu().numpy().reshape(nb, nd)
        assert np.isfinite(ca).all() and np.isfinite(cb).all()
        _assert_equals_rule([o.cpu().numpy() for o in outs], ar.align_batch([na], ca, [nb], cb, 1, nd), [na], [nb])
        again = _align(env, [na], ca, [nb], cb, nd, 1, nd, 0)  # the same on the library's own stream
        for o, g in zip(outs, again):
            assert o.cpu().numpy().tobytes() == g.tobytes()
