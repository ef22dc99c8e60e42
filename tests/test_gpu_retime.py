"""-m gpu: time-scale modification (wc_retime_parameters_device, wc_synthesis_compute_coded_retimed_device): the rows and the
contour against the numpy restatement of the rule (tests/retime_rule.py) bit for bit, the fused scale / stretch against the
routed calls bit for bit, the independence of the frames, NULL pairs and refusals, ordering on the caller's stream, the coded
Synthesis call against the three calls it stands for, and the whole chain against the reference.  Outputs are NaN-filled with a
guard row behind them that must stay NaN."""
import ctypes as C

import numpy as np
import pytest

import retime_rule as rr

pytestmark = pytest.mark.gpu
Y_ABS = 1e-8        # the project's Synthesis tolerance (test_gpu_synth_coded.py)
ATOMIC_ABS = 1e-12  # the FP64-atomic overlap-add at fft 512 / 4096 (test_gpu_synth_coded.py)
SIZES = [(16000, 512), (24000, 1024), (48000, 2048), (96000, 4096)]
FRAMES = [61, 97, 74]


@pytest.fixture(scope="module")
def env():
    import torch
    import world_class_amd as w
    from world_class_amd import codec, io as wio
    w.lib().wc_set_device(0)
    return w, codec, wio, torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).ravel()).cuda()


def _guarded(torch, n, width):
    """n rows of NaN with a guard row of NaN behind them"""
    return torch.full(((n + 1) * width,), np.nan, dtype=torch.float64, device="cuda")


def _rows(t, n, width):
    a = t.cpu().numpy().reshape(n + 1, width)
    assert np.isnan(a[n]).all(), "the guard row was written"
    return a[:n]


def _retime(env, fs, fft, lengths, f0, sp, ap, out_lengths, pos, scale=None, ratio=None, parts=(True, True, True)):
    """wc_retime_parameters_device into NaN-filled, guarded outputs: (f0, sp, ap), None for a pair that was left out"""
    w, codec, wio, torch = env
    bins, m = fft // 2 + 1, int(sum(out_lengths))
    ins = [_dev(torch, a) if on else None for a, on in zip((f0, sp, ap), parts)]
    outs = [_guarded(torch, m, wd) if on else None for wd, on in zip((1, bins, bins), parts)]
    opt = lambda a: None if a is None else _dev(torch, a)
    torch.cuda.synchronize()
    wio.retime_parameters_device(fs, fft, lengths, ins[0], ins[1], ins[2], out_lengths, _dev(torch, pos), opt(scale), opt(ratio), *outs)
    w.lib().wc_synchronize()
    got = [None if o is None else _rows(o, m, wd) for o, wd in zip(outs, (1, bins, bins))]
    return (None if got[0] is None else got[0][:, 0]), got[1], got[2]


def _batch(fs, fft, seed, first_map):
    """three ragged utterances (61 / 97 / 74 source frames) with a different kind of map each and positions that are not finite
    sprinkled in: lengths, f0, sp, ap, out_lengths, pos"""
    from oracle.gen_golden import synth_params
    parts = [synth_params(fs, fft, n, seed + u) for u, n in enumerate(FRAMES)]
    maps = [rr.map_of(rr.MAPS[(first_map + u) % len(rr.MAPS)], n) for u, n in enumerate(FRAMES)]
    maps[0][[4, 40]] = [np.nan, -np.inf]
    maps[1][[0, len(maps[1]) - 1]] = [np.inf, np.nan]
    maps[2][17] = np.nan
    return (FRAMES, np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]),
            [len(p) for p in maps], np.concatenate(maps))


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


# ---- 3. rows and contour against the numpy restatement ----------------------------------------------------------------------

@pytest.mark.parametrize("k,fs,fft", [(k, fs, fft) for k, (fs, fft) in enumerate(SIZES)])
def test_rows_equal_the_rule_bit_for_bit(env, k, fs, fft):
    """no tolerance: the build keeps every product and sum apart (-ffp-contract=off), so numpy's expression gives the kernel's bits.
    The four sizes start the list of maps three places apart: every map is met"""
    lengths, f0, sp, ap, out_lengths, pos = _batch(fs, fft, 3100 + fft, 3 * k)
    want = rr.retime_batch(lengths, f0, sp, ap, out_lengths, pos)
    got = _retime(env, fs, fft, lengths, f0, sp, ap, out_lengths, pos)
    bad = ~np.isfinite(pos)
    assert bad.sum() == 5
    for g, w_ in zip(got, want):
        assert _same(g, w_)
        assert np.isnan(g[bad]).all() and np.isfinite(g[~bad]).all()
    assert (got[0] == 0).any() and (got[0] > 0).any()  # (voiced and unvoiced stretches both occur)
    scale = 0.5 + np.arange(len(pos)) / 256.0
    scale[9] = np.nan
    got_s = _retime(env, fs, fft, lengths, f0, sp, ap, out_lengths, pos, scale=scale)
    assert _same(got_s[0], rr.retime_batch(lengths, f0, sp, ap, out_lengths, pos, scale)[0]) and np.isnan(got_s[0][9])
    assert _same(got_s[1], want[1]) and _same(got_s[2], want[2])


# ---- 4. fused against routed ------------------------------------------------------------------------------------------------

def _ratios_with_bad(fft, m):
    ratio = rr.cycled(fft, m, 2)
    ratio[[3, 50, 101, m - 1]] = [-1.0, np.nan, np.inf, 1.0 / fft]
    return ratio


@pytest.mark.parametrize("k,fs,fft", [(k, fs, fft) for k, (fs, fft) in enumerate(SIZES)])
def test_scale_and_ratio_equal_the_routed_calls_bit_for_bit(env, k, fs, fft):
    """with d_f0_scale and d_spectral_ratio the call equals itself without them followed by wc_modify_parameters_frames_device on
    its outputs: the eight ratios of test_gpu_modify_frames.py cycled over the output frames, four bad ones among them"""
    w, codec, wio, torch = env
    lengths, f0, sp, ap, out_lengths, pos = _batch(fs, fft, 4100 + fft, 3 * k + 1)
    m, bins = sum(out_lengths), fft // 2 + 1
    ratio = _ratios_with_bad(fft, m)
    scale = 0.8 + (np.arange(m) % 17) / 20.0
    plain = _retime(env, fs, fft, lengths, f0, sp, ap, out_lengths, pos)
    d_f0, d_sp = _dev(torch, plain[0]), _dev(torch, plain[1])
    wio.modify_parameters_frames_device(fs, fft, m, d_f0, d_sp, _dev(torch, scale), _dev(torch, ratio))
    w.lib().wc_synchronize()
    want_f0, want_sp = d_f0.cpu().numpy(), d_sp.cpu().numpy().reshape(m, bins)
    got = _retime(env, fs, fft, lengths, f0, sp, ap, out_lengths, pos, scale=scale, ratio=ratio)
    assert _same(got[0], want_f0) and _same(got[1], want_sp) and _same(got[2], plain[2])
    ok = np.isfinite(pos)
    assert np.isnan(got[1][[3, 50, 101, m - 1]]).all()
    assert np.array_equal(got[1][ok & (ratio == 0.0)], plain[1][ok & (ratio == 0.0)])
    assert np.abs(got[1][ok & (ratio == 1.2)] / plain[1][ok & (ratio == 1.2)] - 1).max() > 1e-3  # (the stretch does change rows)
    # either array alone
    only_r = _retime(env, fs, fft, lengths, f0, sp, ap, out_lengths, pos, ratio=ratio)
    assert _same(only_r[0], plain[0]) and _same(only_r[1], want_sp)
    only_s = _retime(env, fs, fft, lengths, f0, sp, ap, out_lengths, pos, scale=scale)
    assert _same(only_s[0], want_f0) and _same(only_s[1], plain[1])


# ---- 5. a frame depends on its own position and its two source rows alone ---------------------------------------------------

@pytest.mark.parametrize("fs,fft", [(24000, 1024), (48000, 2048)])
def test_frames_depend_on_their_own_position_alone(env, fs, fft):
    from oracle.gen_golden import synth_params
    n = 97
    f0, sp, ap = synth_params(fs, fft, n, 5100)
    pos = rr.map_of("hold_and_back", n)
    pos[[7, 60]] = [np.nan, np.inf]
    m = len(pos)
    ratio, scale = _ratios_with_bad(fft, m), 0.8 + (np.arange(m) % 13) / 16.0
    base = _retime(env, fs, fft, [n], f0, sp, ap, [m], pos, scale, ratio)
    rev = _retime(env, fs, fft, [n], f0, sp, ap, [m], pos[::-1], scale[::-1], ratio[::-1])
    for b, r in zip(base, rev):
        assert _same(r, b[::-1])
    for k in (0, 1, 7, 29, 30, 49, 50, 63, 64, m - 2, m - 1):
        one = _retime(env, fs, fft, [n], f0, sp, ap, [1], pos[k:k + 1], scale[k:k + 1], ratio[k:k + 1])
        for b, o in zip(base, one):
            assert _same(o[0], b[k]), k
    f0b, spb, apb = synth_params(fs, fft, 87, 5200)
    posb = rr.map_of("slow_1.37", 50)
    lengths, out_lengths = [37, n, 50], [len(posb), m, 20]
    emb = _retime(env, fs, fft, lengths, np.concatenate([f0b[:37], f0, f0b[37:]]), np.concatenate([spb[:37], sp, spb[37:]]),
                  np.concatenate([apb[:37], ap, apb[37:]]), out_lengths, np.concatenate([np.minimum(posb, 36), pos, posb[:20]]),
                  np.concatenate([np.ones(len(posb)), scale, np.ones(20)]), np.concatenate([rr.cycled(fft, len(posb)), ratio, rr.cycled(fft, 20, 5)]))
    for b, e in zip(base, emb):
        assert _same(e[len(posb):len(posb) + m], b)


# ---- 6. NULL pairs, empty calls, refusals -----------------------------------------------------------------------------------

def test_null_pairs_and_empty_calls(env):
    w, codec, wio, torch = env
    fs, fft = 24000, 1024
    lengths, f0, sp, ap, out_lengths, pos = _batch(fs, fft, 6100, 2)
    m = sum(out_lengths)
    ratio, scale = rr.cycled(fft, m, 1), np.full(m, 1.1)
    full = _retime(env, fs, fft, lengths, f0, sp, ap, out_lengths, pos, scale, ratio)
    for parts in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        got = _retime(env, fs, fft, lengths, f0, sp, ap, out_lengths, pos, scale, ratio, parts=parts)
        for on, g, f in zip(parts, got, full):
            assert (g is None) if not on else _same(g, f)
    # an utterance without output frames in the middle (its source may be empty too), and a call without any
    l2, o2 = [lengths[0], 0, lengths[1], 5, lengths[2]], [out_lengths[0], 0, out_lengths[1], 0, out_lengths[2]]
    f0x = np.concatenate([f0[:158], np.zeros(5), f0[158:]])
    spx, apx = (np.concatenate([a[:158], np.ones((5, a.shape[1])), a[158:]]) for a in (sp, ap))
    holes = _retime(env, fs, fft, l2, f0x, spx, apx, o2, pos, scale, ratio)
    for h, f in zip(holes, full):
        assert _same(h, f)
    none = _retime(env, fs, fft, lengths, f0, sp, ap, [0, 0, 0], np.zeros(1))
    assert all(len(a) == 0 for a in none)
    empty = _retime(env, fs, fft, [], f0, sp, ap, [], np.zeros(1))
    assert all(len(a) == 0 for a in empty)
    # all three pairs NULL: accepted, nothing to do
    wio.retime_parameters_device(fs, fft, lengths, None, None, None, out_lengths, _dev(torch, pos))


def test_refused_calls_leave_the_outputs_untouched(env):
    w, codec, wio, torch = env
    from oracle.gen_golden import synth_params
    L = w.lib()
    fs, fft, n, m = 48000, 2048, 8, 11
    bins = fft // 2 + 1
    f0, sp, ap = synth_params(fs, fft, n, 6200)
    d_f0, d_sp, d_ap, d_pos = _dev(torch, f0), _dev(torch, sp), _dev(torch, ap), _dev(torch, np.linspace(0, n - 1, m))
    d_one = _dev(torch, np.ones(m))
    o_f0, o_sp, o_ap = _guarded(torch, m, 1), _guarded(torch, m, bins), _guarded(torch, m, bins)
    torch.cuda.synchronize()
    good = dict(fs=fs, fft=fft, n_utt=1, il=[n], f0=d_f0, sp=d_sp, ap=d_ap, ol=[m], pos=d_pos, of0=o_f0, osp=o_sp, oap=o_ap)
    ints = lambda v: None if v is None else (C.c_int * max(1, len(v)))(*v)
    ptr = lambda a: None if a is None else (a if isinstance(a, int) else a.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return wio._io().wc_retime_parameters_device(a["fs"], a["fft"], a["n_utt"], ints(a["il"]), ptr(a["f0"]), ptr(a["sp"]), ptr(a["ap"]), ints(a["ol"]),
                                                     ptr(a["pos"]), d_one.data_ptr(), d_one.data_ptr(), ptr(a["of0"]), ptr(a["osp"]), ptr(a["oap"]))

    bad = [dict(fft=3000), dict(fft=8192), dict(fft=256), dict(fs=0), dict(fs=-48000), dict(n_utt=-1), dict(il=[0]), dict(il=[-1]), dict(ol=[-1]),
           dict(n_utt=2, il=[n, 0], ol=[m, 1]), dict(n_utt=3, il=[n, n, n], ol=[0x7fffffff, 0x7fffffff, 2]),
           dict(n_utt=3, il=[0x7fffffff, 0x7fffffff, 2], ol=[m, 0, 0]), dict(il=None), dict(ol=None), dict(pos=None),
           dict(f0=None), dict(of0=None), dict(sp=None), dict(osp=None), dict(ap=None), dict(oap=None),
           dict(of0=d_f0), dict(osp=d_sp), dict(oap=d_ap)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert w.last_error(), kw
    L.wc_synchronize()
    assert bool(torch.isnan(o_f0).all()) and bool(torch.isnan(o_sp).all()) and bool(torch.isnan(o_ap).all())
    assert np.array_equal(d_f0.cpu().numpy(), f0) and np.array_equal(d_sp.cpu().numpy().reshape(n, bins), sp)
    with pytest.raises(w.WorldClassError):
        wio.retime_parameters_device(fs, 3000, [n], d_f0, d_sp, d_ap, [m], d_pos, None, None, o_f0, o_sp, o_ap)
    with pytest.raises(ValueError):
        wio.retime_parameters_device(fs, fft, [n, n], d_f0, d_sp, d_ap, [m], d_pos, None, None, o_f0, o_sp, o_ap)
    assert call() == 0  # (the same arguments, nothing wrong: accepted)
    L.wc_synchronize()
    assert np.isfinite(_rows(o_sp, m, bins)).all()

    # the coded Synthesis call: its own refusals and those of the two calls it stands for; rng_pos and d_out stay
    nd = 20
    from oracle import port_codec as pc
    csp, cap = pc.code_spectral_envelope(sp, fs, fft, nd), pc.code_aperiodicity(ap, fs, fft)
    d_csp, d_cap = _dev(torch, csp), _dev(torch, cap)
    syn, syn8 = w.Synthesis(fs, fft, 5.0), w.Synthesis(8000, 1024, 5.0)
    ol = [syn.out_length(m)]
    y = torch.full((ol[0],), np.nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g2 = dict(h=syn, n_utt=1, f0=d_f0, fl=[n], csp=d_csp, nd=nd, cap=d_cap, fo=[m], pos=d_pos, ol=ol, y=y)
    for kw in (dict(nd=0), dict(nd=fft // 2 + 1), dict(h=syn8), dict(csp=None), dict(cap=None), dict(f0=None), dict(fl=None), dict(fo=None),
               dict(pos=None), dict(ol=None), dict(y=None), dict(n_utt=0), dict(fl=[1]), dict(fo=[1]), dict(fo=[0]), dict(fo=[-3]), dict(ol=[-1])):
        a = dict(g2, **kw)
        rng = (C.c_uint64 * 1)(5)
        rc = L.wc_synthesis_compute_coded_retimed_device(a["h"]._h, a["n_utt"], ptr(a["f0"]), ints(a["fl"]), ptr(a["csp"]), a["nd"], ptr(a["cap"]),
                                                         ints(a["fo"]), ptr(a["pos"]), d_one.data_ptr(), d_one.data_ptr(), ints(a["ol"]), ptr(a["y"]), rng)
        assert rc == -1 and w.last_error(), kw
        assert list(rng) == [5], kw
    L.wc_synchronize()
    assert bool(torch.isnan(y).all())


# ---- 7. ordering on the caller's stream -------------------------------------------------------------------------------------

def test_retime_is_ordered_on_the_callers_stream(env):
    """a long torch kernel in front on a torch stream handed over by wc_set_stream; the rows, the positions and the two per-frame
    arrays written by torch kernels on that stream; four (fs, fft) combinations interleaved, twice; one synchronisation at the end"""
    w, codec, wio, torch = env
    combos = [(48000, 2048), (24000, 1024), (16000, 512), (96000, 4096)]
    data, want = [], []
    for k, (fs, fft) in enumerate(combos):
        lengths, f0, sp, ap, out_lengths, pos = _batch(fs, fft, 7100 + fft, k)
        m = sum(out_lengths)
        ratio, scale = rr.cycled(fft, m, k), 0.9 + (np.arange(m) % 5) / 10.0
        data.append((lengths, out_lengths, (f0, sp, ap, pos, scale, ratio)))
        want.append(_retime(env, fs, fft, lengths, f0, sp, ap, out_lengths, pos, scale, ratio))
    host = [tuple(torch.from_numpy(np.ascontiguousarray(a).ravel().copy()).pin_memory() for a in d[2]) for d in data]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert w.lib().wc_set_stream(s.cuda_stream) == 0
    try:
        outs = []
        with torch.cuda.stream(s):
            junk = torch.randn(2048, 2048, device="cuda")
            for _ in range(20):  # a long-running kernel in front: the call must wait for it and for the uploads behind it
                junk = junk @ junk * 1e-3
            for rnd in range(2):
                for (fs, fft), (lengths, out_lengths, _), h in zip(combos, data, host):
                    bins, m = fft // 2 + 1, sum(out_lengths)
                    d = [torch.zeros(len(a), dtype=torch.float64, device="cuda") for a in h]
                    o = [_guarded(torch, m, 1), _guarded(torch, m, bins), _guarded(torch, m, bins)]
                    for dst, src in zip(d, h):
                        dst.copy_(src, non_blocking=True)
                        dst.mul_(1.0)  # torch kernels on the stream write every input
                    wio.retime_parameters_device(fs, fft, lengths, d[0], d[1], d[2], out_lengths, d[3], d[4], d[5], *o)
                    outs.append((o, d))
        s.synchronize()  # once
    finally:
        assert w.lib().wc_set_stream(None) == 0
    for i, (o, _) in enumerate(outs):
        fft, m = combos[i % 4][1], sum(data[i % 4][1])
        got = (_rows(o[0], m, 1)[:, 0], _rows(o[1], m, fft // 2 + 1), _rows(o[2], m, fft // 2 + 1))
        for g, w_ in zip(got, want[i % 4]):
            assert _same(g, w_), i


# ---- 8. batch Synthesis from coded rows -------------------------------------------------------------------------------------

def _coded_rows(env, fs, fft, n, seed, nd):
    """seeded rows (oracle/gen_golden.synth_params) coded on the device: f0, coded sp, coded ap as host arrays"""
    w, codec, wio, torch = env
    from oracle.gen_golden import synth_params
    f0, sp, ap = synth_params(fs, fft, n, seed)
    n_ap = codec.number_of_aperiodicities(fs)
    d_csp = torch.empty(n * nd, dtype=torch.float64, device="cuda")
    d_cap = torch.empty(n * n_ap, dtype=torch.float64, device="cuda")
    codec.code_spectral_envelope_device(fs, fft, n, nd, _dev(torch, sp), d_csp)
    codec.code_aperiodicity_device(fs, fft, n, _dev(torch, ap), d_cap)
    w.lib().wc_synchronize()
    return f0, d_csp.cpu().numpy().reshape(n, nd), d_cap.cpu().numpy().reshape(n, n_ap)


@pytest.mark.parametrize("fs,fft", [(24000, 1024), (48000, 2048), (16000, 512), (96000, 4096)])
def test_compute_coded_retimed_equals_decode_retime_synthesis(env, fs, fft):
    """compute_coded_retimed_device == decode_features_device -> retime_parameters_device -> compute_device with the same noise
    positions (bit for bit at fft 1024 / 2048, within ATOMIC_ABS at 512 / 4096, where Synthesis adds with FP64 atomics), ends at
    the same noise positions, and with the identity map and no scale / ratio it is compute_coded_device bit for bit"""
    w, codec, wio, torch = env
    nd = 40
    parts = [_coded_rows(env, fs, fft, n, 8100 + u, nd) for u, n in enumerate(FRAMES)]
    f0, csp, cap = (np.concatenate([p[q] for p in parts]) for q in range(3))
    maps = [rr.map_of(name, n) for name, n in zip(("ramp", "half_speed", "hold_and_back"), FRAMES)]
    fo, pos = [len(p) for p in maps], np.concatenate(maps)
    m, tot, bins = sum(fo), sum(FRAMES), fft // 2 + 1
    ratio = np.concatenate([np.full(fo[0], 1.15), np.linspace(0.8, 1.25, fo[1]), np.where(np.arange(fo[2]) % 9 < 4, 0.0, 0.9)])
    scale = np.concatenate([np.full(fo[0], 0.9), np.linspace(0.8, 1.3, fo[1]), np.ones(fo[2])])
    same = (lambda a, b: np.array_equal(a, b)) if fft in (1024, 2048) else (lambda a, b: len(a) == len(b) and np.abs(a - b).max() < ATOMIC_ABS)
    syn = w.Synthesis(fs, fft, 5.0)
    start = [1000 * u + 7 for u in range(3)]
    d_f0, d_csp, d_cap, d_pos, d_ratio, d_scale = (_dev(torch, a) for a in (f0, csp, cap, pos, ratio, scale))

    def run(ol, fn):
        y = torch.full((sum(ol) + 1,), np.nan, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        end = fn(y)
        w.lib().wc_synchronize()
        y = y.cpu().numpy()
        assert np.isnan(y[-1])
        return y[:-1], end

    ol = [syn.out_length(k) for k in fo]
    d_sp, d_ap = (torch.empty(tot * bins, dtype=torch.float64, device="cuda") for _ in range(2))
    r_f0, r_sp, r_ap = _guarded(torch, m, 1), _guarded(torch, m, bins), _guarded(torch, m, bins)
    codec.decode_features_device(fs, fft, tot, nd, d_csp, d_cap, d_sp, d_ap)
    wio.retime_parameters_device(fs, fft, FRAMES, d_f0, d_sp, d_ap, fo, d_pos, d_scale, d_ratio, r_f0, r_sp, r_ap)
    y_ref, end_ref = run(ol, lambda y: syn.compute_device(r_f0, fo, r_sp, r_ap, ol, y, rng_pos=start))
    y, end = run(ol, lambda y: syn.compute_coded_retimed_device(d_f0, FRAMES, d_csp, nd, d_cap, fo, d_pos, d_scale, d_ratio, ol, y, rng_pos=start))
    assert end == end_ref and end != start
    assert np.isfinite(y).all() and same(y, y_ref)
    y_none, end_none = run(ol, lambda y: syn.compute_coded_retimed_device(d_f0, FRAMES, d_csp, nd, d_cap, fo, d_pos, None, None, ol, y, rng_pos=start))
    assert np.isfinite(y_none).all() and np.abs(y - y_none).max() > 1e-6  # (scale and ratio do change the waveform)
    # the identity map
    ol1 = [syn.out_length(n) for n in FRAMES]
    d_id = _dev(torch, np.concatenate([np.arange(n, dtype=np.float64) for n in FRAMES]))
    y_plain, end_plain = run(ol1, lambda y: syn.compute_coded_device(d_f0, FRAMES, d_csp, nd, d_cap, ol1, y, rng_pos=start))
    y_id, end_id = run(ol1, lambda y: syn.compute_coded_retimed_device(d_f0, FRAMES, d_csp, nd, d_cap, FRAMES, d_id, None, None, ol1, y, rng_pos=start))
    assert end_id == end_plain and same(y_id, y_plain)
    assert np.isfinite(y_plain).all()


# ---- 9. against the reference -----------------------------------------------------------------------------------------------

def _port_frames(fs, fft, sp, ratio):
    """oracle.port_io.parameter_modification frame by frame, with that frame's ratio (0 = none)"""
    from oracle import port_io
    out = np.array(sp, dtype=np.float64)
    for i, r in enumerate(ratio):
        if r != 0.0:
            out[i] = port_io.parameter_modification(fs, fft, np.zeros(1), sp[i:i + 1], None, float(r))[1][0]
    return out


def reference_case(fs, fft, name, nd=60):
    """f0, coded rows, the map, scale and ratio per output frame, and what the reference's chain makes of them up to Synthesis'
    inputs: 120 frames of synth_params coded and decoded by oracle/port_codec, retimed by the numpy restatement, stretched frame by
    frame by oracle.port_io.  F0 scales stay within 0.8 .. 1.6 (the reference's Synthesis has a fixed pulse capacity)."""
    from oracle import port_codec as pc
    from oracle.gen_golden import synth_params
    n = 120
    f0, sp, ap = synth_params(fs, fft, n, 5000 + fs // 1000)
    csp, cap = pc.code_spectral_envelope(sp, fs, fft, nd), pc.code_aperiodicity(ap, fs, fft)
    sp_d, ap_d = pc.decode_spectral_envelope(csp, fs, fft), pc.decode_aperiodicity(cap, fs, fft)
    pos = rr.map_of(name, n)
    m = len(pos)
    scale = np.linspace(0.8, 1.6, m) if name == "half_speed" else 1.0 + 0.2 * np.sin(np.arange(m) / 7.0)
    ratio = np.linspace(0.8, 1.25, m)
    ratio[::11] = 0.0
    f0_r, sp_r, ap_r = rr.retime(f0, sp_d, ap_d, pos, scale)
    return f0, csp, cap, pos, scale, ratio, f0_r, _port_frames(fs, fft, sp_r, ratio), ap_r


@pytest.mark.parametrize("name", rr.MAPS)
@pytest.mark.parametrize("fs,fft", [(16000, 1024), (48000, 2048)])
def test_compute_coded_retimed_matches_the_reference_chain(env, port, checker, fs, fft, name):
    """the reference's chain synthesised from noise position 0 by the reference (the real one where oracle/_ref is built,
    oracle/port.py otherwise): the device call on the coded rows, the map, the scales and the ratios within 1e-8, the project's
    Synthesis tolerance, with equal length and equal final noise position"""
    w, codec, wio, torch = env
    nd = 60
    f0, csp, cap, pos, scale, ratio, f0_r, sp_r, ap_r = reference_case(fs, fft, name, nd)
    n, m = len(f0), len(pos)
    port.rng_seek(0)
    y_ref = port.synthesis(f0_r, sp_r, ap_r, fs, 5.0)
    end = port.rng_position()
    if checker is not None:
        y_ref = checker.stage_at(0, "synthesis", f0_r, sp_r, ap_r, fs, 5.0)
    assert np.isfinite(y_ref).all()
    syn = w.Synthesis(fs, fft, 5.0)
    ol = syn.out_length(m)
    assert ol == len(y_ref)
    y = torch.full((ol + 1,), np.nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    got_end = syn.compute_coded_retimed_device(_dev(torch, f0), [n], _dev(torch, csp), nd, _dev(torch, cap), [m], _dev(torch, pos), _dev(torch, scale),
                                               _dev(torch, ratio), [ol], y, rng_pos=[0])
    w.lib().wc_synchronize()
    y = y.cpu().numpy()
    assert np.isnan(y[-1]) and got_end == [end]
    err = np.abs(y[:-1] - y_ref).max()
    print("compute_coded_retimed against the reference chain, fs %d, %s: %.3e (peak %.2f)" % (fs, name, err, np.abs(y_ref).max()))
    assert err < Y_ABS
    assert checker is None or not checker.fell_back


def test_numpy_front_end(env):
    """io.retime_parameters: one utterance, numpy in and out, scalars broadcast over the output frames"""
    w, codec, wio, torch = env
    from oracle.gen_golden import synth_params
    fs, fft, n = 24000, 1024, 61
    f0, sp, ap = synth_params(fs, fft, n, 9100)
    pos = wio.time_map(n, 0.75)
    got = wio.retime_parameters(f0, sp, ap, pos, fs, fft)
    for g, w_ in zip(got, rr.retime(f0, sp, ap, pos)):
        assert _same(g, w_)
    scale, ratio = np.full(len(pos), 1.25), np.full(len(pos), 0.9)
    want = _retime(env, fs, fft, [n], f0, sp, ap, [len(pos)], pos, scale, ratio)
    got = wio.retime_parameters(f0, sp, ap, pos, fs, fft, f0_scale=1.25, spectral_ratio=0.9)
    for g, w_ in zip(got, want):
        assert _same(g, w_)
