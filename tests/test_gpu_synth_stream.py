"""-m gpu: chunked Synthesis for many concurrent streams (include/world_class_stream.h, wc_synth_stream_*) against ONE whole-utterance
Synthesis call per stream: bit for bit at fft_size 1024 / 2048 (the same response rows summed in the same order), within 1e-12 at
512 / 4096 (FP64 atomics in the batch's block kernels), and the accounting the header states."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Y_ABS = 1e-8


@pytest.fixture(scope="module")
def wca():
    import world_class_amd as w
    w.lib()
    return w


def _batch(wca, fs, fft, fp, params, rng_pos=None):
    s = wca.Synthesis(fs, fft, fp)
    ys = s.compute_batch([p[0] for p in params], [p[1] for p in params], [p[2] for p in params],
                         rng_pos=list(rng_pos) if rng_pos is not None else [0] * len(params))
    return ys[0] if isinstance(ys, tuple) else ys


def _gap(fs, fft):
    lowest = fs // fft + 1.0
    return int(np.ceil(max(2.0 * fs / lowest, fs / 500.0))) + 4


def _stream(wca, fs, fft, fp, params, pattern, max_frames=None, check_latency=True):
    from world_class_amd.stream import StreamSynthesizer
    n = len(params)
    mf = max_frames or max(max(p) for p in pattern)
    st = StreamSynthesizer(fs, fft, fp, n, mf)
    got = [0] * n

    def on_push(u, c):
        got[u] += c
        assert st.samples_committed(u) == got[u]
        F = st.frames_received(u)
        if check_latency and F >= 2 and F < len(params[u][0]):  # not yet flushed: the header's latency bound
            assert got[u] >= (F - 2) * fp / 1000.0 * fs - _gap(fs, fft) - fft // 2, (u, F, got[u])

    ys = st.run_whole(params, pattern, on_push)
    for u, (f0, _, _) in enumerate(params):
        assert len(ys[u]) == wca.synthesis_out_length(len(f0), fp, fs)
    return ys, st


def _params(fs, fft, frames, seed, unvoiced=None, end_unvoiced=False):
    from oracle.gen_golden import synth_params
    f0, sp, ap = synth_params(fs, fft, frames, seed)
    if unvoiced is not None:
        f0[unvoiced] = 0.0
        ap[unvoiced] = 1.0 - 1e-12
    if end_unvoiced:
        f0[-2] = 140.0
        f0[-1] = 0.0
        ap[-1] = 1.0 - 1e-12
    return f0, sp, ap


def test_synth_stream_golden_48k_sixteen_ragged_streams(wca):
    """BASELINE config 4's fixture (tests/golden/synth_only_48k_10s.npz, the real reference's waveforms): the sixteen utterances
    pushed into sixteen streams in ragged frame counts with idle pushes; y bit for bit the batch call, within 1e-8 of the fixture."""
    from oracle.gen_golden import synth_params
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "synth_only_48k_10s.npz"))
    fs, fft, frames, fp, n_utt, first_seed, block, win = [int(v) for v in z["meta"]]
    params = [synth_params(fs, fft, frames, first_seed + u) for u in range(n_utt)]
    shapes = [[1, 7, 40, 333], [333, 0, 1], [7, 0, 0, 40], [200], [1], [13, 97, 0], [40, 7, 1, 0, 333], [64, 128],
              [3, 0, 300], [250, 1, 1], [99], [5, 55, 0, 155], [333, 333, 0], [17], [2, 0, 71], [111, 0]]
    ys, _ = _stream(wca, fs, fft, float(fp), params, shapes, max_frames=333)
    ref = _batch(wca, fs, fft, float(fp), params)
    worst = 0.0
    for u, y in enumerate(ys):
        assert np.array_equal(y, ref[u]), u
        k = "u%d/" % u
        assert len(y) == int(z[k + "y_len"][0])
        for st_, w in zip(z[k + "y_win_start"], z[k + "y_win"]):
            worst = max(worst, float(np.abs(y[st_:st_ + win] - w).max()))
        nb = len(y) // block
        assert np.abs(y[:nb * block].reshape(nb, block).sum(1) - z[k + "y_blocksum"]).max() < Y_ABS * block
    assert worst < Y_ABS, worst


@pytest.mark.parametrize("fs,fp", [(16000, 5.0), (24000, 1.0)])
def test_synth_stream_bit_identical_to_the_batch_at_fft_1024(wca, fs, fp):
    fft = 1024
    frames = int(round(600 / fp))
    params = [_params(fs, fft, frames, 71),                                      # one frame per push: pulses on every boundary
              _params(fs, fft, frames, 72, unvoiced=slice(frames // 5, frames // 2)),  # a long unvoiced stretch
              _params(fs, fft, frames + 3, 73, end_unvoiced=True),                # voiced -> unvoiced at the end: the extrapolated point
              _params(fs, fft, frames - 7, 74)]
    pattern = [[1], [3, 0, 11], [1, 2, 0, 37], [frames]]
    ys, _ = _stream(wca, fs, fft, fp, params, pattern)
    ref = _batch(wca, fs, fft, fp, params)
    for u in range(len(params)):
        assert np.array_equal(ys[u], ref[u]), (u, np.abs(ys[u] - ref[u]).max())


@pytest.mark.parametrize("fs,fft,fp", [(8000, 512, 5.0), (96000, 4096, 5.0)])
def test_synth_stream_atomic_sizes_against_batch_and_oracle(wca, port, fs, fft, fp):
    frames = 90
    params = [_params(fs, fft, frames, 81), _params(fs, fft, frames, 82, unvoiced=slice(10, 40), end_unvoiced=True)]
    ys, _ = _stream(wca, fs, fft, fp, params, [[1, 4, 0], [9, 2]])
    ref = _batch(wca, fs, fft, fp, params)
    for u, (f0, sp, ap) in enumerate(params):
        assert np.abs(ys[u] - ref[u]).max() <= 1e-12
        port.rng_seek(0)
        yo = port.synthesis(f0, sp, ap, fs, fp)
        assert np.abs(ys[u] - yo).max() < Y_ABS
    port.rng_reset()


def test_synth_stream_accounting_idle_reset_flush_and_failed_push(wca):
    from world_class_amd.stream import StreamSynthesizer
    fs, fft, fp = 16000, 1024, 5.0
    p = [_params(fs, fft, 60, 91), _params(fs, fft, 60, 92)]
    ref = _batch(wca, fs, fft, fp, p)
    st = StreamSynthesizer(fs, fft, fp, 2, 16)
    e = lambda: np.zeros((0, fft // 2 + 1))
    acc = [[], []]
    # stream 1 idle while stream 0 runs ahead
    for k in range(0, 30, 10):
        r = st.push([p[0][0][k:k + 10], []], [p[0][1][k:k + 10], e()], [p[0][2][k:k + 10], e()])
        acc[0].append(r[0])
        assert len(r[1]) == 0
    assert st.frames_received(1) == 0 and st.samples_committed(1) == 0
    # a push with too many frames fails and changes nothing
    with pytest.raises(Exception):
        st.push([p[0][0][30:47], p[1][0][:3]], [p[0][1][30:47], p[1][1][:3]], [p[0][2][30:47], p[1][2][:3]])
    assert st.frames_received(0) == 30 and st.frames_received(1) == 0
    # flushing a stream with fewer than two frames is an error, and leaves the other stream where it was
    with pytest.raises(Exception):
        st.push([p[0][0][30:40], p[1][0][:1]], [p[0][1][30:40], p[1][1][:1]], [p[0][2][30:40], p[1][2][:1]], flush=[0, 1])
    assert st.frames_received(0) == 30 and st.samples_committed(0) == sum(len(a) for a in acc[0])
    # the rest in ragged pushes; every sample once, in order
    for k in range(30, 60, 15):
        last = k + 15 >= 60
        r = st.push([p[0][0][k:k + 15], p[1][0][k - 30:k - 15]], [p[0][1][k:k + 15], p[1][1][k - 30:k - 15]],
                    [p[0][2][k:k + 15], p[1][2][k - 30:k - 15]], flush=[1 if last else 0, 0])
        acc[0].append(r[0])
        acc[1].append(r[1])
    y0 = np.concatenate(acc[0])
    assert np.array_equal(y0, ref[0])
    # a flushed stream takes no more frames until it is reset
    with pytest.raises(Exception):
        st.push([p[0][0][:2], []], [p[0][1][:2], e()], [p[0][2][:2], e()])
    for k in (30, 45):
        r = st.push([[], p[1][0][k:k + 15]], [e(), p[1][1][k:k + 15]], [e(), p[1][2][k:k + 15]], flush=[0, 1 if k == 45 else 0])
        acc[1].append(r[1])
    assert np.array_equal(np.concatenate(acc[1]), ref[1])
    # reset: the stream starts again from frame 0 and noise position 0
    st.reset(0)
    assert st.frames_received(0) == 0 and st.rng_position(0) == 0
    ys = []
    for k in range(0, 60, 12):
        r = st.push([p[1][0][k:k + 12], []], [p[1][1][k:k + 12], e()], [p[1][2][k:k + 12], e()], flush=[1 if k + 12 >= 60 else 0, 0])
        ys.append(r[0])
    assert np.array_equal(np.concatenate(ys), ref[1])


def test_synth_stream_noise_positions_carry_and_may_lie_far_apart(wca):
    from world_class_amd.stream import StreamSynthesizer
    fs, fft, fp = 24000, 1024, 1.0
    p = [_params(fs, fft, 300, 101), _params(fs, fft, 300, 102)]
    starts = [12345, (1 << 40) + 777]
    ref, ends = wca.Synthesis(fs, fft, fp).compute_batch([q[0] for q in p], [q[1] for q in p], [q[2] for q in p], rng_pos=list(starts[:1]) * 2)
    # (one batch call cannot hold positions this far apart: one call per utterance)
    ref_far = [_batch(wca, fs, fft, fp, [p[u]], rng_pos=[starts[u]])[0] for u in range(2)]
    st = StreamSynthesizer(fs, fft, fp, 2, 50)
    for u in range(2):
        st.set_rng_position(u, starts[u])
        assert st.rng_position(u) == starts[u]
    ys = st.run_whole(p, [[50], [7, 43]])
    assert np.array_equal(ys[0], ref_far[0]) and np.array_equal(ys[1], ref_far[1])
    assert st.rng_position(0) == ends[0]  # the batch's end position (reference :106-107: draws up to the last pulse)
    assert np.array_equal(ys[0], ref[0])


def test_synth_stream_512_streams_config5_shape(wca):
    """BASELINE config 5's shape for the synthesis half: 512 streams x 24 kHz x 1 ms frames, 200-frame pushes; identical inputs
    give identical samples on every stream, and the totals add up."""
    from world_class_amd import DeviceArray
    from world_class_amd.stream import StreamSynthesizer
    fs, fft, fp, n, chunk = 24000, 1024, 1.0, 512, 200
    f0, sp, ap = _params(fs, fft, 3 * chunk, 111)
    st = StreamSynthesizer(fs, fft, fp, n, chunk)
    d_y = DeviceArray(n * st.max_samples)
    parts = []
    for k in range(3):
        sl = slice(k * chunk, (k + 1) * chunk)
        d = [DeviceArray.from_host(np.ascontiguousarray(np.tile(a[sl], (n, 1)) if a.ndim == 2 else np.tile(a[sl], n))) for a in (f0, sp, ap)]
        counts = st.push_device([chunk] * n, d[0], d[1], d[2], flush=[1 if k == 2 else 0] * n, d_y=d_y)
        for a in d:
            a.free()
        assert len(set(counts)) == 1
        y = d_y.to_host()[:sum(counts)].reshape(n, counts[0])
        assert (y == y[0]).all()
        parts.append(y[0].copy())
    y = np.concatenate(parts)
    assert len(y) == wca.synthesis_out_length(3 * chunk, fp, fs)
    assert np.array_equal(y, _batch(wca, fs, fft, fp, [(f0, sp, ap)])[0])
    d_y.free()


def _whole_stages(wca, x, fs, fft, f0_scale=None):
    """whole-utterance stage calls, each with its noise from position 0: Harvest on the signal up to the last multiple of the
    decimation ratio (the analysis stream's rule, include/world_class_stream.h), CheapTrick and D4C on all of it"""
    r = max(1, min(12, int(fs / 8000.0 + 0.5)))
    tpos, f0 = wca.Harvest(fs, frame_period=1.0).compute(x[:len(x) - len(x) % r])
    wca.rng_set_position(0)
    sp = wca.CheapTrick(fs).compute(x, tpos, f0)
    wca.rng_set_position(0)
    ap = wca.D4C(fs).compute(x, tpos, f0, fft)
    wca.rng_set_position(0)
    return tpos, f0, sp, ap


def _modify(wca, fs, fft, f0, sp, scale):
    from world_class_amd import DeviceArray
    from world_class_amd import io as wio
    d_f, d_sp = DeviceArray.from_host(np.ascontiguousarray(f0)), DeviceArray.from_host(np.ascontiguousarray(sp))
    wio.modify_parameters_device(fs, fft, len(f0), d_f, d_sp, f0_scale=scale)
    out = d_f.to_host()[:len(f0)].copy(), d_sp.to_host()[:sp.size].reshape(sp.shape).copy()
    d_f.free(); d_sp.free()
    return out


def test_analysis_stream_aperiodicity_against_whole_d4c(wca, port):
    """D4C on the committed frames of the analysis stream: against one whole-utterance D4C on the stream's own committed F0 (the
    library's and the CPU oracle's) within 1e-7 with the same LoveTrain voicing; the option changes nothing else"""
    from world_class_amd.stream import StreamAnalyzer
    from world_class_amd.synth import make_utterance
    fs = 24000
    xs = [make_utterance(fs, sec, 5200 + i) for i, sec in enumerate((2.2, 0.9))]
    xs[0] = xs[0][:-377]
    kw = dict(frame_period=1.0, chunk_ms=200, lookback_ms=400, lookahead_ms=560, context_ms=160)
    on = StreamAnalyzer(fs, len(xs), aperiodicity=True, **kw)
    off = StreamAnalyzer(fs, len(xs), **kw)
    r_on, r_off = on.run_whole(xs), off.run_whole(xs)
    for u, x in enumerate(xs):
        for k in ("tpos", "f0", "sp"):
            assert np.array_equal(r_on[u][k], r_off[u][k]), (u, k)
        assert "ap" not in r_off[u]
        assert on.rng_position(u) == off.rng_position(u)
        assert on.d4c_rng_position(u) > 0 and off.d4c_rng_position(u) == 0
        tpos, f0, ap = r_on[u]["tpos"], r_on[u]["f0"], r_on[u]["ap"]
        wca.rng_set_position(0)
        want = wca.D4C(fs).compute(x, tpos, f0, on.fft_size)
        wca.rng_set_position(0)
        port.rng_reset()
        want_o = port.d4c(x, fs, tpos, f0, on.fft_size)
        port.rng_reset()
        for w in (want, want_o):
            unv = lambda a: (a > 1.0 - 1e-9).all(axis=1)  # LoveTrain's unvoiced frames: 1 - kMySafeGuardMinimum everywhere
            assert np.array_equal(unv(ap), unv(w)), u
            assert np.abs(ap - w).max() <= 1e-7, (u, np.abs(ap - w).max())
    from world_class_amd import _check
    from world_class_amd.stream import _lib
    with pytest.raises(Exception):  # the option comes before the first push
        _check(_lib().wc_stream_set_aperiodicity(on._h, 0.85))


def test_whole_loop_analysis_modify_synthesis(wca):
    """24 kHz, 1 ms frames, four ragged streams: analysis with ap -> F0 x 1.2 on the committed rows (wc_modify_parameters_device)
    -> synthesis streams.  y is bit for bit one whole-utterance Synthesis of the concatenated modified stream parameters, and
    against whole-utterance stage calls on the complete signals (each stage's noise from position 0) the voicing is identical and
    y within 1e-6."""
    from world_class_amd import io as wio
    from world_class_amd.stream import StreamAnalyzer, StreamSynthesizer
    from world_class_amd.synth import make_utterance
    fs, scale = 24000, 1.2
    xs = [make_utterance(fs, sec, 5300 + i) for i, sec in enumerate((1.5, 1.1, 2.0, 0.7))]
    xs[2] = xs[2][:-377]
    n = len(xs)
    sa = StreamAnalyzer(fs, n, frame_period=1.0, chunk_ms=200, lookback_ms=400, lookahead_ms=560, context_ms=160, aperiodicity=True)
    ss = StreamSynthesizer(fs, sa.fft_size, 1.0, n, sa.max_frames)
    bins, cs = sa.bins, sa.chunk_samples
    par = [dict(f0=[], sp=[], ap=[]) for _ in xs]
    ys = [[] for _ in xs]
    pos, done = 0, [False] * n
    while not all(done):
        chunks, flush = [], []
        for u, x in enumerate(xs):
            last = not done[u] and pos + cs >= len(x)
            chunks.append(np.zeros(0) if done[u] else x[pos:pos + cs])
            flush.append(1 if last else 0)
        from world_class_amd import DeviceArray
        flat = np.concatenate([c for c in chunks if len(c)])
        d = DeviceArray.from_host(flat)
        counts = sa.push_device(d, [len(c) for c in chunks], flush, d_ap=sa._d_ap)
        d.free()
        tot = sum(counts)
        if tot:
            wio.modify_parameters_device(fs, sa.fft_size, tot, sa._d_f, sa._d_sp, f0_scale=scale)
        out = ss.push_device(counts, sa._d_f, sa._d_sp, sa._d_ap, flush)
        f = sa._d_f.to_host()[:tot]
        sp = sa._d_sp.to_host()[:tot * bins].reshape(tot, bins)
        ap = sa._d_ap.to_host()[:tot * bins].reshape(tot, bins)
        y = ss._d_y.to_host()[:sum(out)]
        o = oy = 0
        for u in range(n):
            par[u]["f0"].append(f[o:o + counts[u]]); par[u]["sp"].append(sp[o:o + counts[u]]); par[u]["ap"].append(ap[o:o + counts[u]])
            ys[u].append(y[oy:oy + out[u]])
            o += counts[u]; oy += out[u]
            done[u] = done[u] or bool(flush[u])
        pos += cs
    params = [tuple(np.concatenate(p[k]) for k in ("f0", "sp", "ap")) for p in par]
    ys = [np.concatenate(y) for y in ys]
    ref = _batch(wca, fs, sa.fft_size, 1.0, params)
    worst = 0.0
    for u, x in enumerate(xs):
        assert np.array_equal(ys[u], ref[u]), u
        tpos, f0, sp, ap = _whole_stages(wca, x, fs, sa.fft_size)
        f0m, spm = _modify(wca, fs, sa.fft_size, f0, sp, scale)
        assert np.array_equal(params[u][0] == 0, f0m == 0), u
        wca.rng_set_position(0)
        yw = wca.Synthesis(fs, sa.fft_size, 1.0).compute(f0m, spm, ap)
        wca.rng_set_position(0)
        assert len(yw) == len(ys[u])
        worst = max(worst, float(np.abs(ys[u] - yw).max()))
    assert worst < 1e-6, worst
