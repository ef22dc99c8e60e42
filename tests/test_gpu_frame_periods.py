"""-m gpu: Synthesis, the synthesis streams, Harvest's output grid, CheapTrick, D4C and the pipeline at frame periods that are no
whole number of samples, or not representable in seconds: hop 256 at 22.05 / 44.1 kHz, hop 512 at 96 kHz, 12.5, 7.3, 5.03125, 2.5,
0.7 and 16 ms, 5 ms at 44.1 kHz.  There floor(t / fp), ceil(t / fp), t / fp - floor and the comparison of t with (j + 1) * fp are
decided by single roundings on the sample that nominally sits on a frame boundary, and a push of the streams finalises a varying
number of samples.

The inputs come from tests/frame_periods.py: contours whose pulses land on such samples (of both kinds, held on the CPU by
tests/test_frame_periods_rule.py), the same over rows stepped by 1e18 at those boundaries (a few ulps of the interpolation weight
then set the envelope), a voiced -> unvoiced end, a two-frame contour, a long unvoiced gap.  The checkers are the real reference's
waveforms and contours in tests/golden/frame_periods.npz and the CPU restatement, pinned to each other by the rule file.  Every
tolerance is imported from the stage files; the worst differences are printed.

Measured on an MI355X when the file was written, worst over all cases: y 1.1e-14 against the restatement and 7.1e-15 against the
fixture (the steep contours, whose samples reach 40; 4.6e-16 on the plain ones), the streams bit for bit the batch call at 1024 /
2048; F0 2.4e-12 Hz; spectrogram 1.8e-10 relative, aperiodicity 2.9e-12.  With t * (1.0 / fp) in place of t / fp in the fft-1024
pulse kernel (a scratch build) the steep contours of 16 kHz / 12.5 ms, 22.05 kHz / hop 256 and 16 kHz / 5.03125 ms miss Y_ABS by
1e-6; the plain boundary contours do not notice it -- floor k - 1 with a weight of 1 - 1e-16 and floor k read the same row to an ulp."""
import numpy as np
import pytest

import frame_periods as fpm
import stream_speed_rule as sr
import test_gpu_synth_stream_speed as tss
from test_frame_periods_rule import against_fixture, check_params
from test_gpu_cheaptrick import SP_REL
from test_gpu_d4c import AP_ABS
from test_gpu_harvest import check_f0
from test_gpu_synth_stream import _batch, _gap, _stream
from test_gpu_synthesis import Y_ABS

pytestmark = pytest.mark.gpu

ONE_PER_FFT = ["16k_12.5ms", "48k_2.5ms", "8k_16ms", "96k_hop512"]  # fft 1024, 2048, 512, 4096


@pytest.fixture(scope="module")
def wca():
    import world_class_amd as w
    w.lib().wc_set_device(0)
    return w


@pytest.fixture(scope="module")
def fixture():
    return np.load(fpm.fixture_path())


@pytest.fixture(scope="module")
def cases(port):
    """name -> kind -> (params, the restatement's waveform from noise position 0, its end position), computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            fs, fft, fp, _, _ = fpm.CASES[name]
            cache[name] = {}
            for kind in fpm.contours(name):
                p = fpm.contour(name, kind)
                port.rng_seek(0)
                y = port.synthesis(*p, fs, fp)
                y.setflags(write=False)
                cache[name][kind] = (p, y, port.rng_position())
            port.rng_reset()
        return cache[name]
    return get


def _handle(make, env):
    """a handle created under the environment switches it reads at creation"""
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        return make()


def _groups(kinds):
    """at most four utterances per call"""
    return [kinds[:2], kinds[2:]] if len(kinds) > 4 else [kinds]


def _run(s, params):
    ys, pos = s.compute_batch([p[0] for p in params], [p[1] for p in params], [p[2] for p in params], rng_pos=[0] * len(params))
    return ys, list(pos)


# ---- the Synthesis stage ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fpm.NAMES)
def test_synthesis_stage_against_the_fixture_the_restatement_and_its_twins(wca, cases, fixture, name):
    """every contour of the case through Synthesis.compute_batch: the real reference's waveform and the restatement's within Y_ABS,
    the noise end positions equal, the length wc_synthesis_out_length; and the twins of tests/test_gpu_synthesis.py and
    tests/test_gpu_synth_split.py at their tolerances -- the workgroup-per-pulse kernel and the run without a row budget within
    1e-12, the single launch at fft 2048 and a second run at 1024 / 2048 bit for bit"""
    fs, fft, fp, _, _ = fpm.CASES[name]
    c = cases(name)
    twins = [("block", {"WC_SYN_IMPL": "block"}, 1e-12), ("no row budget", {"WC_SYN_ROWS_BUDGET_MB": "0"}, 1e-12)]
    if fft == 2048:
        twins.append(("single launch", {"WC_SYN_SPLIT": "0"}, 0.0))
    if fft in (1024, 2048):
        twins.append(("second run", {}, 0.0))
    worst = {"fixture": 0.0, "restatement": 0.0}
    for kinds in _groups(fpm.contours(name)):
        params = [c[k][0] for k in kinds]
        ys, pos = _run(wca.Synthesis(fs, fft, fp), params)
        for kind, y, p1 in zip(kinds, ys, pos):
            p, want, end = c[kind]
            check_params(fixture, name, kind, p)
            assert len(y) == wca.synthesis_out_length(len(p[0]), fp, fs) == fpm.out_length(len(p[0]), fp, fs) == len(want)
            assert p1 == end, (kind, p1, end)
            worst["restatement"] = max(worst["restatement"], float(np.abs(y - want).max()))
            assert np.abs(y - want).max() < Y_ABS, (kind, float(np.abs(y - want).max()))
            worst["fixture"] = max(worst["fixture"], against_fixture(fixture, name, kind, y, Y_ABS))
        for what, env, tol in twins:
            yt, post = _run(_handle(lambda: wca.Synthesis(fs, fft, fp), env), params)
            assert post == pos, what
            for kind, a, b in zip(kinds, ys, yt):
                d = float(np.abs(a - b).max())
                worst[what] = max(worst.get(what, 0.0), d)
                assert (np.array_equal(a, b) if tol == 0.0 else d < tol), (what, kind, d)
    print("synthesis %s: y" % name, ", ".join("%s %.2e" % kv for kv in worst.items()))


@pytest.mark.parametrize("name", ONE_PER_FFT)
def test_time_base_modes_agree_on_the_boundary_contours(wca, cases, name):
    """the modes of test_exact_parallel_phase_accumulation_matches_the_serial_chain (tests/test_gpu_synthesis.py) with its assertions:
    the pulse positions hang on the sequential phase sum, and here pulses sit on the samples where Coarse::at's product and the
    pulse kernels' quotient may take different sides"""
    fs, fft, fp, _, _ = fpm.CASES[name]
    c = cases(name)
    kinds = [k for k in ("boundary", "steep") if k in c]
    ys = {}
    for mode, env in (("parallel", {}), ("serial", {"WC_SYN_TIMEBASE": "serial"}), ("utterance", {"WC_SYN_PULSES": "utterance"}),
                      ("single", {"WC_SYN_PHASE": "single"})):
        ys[mode] = _run(_handle(lambda: wca.Synthesis(fs, fft, fp), env), [c[k][0] for k in kinds])
    for i, kind in enumerate(kinds):
        a, b, cc, d = (ys[m][0][i] for m in ("parallel", "serial", "utterance", "single"))
        assert ys["parallel"][1] == ys["serial"][1] == ys["utterance"][1] == ys["single"][1]
        assert np.abs(a - b).max() < 1e-9    # a pulse moved by one sample shows up as ~1e-2
        assert np.abs(a - cc).max() < 1e-9
        assert (np.array_equal(a, d) and np.array_equal(a, b)) if fft == 2048 else np.abs(a - d).max() < 1e-12
        assert np.abs(a - c[kind][1]).max() < 1e-8
        print("time base %s %s: serial %.2e, utterance %.2e, single %.2e" % (name, kind, np.abs(a - b).max(), np.abs(a - cc).max(), np.abs(a - d).max()))


def test_sixteen_contours_in_two_halves_equal_one_piece(wca, port, cases):
    """a batch of 16 runs as two halves with a twin handle (n_utt >= 16): the same bits as one piece (WC_SYN_HALVES=0), at 12.5 ms"""
    name = "16k_12.5ms"
    fs, fft, fp, _, _ = fpm.CASES[name]
    c = cases(name)
    params = [c["boundary"][0], c["steep"][0], c["end_unvoiced"][0], c["gap"][0]]
    params += [fpm.piecewise(fs, fft, 30 + 5 * i, 900 + i) for i in range(12)]
    start = [1000 * i + 7 for i in range(16)]
    arg = [p[0] for p in params], [p[1] for p in params], [p[2] for p in params]
    ys, pos = wca.Synthesis(fs, fft, fp).compute_batch(*arg, rng_pos=start)
    y1, pos1 = _handle(lambda: wca.Synthesis(fs, fft, fp), {"WC_SYN_HALVES": "0"}).compute_batch(*arg, rng_pos=start)
    assert list(pos) == list(pos1)
    for a, b in zip(ys, y1):
        assert np.array_equal(a, b)
    for u in (0, 1, 8, 15):
        port.rng_seek(start[u])
        want = port.synthesis(*params[u], fs, fp)
        assert port.rng_position() == pos[u]
        assert np.abs(ys[u] - want).max() < Y_ABS
    port.rng_reset()


# ---- the synthesis streams -------------------------------------------------------------------------------------------------------
def final_limit(F, fs, fp):
    """the first sample with i / fs >= (F - 1) * fp (fp in seconds): samples before it are final once F frames are in"""
    if F < 2:
        return 0
    edge = (F - 1) * (fp / 1000.0)
    g = max(int(np.floor(edge * fs)) - 2, 0)
    while g / fs < edge:
        g += 1
    assert g == 0 or (g - 1) / fs < edge
    return g


def check_commits(log, params, fs, fft, fp):
    """samples_committed after every push against the header's rule (include/world_class_stream.h): with F frames in and no flush,
    the samples below E = min(final_limit(F), out_length(F) - 1) are final; pulses up to the waiting one are added, the waiting one
    lies less than a pulse gap below E and reaches fft / 2 - 1 samples back -- so E - fft / 2 - gap <= committed <= E - fft / 2.
    After the flush everything is committed."""
    M = fft // 2
    seen = 0
    for u, got, F in log:
        total = len(params[u][0])
        if F >= total:
            assert got == fpm.out_length(total, fp, fs), (u, F, got)
            continue
        E = min(final_limit(F, fs, fp), max(fpm.out_length(max(F, 2), fp, fs) - 1, 0))
        assert max(E - M - _gap(fs, fft), 0) <= got <= max(E - M, 0), (u, F, got, E)
        seen += 1
    return seen


@pytest.mark.parametrize("kind", list(fpm.PATTERNS))
@pytest.mark.parametrize("name", fpm.NAMES)
def test_streams_equal_the_batch_call_push_by_push(wca, cases, fixture, name, kind):
    """every contour as a stream -- one frame per push, ragged pushes with idle ones, everything in one push -- against ONE batch
    call: bit for bit at fft 1024 / 2048, within 1e-12 at 512 / 4096; against the reference's waveform within Y_ABS; the latency
    bound of tests/test_gpu_synth_stream.py at every push, and samples_committed against final_limit's definition"""
    from world_class_amd.stream import StreamSynthesizer
    fs, fft, fp, _, _ = fpm.CASES[name]
    c = cases(name)
    worst, pushes = 0.0, 0
    for kinds in _groups(fpm.contours(name)):
        params = [c[k][0] for k in kinds]
        pat = [fpm.pattern(kind, len(p[0])) for p in params]
        pat = [p[u % len(p):] + p[:u % len(p)] for u, p in enumerate(pat)]  # (ragged: every stream at another place of the cycle)
        log = []
        with pytest.MonkeyPatch.context() as mp:
            committed = StreamSynthesizer.samples_committed

            def logged(self, u):
                got = committed(self, u)
                log.append((u, got, self.frames_received(u)))
                return got
            mp.setattr(StreamSynthesizer, "samples_committed", logged)  # (called by _stream after every push)
            ys, st = _stream(wca, fs, fft, fp, params, pat)
        pushes += check_commits(log, params, fs, fft, fp)
        ref = _batch(wca, fs, fft, fp, params)
        for k, y, r in zip(kinds, ys, ref):
            d = float(np.abs(y - r).max())
            assert (np.array_equal(y, r) if fft in (1024, 2048) else d <= 1e-12), (k, d)
            assert np.abs(y - c[k][1]).max() < Y_ABS
            worst = max(worst, against_fixture(fixture, name, k, y, Y_ABS))
            assert st.rng_position(kinds.index(k)) == c[k][2]
    assert kind == "all" or pushes >= 20  # (pushes that were not the flush)
    print("streams %s %s: y against the fixture %.2e, %d pushes checked against final_limit" % (name, kind, worst, pushes))


@pytest.mark.parametrize("name", ["16k_12.5ms", "44k_5ms"])
def test_coded_pushes_and_a_speed_equal_the_whole_utterance_call(wca, cases, name):
    """coded pushes (one stream neutral, one at speed 1 / 1.37) and full rows at speeds 1.5 and 0.5, ragged, against the
    whole-utterance calls of tests/test_gpu_synth_stream_speed.py (whole_coded, whole_rows): bit for bit at fft 1024 / 2048"""
    import torch
    from world_class_amd import codec, io as wio
    from world_class_amd.stream import StreamSynthesizer
    env = (wca, codec, wio, torch)
    fs, fft, fp, _, _ = fpm.CASES[name]
    c = cases(name)
    raw = [c["boundary"][0], c["end_unvoiced"][0]]
    pats = [[3, 0, 11, 1], [1, 2, 0, 17]]
    srcs = [tss._code(env, fs, fft, p) for p in raw]
    speeds = [None, 1 / 1.37]
    st = StreamSynthesizer(fs, fft, fp, 2, 64)
    ys, pushes, sp_ = tss.drive(st, srcs, pats, lambda u, k: speeds[u] if k == 0 else None, coded=True)
    for u, src in enumerate(srcs):
        pos, _ = sr.positions(pushes[u], sp_[u])
        if speeds[u] is None:
            assert np.array_equal(pos, np.arange(len(src[0])))
        want, end = tss.whole_coded(env, fs, fft, fp, src, pos, 1.0, 0.0)
        assert np.isfinite(want).all() and np.array_equal(ys[u], want), (u, len(ys[u]), len(want))
        assert st.rng_position(u) == end
    speeds = [1.5, 0.5]
    st = StreamSynthesizer(fs, fft, fp, 2, 64)
    ys, pushes, sp_ = tss.drive(st, raw, pats, lambda u, k: speeds[u] if k == 0 else None)
    for u, src in enumerate(raw):
        pos, _ = sr.positions(pushes[u], sp_[u])
        want, end = tss.whole_rows(env, fs, fft, fp, src, pos)
        assert np.array_equal(ys[u], want), u
        assert st.rng_position(u) == end


# ---- Harvest's output grid ---------------------------------------------------------------------------------------------------------
def round_half_away(v):
    """the reference's matlab_round (src/world_matlabfunctions.cpp:212-214) for positive arguments"""
    return np.where(v > 0, (v + 0.5).astype(np.int64), (v - 0.5).astype(np.int64))


def check_grid(h, u, tpos, f0, fp, n):
    """tpos is i * fp / 1000.0 bit for bit, the frame count is wc_get_samples, and -- independently of the signal -- every output
    frame is the 1 ms contour's value at the index the reference picks, with exactly its expression.  Returns the frames on x.5"""
    i = np.arange(len(f0))
    assert len(f0) == h.get_samples(n) == fpm.get_samples(h.fs, n, fp)
    assert np.array_equal(tpos, i * fp / 1000.0)
    f1 = h.debug_fetch("f0_1ms", u)
    idx = np.minimum(len(f1) - 1, round_half_away(i * fp / 1000.0 * 1000.0))
    assert np.array_equal(f0, f1[idx])
    return int((np.abs((i * fp) % 1.0 - 0.5) < 1e-9).sum())


@pytest.mark.parametrize("name,fs,fp", fpm.HARVEST_PERIODS)
def test_harvest_output_grid_at_fractional_periods(wca, port, checker, fixture, name, fs, fp):
    x = fpm.harvest_signal(fs)
    h = wca.Harvest(fs, frame_period=fp)
    tpos, f0 = h.compute(x)
    halves = check_grid(h, 0, tpos, f0, fp, len(x))
    if name in ("2.5ms", "12.5ms", "0.5ms"):
        assert halves >= len(f0) // 2 - 1  # every other frame sits on x.5
    want = fixture["harvest/%s/f0" % name]
    check_f0(f0, want)
    fell_back = len(checker.fell_back) if checker else 0
    tr, fr = (checker or port).harvest(x, fs, frame_period=fp)
    assert not checker or len(checker.fell_back) == fell_back  # (the reference's Harvest runs at every one of these)
    assert np.array_equal(tpos, tr)
    check_f0(f0, fr)
    print("harvest %s: F0 against the fixture %.2e Hz, against the checker %.2e Hz, %d of %d frames on x.5"
          % (name, np.abs(f0 - want).max(), np.abs(f0 - fr).max(), halves, len(f0)))


@pytest.mark.parametrize("fs,fp", [(16000, 12.5), (48000, 2.5), (22050, fpm.HOP256_22K)])
def test_harvest_ragged_batch_at_fractional_periods(wca, port, fs, fp):
    """four lengths, two of them exact multiples of the hop (where get_samples' truncation decides the frame count)"""
    from world_class_amd.synth import make_utterance
    hop = fp / 1000.0 * fs
    lengths = [int(round(37 * hop)), int(0.31 * fs) + 1, int(round(20 * hop)), int(0.45 * fs)]
    xs = [make_utterance(fs, 0.5, 7400 + u)[:n] for u, n in enumerate(lengths)]
    h = wca.Harvest(fs, frame_period=fp)
    res = h.compute_batch(xs)
    worst = 0.0
    for u, (x, (t, f)) in enumerate(zip(xs, res)):
        check_grid(h, u, t, f, fp, len(x))
        tr, fr = port.harvest(x, fs, frame_period=fp)
        assert np.array_equal(t, tr)
        check_f0(f, fr)
        worst = max(worst, float(np.abs(f - fr).max()))
    print("harvest ragged %d %.4f ms: F0 %.2e Hz" % (fs, fp, worst))


# ---- CheapTrick and D4C on the fractional grids ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fs,fp", [(16000, 12.5), (22050, fpm.HOP256_22K), (48000, 2.5), (44100, 10.0 / 3.0), (8000, 16.0)])
def test_cheaptrick_and_d4c_on_fractional_grids(wca, port, fs, fp):
    """the one-wavefront kernels of fft 1024 and 2048 and the block kernels of 512 on temporal positions i * fp / 1000.0"""
    x = fpm.harvest_signal(fs)
    tpos, f0 = port.harvest(x, fs, frame_period=fp)
    ct = wca.CheapTrick(fs)
    wca.rng_set_position(0)
    sp = ct.compute(x, tpos, f0)
    p_sp = wca.rng_get_position()
    wca.rng_set_position(0)
    ap = wca.D4C(fs).compute(x, tpos, f0, ct.fft_size)
    p_ap = wca.rng_get_position()
    wca.rng_set_position(0)
    port.rng_reset()
    sp_o = port.cheaptrick(x, fs, tpos, f0)
    assert port.rng_position() == p_sp
    port.rng_reset()
    ap_o = port.d4c(x, fs, tpos, f0, ct.fft_size)
    assert port.rng_position() == p_ap
    port.rng_reset()
    e_sp, e_ap = float((np.abs(sp - sp_o) / sp_o).max()), float(np.abs(ap - ap_o).max())
    print("cheaptrick / d4c %d %.4f ms (fft %d, %d frames): sp %.2e relative, ap %.2e" % (fs, fp, ct.fft_size, len(f0), e_sp, e_ap))
    assert e_sp < SP_REL and e_ap < AP_ABS


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["16k_12.5ms", "48k_2.5ms", "8k_16ms"])
def test_pipeline_at_fractional_periods(wca, port, name):
    """four 0.5 s utterances through Pipeline.run_batch against the restatement's pipeline, at tests/test_gpu_pipeline.py's tolerances"""
    from world_class_amd.synth import make_utterance
    fs, fft, fp, _, _ = fpm.CASES[name]
    xs = [make_utterance(fs, 0.5, 7500 + u) for u in range(4)]
    xs = [x[:len(x) - 37 * u] for u, x in enumerate(xs)]
    outs, pos = wca.Pipeline(fs, frame_period=fp).run_batch(xs, rng_pos=[0] * 4)
    worst = [0.0] * 4
    for x, r in zip(xs, outs):
        o = port.pipeline(x, fs, frame_period=fp)
        assert (o["sp"].shape[1] - 1) * 2 == fft
        assert np.array_equal(r["tpos"], o["tpos"]) and len(r["y"]) == len(o["y"]) == fpm.out_length(len(o["f0"]), fp, fs)
        assert np.array_equal(r["f0"] == 0, o["f0"] == 0)
        errs = [np.abs(r["f0"] - o["f0"]).max(), (np.abs(r["sp"] - o["sp"]) / o["sp"]).max(), np.abs(r["ap"] - o["ap"]).max(),
                np.abs(r["y"] - o["y"]).max()]
        worst = [max(a, float(b)) for a, b in zip(worst, errs)]
    port.rng_reset()
    print("pipeline %s: F0 %.2e Hz, sp %.2e relative, ap %.2e, y %.2e" % ((name,) + tuple(worst)))
    assert worst[0] < 1e-6 and worst[1] < 1e-7 and worst[2] < 1e-7 and worst[3] < 1e-8


# ---- host formulas ---------------------------------------------------------------------------------------------------------------
def test_host_length_formulas_on_the_grid_of_the_rule_test(wca):
    """wc_get_samples and wc_synthesis_out_length truncate as the reference does, also where that drops a frame or a sample"""
    for fs, fp, ns in fpm.length_grid():
        for n in ns:
            assert wca.get_samples(fs, n, fp) == fpm.get_samples(fs, n, fp), (fs, fp, n)
        for frames in list(range(2, 122)) + [998, 4002]:
            assert wca.synthesis_out_length(frames, fp, fs) == fpm.out_length(frames, fp, fs), (fs, fp, frames)
    assert wca.synthesis_out_length(57, 256 / 24000 * 1000, 24000) == 14336
