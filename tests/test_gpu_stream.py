"""-m gpu: chunked Harvest + CheapTrick (include/world_class_stream.h, BASELINE config 5) against ONE whole-utterance call of
the same stages on the complete signal.  The reference has no streaming mode (Harvest is non-causal, reference
src/harvest.cpp:431-440, :676-703); the parity claim is the one the header makes: with lookahead and lookback of 400 ms the
committed frames equal the whole-utterance result -- identical voicing decisions, F0 within 1e-9 Hz (last-bit differences
from the smoothing filter's backward limit cycle), spectrogram within 1e-7 relative, the noise draws being the very same
stream positions."""
import numpy as np
import pytest

from world_class_amd.synth import make_utterance

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wca():
    import world_class_amd as w
    w.lib()
    return w


def whole(wca, x, fs, fp):
    """one whole-utterance call of each stage.  Harvest's decimator aligns its phase to the END of its input (reference
    src/world_matlabfunctions.cpp:201-206), so its contour depends on (length mod ratio); the stream is defined as Harvest on
    the signal up to the last multiple of the ratio (include/world_class_stream.h), CheapTrick on all of it."""
    r = max(1, min(12, int(fs / 8000.0 + 0.5)))
    wca.rng_set_position(0)
    tpos, f0 = wca.Harvest(fs, frame_period=fp).compute(x[:len(x) - len(x) % r])
    sp = wca.CheapTrick(fs).compute(x, tpos, f0)
    wca.rng_set_position(0)
    return tpos, f0, sp


def oracle_whole(port, x, fs, fp):
    """the same whole-utterance call by the CPU oracle (oracle/port.py, pinned to the real reference by tests/test_oracle_golden.py):
    Harvest on the signal up to the last multiple of the decimation ratio, CheapTrick on all of it, noise stream from position 0"""
    r = max(1, min(12, int(fs / 8000.0 + 0.5)))
    tpos, f0 = port.harvest(x[:len(x) - len(x) % r], fs, frame_period=fp)
    port.rng_reset()
    sp = port.cheaptrick(x, fs, tpos, f0)
    port.rng_reset()
    return tpos, f0, sp


def compare_oracle(got, want, what):
    """every committed frame against the oracle, at the tolerances of SURVEY.md section 8(c): identical voicing, F0 1e-6 Hz, sp 1e-7"""
    tpos, f0, sp = want
    assert len(got["f0"]) == len(f0), what
    assert np.abs(got["tpos"] - tpos).max() < 1e-12, what
    assert np.array_equal(got["f0"] == 0, f0 == 0), what + ": voicing"
    assert np.abs(got["f0"] - f0).max() < 1e-6, what
    assert (np.abs(got["sp"] - sp) / sp).max() < 1e-7, what


def compare(got, want, what):
    tpos, f0, sp = want
    assert len(got["f0"]) == len(f0), what
    assert np.array_equal(got["tpos"], tpos), what
    assert np.array_equal(got["f0"] == 0, f0 == 0), what + ": voicing"
    assert np.abs(got["f0"] - f0).max() < 1e-9, what
    assert (np.abs(got["sp"] - sp) / sp).max() < 1e-7, what
    return float(np.mean(got["f0"] == f0)), float(np.abs(got["f0"] - f0).max()), float((np.abs(got["sp"] - sp) / sp).max())


# whole windows (lookahead 400 ms) and the incremental mode (context 160 ms inside a lookahead of 560 ms: the tail sees the same 400)
MODES = [dict(lookahead_ms=400, context_ms=0), dict(lookahead_ms=560, context_ms=160)]


@pytest.mark.parametrize("mode", MODES, ids=["whole_windows", "incremental"])
def test_streams_equal_whole_utterances_24k_1ms(wca, port, mode):
    """BASELINE config 5's shape: 24 kHz, 1 ms frames; ragged lengths, one of them not a whole number of chunks or ms"""
    from world_class_amd.stream import StreamAnalyzer
    fs = 24000
    xs = [make_utterance(fs, sec, 5000 + i) for i, sec in enumerate((3.0, 2.2, 4.1, 0.9))]
    xs[2] = xs[2][:-377]
    sa = StreamAnalyzer(fs, len(xs), frame_period=1.0, chunk_ms=200, lookback_ms=400, **mode)
    assert sa.latency_ms == 200 + mode["lookahead_ms"] and sa.chunk_samples == 4800
    res = sa.run_whole(xs)
    for u, (x, r) in enumerate(zip(xs, res)):  # first of all: against the oracle's whole-utterance result
        compare_oracle(r, oracle_whole(port, x, fs, 1.0), "stream %d vs oracle" % u)
    stats = [compare(r, whole(wca, x, fs, 1.0), "stream %d" % u) for u, (x, r) in enumerate(zip(xs, res))]
    # 40-100 % of the frames are bit-equal; the rest differ in the last bits only (1e-14 relative: the smoothing filter's backward
    # pass starts where the window ends and runs into its last-bit limit cycle with another phase)
    assert max(s[1] for s in stats) < 1e-11 and max(s[2] for s in stats) < 1e-9, stats
    if not mode["context_ms"]:
        assert stats[3][0] == 1.0  # a stream shorter than one window IS the whole-utterance call
    for u, x in enumerate(xs):
        assert sa.frames_committed(u) == wca.get_samples(fs, len(x) - len(x) % 3, 1.0)
    assert len(xs[2]) % 3 != 0 and len(xs[0]) % 3 == 0  # both cases of the decimation-phase rule are in the batch


@pytest.mark.parametrize("mode", MODES, ids=["whole_windows", "incremental"])
def test_streams_equal_whole_utterances_48k_5ms(wca, port, mode):
    from world_class_amd.stream import StreamAnalyzer
    fs = 48000
    xs = [make_utterance(fs, sec, 5100 + i) for i, sec in enumerate((2.5, 1.7))]
    sa = StreamAnalyzer(fs, len(xs), frame_period=5.0, chunk_ms=200, lookback_ms=400, **mode)
    res = sa.run_whole(xs)
    for u, (x, r) in enumerate(zip(xs, res)):
        compare_oracle(r, oracle_whole(port, x, fs, 5.0), "stream %d vs oracle" % u)
        compare(r, whole(wca, x, fs, 5.0), "stream %d" % u)


def test_streams_act_on_ties_in_both_modes(wca):
    """A train of impulses whose period is a whole number of decimated samples puts Harvest's raw candidates on ties of the
    refinement's integer cuts; a window that raises the tie flag is analysed again with the band-pass as
    direct FIR sums.  Whole windows go through the stage call, which has done so since the flag exists; the incremental mode runs
    Harvest's front and tail on separate handles, and since round 5 its front does the same (the twin's candidate and score rows
    are copied into the front's own).  On such a train every implementation decides the ties by its last bit -- two builds of
    the reference part by 1.4e-3 Hz (tests/golden/ref_self_spread.json) -- and the two modes decimate different stretches of
    the signal, so they are held to the bound of tests/test_gpu_sweeps.py for this class, twice that spread, with identical
    voicing (measured: 4.9e-4 Hz); on speech they agree to 1e-9 Hz (the tests above)."""
    from world_class_amd.stream import StreamAnalyzer
    fs = 24000
    xs = []
    for period in (240, 150, 96):  # 100, 160, 250 Hz: 80, 50, 32 samples at the internal 8 kHz
        x = np.zeros(int(2.0 * fs))
        x[7::period] = 0.9
        xs.append(x)
    res = []
    for mode in MODES:
        sa = StreamAnalyzer(fs, len(xs), frame_period=1.0, chunk_ms=200, lookback_ms=400, **mode)
        res.append(sa.run_whole(xs))
    for u in range(len(xs)):
        a, b = res[0][u], res[1][u]
        assert (a["f0"] > 0).mean() > 0.8, u  # (voiced: the comparison is not one of zeros)
        assert np.array_equal(a["f0"] == 0, b["f0"] == 0), "stream %d: voicing" % u
        assert np.abs(a["f0"] - b["f0"]).max() < 2 * 1.43e-3, (u, float(np.abs(a["f0"] - b["f0"]).max()))
        assert abs(float(np.median(a["f0"][a["f0"] > 0])) - fs / (240, 150, 96)[u]) < 0.1, u  # (the contour bends by a few hertz at the ends)


@pytest.mark.parametrize("mode", MODES, ids=["whole_windows", "incremental"])
def test_idle_streams_resets_and_frame_accounting(wca, mode):
    """streams need not move in lockstep: one idles, one is reset and starts a new signal; every absolute frame is committed
    exactly once, `chunk / frame_period` per push in the steady state, the rest at the flush"""
    from world_class_amd.stream import StreamAnalyzer
    fs = 16000
    a, b, c = (make_utterance(fs, sec, 5200 + i) for i, sec in enumerate((1.6, 1.2, 1.0)))
    sa = StreamAnalyzer(fs, 2, frame_period=1.0, chunk_ms=160, lookback_ms=400, **mode)
    ahead = mode["lookahead_ms"]
    cs = sa.chunk_samples
    acc = {0: [], 1: []}

    def push(c0, c1, f0=0, f1=0):
        r = sa.push([c0, c1], [f0, f1])
        acc[0].append(r[0])
        acc[1].append(r[1])
        return [len(v["f0"]) for v in r]

    counts = []
    na, nb = 0, 0
    # stream 0 gets `a`; stream 1 idles for three pushes, then gets `b`
    for k in range(4):
        counts.append(push(a[na:na + cs], np.zeros(0)))
        na += cs
    assert [c[1] for c in counts] == [0, 0, 0, 0] and counts[0][0] == 0 and sum(c[0] for c in counts) == 4 * 160 - ahead
    while na + cs < len(a):
        n = push(a[na:na + cs], b[nb:nb + cs])
        assert n[0] == 160
        na += cs
        nb += cs
    push(a[na:], b[nb:nb + cs], 1, 0)
    nb += cs
    while nb + cs < len(b):
        push(np.zeros(0), b[nb:nb + cs])
        nb += cs
    push(np.zeros(0), b[nb:], 0, 1)
    got = {u: {k: np.concatenate([r[k] for r in acc[u]]) for k in ("tpos", "f0", "sp")} for u in (0, 1)}
    compare(got[0], whole(wca, a, fs, 1.0), "a")
    compare(got[1], whole(wca, b, fs, 1.0), "b")
    with pytest.raises(wca.WorldClassError, match="flushed"):
        sa.push([a[:cs], np.zeros(0)])
    # a new signal on stream 0 after a reset
    sa.reset(0)
    acc[0] = []
    nc = 0
    while nc + cs < len(c):
        push(c[nc:nc + cs], np.zeros(0))
        nc += cs
    push(c[nc:], np.zeros(0), 1, 0)
    got0 = {k: np.concatenate([r[k] for r in acc[0]]) for k in ("tpos", "f0", "sp")}
    compare(got0, whole(wca, c, fs, 1.0), "c after reset")


def test_stream_arguments_are_checked(wca):
    from world_class_amd.stream import StreamAnalyzer
    with pytest.raises(wca.WorldClassError, match="multiple of 1000"):
        StreamAnalyzer(44100, 2)
    with pytest.raises(wca.WorldClassError, match="multiples of lcm"):
        StreamAnalyzer(24000, 2, chunk_ms=100)
    with pytest.raises(wca.WorldClassError, match="multiples of lcm"):
        StreamAnalyzer(24000, 2, frame_period=5.0, chunk_ms=200, lookback_ms=400, lookahead_ms=408)
    sa = StreamAnalyzer(24000, 2)
    with pytest.raises(wca.WorldClassError, match="short chunk"):
        sa.push([np.zeros(sa.chunk_samples), np.zeros(100)])
    # the refused push left both streams where they were (the first one's chunk was fine and must not have been taken)
    assert int(wca.lib().wc_stream_samples_received(sa._h, 0)) == 0 and sa.frames_committed(0) == 0


def test_noise_positions_are_carried_and_may_lie_far_apart(wca):
    """CheapTrick's draws come from the stream's own position in the reference's sequence; a stream may continue the numbering of
    an earlier analysis, and streams whose positions lie further apart than one draw table covers are served one by one"""
    from world_class_amd.stream import StreamAnalyzer
    fs = 16000
    x = make_utterance(fs, 1.3, 5300)
    x = x[:len(x) - len(x) % 2]
    far = (1 << 30) + 12345
    sa = StreamAnalyzer(fs, 2, frame_period=5.0, chunk_ms=200, lookback_ms=400, lookahead_ms=400)
    sa.set_rng_position(1, far)
    res = sa.run_whole([x, x])
    t, f0, sp0 = whole(wca, x, fs, 5.0)
    wca.rng_set_position(far)
    sp1 = wca.CheapTrick(fs).compute(x, t, f0)
    end1 = wca.rng_get_position()
    wca.rng_set_position(0)
    assert np.array_equal(res[0]["f0"] == 0, f0 == 0) and np.array_equal(res[1]["f0"], res[0]["f0"])
    assert (np.abs(res[0]["sp"] - sp0) / sp0).max() < 1e-9
    assert (np.abs(res[1]["sp"] - sp1) / sp1).max() < 1e-9
    assert not np.array_equal(res[0]["sp"], res[1]["sp"])       # other draws, other last bits
    assert sa.rng_position(1) == end1 and sa.rng_position(0) == end1 - far


@pytest.mark.parametrize("mode", MODES, ids=["whole_windows", "incremental"])
def test_non_finite_samples_stay_in_their_stream(wca, mode):
    """a burst of NaN / inf samples in one stream never hangs a push, never reaches the other stream, and the damaged stream is
    accounted for frame by frame and recovers once the burst has left its window"""
    from world_class_amd.stream import StreamAnalyzer
    fs = 16000
    x = make_utterance(fs, 3.0, 5400)
    x = x[:len(x) - len(x) % 2]
    bad = x.copy()
    bad[9000:9040] = np.nan
    bad[9100] = np.inf
    sa = StreamAnalyzer(fs, 2, frame_period=5.0, chunk_ms=200, lookback_ms=400, **mode)
    res = sa.run_whole([x, bad])
    want = whole(wca, x, fs, 5.0)
    compare(res[0], want, "clean stream next to a damaged one")
    assert len(res[1]["f0"]) == len(want[1]) and np.array_equal(res[1]["tpos"], want[0])
    # far behind the burst (0.57 s + window) the damaged stream is the clean one again
    late = res[1]["tpos"] > 2.2
    assert np.array_equal(res[1]["f0"][late] == 0, want[1][late] == 0)
    assert np.abs(res[1]["f0"][late] - want[1][late]).max() < 1e-9


def test_chunks_as_int16_pcm_and_float32(wca):
    """new samples as they come off a WAV file or a capture device: widened on the device, same frames as float64 chunks"""
    from world_class_amd.stream import StreamAnalyzer
    fs = 16000
    x = make_utterance(fs, 1.2, 5500)             # int16-quantised by construction: x * 32768 is a whole number
    x = x[:len(x) - len(x) % 2]
    pcm = np.round(x * 32768.0).astype(np.int16)
    assert np.array_equal(pcm.astype(np.float64) / 32768.0, x)
    want = StreamAnalyzer(fs, 1, frame_period=5.0).run_whole([x])[0]
    for src in (pcm, x.astype(np.float32)):
        got = StreamAnalyzer(fs, 1, frame_period=5.0).run_whole([src])[0]
        assert np.array_equal(got["f0"], want["f0"]) and np.array_equal(got["sp"], want["sp"])


def test_config5_shape_512_streams_frame_accounting_and_identical_streams(wca, port):
    """BASELINE config 5 at one GPU's size: 512 concurrent 24 kHz streams, 1 ms frames, 200 ms chunks (incremental mode).  Every
    absolute frame is committed exactly once; everything is finite; streams fed the same signal return the same bits whatever
    their slot; and one stream of each distinct signal is checked against the oracle's whole-utterance result."""
    from world_class_amd.stream import StreamAnalyzer
    fs, n = 24000, 512
    sig = [make_utterance(fs, 0.9, 5300 + i) for i in range(4)]
    xs = [sig[u % 4] for u in range(n)]
    sa = StreamAnalyzer(fs, n, frame_period=1.0, chunk_ms=200, lookback_ms=400, lookahead_ms=560, context_ms=160)
    res = sa.run_whole(xs)
    for u in range(n):
        want = wca.get_samples(fs, len(xs[u]) - len(xs[u]) % 3, 1.0)
        assert sa.frames_committed(u) == want and len(res[u]["f0"]) == want
        assert np.isfinite(res[u]["f0"]).all() and np.isfinite(res[u]["sp"]).all()
    for u in range(4, n):
        assert np.array_equal(res[u]["f0"], res[u % 4]["f0"]) and np.array_equal(res[u]["sp"], res[u % 4]["sp"]), u
    for u in range(4):
        compare_oracle(res[u], oracle_whole(port, xs[u], fs, 1.0), "stream %d vs oracle" % u)


def test_a_stream_that_commits_nothing_next_to_one_far_away_in_the_noise(wca):
    """Two analysis streams with aperiodicity, stream 1's noise positions 2^33 draws away.  In one push stream 0 commits no frames
    (its look-ahead is not filled yet) while stream 1 commits some: the stages' call on both must size the draw table over the
    stream that draws alone.  Utterances of 0.3 s end with their second push at chunk 200 / lookahead 400 ms, so no push there has a
    stream without frames next to one with frames; the smallest settings the streams take with 5 ms frames and aperiodicity do:
    chunk, lookback and lookahead of 40 ms (multiples of lcm(8 ms, frame period), at least 38 ms around a frame for D4C)."""
    from world_class_amd.stream import StreamAnalyzer
    fs, far = 16000, 2 ** 33 + 12345
    x = make_utterance(fs, 0.3, 5310)
    sa = StreamAnalyzer(fs, 2, frame_period=5.0, chunk_ms=40, lookback_ms=40, lookahead_ms=40, aperiodicity=True)
    sa.set_rng_position(1, far)
    sa.set_d4c_rng_position(1, far)
    cs, none = sa.chunk_samples, np.zeros(0)
    acc = [dict(tpos=[], f0=[], sp=[], ap=[]) for _ in range(2)]
    at = [0, 0]  # samples fed per stream

    def push(streams):
        chunks = [x[at[u]:at[u] + cs] if u in streams else none for u in range(2)]
        flush = [1 if u in streams and at[u] + cs >= len(x) else 0 for u in range(2)]
        before = [sa.frames_committed(u) for u in range(2)]
        for u, r in enumerate(sa.push(chunks, flush)):
            for k in acc[u]:
                acc[u][k].append(r[k])
        for u in streams:
            at[u] += cs
        return [sa.frames_committed(u) - before[u] for u in range(2)]

    while sa.frames_committed(1) == 0:  # stream 1 alone until it commits frames
        push([1])
    assert at[1] < len(x) - cs
    got = push([0, 1])
    assert got[0] == 0 and got[1] > 0, got
    while at[0] < len(x):
        push([u for u in range(2) if at[u] < len(x)])
    res = [{k: np.concatenate(v) for k, v in a.items()} for a in acc]
    assert np.array_equal(res[0]["f0"], res[1]["f0"]) and np.array_equal(res[0]["tpos"], res[1]["tpos"]) and (res[0]["f0"] > 0).any()
    ends = []
    for u, start in enumerate((0, far)):
        wca.rng_set_position(start)
        want = wca.D4C(fs).compute(x, res[u]["tpos"], res[u]["f0"], sa.fft_size)
        ends.append(wca.rng_get_position())
        unv = lambda a: (a > 1.0 - 1e-9).all(axis=1)  # LoveTrain's unvoiced frames
        assert np.array_equal(unv(res[u]["ap"]), unv(want)), u
        assert np.abs(res[u]["ap"] - want).max() <= 1e-7, (u, np.abs(res[u]["ap"] - want).max())
    wca.rng_set_position(0)
    assert sa.d4c_rng_position(1) == ends[1] and sa.d4c_rng_position(0) == ends[1] - far == ends[0]
    assert sa.rng_position(1) - far == sa.rng_position(0) > 0
