"""-m gpu: Synthesis at 48 kHz with the pulse kernel split by class (syn_pulse_wave_kernel<., 1> on the voiced pulses, <., 2> on the
unvoiced ones, one launch per device-built class list) against its single-launch twin (WC_SYN_SPLIT=0): the same bits in y and the
same noise positions, on the contours where the two kernels differ from the one -- an unvoiced pulse whose noise takes the generic
path, an empty list of either class, voiced pulses without a periodic part, ragged batches, noise positions per utterance -- and
against the CPU restatement, on a second run, and through the synthesis streams.

Synthesis alone, fft_size 2048, 5 ms hop, contours of 0.3 - 0.6 s built here (as test_aperiodicity_next_to_its_clamp builds its)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FS, FFT, FP = 48000, 2048, 5.0
Y_ABS = 1e-8  # tests/test_gpu_synthesis.py


@pytest.fixture(scope="module")
def wca():
    import world_class_amd as w
    w.lib()
    return w


def _rows(nfr, seed, ap_all=None):
    """smooth random spectrogram rows and aperiodicity rows that rise from 0.001 at bin 0 (a periodic part wherever F0 > 0)"""
    rng = np.random.default_rng(seed)
    bins = FFT // 2 + 1
    k = np.arange(bins) / (bins - 1.0)
    sp = np.stack([1e-4 + 1e-2 * np.exp(-((k - rng.uniform(0.1, 0.3)) / 0.05) ** 2) for _ in range(nfr)])
    ap = np.stack([np.interp(k, [0.0, 0.3, 0.6, rng.uniform(0.7, 0.9), 1.0], [0.001, rng.uniform(0.05, 0.4), rng.uniform(0.5, 0.99), 0.995, 0.999])
                   for _ in range(nfr)])
    if ap_all is not None:
        ap[:] = ap_all
    return sp, ap


def _mixed(nfr, seed):
    """voiced 180 Hz, an unvoiced gap, voiced 72 Hz: the last unvoiced pulse's interval (up to the first 72 Hz pulse) exceeds 512
    samples -- the generic noise path inside the unvoiced kernel; the gap's aperiodicity rows stay arbitrary (never read)"""
    f0 = np.zeros(nfr)
    f0[:nfr * 35 // 100] = 180.0
    f0[nfr * 60 // 100:] = 72.0
    return (f0,) + _rows(nfr, seed)


def _cases():
    c = {}
    c["mixed"] = ([_mixed(100, 1)], [0])
    c["unvoiced"] = ([(np.zeros(80),) + _rows(80, 2)], [0])                                   # the voiced list is empty
    c["voiced"] = ([(140.0 + 20.0 * np.sin(np.arange(90) / 9.0),) + _rows(90, 3)], [0])     # unvoiced: the edge pulses at most
    c["clamped"] = ([(np.full(70, 150.0),) + _rows(70, 4, ap_all=1.0 - 1e-12)], [0])         # aperiodic_ratio[0] > 0.999: voiced, no periodic part
    gap = np.full(90, 80.0)
    gap[40] = 0.0                                                                            # 240 samples unvoiced inside a 600-sample interval
    # (two frames, one frame interval: the shortest contour the stage takes -- f0_length >= 2, reference src/synthesis.cpp:241-242)
    c["ragged"] = ([(np.full(2, 200.0),) + _rows(2, 5), (np.zeros(70),) + _rows(70, 6, ap_all=1.0 - 1e-12),
                    (gap,) + _rows(90, 7), _mixed(60, 8)], [0, 10, 0, 5])
    c["positions"] = ([_mixed(64, 9), (np.zeros(61),) + _rows(61, 10), _mixed(77, 11)], [12345, 7, 999983])
    return c


def _run(wca, params, start):
    s = wca.Synthesis(FS, FFT, FP)
    ys, pos = s.compute_batch([p[0] for p in params], [p[1] for p in params], [p[2] for p in params], rng_pos=list(start))
    return ys, list(pos)


@pytest.fixture(scope="module")
def runs(wca):
    """every case once through the split launch (the default) and once through its twin"""
    cases = _cases()
    out = {}
    for name, (params, start) in cases.items():
        out[name] = {"params": params, "start": start, "split": _run(wca, params, start)}
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("WC_SYN_SPLIT", "0")  # (read when the handle is created)
        for name, (params, start) in cases.items():
            out[name]["twin"] = _run(wca, params, start)
    return out


@pytest.mark.parametrize("name", ["mixed", "unvoiced", "voiced", "clamped", "ragged", "positions"])
def test_split_launch_gives_the_bits_of_the_single_launch(runs, name):
    r = runs[name]
    (ys, pos), (yt, post) = r["split"], r["twin"]
    assert pos == post
    assert max(np.abs(b).max() for b in yt) > 1e-4  # (there is a waveform to compare; the two-frame utterance's own is silent)
    for u, (a, b) in enumerate(zip(ys, yt)):
        assert len(a) == len(b)
        assert np.array_equal(a, b), (name, u, float(np.abs(a - b).max()))


@pytest.mark.parametrize("name", ["mixed", "ragged"])
def test_split_launch_against_the_cpu_restatement(runs, port, name):
    r = runs[name]
    ys, pos = r["split"]
    for (f0, sp, ap), y, p0, p1 in zip(r["params"], ys, r["start"], pos):
        port.rng_seek(p0)
        ref = port.synthesis(f0, sp, ap, FS, FP)
        assert port.rng_position() == p1
        worst = float(np.abs(y - ref).max())
        print(name, len(f0), worst)
        assert worst < Y_ABS
    port.rng_reset()


def test_split_launch_same_bits_on_a_second_run(wca, runs):
    """ordered sums of response rows, no atomics: a fresh handle gives the same bits"""
    r = runs["mixed"]
    ys, pos = _run(wca, r["params"], r["start"])
    assert pos == r["split"][1]
    assert np.array_equal(ys[0], r["split"][0][0])


def test_split_launch_in_the_synthesis_streams(wca, runs):
    """wc_synth_stream at 48 kHz launches the same two kernels on the pulses of a push: two pushes over the mixed contour, bit for
    bit the stage call (as tests/test_gpu_synth_stream.py compares them)"""
    from world_class_amd.stream import StreamSynthesizer
    r = runs["mixed"]
    params = r["params"]
    nfr = len(params[0][0])
    st = StreamSynthesizer(FS, FFT, FP, 1, nfr // 2)
    ys = st.run_whole(params, [[nfr // 2]])
    assert len(ys[0]) == wca.synthesis_out_length(nfr, FP, FS)
    assert np.array_equal(ys[0], r["split"][0][0])
