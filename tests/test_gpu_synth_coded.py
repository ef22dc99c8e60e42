"""-m gpu: Synthesis from coded features (mel-cepstrum and band aperiodicity, reference src/codec.cpp): the one-pass decoder
wc_decode_features_device against the real reference's decoded rows, wc_synthesis_compute_coded_device against the reference's
Synthesis and bit for bit against decode + wc_synthesis_compute_device, the host front-end, the analysis -> coded -> synthesis
round trip, the coded stream push, and the refused calls."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("c1_16k_2s_floor71", "m24k_1s_1ms", "m48k_1s")
Y_ABS = 1e-8  # the synthesis tolerance of the other parity tests
# At fft 512 / 4096 Synthesis adds its pulses into the output with FP64 atomics, in any order (test_gpu_synthesis.py,
# include/world_class_stream.h): two runs on the same rows agree within this, not bit for bit.  The decoded rows themselves are the
# codec's bit for bit there (test_decode_features_every_size).
ATOMIC_ABS = 1e-12


def same_waveform(y, ref, fft):
    return np.array_equal(y, ref) if fft in (1024, 2048) else len(y) == len(ref) and np.abs(y - ref).max() < ATOMIC_ABS


@pytest.fixture(scope="module")
def env():
    import torch
    import world_class_amd as w
    from world_class_amd import codec
    w.lib().wc_set_device(0)
    return w, codec, torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).ravel()).cuda()


def _coded_batch(env, fs, fft, frames, first_seed, nd):
    """seeded (f0, sp, ap) per utterance (oracle/gen_golden.synth_params), coded on the device with the codec's own kernels"""
    w, codec, torch = env
    from oracle.gen_golden import synth_params
    params = [synth_params(fs, fft, n, first_seed + u) for u, n in enumerate(frames)]
    n_ap, tot = codec.number_of_aperiodicities(fs), sum(frames)
    d_sp = _dev(torch, np.concatenate([p[1] for p in params]))
    d_ap = _dev(torch, np.concatenate([p[2] for p in params]))
    d_csp = torch.empty(tot * nd, dtype=torch.float64, device="cuda")
    d_cap = torch.empty(tot * n_ap, dtype=torch.float64, device="cuda")
    codec.code_spectral_envelope_device(fs, fft, tot, nd, d_sp, d_csp)
    codec.code_aperiodicity_device(fs, fft, tot, d_ap, d_cap)
    w.lib().wc_synchronize()
    return _dev(torch, np.concatenate([p[0] for p in params])), d_csp, d_cap


@pytest.mark.parametrize("case", CASES)
def test_decode_features_golden(env, case):
    """the one-pass decoder against the real reference's decoded rows (tests/golden/io/codec_golden.npz); m48k_1s is fft 2048, the
    one-wavefront path, with nd above and below the pruned first stage's 256; the other sizes are the codec's own kernels"""
    w, codec, torch = env
    g = np.load(os.path.join(ROOT, "tests", "golden", "io", "codec_golden.npz"))
    fs, fft = int(g[case + "/fs"]), int(g[case + "/fft"])
    cap = g[case + "/ap_coded"]
    n, bins = cap.shape[0], fft // 2 + 1
    d_cap = _dev(torch, cap)
    ap_old = torch.empty(n * bins, dtype=torch.float64, device="cuda")
    codec.decode_aperiodicity_device(fs, fft, n, d_cap, ap_old)
    sp_old = {}
    for nd in (25, 60, fft // 4 + 1):
        sp_old[nd] = codec.decode_spectral_envelope(g[f"{case}/sp_coded_{nd}"], fs, fft)
        d_csp = _dev(torch, g[f"{case}/sp_coded_{nd}"])
        d_sp = torch.full((n * bins,), np.nan, dtype=torch.float64, device="cuda")
        d_ap = torch.full((n * bins,), np.nan, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()  # (torch's fills run on its own stream, the library's kernels on another)
        codec.decode_features_device(fs, fft, n, nd, d_csp, d_cap, d_sp, d_ap)
        w.lib().wc_synchronize()
        sp, ap = d_sp.cpu().numpy().reshape(n, bins), d_ap.cpu().numpy().reshape(n, bins)
        assert np.abs(sp / g[f"{case}/sp_decoded_{nd}"] - 1).max() < 1e-11, nd
        assert np.abs(ap - g[case + "/ap_decoded"]).max() < 1e-13, nd
        if fft != 2048:
            assert np.array_equal(ap, ap_old.cpu().numpy().reshape(n, bins)) and np.array_equal(sp, sp_old[nd])


def _sizes():
    return np.load(os.path.join(ROOT, "tests", "golden", "io", "codec_sizes.npz"))


def _decode_features(env, fs, fft, nd, csp, cap):
    w, codec, torch = env
    n, bins = csp.shape[0], fft // 2 + 1
    d_sp = torch.full((n * bins,), np.nan, dtype=torch.float64, device="cuda")
    d_ap = torch.full((n * bins,), np.nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    codec.decode_features_device(fs, fft, n, nd, _dev(torch, csp), _dev(torch, cap), d_sp, d_ap)
    w.lib().wc_synchronize()
    return d_sp.cpu().numpy().reshape(n, bins), d_ap.cpu().numpy().reshape(n, bins)


def _check_sizes_case(env, g, fs, fft, seed):
    """decode_features_device on the three frames of every nd of a case of tests/golden/io/codec_sizes.npz (the reference's coded
    rows at nd <= fft/4+1, the decode-only rows up to fft/2), each frame paired with another of the coded aperiodicity rows (the
    reference's and the hand-made ones: exact mean -0.5, an ulp above, -60 dB, above 0 dB, a NaN band); at fft != 2048 also bit for
    bit the codec's two decoders"""
    w, codec, torch = env
    from oracle.gen_golden_codec_sizes import case_data, close_ap, sp_decode_cases
    sp, ap, only, cap_all, k = case_data(g, fs, fft, seed)
    for i, (nd, csp, ref) in enumerate(sp_decode_cases(g, k, fft, only)):
        rows = [(3 * i + j) % len(cap_all) for j in range(len(csp))]
        cap = cap_all[rows]
        dsp, dap = _decode_features(env, fs, fft, nd, csp, cap)
        assert np.abs(dsp / ref - 1).max() < 1e-11, (fs, nd)
        assert close_ap(dap, g[k + "ap_decoded"][rows]), (fs, nd)
        if fft != 2048:
            assert np.array_equal(dsp, codec.decode_spectral_envelope(csp, fs, fft)), (fs, nd)
            assert np.array_equal(dap, codec.decode_aperiodicity(cap, fs, fft), equal_nan=True), (fs, nd)


def _sizes_cases_from(fs_min):
    from oracle.gen_golden_codec_sizes import CASES
    return [c for c in CASES if c[0] >= fs_min]


@pytest.mark.parametrize("fs,fft,seed", _sizes_cases_from(12000))
def test_decode_features_every_size(env, fs, fft, seed):
    """every case of the sizes fixture that coded Synthesis accepts: fft 512 .. 4096, 1 .. 5 bands; at fft 2048 the one-wavefront
    decoder either side of its pruned first stage (nd 256 / 257), at nd 1 and up to fft/2"""
    _check_sizes_case(env, _sizes(), fs, fft, seed)


def test_decode_features_plan_cache(env):
    """the one-wavefront decoder keeps a plan per (device, fs): four rates in turn in one process, one of them again, each against
    its own reference rows"""
    g = _sizes()
    seeds = {fs: seed for fs, fft, seed in _sizes_cases_from(12000) if fft == 2048}
    for fs in (16000, 32000, 44100, 32000):
        _check_sizes_case(env, g, fs, 2048, seeds[fs])


def test_compute_coded_matches_reference(env, port, checker):
    """a seeded 48 kHz signal analysed by the reference, coded and decoded by the reference's codec, synthesised by the reference
    (the real one where oracle/_ref is built) from noise position 0: compute_coded on the coded rows within 1e-8"""
    w, codec, torch = env
    from oracle import port_codec as pc
    from world_class_amd.synth import make_utterance
    fs, fft, nd = 48000, 2048, 60
    port.rng_reset()
    r = port.pipeline(make_utterance(fs, 0.6, 77), fs)
    f0, sp, ap = r["f0"], r["sp"], r["ap"]
    csp, cap = pc.code_spectral_envelope(sp, fs, fft, nd), pc.code_aperiodicity(ap, fs, fft)
    sp_d, ap_d = pc.decode_spectral_envelope(csp, fs, fft), pc.decode_aperiodicity(cap, fs, fft)
    port.rng_seek(0)
    y_ref = port.synthesis(f0, sp_d, ap_d, fs, 5.0)
    end = port.rng_position()
    if checker is not None:
        y_ref = checker.stage_at(0, "synthesis", f0, sp_d, ap_d, fs, 5.0)
    w.rng_set_position(0)
    y = w.Synthesis(fs, fft, 5.0).compute_coded(f0, csp, cap)
    assert w.rng_get_position() == end
    w.rng_set_position(0)
    assert len(y) == len(y_ref) and np.abs(y - y_ref).max() < Y_ABS


@pytest.mark.parametrize("fs,fft,nd", [(12000, 512, 40), (16000, 2048, 300), (44100, 2048, 60), (96000, 4096, 1025)])
def test_compute_coded_matches_reference_sizes(env, port, checker, fs, fft, nd):
    """seeded rows (oracle/gen_golden.synth_params) coded and decoded by the reference's codec (its restatement, pinned by
    tests/test_codec_oracle.py), synthesised by the reference (the real one where oracle/_ref is built) from noise position 0:
    compute_coded on the coded rows within 1e-8, and the same end position.  fft 512 and 4096 decode with the codec's workgroup
    kernels, fft 2048 with the one-wavefront decoder (nd 300: the unpruned first stage)"""
    w, codec, torch = env
    from oracle import port_codec as pc
    from oracle.gen_golden import synth_params
    f0, sp, ap = synth_params(fs, fft, 70, 4000 + fs // 1000)
    csp, cap = pc.code_spectral_envelope(sp, fs, fft, nd), pc.code_aperiodicity(ap, fs, fft)
    sp_d, ap_d = pc.decode_spectral_envelope(csp, fs, fft), pc.decode_aperiodicity(cap, fs, fft)
    port.rng_seek(0)
    y_ref = port.synthesis(f0, sp_d, ap_d, fs, 5.0)
    end = port.rng_position()
    if checker is not None:
        y_ref = checker.stage_at(0, "synthesis", f0, sp_d, ap_d, fs, 5.0)
    w.rng_set_position(0)
    y = w.Synthesis(fs, fft, 5.0).compute_coded(f0, csp, cap)
    assert w.rng_get_position() == end
    w.rng_set_position(0)
    assert len(y) == len(y_ref) and np.abs(y - y_ref).max() < Y_ABS


@pytest.mark.parametrize("fs,fft", [(24000, 1024), (48000, 2048), (12000, 512), (96000, 4096)])
@pytest.mark.parametrize("n_utt", [4, 16])
def test_coded_device_equals_decode_then_synthesis(env, fs, fft, n_utt):
    """compute_coded_device == wc_decode_features_device + wc_synthesis_compute_device, with the same end positions, on both
    Synthesis paths (n_utt >= 16: the two halves with the twin handle); bit for bit at fft 1024 / 2048, within ATOMIC_ABS at 512 /
    4096 (the decode there is the codec's workgroup kernels, called inside the handle's device lock)"""
    w, codec, torch = env
    nd = 40
    frames = [60 + 37 * (u % 5) for u in range(n_utt)]
    d_f0, d_csp, d_cap = _coded_batch(env, fs, fft, frames, 500, nd)
    syn = w.Synthesis(fs, fft, 5.0)
    ol = [syn.out_length(n) for n in frames]
    start = [1000 * u + 7 for u in range(n_utt)]
    tot, bins = sum(frames), fft // 2 + 1
    d_sp = torch.empty(tot * bins, dtype=torch.float64, device="cuda")
    d_ap = torch.empty(tot * bins, dtype=torch.float64, device="cuda")
    codec.decode_features_device(fs, fft, tot, nd, d_csp, d_cap, d_sp, d_ap)
    y_ref = torch.zeros(sum(ol), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    end_ref = syn.compute_device(d_f0, frames, d_sp, d_ap, ol, y_ref, rng_pos=start)
    y_ref = y_ref.cpu().numpy()
    y = torch.full((sum(ol),), np.nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    end = syn.compute_coded_device(d_f0, frames, d_csp, nd, d_cap, ol, y, rng_pos=start)
    assert end == end_ref
    assert same_waveform(y.cpu().numpy(), y_ref, fft)


def test_host_front_end_coded(env):
    """compute_batch_coded (ragged host arrays through page-locked staging) == the device call bit for bit; with y_pcm16 it is
    wc_double_to_pcm16_device of that waveform"""
    _host_front_end(env, 48000, 2048)


def test_host_front_end_coded_96k(env):
    """the same at fft 4096, where the decode is the codec's workgroup kernels inside the handle's device lock: within ATOMIC_ABS,
    and the int16 samples equal but where the waveform lies within 1e-7 LSB of a truncation step"""
    _host_front_end(env, 96000, 4096)


def _host_front_end(env, fs, fft):
    w, codec, torch = env
    from world_class_amd import io as wio
    nd = 60
    frames = [91, 203, 57, 150, 120]
    d_f0, d_csp, d_cap = _coded_batch(env, fs, fft, frames, 900, nd)
    n_ap = codec.number_of_aperiodicities(fs)
    f0, csp, cap = d_f0.cpu().numpy(), d_csp.cpu().numpy().reshape(-1, nd), d_cap.cpu().numpy().reshape(-1, n_ap)
    cut = np.cumsum([0] + frames)
    f0s = [f0[a:b] for a, b in zip(cut[:-1], cut[1:])]
    csps = [csp[a:b] for a, b in zip(cut[:-1], cut[1:])]
    caps = [cap[a:b] for a, b in zip(cut[:-1], cut[1:])]
    syn = w.Synthesis(fs, fft, 5.0)
    ol = [syn.out_length(n) + d for n, d in zip(frames, (0, -100, 37, 0, 5))]
    start = [11, 0, 123456, 5, 999]
    d_y = torch.zeros(sum(ol), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    end_dev = syn.compute_coded_device(d_f0, frames, d_csp, nd, d_cap, ol, d_y, rng_pos=start)
    ys, end = syn.compute_batch_coded(f0s, csps, caps, out_lengths=ol, rng_pos=start)
    assert end == end_dev
    yo = np.cumsum([0] + ol)
    y_dev = d_y.cpu().numpy()
    for u, y in enumerate(ys):
        assert same_waveform(y, y_dev[yo[u]:yo[u + 1]], fft), u
    d_pcm = torch.empty(sum(ol), dtype=torch.int16, device="cuda")
    wio.double_to_pcm16_device(d_y, sum(ol), d_pcm)
    w.lib().wc_synchronize()
    pcm = d_pcm.cpu().numpy()
    ys16, end16 = syn.compute_batch_coded(f0s, csps, caps, out_lengths=ol, y_pcm16=True, rng_pos=start)
    assert end16 == end_dev
    for u, y in enumerate(ys16):
        ref = pcm[yo[u]:yo[u + 1]]
        assert y.dtype == np.int16 and len(y) == len(ref), u
        if fft in (1024, 2048):
            assert np.array_equal(y, ref), u
        else:  # (wc_double_to_pcm16_device truncates y * 32767: a step is crossed only by a sample that lies on it)
            v = y_dev[yo[u]:yo[u + 1]][y != ref] * 32767
            assert np.abs(y.astype(np.int64) - ref).max() <= 1 and (np.abs(v - np.round(v)) < 1e-7).all(), u


def test_round_trip_analysis_coded_synthesis(env, port, checker):
    """Pipeline.run_batch_host_coded on a seeded 48 kHz batch; its f0 / csp / cap into compute_batch_coded from the pipeline's end
    positions; against the reference's codec decoding the same rows and the reference's Synthesis from those positions"""
    w, codec, torch = env
    from oracle import port_codec as pc
    from world_class_amd.synth import make_utterance
    fs, nd = 48000, 60
    xs = [make_utterance(fs, sec, seed) for sec, seed in ((0.5, 61), (0.35, 62), (0.8, 63))]
    p = w.Pipeline(fs)
    fft = p.fft_size
    coded, pos = p.run_batch_host_coded(xs, number_of_dimensions=nd, want=("f0", "csp", "cap"), rng_pos=[0] * len(xs))
    syn = w.Synthesis(fs, fft, 5.0)
    ys, _ = syn.compute_batch_coded([c["f0"] for c in coded], [c["csp"] for c in coded], [c["cap"] for c in coded], rng_pos=pos)
    for u, c in enumerate(coded):
        sp_d, ap_d = pc.decode_spectral_envelope(c["csp"], fs, fft), pc.decode_aperiodicity(c["cap"], fs, fft)
        port.rng_seek(pos[u])
        y_ref = port.synthesis(c["f0"], sp_d, ap_d, fs, 5.0)
        if checker is not None:
            try:
                y_ref = checker.stage_at(pos[u], "synthesis", c["f0"], sp_d, ap_d, fs, 5.0)
            except Exception:  # (the reference's Synthesis overflows its pulse arrays on some contours: DESIGN.md section 8)
                print("round trip, utterance %d: the real reference crashed; the CPU restatement answers" % u)
        assert len(ys[u]) == len(y_ref) and np.abs(ys[u] - y_ref).max() < Y_ABS, u


@pytest.mark.parametrize("fs,fft", [(24000, 1024), (48000, 2048), (12000, 512), (96000, 4096)])
def test_stream_push_coded_equals_batch(env, fs, fft):
    """uneven push_coded pushes across 8 streams reproduce one compute_coded_device call per stream, bit for bit at fft 1024 / 2048
    and within 1e-12 at 512 / 4096 (what include/world_class_stream.h promises there); a refused push in the middle (nd out of
    range) leaves every stream as it was"""
    w, codec, torch = env
    from world_class_amd.stream import StreamSynthesizer
    nd, n = 30, 8
    frames = [80 + 23 * u for u in range(n)]
    d_f0, d_csp, d_cap = _coded_batch(env, fs, fft, frames, 300, nd)
    n_ap = codec.number_of_aperiodicities(fs)
    f0, csp, cap = d_f0.cpu().numpy(), d_csp.cpu().numpy().reshape(-1, nd), d_cap.cpu().numpy().reshape(-1, n_ap)
    cut = np.cumsum([0] + frames)
    syn = w.Synthesis(fs, fft, 5.0)
    ref = []
    for u in range(n):
        a, b = cut[u], cut[u + 1]
        y = torch.zeros(syn.out_length(frames[u]), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        syn.compute_coded_device(_dev(torch, f0[a:b]), [frames[u]], _dev(torch, csp[a:b]), nd, _dev(torch, cap[a:b]), [len(y)], y, rng_pos=[0])
        ref.append(y.cpu().numpy())
    pattern = [[1, 7, 40], [33, 0, 1], [7, 0, 0, 40], [50], [2], [13, 27, 0], [40, 7, 1, 0], [19, 50]]
    st = StreamSynthesizer(fs, fft, 5.0, n, 50)
    pos, k, done, acc = [0] * n, [0] * n, [False] * n, [[] for _ in range(n)]
    pushes = 0
    while not all(done):
        f0s, csps, caps, flush = [], [], [], []
        for u in range(n):
            c = 0 if done[u] else min(pattern[u][k[u] % len(pattern[u])], frames[u] - pos[u])
            k[u] += 1
            a = cut[u] + pos[u]
            f0s.append(f0[a:a + c])
            csps.append(csp[a:a + c])
            caps.append(cap[a:a + c])
            flush.append(1 if not done[u] and pos[u] + c >= frames[u] else 0)
            pos[u] += c
        if pushes == 3:
            before = [(st.frames_received(u), st.samples_committed(u), st.rng_position(u)) for u in range(n)]
            d = [_dev(torch, np.concatenate(v)) for v in (f0s, csps, caps)]
            for bad_nd in (0, fft // 2 + 1):
                with pytest.raises(w.WorldClassError):
                    st.push_coded_device([len(v) for v in f0s], d[0], d[1], bad_nd, d[2], flush)
            assert before == [(st.frames_received(u), st.samples_committed(u), st.rng_position(u)) for u in range(n)]
        for u, y in enumerate(st.push_coded(f0s, csps, caps, flush)):
            acc[u].append(y)
        for u in range(n):
            done[u] = done[u] or bool(flush[u])
        pushes += 1
    for u in range(n):
        assert same_waveform(np.concatenate(acc[u]), ref[u], fft), u


def test_coded_calls_refuse_bad_arguments(env):
    """nd = 0, nd > fft/2, fs = 8000 and a null coded table are refused; the noise positions and the outputs stay as they were"""
    w, codec, torch = env
    L = w.lib()
    fs, fft, nd = 48000, 2048, 20
    frames = [40, 50]
    d_f0, d_csp, d_cap = _coded_batch(env, fs, fft, frames, 700, nd)
    syn, syn8 = w.Synthesis(fs, fft, 5.0), w.Synthesis(8000, 1024, 5.0)
    ol = [syn.out_length(n) for n in frames]
    ints = lambda v: (C.c_int * len(v))(*v)
    ptr = lambda a: a if isinstance(a, int) else a.data_ptr()
    y = torch.full((sum(ol),), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for h, a_csp, a_nd, a_cap in ((syn, d_csp, 0, d_cap), (syn, d_csp, fft // 2 + 1, d_cap), (syn8, d_csp, nd, d_cap), (syn, 0, nd, d_cap),
                                  (syn, d_csp, nd, 0)):
        pos = (C.c_uint64 * 2)(5, 9)
        rc = L.wc_synthesis_compute_coded_device(h._h, 2, d_f0.data_ptr(), ints(frames), ptr(a_csp), a_nd, ptr(a_cap), ints(ol),
                                                 y.data_ptr(), pos)
        assert rc == -1 and w.last_error()
        assert list(pos) == [5, 9]
    L.wc_synchronize()
    assert bool((y == 7.0).all())
    n_ap = codec.number_of_aperiodicities(fs)
    f0 = d_f0.cpu().numpy()
    csp, cap = d_csp.cpu().numpy().reshape(-1, nd), d_cap.cpu().numpy().reshape(-1, n_ap)
    VP = C.c_void_p * 2
    f0s, csps, caps = [f0[:40].copy(), f0[40:].copy()], [csp[:40].copy(), csp[40:].copy()], [cap[:40].copy(), cap[40:].copy()]
    ys = [np.full(n, 3.0) for n in ol]
    tab = lambda arrs: VP(*[a.ctypes.data if a is not None else None for a in arrs])
    for h, t_csp, a_nd in ((syn, tab(csps), 0), (syn, tab(csps), fft // 2 + 1), (syn8, tab(csps), nd), (syn, tab([csps[0], None]), nd), (syn, None, nd)):
        pos = (C.c_uint64 * 2)(5, 9)
        rc = L.wc_synthesis_run_batch_host_coded(h._h, 2, tab(f0s), ints(frames), t_csp, a_nd, tab(caps), ints(ol), tab(ys), 0, pos)
        assert rc == -1 and w.last_error()
        assert list(pos) == [5, 9]
    assert all((v == 3.0).all() for v in ys)
    d = torch.empty(4096, dtype=torch.float64, device="cuda")
    for args in ((fs, fft, 1, 0), (fs, fft, 1, fft // 2 + 1), (8000, 1024, 1, nd)):
        with pytest.raises(w.WorldClassError):
            codec.decode_features_device(*args, d, d, d, d)
    with pytest.raises(w.WorldClassError):
        codec.decode_features_device(fs, fft, 1, nd, 0, d, d, d)
