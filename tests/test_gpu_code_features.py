"""-m gpu: feature coding on the device (wc_code_features_device, wc_pipeline_run_coded_device, wc_stream_push_coded_device):
the one-pass coder against the real reference's coded rows at every size, against the CPU restatement on analysis rows, its frame
independence and stream ordering, the coded pipeline step and the coded analysis push against their plain twins bit for bit, the
loop analysis stream -> synthesis stream in the coded domain, and the refused calls.  The bound on coded values is the 1e-11 that
test_gpu_codec.py::test_codec_golden and test_gpu_codec_sizes.py::test_codec_sizes_device hold the single coders to."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle.gen_golden_codec_sizes import CASES, RAMP_ONLY, case_data, code_nds

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-11
GOLDEN_CASES = ("c1_16k_2s_floor71", "m24k_1s_1ms", "m48k_1s")


@pytest.fixture(scope="module")
def env():
    import torch
    import world_class_amd as w
    from world_class_amd import codec
    w.lib().wc_set_device(0)
    return w, codec, torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).ravel()).cuda()


def _code(env, fs, fft, nd, sp, ap=None):
    """(coded sp, coded ap or None) of the rows through wc_code_features_device; the outputs are NaN-filled with a guard row
    behind them that must stay NaN"""
    w, codec, torch = env
    n = len(sp)
    n_ap = codec.number_of_aperiodicities(fs) if ap is not None else 0
    d_sp = _dev(torch, sp) if n else torch.zeros(1, dtype=torch.float64, device="cuda")
    d_ap = (_dev(torch, ap) if n else torch.zeros(1, dtype=torch.float64, device="cuda")) if ap is not None else None
    d_csp = torch.full(((n + 1) * nd,), np.nan, dtype=torch.float64, device="cuda")
    d_cap = torch.full(((n + 1) * max(n_ap, 1),), np.nan, dtype=torch.float64, device="cuda") if ap is not None else None
    torch.cuda.synchronize()  # (torch's fills run on its own stream, the library's kernels on another)
    codec.code_features_device(fs, fft, n, nd, d_sp, d_ap, d_csp, d_cap)
    w.lib().wc_synchronize()
    csp = d_csp.cpu().numpy()
    assert np.isnan(csp[n * nd:]).all(), "the coder wrote behind its last row"
    cap = None
    if ap is not None:
        cap = d_cap.cpu().numpy()
        assert np.isnan(cap[n * n_ap:]).all(), "the coder wrote behind its last row"
        cap = cap[:n * n_ap].reshape(n, n_ap)
    return csp[:n * nd].reshape(n, nd), cap


_rows_cache = {}


def _analysis_rows(fs):
    """sp / ap rows of one make_utterance signal through the CPU restatement's pipeline, as test_codec_device_batch_vs_oracle makes them"""
    if fs == 96000 and fs not in _rows_cache:  # (frame independence at fft 4096 only: seeded rows, no 96 kHz analysis on the CPU)
        from oracle.gen_golden import synth_params
        _, sp, ap = synth_params(fs, 4096, 101, 9696)
        _rows_cache[fs] = (np.ascontiguousarray(sp), np.ascontiguousarray(ap))
    if fs not in _rows_cache:
        from oracle import port
        from world_class_amd.synth import make_utterance
        P = port.Port()
        P.rng_reset()
        r = P.pipeline(make_utterance(fs, 0.5, 99 + fs // 1000), fs)
        P.rng_reset()
        _rows_cache[fs] = (np.ascontiguousarray(r["sp"]), np.ascontiguousarray(r["ap"]))
    return _rows_cache[fs]


# ---- 1. against the real reference ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fs,fft,seed", [c for c in CASES if c[0] not in RAMP_ONLY])
def test_code_features_every_size_against_the_reference(env, fs, fft, seed):
    """every case of codec_sizes.npz, every code_nds(fft), both outputs; sp only where there is no band (8 kHz)"""
    w, codec, torch = env
    g = np.load(os.path.join(ROOT, "tests", "golden", "io", "codec_sizes.npz"))
    sp, ap, only, cap_in, k = case_data(g, fs, fft, seed)
    n_ap = int(g[k + "n_ap"])
    assert n_ap == codec.number_of_aperiodicities(fs)
    pick = np.arange(len(ap)) % len(sp)  # three sp rows, five ap rows: the sp rows repeat
    for nd in code_nds(fft):
        csp, cap = _code(env, fs, fft, nd, sp[pick], ap if n_ap else None)
        err = np.abs(csp - g[k + "sp_coded"][pick, :nd]).max()
        print("fs %d fft %d nd %d: max |coded sp - reference| = %.3e" % (fs, fft, nd, err))
        assert err < TOL, nd
        if n_ap:
            err = np.abs(cap - g[k + "ap_coded"]).max()
            print("fs %d fft %d nd %d: max |coded ap - reference| = %.3e" % (fs, fft, nd, err))
            assert err < TOL, nd
    csp, _ = _code(env, fs, fft, 1, sp)  # sp only is accepted at every rate
    assert np.abs(csp - g[k + "sp_coded"][:, :1]).max() < TOL


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_code_features_golden(env, case):
    w, codec, torch = env
    g = np.load(os.path.join(ROOT, "tests", "golden", "io", "codec_golden.npz"))
    fs, fft = int(g[case + "/fs"]), int(g[case + "/fft"])
    for nd in (25, 60, fft // 4 + 1):
        csp, cap = _code(env, fs, fft, nd, g[case + "/sp"], g[case + "/ap"])
        e1, e2 = np.abs(csp - g[f"{case}/sp_coded_{nd}"]).max(), np.abs(cap - g[case + "/ap_coded"]).max()
        print("%s nd %d: max |coded - reference| sp %.3e ap %.3e" % (case, nd, e1, e2))
        assert e1 < TOL and e2 < TOL, nd


# ---- 2. more frames than the fixtures have -----------------------------------------------------------------------------------

@pytest.mark.parametrize("fs,fft", [(48000, 2048), (24000, 1024)])
@pytest.mark.parametrize("rows", [3, 16])
def test_code_features_analysis_rows_against_the_restatement(env, fs, fft, rows):
    from oracle import port_codec as pc
    sp, ap = _analysis_rows(fs)
    idx = np.linspace(0, len(sp) - 1, rows).astype(int)
    for nd in (25, 60, fft // 4 + 1):
        csp, cap = _code(env, fs, fft, nd, sp[idx], ap[idx])
        e1 = np.abs(csp - pc.code_spectral_envelope(sp[idx], fs, fft, nd)).max()
        e2 = np.abs(cap - pc.code_aperiodicity(ap[idx], fs, fft)).max()
        print("fs %d, %d rows, nd %d: max |coded - restatement| sp %.3e ap %.3e" % (fs, rows, nd, e1, e2))
        assert e1 < TOL and e2 < TOL, nd


# ---- 3. frame independence ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fs,fft", [(48000, 2048), (24000, 1024), (96000, 4096)])
def test_a_frames_coded_row_depends_on_that_frame_alone(env, fs, fft):
    w, codec, torch = env
    sp0, ap0 = _analysis_rows(fs)
    n, nd = 131, 60
    idx = (np.arange(n) * 7) % len(sp0)
    scale = 1.0 + 0.01 * np.arange(n)[:, None]
    sp, ap = sp0[idx] * scale, np.minimum(ap0[idx] * (1.0 - 1e-3 * np.arange(n)[:, None] / n), 1.0)
    csp, cap = _code(env, fs, fft, nd, sp, ap)
    assert np.isfinite(csp).all() and np.isfinite(cap).all()
    r_csp, r_cap = _code(env, fs, fft, nd, sp[::-1], ap[::-1])
    assert np.array_equal(r_csp[::-1], csp) and np.array_equal(r_cap[::-1], cap)
    for i in (0, 1, 63, 64, 65, 130):
        c1, a1 = _code(env, fs, fft, nd, sp[i:i + 1], ap[i:i + 1])
        assert np.array_equal(c1[0], csp[i]) and np.array_equal(a1[0], cap[i]), i
    big_sp, big_ap = np.concatenate([sp0[:37], sp, sp0[:50]]), np.concatenate([ap0[:37], ap, ap0[:50]])
    b_csp, b_cap = _code(env, fs, fft, nd, big_sp, big_ap)
    assert np.array_equal(b_csp[37:37 + n], csp) and np.array_equal(b_cap[37:37 + n], cap)
    e_csp, e_cap = _code(env, fs, fft, nd, sp[:0], ap[:0])  # n_frames 0: a no-op
    assert e_csp.shape == (0, nd) and e_cap.shape[0] == 0
    s_csp, none = _code(env, fs, fft, nd, sp)  # sp only: the same bits
    assert none is None and np.array_equal(s_csp, csp)


# ---- 4. no hidden synchronisation, the caller's stream, the plan cache --------------------------------------------------------

def test_code_features_is_ordered_on_the_callers_stream_and_keys_its_plans(env):
    w, codec, torch = env
    from oracle import port_codec as pc
    sp48, ap48 = _analysis_rows(48000)
    sp24, ap24 = _analysis_rows(24000)
    nd, n = 60, 64
    combos = [(48000, 2048, sp48[:n], ap48[:n]), (24000, 1024, sp24[:n], ap24[:n]), (44100, 2048, sp48[:n], ap48[:n]),
              (16000, 1024, sp24[:n], ap24[:n])]
    want = [(pc.code_spectral_envelope(sp, fs, fft, nd), pc.code_aperiodicity(ap, fs, fft)) for fs, fft, sp, ap in combos]
    host = [(torch.from_numpy(sp.ravel().copy()).pin_memory(), torch.from_numpy(ap.ravel().copy()).pin_memory()) for _, _, sp, ap in combos]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert w.lib().wc_set_stream(s.cuda_stream) == 0
    try:
        outs = []
        with torch.cuda.stream(s):
            junk = torch.randn(2048, 2048, device="cuda")
            for _ in range(20):  # a long-running kernel in front: the coder must wait for it and for the uploads behind it
                junk = junk @ junk * 1e-3
            for rnd in range(2):  # the four plans interleaved, twice: the second round finds them cached
                for (fs, fft, sp, ap), (h_sp, h_ap) in zip(combos, host):
                    n_ap = codec.number_of_aperiodicities(fs)
                    d_sp = torch.zeros(n * (fft // 2 + 1), dtype=torch.float64, device="cuda")
                    d_ap = torch.zeros(n * (fft // 2 + 1), dtype=torch.float64, device="cuda")
                    d_csp = torch.full((n * nd,), np.nan, dtype=torch.float64, device="cuda")
                    d_cap = torch.full((n * n_ap,), np.nan, dtype=torch.float64, device="cuda")
                    d_sp.copy_(h_sp, non_blocking=True)
                    d_ap.copy_(h_ap, non_blocking=True)
                    d_sp.mul_(1.0)  # a torch kernel on the stream writes the rows
                    codec.code_features_device(fs, fft, n, nd, d_sp, d_ap, d_csp, d_cap)
                    outs.append((d_sp, d_ap, d_csp, d_cap))
        s.synchronize()  # once
    finally:
        assert w.lib().wc_set_stream(None) == 0
    for i, (_, _, d_csp, d_cap) in enumerate(outs):
        ref_csp, ref_cap = want[i % 4]
        assert np.abs(d_csp.cpu().numpy().reshape(n, nd) - ref_csp).max() < TOL, i
        assert np.abs(d_cap.cpu().numpy().reshape(n, -1) - ref_cap).max() < TOL, i
    for i in range(4):
        assert torch.equal(outs[i][2], outs[i + 4][2]) and torch.equal(outs[i][3], outs[i + 4][3])


# ---- 5. pipeline -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fs", [16000, 48000])
@pytest.mark.parametrize("n_utt", [4, 16])
def test_pipeline_run_coded_device_equals_run_device_then_the_coder(env, fs, n_utt):
    w, codec, torch = env
    from oracle import port_codec as pc
    from world_class_amd.synth import make_utterance
    nd = 60
    xs = [make_utterance(fs, 0.3 + 0.05 * ((u * 5) % 7), 400 + u) for u in range(n_utt)]
    xl = [len(x) for x in xs]
    p = w.Pipeline(fs)
    fft, bins = p.fft_size, p.bins
    assert fft == (2048 if fs == 48000 else 1024)
    fl, yl = p.lengths(xl)
    nf, n_ap = sum(fl), codec.number_of_aperiodicities(fs)
    d_x = _dev(torch, np.concatenate(xs))
    z = lambda n, v=0.0: torch.full((n,), v, dtype=torch.float64, device="cuda")
    t1, f1, sp1, ap1, y1 = z(nf), z(nf), z(nf * bins), z(nf * bins), z(sum(yl))
    t2, f2, y2 = z(nf), z(nf), z(sum(yl))
    csp, cap = z(nf * nd, np.nan), z(nf * n_ap, np.nan)
    start = [11 * u for u in range(n_utt)]
    torch.cuda.synchronize()
    pos1 = p.run_device(d_x, xl, t1, f1, sp1, ap1, y1, rng_pos=start)
    pos2 = p.run_coded_device(d_x, xl, t2, f2, csp, nd, cap, y2, rng_pos=start)
    w.lib().wc_synchronize()
    assert pos1 == pos2
    assert torch.equal(t1, t2) and torch.equal(f1, f2) and torch.equal(y1, y2)
    c2, a2 = z(nf * nd, np.nan), z(nf * n_ap, np.nan)
    torch.cuda.synchronize()
    codec.code_features_device(fs, fft, nf, nd, sp1, ap1, c2, a2)
    w.lib().wc_synchronize()
    assert torch.equal(csp, c2) and torch.equal(cap, a2)
    sp, ap = sp1.cpu().numpy().reshape(nf, bins), ap1.cpu().numpy().reshape(nf, bins)
    e1 = np.abs(csp.cpu().numpy().reshape(nf, nd) - pc.code_spectral_envelope(sp, fs, fft, nd)).max()
    e2 = np.abs(cap.cpu().numpy().reshape(nf, n_ap) - pc.code_aperiodicity(ap, fs, fft)).max()
    print("pipeline fs %d, %d utterances: max |coded - restatement| sp %.3e ap %.3e" % (fs, n_utt, e1, e2))
    assert e1 < TOL and e2 < TOL
    # sp only, and the refused calls leave their outputs alone
    c3 = z(nf * nd, np.nan)
    torch.cuda.synchronize()
    p.run_coded_device(d_x, xl, t2, f2, c3, nd, None, y2, rng_pos=start)
    w.lib().wc_synchronize()
    assert torch.equal(c3, csp)
    c4 = z(nf * nd, np.nan)
    torch.cuda.synchronize()
    for bad in (0, fft // 4 + 2):
        with pytest.raises(w.WorldClassError):
            p.run_coded_device(d_x, xl, t2, f2, c4, bad, cap, y2, rng_pos=start)
    w.lib().wc_synchronize()
    assert bool(torch.isnan(c4).all()) and torch.equal(cap, a2)


# ---- 6. stream ---------------------------------------------------------------------------------------------------------------

def _schedule(fs, cs):
    """pushes of three streams: stream 0 runs through, stream 1 idles for two pushes, stream 2 is reset in the middle of a signal and
    starts another; every signal ends in a short chunk with a flush.  Yields (streams to reset, chunks, flush)."""
    from world_class_amd.synth import make_utterance
    a, b, c1, c2 = (make_utterance(fs, sec, 6100 + i) for i, sec in enumerate((2.1, 1.5, 1.9, 1.3)))
    starts = {0: [(0, a)], 1: [(2, b)], 2: [(0, c1), (4, c2)]}
    cur, pos = {u: None for u in starts}, {u: 0 for u in starts}
    out = []
    for k in range(40):
        resets, chunks, flush = [], [], []
        for u in sorted(starts):
            for st, x in starts[u]:
                if st == k:
                    if cur[u] is not None:
                        resets.append(u)
                    cur[u], pos[u] = x, 0
            if cur[u] is None:
                chunks.append(np.zeros(0))
                flush.append(0)
                continue
            x = cur[u]
            last = pos[u] + cs >= len(x)
            chunks.append(x[pos[u]:pos[u] + cs])
            flush.append(1 if last else 0)
            pos[u] += cs
            if last:
                cur[u] = None
        if all(len(c) == 0 for c in chunks) and k > 4:
            break
        out.append((resets, chunks, flush))
    return out


@pytest.mark.parametrize("fs,aperiodicity", [(24000, True), (48000, True), (24000, False)])
def test_stream_push_coded_equals_the_plain_push_then_the_coder(env, fs, aperiodicity):
    w, codec, torch = env
    from world_class_amd.stream import StreamAnalyzer
    nd, n = 60, 3
    mk = lambda: StreamAnalyzer(fs, n, frame_period=5.0, chunk_ms=200, lookback_ms=400, lookahead_ms=400, aperiodicity=aperiodicity)
    A, B = mk(), mk()
    fft, bins = A.fft_size, A.bins
    n_ap = codec.number_of_aperiodicities(fs) if aperiodicity else 0
    cap_rows = n * A.max_frames
    z = lambda m, v=np.nan: torch.full((max(m, 1),), v, dtype=torch.float64, device="cuda")
    tA, fA, tB, fB = z(cap_rows), z(cap_rows), z(cap_rows), z(cap_rows)
    cspA, capA = z(cap_rows * nd), (z(cap_rows * n_ap) if aperiodicity else None)
    spB, apB = z(cap_rows * bins), (z(cap_rows * bins) if aperiodicity else None)
    state = lambda S: [(S.frames_committed(u), S.rng_position(u), S.d4c_rng_position(u)) for u in range(n)]
    committed = 0
    for k, (resets, chunks, flush) in enumerate(_schedule(fs, A.chunk_samples)):
        for u in resets:
            A.reset(u)
            B.reset(u)
        n_new = [len(c) for c in chunks]
        d_chunk = _dev(torch, np.concatenate(chunks)) if sum(n_new) else torch.zeros(1, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        if k == 5:  # refused pushes in the middle of the run: every stream stays where it was
            before = state(A)
            junk_csp, junk_cap = z(cap_rows * nd), z(cap_rows * 5)
            torch.cuda.synchronize()
            for bad_nd in (0, fft // 4 + 2):
                with pytest.raises(w.WorldClassError):
                    A.push_coded_device(d_chunk, junk_csp, bad_nd, junk_cap if aperiodicity else None, n_new, flush, tA, fA)
            with pytest.raises(w.WorldClassError):  # d_coded_ap without the option / the option without d_coded_ap
                A.push_coded_device(d_chunk, junk_csp, nd, None if aperiodicity else junk_cap, n_new, flush, tA, fA)
            w.lib().wc_synchronize()
            assert state(A) == before and bool(torch.isnan(junk_csp).all()) and bool(torch.isnan(junk_cap).all())
        cA = A.push_coded_device(d_chunk, cspA, nd, capA, n_new, flush, tA, fA)
        cB = B.push_device(d_chunk, n_new, flush, tB, fB, spB, d_ap=apB)
        w.lib().wc_synchronize()
        assert cA == cB, k
        tot = sum(cA)
        committed += tot
        assert torch.equal(tA[:tot], tB[:tot]) and torch.equal(fA[:tot], fB[:tot]), k
        if tot:
            c2, a2 = z(tot * nd), (z(tot * n_ap) if aperiodicity else None)
            torch.cuda.synchronize()
            codec.code_features_device(fs, fft, tot, nd, spB, apB, c2, a2)
            w.lib().wc_synchronize()
            assert torch.equal(cspA[:tot * nd], c2[:tot * nd]), k
            assert bool(torch.isfinite(c2[:tot * nd]).all())
            if aperiodicity:
                assert torch.equal(capA[:tot * n_ap], a2[:tot * n_ap]), k
        assert state(A) == state(B), k
    assert committed > 4 * 200 // 5


def test_push_coded_host_convenience(env):
    """StreamAnalyzer.push_coded / run_whole(coded=nd): dicts with tpos, f0, csp, cap that equal the plain run's rows coded"""
    w, codec, torch = env
    from world_class_amd.stream import StreamAnalyzer
    from world_class_amd.synth import make_utterance
    fs, nd = 24000, 40
    xs = [make_utterance(fs, sec, 6300 + i) for i, sec in enumerate((1.1, 0.9))]
    mk = lambda: StreamAnalyzer(fs, 2, frame_period=5.0, chunk_ms=200, lookback_ms=400, lookahead_ms=400, aperiodicity=True)
    got, ref = mk().run_whole(xs, coded=nd), mk().run_whole(xs)
    for g, r in zip(got, ref):
        assert sorted(g) == ["cap", "csp", "f0", "tpos"]
        assert np.array_equal(g["tpos"], r["tpos"]) and np.array_equal(g["f0"], r["f0"])
        csp, cap = _code(env, fs, 1024, nd, r["sp"], r["ap"])
        assert np.array_equal(g["csp"], csp) and np.array_equal(g["cap"], cap)


# ---- 7. the coded loop ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fft", [1024, 2048])
def test_coded_loop_analysis_stream_to_synthesis_stream(env, fft):
    """8 streams at 24 kHz: push_coded_device -> StreamSynthesizer.push_coded_device on device pointers only; the samples equal
    Synthesis.compute_coded on each stream's concatenated coded rows bit for bit"""
    w, codec, torch = env
    from world_class_amd.stream import StreamAnalyzer, StreamSynthesizer
    from world_class_amd.synth import make_utterance
    fs, n, nd, fp = 24000, 8, 60, 5.0
    n_ap = codec.number_of_aperiodicities(fs)
    xs = [make_utterance(fs, 0.9 + 0.13 * (u % 4), 6400 + u) for u in range(n)]
    sa = StreamAnalyzer(fs, n, frame_period=fp, chunk_ms=200, lookback_ms=400, lookahead_ms=400, fft_size=fft, aperiodicity=True)
    assert sa.fft_size == fft
    ss = StreamSynthesizer(fs, fft, fp, n, sa.max_frames)
    cap_rows = n * sa.max_frames
    d_t, d_f = torch.zeros(cap_rows, dtype=torch.float64, device="cuda"), torch.zeros(cap_rows, dtype=torch.float64, device="cuda")
    d_csp = torch.zeros(cap_rows * nd, dtype=torch.float64, device="cuda")
    d_cap = torch.zeros(cap_rows * n_ap, dtype=torch.float64, device="cuda")
    d_y = torch.zeros(n * ss.max_samples, dtype=torch.float64, device="cuda")
    cs = sa.chunk_samples
    acc = [dict(f0=[], csp=[], cap=[], y=[]) for _ in range(n)]
    done, pos = [False] * n, 0
    while not all(done):
        chunks, flush = [], []
        for u, x in enumerate(xs):
            if done[u]:
                chunks.append(np.zeros(0))
                flush.append(0)
                continue
            last = pos + cs >= len(x)
            chunks.append(x[pos:pos + cs])
            flush.append(1 if last else 0)
            done[u] = last
        pos += cs
        d_chunk = _dev(torch, np.concatenate(chunks))
        torch.cuda.synchronize()
        counts = sa.push_coded_device(d_chunk, d_csp, nd, d_cap, [len(c) for c in chunks], flush, d_t, d_f)
        outs = ss.push_coded_device(counts, d_f, d_csp, nd, d_cap, flush, d_y)
        w.lib().wc_synchronize()
        f0, csp, cap, y = (a.cpu().numpy() for a in (d_f, d_csp, d_cap, d_y))
        o, oy = 0, 0
        for u in range(n):
            c, m = counts[u], outs[u]
            acc[u]["f0"].append(f0[o:o + c].copy())
            acc[u]["csp"].append(csp[o * nd:(o + c) * nd].reshape(c, nd).copy())
            acc[u]["cap"].append(cap[o * n_ap:(o + c) * n_ap].reshape(c, n_ap).copy())
            acc[u]["y"].append(y[oy:oy + m].copy())
            o += c
            oy += m
    syn = w.Synthesis(fs, fft, fp)
    for u in range(n):
        f0, csp, cap, y = (np.concatenate(acc[u][k]) for k in ("f0", "csp", "cap", "y"))
        assert len(f0) > 100
        w.rng_set_position(0)
        ref = syn.compute_coded(f0, csp, cap)
        assert len(y) == len(ref) and np.array_equal(y, ref), u
    w.rng_set_position(0)


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------

def test_code_features_refuses_bad_arguments(env):
    w, codec, torch = env
    L = codec._L()
    n, nd = 4, 20
    d_in = torch.full((n * 2049,), 0.5, dtype=torch.float64, device="cuda")
    d_csp = torch.full((n * 1100,), np.nan, dtype=torch.float64, device="cuda")
    d_cap = torch.full((n * 8,), np.nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    i, a, c, b = d_in.data_ptr(), d_in.data_ptr(), d_csp.data_ptr(), d_cap.data_ptr()
    bad = [
        (48000, 1000, n, nd, i, a, c, b),            # fft_size
        (48000, 8192, n, nd, i, a, c, b),
        (48000, 2048, n, 0, i, a, c, b),             # number_of_dimensions
        (48000, 2048, n, 2048 // 4 + 2, i, a, c, b),
        (24000, 1024, n, 1024 // 4 + 2, i, a, c, b),
        (8000, 512, n, nd, i, a, c, b),              # aperiodicity below 12 kHz: no band
        (11025, 512, n, nd, i, a, c, b),
        (48000, 2048, n, nd, i, None, c, b),         # exactly one of d_ap / d_coded_ap
        (48000, 2048, n, nd, i, a, c, None),
        (48000, 2048, n, nd, None, a, c, b),         # null sp arrays
        (48000, 2048, n, nd, i, a, None, b),
        (48000, 2048, -1, nd, i, a, c, b),           # n_frames
        (48000, 2048, 1 << 32, nd, i, a, c, b),
    ]
    for args in bad:
        rc = L.wc_code_features_device(*args)
        assert rc == -1 and w.last_error(), args
    w.lib().wc_synchronize()
    assert bool(torch.isnan(d_csp).all()) and bool(torch.isnan(d_cap).all())
    assert L.wc_code_features_device(48000, 2048, 0, nd, None, None, None, None) == 0  # n_frames 0: a no-op
    assert L.wc_code_features_device(8000, 512, n, nd, i, None, c, None) == 0          # sp only: any fs
    w.lib().wc_synchronize()
    assert bool(torch.isfinite(d_csp[:n * nd]).all()) and bool(torch.isnan(d_csp[n * nd:]).all()) and bool(torch.isnan(d_cap).all())


@pytest.mark.parametrize("fs,fft", [(48000, 2048), (24000, 1024), (96000, 4096)])
@pytest.mark.parametrize("poison", [0.0, -1.0, np.inf, np.nan])
def test_a_bad_bin_spoils_its_own_frame_only(env, fs, fft, poison):
    sp0, ap0 = _analysis_rows(fs)
    sp, ap = sp0[10:13].copy(), ap0[10:13].copy()
    good_csp, good_cap = _code(env, fs, fft, 60, sp, ap)
    sp[1, 300] = poison
    csp, cap = _code(env, fs, fft, 60, sp, ap)
    assert not np.isfinite(csp[1]).any()
    assert np.array_equal(csp[[0, 2]], good_csp[[0, 2]]) and np.array_equal(cap, good_cap)
