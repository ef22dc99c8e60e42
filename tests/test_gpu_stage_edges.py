"""-m gpu: the one-wavefront kernels of CheapTrick, D4C and Synthesis on both sides of every length at which they change their code
path -- the pruned first stage of a forward transform, the second launch for long windows, the slot-0-only noise path -- and on both
sides of the predicate that hands a frame to the block kernel behind them (ct_wave_can, d4c2_can, d4c1_can), found by bisection on
the library's own exports down to adjacent doubles.  Against the block kernels, against the CPU restatement, and with the noise
stream's end positions equal everywhere.

The inputs come from tests/stage_edges.py; that they reach the edges they are named after -- window lengths, LoveTrain's gate, the
pulse intervals of the glides and onsets -- is held on the CPU by tests/test_stage_edges_rule.py.  The tolerances are those of the
stage files."""
import ctypes as C

import numpy as np
import pytest

import stage_edges as se
from test_gpu_cheaptrick import SP_REL
from test_gpu_d4c import AP_ABS
from test_gpu_synthesis import Y_ABS

pytestmark = pytest.mark.gpu

RATES = [(48000, 2048), (16000, 1024), (24000, 1024)]
SENTINEL = 1.0 - 1e-12


@pytest.fixture(scope="module")
def wca():
    import world_class_amd as w
    L = w.lib()
    for name in ("wc_debug_ct_wave_takes", "wc_debug_d4c_wave_takes"):
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = [C.c_int, C.c_double, C.c_int]
    return w


def rel(a, b):
    return float((np.abs(a - b) / np.abs(b)).max())


def _handle(make, env):
    """a handle created under the environment switches it reads at creation"""
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        return make()


def _report_hand_over(what, names, a, b):
    """printed, not asserted: a frame the kernel leaves out is done by the block kernel in either run, one it takes is not.  Without
    every utterance's first and last frame: in CheapTrick's batches they carry another F0 (in D4C's the cut is harmless)."""
    for nm in ("first_outside", "last_inside"):
        u = names.index(nm)
        differ = int((a[u][1:-1] != b[u][1:-1]).any(axis=1).sum())
        print("%s %s: %d of %d frames differ from the block run in some bit" % (what, nm, differ, len(a[u]) - 2))


# ---- CheapTrick ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs,fft", RATES)
def test_cheaptrick_at_the_pruning_edges_the_floor_and_the_hand_over(wca, port, fs, fft):
    """ct_wave_kernel and ct_wave_split_kernel (48 kHz), ct_wave8_kernel (16 / 24 kHz): windows of fft / 4 -+ 1 and fft / 2 -+ 1
    samples, the longest window the floor allows (also as every utterance's first and last frame, hanging over the signal's ends),
    a frame at the floor (-> 500 Hz), the last F0 inside ct_wave_can, the first outside it (listed for the block kernel, from
    utterances behind the first) and one whose smoothing is one bin narrower than the capacity."""
    L = wca.lib()
    assert wca.cheaptrick_fft_size(fs) == fft
    assert L.wc_debug_ct_wave_takes(512, 100.0, fs) == -1 and L.wc_debug_ct_wave_takes(4096, 100.0, fs) == -1
    takes = lambda f: L.wc_debug_ct_wave_takes(fft, f, fs) == 1
    f0s = se.ct_f0s(fs, fft, takes)
    for nm in ("last_inside", "first_outside", "one_below_capacity", "longest"):
        assert se.ct_wave_takes(fft, f0s[nm], fs) == takes(f0s[nm]), (nm, f0s[nm])
    assert takes(f0s["last_inside"]) and not takes(f0s["first_outside"]) and np.nextafter(f0s["last_inside"], np.inf) == f0s["first_outside"]
    names, xs, tps, cs = se.ct_case(fs, fft, f0s, se.CT_FIRST_SEED[fs])
    start = [1000 * i + 3 for i in range(len(names))]
    impls = [("default", {}), ("block", {"WC_CT_IMPL": "block"})] + ([("split", {"WC_CT_IMPL": "split"})] if fft == 2048 else [])
    runs = {}
    for impl, env in impls:
        ct = _handle(lambda: wca.CheapTrick(fs), env)
        assert ct.fft_size == fft
        runs[impl] = ct.compute_batch(xs, tps, cs, rng_pos=list(start))
    refs, ends = [], []
    for x, t, c, p0 in zip(xs, tps, cs, start):
        port.rng_seek(p0)
        refs.append(port.cheaptrick(x, fs, t, c))
        ends.append(port.rng_position())
    port.rng_reset()
    for impl, _ in impls:
        assert list(runs[impl][1]) == ends, impl
    blk = runs["block"][0]
    for impl in [i for i, _ in impls if i != "block"]:
        out = runs[impl][0]
        for u, nm in enumerate(names):
            assert np.isfinite(out[u]).all()
            vb, vr = rel(out[u], blk[u]), rel(out[u], refs[u])
            line = "cheaptrick %d %s %s %.6f Hz: vs block %.2e, vs oracle %.2e" % (fs, impl, nm, f0s[nm], vb, vr)
            if impl == "split":
                vd = rel(out[u], runs["default"][0][u])
                line += ", vs default %.2e" % vd
            print(line)
            assert vb < SP_REL and vr < SP_REL, line
            if impl == "split":
                assert vd < 1e-10, line
        _report_hand_over("cheaptrick %d %s" % (fs, impl), names, out, blk)
    for u, nm in enumerate(names):
        assert rel(blk[u], refs[u]) < SP_REL, nm


# ---- D4C -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs,fft", RATES)
def test_d4c_at_the_group_edges_the_long_launch_the_floor_and_the_hand_over(wca, port, fs, fft):
    """d4c2_* (48 kHz), d4c1_* (16 / 24 kHz) on harmonic signals that LoveTrain gates in on every frame: main windows on both sides
    of every group count the rate reaches and of the LONG launch, LoveTrain's window on both sides of its own LONG launch, F0 at the
    47 Hz floor and below it, the last F0 inside d4c2_can / d4c1_can (the smoothing at the capacity of its half width) and the first
    outside it (listed for the block kernel behind)."""
    L = wca.lib()
    n = se.d4c_fft_size(fs)
    assert L.wc_debug_d4c_wave_takes(1024, 100.0, fs) == -1 and L.wc_debug_d4c_wave_takes(8192, 100.0, fs) == -1
    takes = lambda f: L.wc_debug_d4c_wave_takes(n, f, fs) == 1
    f0s = se.d4c_f0s(fs, takes)
    for nm in f0s:
        assert se.d4c_wave_takes(n, max(f0s[nm], se.D4C_FLOOR), fs) == takes(max(f0s[nm], se.D4C_FLOOR)), (nm, f0s[nm])
    assert takes(f0s["last_inside"]) and not takes(f0s["first_outside"]) and np.nextafter(f0s["last_inside"], np.inf) == f0s["first_outside"]
    names, xs, tps, cs = se.d4c_case(fs, f0s, se.D4C_FIRST_SEED)
    start = [1000 * i + 11 for i in range(len(names))]
    runs = {}
    for impl, env in (("default", {}), ("block", {"WC_D4C_IMPL": "block"})):
        d = _handle(lambda: wca.D4C(fs), env)
        runs[impl] = d.compute_batch(xs, tps, cs, fft, rng_pos=list(start))
    refs, ends = [], []
    for x, t, c, p0 in zip(xs, tps, cs, start):
        port.rng_seek(p0)
        refs.append(port.d4c(x, fs, t, c, fft))
        ends.append(port.rng_position())
    port.rng_reset()
    assert list(runs["default"][1]) == ends and list(runs["block"][1]) == ends
    a, b = runs["default"][0], runs["block"][0]
    for u, nm in enumerate(names):
        assert np.isfinite(a[u]).all()
        sent = [(m == SENTINEL).all(axis=1) for m in (a[u], b[u], refs[u])]
        vb, vr = float(np.abs(a[u] - b[u]).max()), float(np.abs(a[u] - refs[u]).max())
        line = "d4c %d %s %.6f Hz: %d frames, vs block %.2e, vs oracle %.2e" % (fs, nm, f0s[nm], len(a[u]), vb, vr)
        print(line)
        assert np.array_equal(sent[0], sent[1]) and np.array_equal(sent[0], sent[2]), line
        assert not sent[0].any(), line  # every frame under test went through the kernels
        assert vb < AP_ABS and vr < AP_ABS, line
        assert float(np.abs(b[u] - refs[u]).max()) < AP_ABS, line
    _report_hand_over("d4c %d" % fs, names, a, b)


# ---- Synthesis -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs,fft", RATES)
def test_synthesis_at_the_noise_class_edges_and_the_longest_interval(wca, port, fs, fft):
    """syn_pulse_wave_kernel<., 1 | 2> (48 kHz), syn_pulse_wave8_kernel (16 / 24 kHz): glides whose voiced pulse intervals hold both
    fft / 4, fft / 4 + 1 and fft / 2, fft / 2 + 1; at 48 kHz onsets whose last unvoiced pulse draws 128 / 129 samples (the slot-0-only
    path and the generic one); a constant F0 just above fs / fft + 1, the longest interval there is, and just below it, unvoiced."""
    names, params, start = se.syn_case(fs, fft)
    arg = ([p[0] for p in params], [p[1] for p in params], [p[2] for p in params])
    envs = [("default", {}), ("block", {"WC_SYN_IMPL": "block"})] + ([("twin", {"WC_SYN_SPLIT": "0"})] if fs == 48000 else [])
    runs = {}
    for impl, env in envs:
        s = _handle(lambda: wca.Synthesis(fs, fft, 5.0), env)
        ys, pos = s.compute_batch(*arg, rng_pos=list(start))
        runs[impl] = (ys, list(pos))
    ys, pos = runs["default"]
    for u, (nm, (f0, sp, ap)) in enumerate(zip(names, params)):
        port.rng_seek(start[u])
        ref = port.synthesis(f0, sp, ap, fs, 5.0)
        end = port.rng_position()
        vr, vb = float(np.abs(ys[u] - ref).max()), float(np.abs(ys[u] - runs["block"][0][u]).max())
        line = "synthesis %d %s: %d frames, peak %.2e, vs oracle %.2e, vs block %.2e" % (fs, nm, len(f0), np.abs(ref).max(), vr, vb)
        print(line)
        assert len(ys[u]) == len(ref) and np.abs(ref).max() > 1e-4, line
        assert pos[u] == end and runs["block"][1][u] == end, line
        assert vr < Y_ABS, line
        assert vb < 1e-12, line
        if fs == 48000:
            assert runs["twin"][1][u] == end and np.array_equal(ys[u], runs["twin"][0][u]), line
    port.rng_reset()
    if fs == 48000:
        # the glide through 1024 | 1025 in two pushes of a synthesis stream: the stage call's bits
        from world_class_amd.stream import StreamSynthesizer
        u = names.index("glide%d" % (fft // 2))
        nfr = len(params[u][0])
        assert start[u] == 0
        st = StreamSynthesizer(fs, fft, 5.0, 1, (nfr + 1) // 2)
        got = st.run_whole([params[u]], [[(nfr + 1) // 2]])
        assert len(got[0]) == wca.synthesis_out_length(nfr, 5.0, fs)
        assert np.array_equal(got[0], ys[u])
