"""-m gpu: the 4096-point band stage of D4C (32, 44.1 and 48 kHz) at three wavefronts per SIMD (d4c2_band_kernel<3>, the second stage's
twiddles in LDS) against its two-wavefront twin (WC_D4C_BAND_WAVES=2), and LoveTrain's long-window launch over a device-built list
against its twin on a grid of every frame (WC_D4C_LT_LIST=0): the same bits in ap and the same noise positions.

Everything is a D4C stage call on a given contour (D4C.compute_device), utterances of 0.3 - 0.5 s at a 5 ms hop -- except the one
input that is certain to send the band selection into its 64-bit tail: group-delay rows whose band segments are an impulse, so that
all keys of a band share their high word, handed to the band stage alone (wc_debug_d4c_bands)."""
import ctypes as C

import numpy as np
import pytest

from world_class_amd.synth import make_utterance

pytestmark = pytest.mark.gpu

HOP = 0.005
SENTINEL = 1.0 - 1e-12
RATES = [32000, 44100, 48000]  # band windows of 769, 557 and 513 samples (513: packed point 257 alone in lane 0's fifth slot)


@pytest.fixture(scope="module")
def wca():
    import world_class_amd as w
    L = w.lib()
    L.wc_debug_d4c_band_tails.restype = C.c_int
    L.wc_debug_d4c_band_tails.argtypes = [C.c_void_p, C.POINTER(C.c_uint)]
    L.wc_debug_d4c_lt_listed.restype = C.c_int
    L.wc_debug_d4c_lt_listed.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.wc_debug_d4c_bands.restype = C.c_int
    L.wc_debug_d4c_bands.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    return w


def _handle(wca, fs, threshold, env):
    """a handle created under the environment switches it reads at creation"""
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        return wca.D4C(fs, threshold)


def _stage(wca, d, fs, utts, start):
    """one D4C.compute_device call on the batch [(x, f0), ...]: the aperiodicity matrices and the noise positions it ends at"""
    import torch
    fft = wca.cheaptrick_fft_size(fs)
    bins = fft // 2 + 1
    xs = [np.ascontiguousarray(x, dtype=np.float64) for x, _ in utts]
    f0s = [np.ascontiguousarray(f, dtype=np.float64) for _, f in utts]
    dev = lambda v: torch.from_numpy(np.concatenate(v)).to("cuda")
    d_x, d_f0, d_t = dev(xs), dev(f0s), dev([np.arange(len(f)) * HOP for f in f0s])
    total = sum(len(f) for f in f0s)
    d_ap = torch.full((total * bins + 1,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    end = d.compute_device(d_x, [len(x) for x in xs], d_t, d_f0, [len(f) for f in f0s], fft, d_ap, rng_pos=list(start))
    wca.lib().wc_synchronize()
    ap = d_ap.cpu().numpy()
    assert np.isnan(ap[-1])  # (nothing written behind the last row)
    return ap[:-1].reshape(total, bins), list(end)


def _tails(wca, d):
    n = C.c_uint(0)
    assert wca.lib().wc_debug_d4c_band_tails(d._h, C.byref(n)) == 0
    return n.value


def _segments(n, pattern):
    """a contour of n frames from (share, f0) stretches"""
    f0 = np.zeros(n)
    at = 0.0
    for share, f in pattern:
        f0[int(round(at * n)):int(round((at + share) * n))] = f
        at += share
    return f0


def _speech(fs):
    """two utterances of different length, voiced and unvoiced stretches in turn; F0 at the 47 Hz floor, 94, 400 and 800 Hz, and one
    frame above what the one-wavefront kernels take (d4c2_can: ~1.4 kHz at 48 kHz, ~930 Hz at 32 kHz) for the block kernel behind"""
    a = _segments(101, [(0.08, 0.0), (0.2, 47.0), (0.07, 0.0), (0.2, 94.0), (0.05, 0.0), (0.2, 400.0), (0.2, 800.0)])
    a[60] = 1500.0
    b = _segments(61, [(0.3, 800.0), (0.1, 0.0), (0.3, 94.0), (0.05, 0.0), (0.25, 47.0)])
    return [(make_utterance(fs, 0.5, 4100 + fs % 97), a), (make_utterance(fs, 0.3, 4200 + fs % 89), b)]


def _band_cases():
    c = {}
    for fs in RATES:
        c["speech_%d" % fs] = (fs, _speech(fs), 0.85, {}, [0, 31337])
    n = int(0.3 * 48000)
    impulse = np.zeros(n)
    impulse[n // 2] = 0.5
    # digital silence under a voiced contour: keys of the noise floor only (threshold 0: every frame passes the gate, as it does
    # for the impulse, whose LoveTrain ratio is that of a flat spectrum)
    c["zeros"] = (48000, [(np.zeros(n), np.full(61, 150.0))], 0.0, {}, [7])
    c["impulse"] = (48000, [(impulse, np.full(61, 200.0))], 0.0, {}, [0])
    c["quiet_default_gate"] = (48000, [(np.zeros(n), np.full(61, 150.0)), (impulse, np.full(61, 200.0))], 0.85, {}, [0, 0])
    c["nothing_gated"] = (48000, _speech(48000), 1.0, {}, [0, 5])  # threshold raised: no frame reaches the band stage
    c["select64"] = (48000, _speech(48000), 0.85, {"WC_D4C_SELECT": "64"}, [0, 0])  # takes the twin either way
    return c


@pytest.fixture(scope="module")
def band_runs(wca):
    out = {}
    for name, (fs, utts, thr, env, start) in _band_cases().items():
        d3 = _handle(wca, fs, thr, dict(env, WC_D4C_BAND_WAVES="3", WC_D4C_BAND_TAILS="1"))
        three = _stage(wca, d3, fs, utts, start)
        tails = _tails(wca, d3)
        two = _stage(wca, _handle(wca, fs, thr, dict(env, WC_D4C_BAND_WAVES="2")), fs, utts, start)
        out[name] = dict(three=three, two=two, tails=tails, utts=utts)
    return out


@pytest.mark.parametrize("name", list(_band_cases()))
def test_three_wavefront_band_stage_gives_the_bits_of_its_twin(band_runs, name):
    r = band_runs[name]
    (a, pa), (b, pb) = r["three"], r["two"]
    f0 = np.concatenate([f for _, f in r["utts"]])
    banded = (b < 0.999).any(axis=1)  # frames that went through the band kernels
    print(name, "frames", len(f0), "voiced", int((f0 > 0).sum()), "through the band stage", int(banded.sum()), "wavefronts in the 64-bit tail", r["tails"])
    assert pa == pb
    assert np.isfinite(b).all()
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert (b[f0 == 0.0] == SENTINEL).all()
    if name.startswith("speech") or name in ("zeros", "impulse", "select64"):
        assert banded.sum() >= 20
    if name.startswith("speech"):
        assert (~banded).sum() >= 20  # frames that pass the gate alternate with frames whose wavefronts leave at once
    if name == "nothing_gated":
        assert not banded.any() and (b == SENTINEL).all() and r["tails"] == 0
    if name == "select64":
        assert r["tails"] == 0  # (the twin does not count)


@pytest.mark.parametrize("fs", RATES)
def test_band_selection_in_its_64_bit_tail(wca, fs):
    """A band whose windowed segment is one impulse has a flat power spectrum: all 2049 keys lie within rounding of one value and share
    their high word, so the search on the high words ends with no key below and all keys at its bracket, and the 64-bit search takes
    over in EVERY wavefront whose window holds the impulse (counted by the kernel itself) -- the path that reads the keys' low words.
    (On the stage calls above no wavefront enters it: neighbours of the ranking share a high word once in ten thousand bands.)  Both
    forms, the same bits."""
    d3 = _handle(wca, fs, 0.85, {"WC_D4C_BAND_WAVES": "3", "WC_D4C_BAND_TAILS": "1"})
    d2 = _handle(wca, fs, 0.85, {"WC_D4C_BAND_WAVES": "2"})
    n_ap = int(min(15000.0, fs / 2.0 - 3000.0) / 3000.0)
    wln = int(3000.0 * 4096 / fs) * 2 + 1
    n = 13  # (not a multiple of 8: the padded tail of the grid)
    centers = [int(3000.0 * (b + 1) * 4096 / fs) for b in range(n_ap)]
    rows = np.zeros((n, 2049))
    inside = np.zeros((n, n_ap), dtype=bool)
    for f in range(n):
        # ONE impulse per row (a second one inside a band's window and its spectrum is no longer flat), a little above the centre of
        # band f % n_ap; the neighbouring bands' windows hold it near their ends or not at all.  An amplitude whose square is no short
        # binary fraction: keys within rounding of 9.0, say, would lie on both sides of a high word's end.
        # (2 .. 21 above it: at 44.1 kHz the next band's window starts 0 or 1 sample above this centre, and its first weight is a
        # rounding residue of the Nuttall sum, not a weight to build on)
        at = centers[f % n_ap] + 2 + (7 * f) % 20
        rows[f, at] = 1.3 + 0.11 * f
        inside[f] = [0 < at - (c - wln // 2) < wln - 1 for c in centers]
    out = []
    for d in (d3, d2):
        coarse = np.full((n, 5), np.nan)
        assert wca.lib().wc_debug_d4c_bands(d._h, n, rows.ctypes.data_as(C.POINTER(C.c_double)), coarse.ctypes.data_as(C.POINTER(C.c_double))) == 0
        out.append(coarse)
    tails = _tails(wca, d3)
    print(fs, "window", wln, "bands", n_ap, "wavefronts in the 64-bit tail", tails, "with the impulse inside their window", int(inside.sum()), "of", n * n_ap)
    assert np.array_equal(out[0].view(np.uint64), out[1].view(np.uint64))
    flat = out[1][:, :n_ap][inside]  # K equal keys of 2049: 10 log10(K / 2049), F0 = 100 Hz adds nothing
    assert np.allclose(flat, 10 * np.log10((2048 - round(4096 * 8.0 / wln)) / 2049.0), rtol=0, atol=1e-9)
    assert inside.sum() >= n and tails == inside.sum()


# ---- LoveTrain's long windows (F0 below 70.35 Hz at 48 kHz: 2 round(3 fs / f0 / 2) + 1 > 2048) over a list ------------------------------
def _lt_cases():
    n = 81
    cyc = lambda vals: np.array([vals[i % len(vals)] for i in range(n)])
    c = {}
    c["none_long"] = [cyc([120.0, 70.4, 0.0, 120.0])]
    one = cyc([120.0, 70.4, 0.0])
    one[40] = 55.0
    c["one_long"] = [one]
    c["all_long"] = [cyc([40.0, 55.0, 69.0])]
    c["mixed"] = [cyc([40.0, 0.0, 55.0, 120.0, 69.0, 70.4, 0.0]), cyc([69.0, 70.4])[:47]]
    c["unvoiced"] = [np.zeros(n)]
    return c


def _lt_long(f0):
    v = f0[f0 > 0]
    return int((2 * np.floor(3.0 * 48000 / np.maximum(v, 40.0) / 2.0 + 0.5) + 1 > 2048).sum())


@pytest.mark.parametrize("name", list(_lt_cases()))
def test_lovetrain_list_gives_the_bits_of_the_full_grid(wca, name):
    fs = 48000
    f0s = _lt_cases()[name]
    utts = [(make_utterance(fs, HOP * (len(f) - 1), 5100 + u), f) for u, f in enumerate(f0s)]
    start = [3 * u for u in range(len(utts))]
    dl = _handle(wca, fs, 0.85, {"WC_D4C_LT_LIST": "1"})
    a, pa = _stage(wca, dl, fs, utts, start)
    listed = C.c_int(-2)
    assert wca.lib().wc_debug_d4c_lt_listed(dl._h, C.byref(listed)) == 0
    b, pb = _stage(wca, _handle(wca, fs, 0.85, {"WC_D4C_LT_LIST": "0"}), fs, utts, start)
    want = sum(_lt_long(f) for f in f0s)
    print(name, "frames", sum(len(f) for f in f0s), "listed", listed.value, "expected", want)
    assert listed.value == want
    assert want == {"none_long": 0, "one_long": 1, "all_long": 81, "mixed": 59, "unvoiced": 0}[name]
    assert pa == pb
    assert np.isfinite(b).all()
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    if name == "unvoiced":
        assert (a == SENTINEL).all() and pa == start
    # a second call on the same handle starts from an empty list again
    a2, pa2 = _stage(wca, dl, fs, utts, start)
    assert wca.lib().wc_debug_d4c_lt_listed(dl._h, C.byref(listed)) == 0 and listed.value == want
    assert pa2 == pa and np.array_equal(a2.view(np.uint64), a.view(np.uint64))
