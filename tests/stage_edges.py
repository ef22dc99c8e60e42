"""What tests/test_stage_edges_rule.py and tests/test_gpu_stage_edges.py share; a helper, not a test module.

The one-wavefront kernels of CheapTrick, D4C and Synthesis choose their code path from a length computed per frame or per pulse: a
pruned first stage of the forward transform, a second launch for long windows, a slot-0-only noise path, and -- the hand-over -- a
predicate that leaves the frame to the block kernel behind.  This module states those lengths as the reference states them, hands
out F0 values that land on a chosen side of an edge, restates the three hand-over predicates, and builds the inputs on which the
edges can be seen: harmonic signals that D4C's LoveTrain gates in, and F0 contours whose pulse intervals straddle a noise class.

CPU only: numpy, and the CPU restatement (oracle/port.py) where a function takes `port`."""
import math

import numpy as np

DEFAULT_F0 = 500.0       # reference include/world_constantnumbers.hpp:17 (kDefaultF0)
D4C_FLOOR = 47.0         # reference include/world_constantnumbers.hpp:31 (kFloorF0D4C)
LOVETRAIN_FLOOR = 40.0   # reference src/d4c.cpp:102 (lowest_f0_)


def matlab_round(x):
    """reference src/world_matlabfunctions.cpp:212"""
    return int(x + 0.5) if x > 0 else int(x - 0.5)


# ---- window lengths as the reference states them --------------------------------------------------------------------------------
def ct_f0_floor(fs, fft_size):
    """reference src/cheaptrick.cpp:44 (GetF0FloorForCheapTrick): 3 fs / (fft_size - 3)"""
    return 3.0 * fs / (fft_size - 3.0)


def ct_half_length(fs, f0, f0_floor):
    """reference src/cheaptrick.cpp:76 (f0 <= f0_floor -> 500 Hz) and :141 (half_window_length); the window has 2 hl + 1 samples"""
    f0c = DEFAULT_F0 if f0 <= f0_floor else f0
    return matlab_round(1.5 * fs / f0c)


def d4c_half_length(fs, f0):
    """D4C's main windows: reference src/d4c.cpp:157 (the floor at 47 Hz) and :250 with window_length_ratio = 4"""
    return matlab_round(4.0 * fs / max(D4C_FLOOR, f0) / 2.0)


def lovetrain_half_length(fs, f0):
    """LoveTrain's window: reference src/d4c.cpp:203 (the floor at 40 Hz) and :216 / :250 with window_length_ratio = 3, as
    d4c_lt_count_kernel counts it"""
    return matlab_round(3.0 * fs / max(LOVETRAIN_FLOOR, f0) / 2.0)


def d4c_fft_size(fs):
    """D4C's own transform size: reference src/d4c.cpp:64"""
    return int(2 ** (1 + int(math.log(4.0 * fs / D4C_FLOOR + 1) / math.log(2.0))))


def half_length(kind, fs, f0, f0_floor=0.0):
    if kind == "ct":
        return ct_half_length(fs, f0, f0_floor)
    if kind == "d4c":
        return d4c_half_length(fs, f0)
    assert kind == "lovetrain", kind
    return lovetrain_half_length(fs, f0)


_RATIO = {"ct": 1.5, "d4c": 2.0, "lovetrain": 1.5}


def f0_for_half_length(kind, fs, hl):
    """an F0 strictly inside the interval whose window has half length hl (hl = round(c fs / F0)): the F0 at which c fs / F0 is
    hl + 1/4, a quarter of a sample from the nearer neighbour.  Not c fs / hl itself: at hl = 2^k that F0 is a whole number of bins of
    the transform, the partials of a harmonic signal then leak nothing into the bins between and above them, and CheapTrick's
    smoothing (differences of a running sum) loses nine digits there -- the CPU restatement itself moves by 6e-9 (hl = 256) and 1e-8
    (hl = 512) relative at 48 kHz when the signal's samples move by one ulp, against 2e-12 at hl = 255."""
    f0 = _RATIO[kind] * fs / (hl + 0.25)
    assert half_length(kind, fs, f0) == hl, (kind, fs, hl, f0)
    assert half_length(kind, fs, _RATIO[kind] * fs / (hl + 0.45)) == hl and half_length(kind, fs, _RATIO[kind] * fs / (hl - 0.45)) == hl
    return f0


def edge_pair(kind, fs, last_odd_length):
    """(F0 whose window has last_odd_length samples, F0 whose window has two more): the two sides of a `wl <= 2^k` switch"""
    hl = (last_odd_length - 1) // 2
    return f0_for_half_length(kind, fs, hl), f0_for_half_length(kind, fs, hl + 1)


# ---- the code paths the kernels choose from those lengths -----------------------------------------------------------------------
def ct_prune_class(fft_size, wl):
    """leading passes of the forward transform that see non-zero input: wdft16<+1, 1|2|4> at 2048 points (ct_wave_kernel,
    ct_wave_split_kernel), wdft8p<+1, 1|2|4> at 1024 (ct_wave8_kernel) -- a quarter, a half or all of the transform's length"""
    return 1 if 4 * wl <= fft_size else (2 if 2 * wl <= fft_size else 4)


def d4c_groups(wl):
    """d4c2_groups of wc_d4c.hip: four-slot groups of 512 samples that a window reaches; beyond 2048 samples the LONG launch"""
    return 4 if wl > 2048 else (wl + 511) >> 9


def d4c_is_long(wl):
    return wl > 2048


def syn_noise_class(fft_size, noise_size):
    """the noise transform's pruning in the pulse kernels: a quarter, a half or all of the packed 1024 / 512 points"""
    return 1 if 4 * noise_size <= fft_size else (2 if 2 * noise_size <= fft_size else 4)


# ---- the hand-over predicates, restated -----------------------------------------------------------------------------------------
def ct_half_width(fft_size, f0c, fs):
    """half width in bins of CheapTrick's smoothing (width 2 F0 / 3), as ct_wave_can counts it"""
    return int(f0c * 2.0 / 3.0 * fft_size / fs) + 1


def d4c_half_width(fft_size, f0, fs):
    """half width in bins of D4C's widest smoothing (width F0), as d4c2_can / d4c1_can count it"""
    return int(f0 * fft_size / fs) + 1


def ct_wave_takes(fft_size, f0c, fs):
    """ct_wave_can<fft_size> of wc_cheaptrick.hip"""
    return ct_half_width(fft_size, f0c, fs) <= 60 and 2 + int(f0c * fft_size / fs) <= 120


def d4c2_takes(f0, fs):
    """d4c2_can of wc_d4c.hip (D4C transform of 4096 points)"""
    return d4c_half_width(4096, f0, fs) <= 120 and int(f0 * 4096 / fs) + 2 <= 122


def d4c1_takes(f0, fs):
    """d4c1_can of wc_d4c.hip (D4C transform of 2048 points)"""
    return d4c_half_width(2048, f0, fs) <= 120 and int(f0 * 2048 / fs) + 2 <= 122


def d4c_wave_takes(fft_size_d4c, f0, fs):
    return d4c2_takes(f0, fs) if fft_size_d4c == 4096 else d4c1_takes(f0, fs)


def bisect_edge(takes, lo, hi):
    """(last F0 for which takes() holds, first for which it does not): adjacent doubles, from takes(lo) and not takes(hi)"""
    assert takes(lo) and not takes(hi)
    while np.nextafter(lo, np.inf) < hi:
        mid = lo + (hi - lo) / 2.0
        if takes(mid):
            lo = mid
        else:
            hi = mid
    return float(lo), float(hi)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def harmonic_signal(fs, f0, seconds, seed, sigma=1e-3):
    """partials k f0 up to 0.45 fs at amplitude 1 / k with seeded phases, peak 0.3, plus white noise of sigma 1e-3: periodic enough
    for LoveTrain to gate every frame in, noisy enough for the band aperiodicity to lie between its clamps"""
    rng = np.random.default_rng(seed)
    n = int(round(fs * seconds))
    t = np.arange(n, dtype=np.float64) / fs
    x = np.zeros(n)
    for k in range(1, int(0.45 * fs / f0) + 1):
        x += np.sin(2.0 * np.pi * k * f0 * t + rng.uniform(0.0, 2.0 * np.pi)) / k
    x *= 0.3 / np.abs(x).max()
    return x + rng.normal(0.0, sigma, n)


def frame_times(seconds, frame_period=5.0):
    """frame positions of a signal of that length, as the reference's GetSamplesForDIO counts them"""
    n = int(1000.0 * seconds / frame_period) + 1
    return np.arange(n) * frame_period / 1000.0


def rows(fft_size, nfr, seed):
    """smooth random spectrogram rows, and aperiodicity rows that are 0.001 at bin 0 and rise to 0.999 (both parts of a voiced pulse
    exist), as _rows of tests/test_gpu_synth_split.py builds them"""
    rng = np.random.default_rng(seed)
    bins = fft_size // 2 + 1
    k = np.arange(bins) / (bins - 1.0)
    sp = np.stack([1e-4 + 1e-2 * np.exp(-((k - rng.uniform(0.1, 0.3)) / 0.05) ** 2) for _ in range(nfr)])
    ap = np.stack([np.interp(k, [0.0, 0.3, 0.6, rng.uniform(0.7, 0.9), 1.0], [0.001, rng.uniform(0.05, 0.4), rng.uniform(0.5, 0.99), 0.995, 0.999])
                   for _ in range(nfr)])
    return sp, ap


def glide_contour(fs, b, nfr, spread=5):
    """F0 falling linearly from fs / (b - spread) to fs / (b + spread): pulse intervals that grow through b and b + 1"""
    return np.linspace(fs / (b - float(spread)), fs / (b + float(spread)), nfr)


def onset_contour(f0, nfr, n_unvoiced):
    """unvoiced frames, then a constant F0: the last unvoiced pulse's interval reaches up to the first voiced pulse"""
    c = np.full(nfr, float(f0))
    c[:n_unvoiced] = 0.0
    return c


def syn_lowest_f0(fs, fft_size):
    """below this F0 a frame is unvoiced to Synthesis: reference src/synthesis.cpp:97 (fs / fft_size in integers, plus one)"""
    return fs // fft_size + 1.0


def pulse_intervals(port, f0, fft_size, fs, frame_period=5.0):
    """(noise sizes, voiced flags) of all pulses but the last (which draws nothing), from the CPU restatement's own time base"""
    index, voiced = port.synthesis_pulse_list(f0, fft_size, fs, frame_period)
    return np.diff(index), voiced[:-1]


# ---- the cases, shared by the rule file (preconditions, no device) and the device file ------------------------------------------
CT_SECONDS = 0.25
CT_SIGMA = 1e-2  # (the noise level of world_class_amd.synth.make_utterance: CheapTrick's envelope is a quotient of smoothed power spectra,
                 # and the emptier the bins above the last partial, the more digits the smoothing loses there; see one_ulp_response)
D4C_SECONDS = 0.3


def _between(a, b):
    return a + (b - a) / 2.0


def ct_f0s(fs, fft_size, takes):
    """name -> F0 of CheapTrick's cases at one rate; takes(f0c) is the hand-over predicate (the library's or the restatement)"""
    floor = ct_f0_floor(fs, fft_size)
    out = {}
    for last in (fft_size // 4 - 1, fft_size // 2 - 1):  # wl <= N / 4, wl <= N / 2
        a, b = edge_pair("ct", fs, last)
        out["wl%d" % last], out["wl%d" % (last + 2)] = a, b
    out["longest"] = float(np.nextafter(floor, np.inf))
    out["below_floor"] = float(np.nextafter(floor, 0.0))
    last_in, first_out = bisect_edge(takes, 1000.0, 4000.0)
    out["last_inside"], out["first_outside"] = last_in, first_out
    b_cap = ct_half_width(fft_size, last_in, fs)
    out["one_below_capacity"] = (b_cap - 1.5) * 1.5 * fs / fft_size
    return out


def d4c_f0s(fs, takes):
    """name -> F0 of D4C's cases at one rate"""
    longest = 2 * d4c_half_length(fs, D4C_FLOOR) + 1
    out = {}
    for last in (511, 1023, 1535, 2047):
        if last + 2 <= longest:
            a, b = edge_pair("d4c", fs, last)
            out["wl%d" % last], out["wl%d" % (last + 2)] = a, b
    if 2 * lovetrain_half_length(fs, LOVETRAIN_FLOOR) + 1 > 2048:
        a, b = edge_pair("lovetrain", fs, 2047)
        out["lt%d" % 2047], out["lt%d" % 2049] = a, b
    out["floor"] = D4C_FLOOR
    out["floored"] = 30.0
    last_in, first_out = bisect_edge(takes, 500.0, 3000.0)
    out["last_inside"], out["first_outside"] = last_in, first_out
    return out


def one_ulp_response(port, x, fs, tpos, f0, trials=3):
    """the largest relative change of the CPU restatement's CheapTrick envelope when every sample of x moves by one ulp up or down
    (seeded signs): the error the reference itself carries on this input, which a bound between two kernels has to stay above"""
    port.rng_reset()
    a = port.cheaptrick(x, fs, tpos, f0)
    worst = 0.0
    for trial in range(trials):
        sign = np.random.default_rng(trial).choice([-1.0, 1.0], len(x))
        port.rng_reset()
        b = port.cheaptrick(x * (1.0 + 1.1e-16 * sign), fs, tpos, f0)
        worst = max(worst, float((np.abs(a - b) / np.abs(a)).max()))
    port.rng_reset()
    return worst


def ct_case(fs, fft_size, f0s, first_seed):
    """one utterance per F0 (the signal's F0 is the contour's), the first and the last frame at the longest window"""
    names = list(f0s)
    xs, tps, cs = [], [], []
    for i, nm in enumerate(names):
        xs.append(harmonic_signal(fs, f0s[nm], CT_SECONDS, first_seed + i, CT_SIGMA))
        t = frame_times(CT_SECONDS)
        c = np.full(len(t), f0s[nm])
        c[0] = c[-1] = f0s["longest"]
        tps.append(t)
        cs.append(c)
    return names, xs, tps, cs


def d4c_case(fs, f0s, first_seed):
    names = list(f0s)
    xs, tps, cs = [], [], []
    for i, nm in enumerate(names):
        xs.append(harmonic_signal(fs, f0s[nm], D4C_SECONDS, first_seed + i))
        t = frame_times(D4C_SECONDS)
        tps.append(t)
        cs.append(np.full(len(t), f0s[nm]))
    return names, xs, tps, cs


# Synthesis: (edge b, frames of the glide) per (fs, fft_size), and (F0, unvoiced frames, frames) of the onsets whose last unvoiced
# pulse has an interval of 128 / 129 samples -- found by search on the CPU restatement's time base, held by
# tests/test_stage_edges_rule.py
SYN_GLIDES = {(48000, 2048): ((512, 31), (1024, 61)), (16000, 1024): ((256, 71), (512, 81)), (24000, 1024): ((256, 51), (512, 61))}
SYN_ONSETS = {128: (335.0, 10, 50), 129: (328.0, 10, 50)}
SYN_EXTREME_FRAMES = 80
D4C_FIRST_SEED = 120  # (at 24 kHz the first and the last frame of the 1406 Hz utterances are gated in on some seeds only)
# CheapTrick's first seed per rate: a batch on which the CPU restatement's own response to one ulp of the input (one_ulp_response)
# stays under the 1e-10 that the split kernel is held to against the default one (it is 2e-11 here); most seeds do, some reach 3e-10
CT_FIRST_SEED = {48000: 360, 16000: 320, 24000: 300}


def syn_case(fs, fft_size, first_seed=500):
    """names, [(f0, sp, ap)] and noise start positions of the Synthesis batch of one size; the glide through the largest edge starts
    at position 0 (a synthesis stream starts there)"""
    names, f0s = [], []
    for b, nfr in SYN_GLIDES[(fs, fft_size)]:
        names.append("glide%d" % b)
        f0s.append(glide_contour(fs, b, nfr))
    if fft_size == 2048:
        for size, (f0, nu, nfr) in sorted(SYN_ONSETS.items()):
            names.append("onset%d" % size)
            f0s.append(onset_contour(f0, nfr, nu))
    lowest = syn_lowest_f0(fs, fft_size)
    names += ["longest", "below_lowest"]
    f0s += [np.full(SYN_EXTREME_FRAMES, np.nextafter(lowest, np.inf)), np.full(SYN_EXTREME_FRAMES, np.nextafter(lowest, 0.0))]
    params = [(f0,) + rows(fft_size, len(f0), first_seed + i) for i, f0 in enumerate(f0s)]
    start = [0 if nm == "glide%d" % SYN_GLIDES[(fs, fft_size)][-1][0] else 1000 * i + 7 for i, nm in enumerate(names)]
    return names, params, start
