"""Inputs of the frame-period tests (tests/test_frame_periods_rule.py on the CPU, tests/test_gpu_frame_periods.py on the device):
frame periods that are no whole number of samples, or whose value in seconds (frame_period / 1000) is not representable, so that
floor(t / fp), ceil(t / fp) and the comparison of t with (j + 1) * fp are each decided by a single rounding on the sample that
nominally sits on a frame boundary.  No test functions here.

A contour is piecewise-constant F0 of the form fs / d (whole pulse intervals) with unvoiced stretches, over spectrogram and
aperiodicity rows of oracle.gen_golden.synth_params.  The "boundary" contour of a case comes from a seeded random search (search()
below, run once; the seeds found are stored in CASES) for contours whose pulses land ON nominal frame-boundary samples, of both
kinds: floor(i / fs / (fp / 1000)) == k - 1 and == k for the sample i == k fp fs.  Plain constant or all-unvoiced contours put no
pulse there."""
import os

import numpy as np

HOP256_22K = 256 / 22050 * 1000
HOP256_44K = 256 / 44100 * 1000
HOP512_96K = 512 / 96000 * 1000
SENTINEL = 1.0 - 1e-12

# name: fs, fft size, frame period (ms), seed of the boundary contour, frames of the boundary contour
CASES = {
    "16k_12.5ms": (16000, 1024, 12.5, 204, 120),
    "22k_hop256": (22050, 1024, HOP256_22K, 15, 120),
    "16k_7.3ms": (16000, 1024, 7.3, 10, 120),
    "16k_5.03125ms": (16000, 1024, 5.03125, 226, 120),
    "44k_5ms": (44100, 2048, 5.0, 64, 120),
    "44k_hop256": (44100, 2048, HOP256_44K, 127, 120),
    "48k_2.5ms": (48000, 2048, 2.5, 142, 120),
    "48k_0.7ms": (48000, 2048, 0.7, 272, 120),          # more frames than pulses
    "8k_16ms": (8000, 512, 16.0, 201, 120),             # workgroup-per-pulse kernel, FP64 atomics
    "96k_hop512": (96000, 4096, HOP512_96K, 198, 120),  # 5.333... ms; FP64 atomics
}
NAMES = list(CASES)
# the cases whose boundary contour must reach both kinds (tests/test_frame_periods_rule.py): name -> pulses of each kind at least
MUST_REACH = {"16k_12.5ms": 3, "22k_hop256": 1, "44k_5ms": 1, "48k_2.5ms": 1, "16k_5.03125ms": 1}
CONTOURS = ["boundary", "steep", "end_unvoiced", "two", "gap"]
# the steep contour's steps: frames k whose boundary sample carries a pulse of the boundary contour with the quotient's floor at
# k - 1 (of two neighbouring ones the first); found with the seeds.  A case without such a pulse has no steep contour.
STEPS = {
    "16k_12.5ms": [12, 24, 28, 43, 51, 63, 71, 87, 91],
    "22k_hop256": [92, 94],
    "16k_7.3ms": [],
    "16k_5.03125ms": [106],
    "44k_5ms": [114, 116, 118],
    "44k_hop256": [93, 107],
    "48k_2.5ms": [114, 118],
    "48k_0.7ms": [],
    "8k_16ms": [59, 71, 86],
    "96k_hop512": [],
}


def contours(name):
    return [k for k in CONTOURS if k != "steep" or STEPS[name]]

# push patterns of the streams (frames per push, cycled; 0 = an idle push): one frame per push, ragged with idle pushes, everything
PATTERNS = {"one": [1], "ragged": [3, 0, 11, 1, 2, 0, 37], "all": None}

# Harvest: frame periods (ms) and the rate each runs at
HARVEST_PERIODS = [("0.5ms", 16000, 0.5), ("0.7ms", 48000, 0.7), ("2.5ms", 48000, 2.5), ("10/3ms", 44100, 10.0 / 3.0),
                   ("7.3ms", 16000, 7.3), ("12.5ms", 16000, 12.5), ("22k_hop256", 22050, HOP256_22K), ("44k_hop256", 44100, HOP256_44K)]
HARVEST_SECONDS, HARVEST_SEED = 0.6, 7300


def out_length(n_frames, fp, fs):
    """reference test/test.cpp:362-363"""
    return int((n_frames - 1) * fp / 1000.0 * fs) + 1


def get_samples(fs, x_length, fp):
    """reference src/harvest.cpp:173-181"""
    return int(1000.0 * x_length / fs / fp) + 1


def length_grid():
    """(fs, frame period, lengths): sample counts around exact multiples of the nominal hop, where the truncation of a product that is
    nominally an integer drops a frame (get_samples) -- and frame counts, where it drops a sample (out_length)"""
    grid = []
    for fs, fp in [(24000, 256 / 24000 * 1000), (48000, 256 / 48000 * 1000), (22050, HOP256_22K), (44100, HOP256_44K), (96000, HOP512_96K),
                   (16000, 12.5), (48000, 2.5), (8000, 16.0), (16000, 7.3), (16000, 5.03125), (44100, 5.0), (48000, 0.7), (16000, 0.5),
                   (44100, 10.0 / 3.0)]:
        hop = fp / 1000.0 * fs
        ns = sorted({int(round(k * hop)) + d for k in list(range(1, 70)) + [997, 4001] for d in (-1, 0, 1)})
        grid.append((fs, fp, ns))
    return grid


def rows(fs, fft, n_frames, seed):
    """n_frames spectrogram and aperiodicity rows of synth_params that belong to voiced frames there (none is the sentinel)"""
    from oracle.gen_golden import synth_params
    f0, sp, ap = synth_params(fs, fft, 2 * n_frames + 40, seed)
    keep = np.flatnonzero(f0 > 0)[:n_frames]
    assert len(keep) == n_frames
    return sp[keep].copy(), ap[keep].copy()


def _finish(fs, fft, f0, seed):
    sp, ap = rows(fs, fft, len(f0), seed)
    ap[f0 == 0] = SENTINEL
    return f0, sp, ap


def d_range(fs, fft):
    """pulse intervals d (samples) with fs / d between 80 and 400 Hz, above the stage's lowest F0 fs / fft + 1"""
    return int(np.ceil(fs / 400.0)), int(fs / 80.0)


def d_high(fs):
    """a 600 Hz frame keeps the reference's pulse-array capacity (out_length / int(fs / max_f0)) above the 500 Hz pulses of
    unvoiced stretches (as synth_params does)"""
    return int(fs / 600.0)


def piecewise_f0(fs, fft, n_frames, seed):
    """seeded piecewise-constant F0 = fs / d in stretches of 2 .. 14 frames, three in ten of them unvoiced; frame 1 at 600 Hz"""
    rng = np.random.default_rng(seed)
    lo, hi = d_range(fs, fft)
    f0 = np.zeros(n_frames)
    i = 0
    while i < n_frames:
        n = int(rng.integers(2, 15))
        d = int(rng.integers(lo, hi + 1))
        voiced = rng.random() > 0.3
        f0[i:i + n] = fs / d if voiced else 0.0
        i += n
    f0[1] = fs / d_high(fs)
    return f0


def piecewise(fs, fft, n_frames, seed):
    """(f0, sp, ap) of a seeded piecewise contour"""
    return _finish(fs, fft, piecewise_f0(fs, fft, n_frames, seed), seed)


def contour(name, kind):
    """(f0, sp, ap) of contour `kind` of case `name`"""
    fs, fft, fp, seed, n_frames = CASES[name]
    lo, hi = d_range(fs, fft)
    tag = 1000 * (NAMES.index(name) + 1)
    if kind == "boundary":
        return _finish(fs, fft, piecewise_f0(fs, fft, n_frames, seed), tag)
    if kind == "steep":
        # the boundary contour over rows that make the single roundings count: where the quotient i / fs / (fp / 1000) of boundary k's
        # sample falls below k, the reference interpolates rows k - 1 and k for the pulse on it with a weight of a few ulps on row
        # k - 1 -- here 1e18 times row k, so that those ulps set the envelope (floor == k instead reads row k alone: an envelope
        # orders of magnitude away)
        f0, sp, ap = _finish(fs, fft, piecewise_f0(fs, fft, n_frames, seed), tag)
        for k in STEPS[name]:
            sp[k - 1] *= 1e4
            sp[k] *= 1e-14
        return f0, sp, ap
    if kind == "end_unvoiced":  # voiced -> unvoiced at the end: the extrapolated point (reference src/synthesis.cpp:239-242)
        f0 = piecewise_f0(fs, fft, 43, tag + 1)
        f0[-2] = fs / ((lo + hi) // 2)
        f0[-1] = 0.0
        return _finish(fs, fft, f0, tag + 1)
    if kind == "two":           # the shortest contour the stage takes (reference :241-242)
        return _finish(fs, fft, np.full(2, fs / lo), tag + 2)
    if kind == "gap":           # voiced, an unvoiced gap of more than 512 samples, voiced with a long pulse interval
        n = 100
        while (n * 25 // 100) * fp / 1000.0 * fs <= 600:
            n += 10
        assert n <= 120
        f0 = np.zeros(n)
        f0[:n * 35 // 100] = fs / (lo + 7)
        f0[n * 60 // 100:] = fs / min(640, 3 * fft // 4)
        f0[1] = fs / d_high(fs)
        return _finish(fs, fft, f0, tag + 3)
    raise KeyError(kind)


def below_boundaries(fs, fp, n_frames):
    """frames k = 1 .. n_frames - 1 whose boundary falls on the sample grid (|i - k fp fs| < 1e-6) with floor(i / fs / (fp / 1000)) == k - 1"""
    out = []
    for k in range(1, n_frames):
        i = int(round(k * (fp / 1000.0 * fs)))
        if abs(i - k * (fp / 1000.0 * fs)) < 1e-6 and int(np.floor(i / fs / (fp / 1000.0))) == k - 1:
            out.append(k)
    return out


def boundary_pulses(port, f0, fs, fft, fp):
    """pulses of the reference's time base on nominal frame-boundary samples (|i - k fp fs| < 1e-6, k >= 1), as two lists of sample
    indices: those with floor(i / fs / (fp / 1000)) == k - 1 and those with == k"""
    idx, _ = port.synthesis_pulse_list(f0, fft, fs, fp)
    below, at = [], []
    for i in idx:
        i = int(i)
        k = int(round(i / (fp / 1000.0 * fs)))
        if k < 1 or abs(i - k * (fp / 1000.0 * fs)) >= 1e-6:
            continue
        fl = int(np.floor(i / fs / (fp / 1000.0)))
        if fl == k - 1:
            below.append(i)
        elif fl == k:
            at.append(i)
    return below, at


def search(port, name, trials=300):
    """the seeded random search the stored seeds come from: the seed whose contour has the most boundary pulses of the rarer kind
    (then of both), among contours the reference's pulse arrays hold"""
    fs, fft, fp, _, n_frames = CASES[name]
    best = None
    for seed in range(trials):
        f0 = piecewise_f0(fs, fft, n_frames, seed)
        n, cap = port.synthesis_pulses(f0, fft, fs, fp)
        if n > cap:
            continue
        below, at = boundary_pulses(port, f0, fs, fft, fp)
        score = (min(len(below), len(at)), len(below) + len(at))
        if best is None or score > best[0]:
            best = (score, seed, len(below), len(at))
    return best


def pattern(kind, n_frames):
    p = PATTERNS[kind]
    return [n_frames] if p is None else p


def fixture_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_periods.npz")


# the fixture stores a waveform in full up to this many samples, and as windows plus block sums beyond (as synth_only_48k_10s.npz)
FULL_LIMIT, BLOCK, WIN, NWIN = 1500, 480, 192, 6


def windows(n, centres=()):
    """window starts: around the given samples (at most NWIN of them), NWIN evenly spaced ones otherwise"""
    if len(centres):
        return [int(min(max(c - WIN // 2, 0), n - WIN)) for c in list(centres)[:NWIN]]
    return [int(k * (n - WIN) / (NWIN - 1)) for k in range(NWIN)]


def harvest_signal(fs):
    from world_class_amd.synth import make_utterance
    return make_utterance(fs, HARVEST_SECONDS, HARVEST_SEED + fs // 1000)
