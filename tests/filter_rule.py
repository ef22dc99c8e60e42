"""THE rule of include/world_class_filter.h in numpy float64: a waveform filtered by one gain row per frame.

    centres      c_t = floor(((float)t * frame_period_ms) * (float)fs / 1000.0 + 0.5)
    segments     S is the least count with c_{S-1} >= n - 1; segment t uses row min(t, f_length - 1)
    weights      c_t < k < c_{t+1}: up = (k - c_t) / (c_{t+1} - c_t) into segment t+1, 1.0 - up into segment t; k == c_t: 1.0 into t
    span         a_t = (c_{t-1} + 1 if t else 0) .. b_t = min(n - 1, c_{t+1} - 1); s_t[j] = x[a_t + j] * w on N points, zero behind
    response     R = forward(s_t)[0 .. N/2] * M_t (minimum_phase_rule), Hermitian; r_t[j] = Re(sum_k R[k] e^{-2 pi i jk/N}) / N
    bad rows     a value of ls_t that is not finite: r_t is NaN
    output       y[k] = 0.0, then y[k] += r_t[k - a_t] for a_t <= k < a_t + N, t ascending

`mistake` names one of the one-line mistakes tests/test_filter_rule.py holds the committed bound against.  wide_filter is the same
rule with direct transforms in np.longdouble (N = 512 is what the test affords), which gives this file's own error.

The device's bound.  |device - rule| <= K * u with u = 2^-52 * max_t(||s_t||_1 * max_k |M_t[k]|) per utterance (||s_t||_1 max|M_t| is
a rigorous bound on |r_t|).  K is the next power of two above twice the largest |device - rule| / u observed on the MI355X over the
cases of tests/test_gpu_filter.py; the factor two covers inputs other than those (the device's transforms factor otherwise than
pocketfft, its exp / sin / cos / log are the lean forms whose bounds tests/test_lean_math.py holds).

The bound where many rows lie over a sample.  u bounds one row; where rows are summed the rule's own error passes it (0.47 u at hop 1,
above K_NP).  u_at[k] = 2^-52 * sum of ||s_t||_1 max|M_t| over the finite-row segments with a_t <= k < a_t + N bounds the magnitude
that arrives at sample k, and |device - rule|[k] <= K_AT * u_at[k] is what tests/test_gpu_filter_long.py asserts: K_NP_AT and K_AT are
set by the recipe of K_NP and K.
"""
import math

import numpy as np

import minimum_phase_rule as mp

POWER, LOG = 0, 1
SEGMENT_MISTAKES = ("weights_swapped", "a_off_by_one", "m_conjugated", "no_1_over_n", "power_without_half", "row_t_plus_1", "row_not_held")
# the overlap-add's, written over tiles of OLA_TILE outputs the way filter_overlap_add_kernel decides (overlap_add_tiled):
#   ola_last_tap_dropped          a row contributes its taps j < N - 1 only
#   ola_last_tap_segment_skipped  a tile skips the segment that reaches it with its last tap alone (a_t + N == t0 + 1)
#   ola_estimate_taken_as_first   a tile starts at floor((t0 - N) / h) + 2, what a_t + N > t0 gives for a_t = (t - 1) h + 1, and does not
#                                 walk.  (The kernel's estimate is floor((t0 - N) / h) - 1.  Without the - 1 and without the walk it is
#                                 still at or in front of the first segment for every hop >= 1 -- c_{t-1} <= (t - 1) h + 0.5 puts segment
#                                 floor((t0 - N) / h) - 1 and all before it in front of the tile -- and a start in front of the first
#                                 segment costs loads, not bits: tests/test_filter_rule.py holds that variant EQUAL to the rule.  The
#                                 first start that is wrong is this one, two further on.)
#   ola_trip_dropped_at_the_edge  the trip of four is dropped whole when its last segment starts behind the tile
#   ola_tiles_rounded_down        an utterance takes its tile count from its own length rounded down
OVERLAP_ADD_MISTAKES = ("ola_last_tap_dropped", "ola_last_tap_segment_skipped", "ola_estimate_taken_as_first", "ola_trip_dropped_at_the_edge",
                        "ola_tiles_rounded_down")
MISTAKES = SEGMENT_MISTAKES + OVERLAP_ADD_MISTAKES

# K_NP: this file against the wide rule, 0.1731 u as tests/test_filter_rule.py measures it on every run (held below K_NP).
# MEASURED_DEVICE: the largest |device - rule| / u on the MI355X over tests/test_gpu_filter.py and tests/test_gpu_filter_chain.py:
# 0.5209 (fft 512 at 8 kHz, LOG rows; 0.41 at 1024, 0.15 at 2048, 0.03 at 4096; the block form against the wavefront form 0.22 at the
# most).  It is 3 K_np, below the 16 K_np at which a step would have to be named.  K: the next power of two above twice that.
K_NP = 0.25
MEASURED_DEVICE = 0.5209
K = 2.0

# K_NP_AT: this file against the wide rule in units of u_at[k], 0.1017 as tests/test_filter_rule.py measures it on every run over hop 1
# (LOG noise 0.055, POWER envelope 0.069; n = 640), hop 3.2 (POWER noise, n = 900: 0.102) and hop 40 (POWER envelope, n = 2700: 0.015) at
# N = 512 (held below K_NP_AT).  In u the same errors are 0.47, 0.30, 0.30 and 0.013: above K_NP wherever the sum is deep.
# MEASURED_DEVICE_AT: the largest |device - rule|[k] / u_at[k] on the MI355X over tests/test_gpu_filter_long.py, per fft size.  The
# largest are the hop-1 cases on LOG rows of the moving 35-neper notch (0.79 at 512, 0.82 at 1024, 0.31 at 2048; 13 u, 11 u and 4 u);
# hop 1 on POWER rows of noise gives 0.17, 0.19, 0.16, the tile walk at hop 40 .. 1024 0.30 at 512, 0.12 at 1024, 0.04 at 2048 and 0.02
# at 4096, the tie hop 0.21 / 0.10, 300 short utterances 0.64.  The largest is 8 K_np_at, below the 16 at which a step would have to be named.
# K_AT: the next power of two above twice the largest of them.
K_NP_AT = 0.125
MEASURED_DEVICE_AT = {512: 0.7931, 1024: 0.8234, 2048: 0.3109, 4096: 0.0188}
K_AT = 2.0


def centre(t, frame_period_ms, fs):
    return int(math.floor((float(t) * frame_period_ms) * float(fs) / 1000.0 + 0.5))


def hop(frame_period_ms, fs):
    return frame_period_ms * fs / 1000.0


def accepts(fs, fft_size, frame_period_ms):
    """whether create takes the setting"""
    h = hop(frame_period_ms, fs)
    return fft_size in mp.SIZES and fs > 0 and math.isfinite(h) and h >= 1 and 2 * math.ceil(h) - 1 <= fft_size // 2


def segments(n, frame_period_ms, fs):
    if n <= 0:
        return 0
    s = 1
    while centre(s - 1, frame_period_ms, fs) < n - 1:
        s += 1
    return s


def span(t, n, frame_period_ms, fs):
    """(a_t, b_t, L_t)"""
    a = centre(t - 1, frame_period_ms, fs) + 1 if t else 0
    b = min(n - 1, centre(t + 1, frame_period_ms, fs) - 1)
    return a, b, b - a + 1


def weights(t, n, frame_period_ms, fs, mistake=None):
    """the weights of samples a_t .. b_t in segment t"""
    a, b, _ = span(t, n, frame_period_ms, fs)
    cm, c0, cp = (centre(t + d, frame_period_ms, fs) for d in (-1, 0, 1))
    w = np.ones(b - a + 1)
    for k in range(a, b + 1):
        if k < c0:
            up = float(k - cm) / float(c0 - cm)
            w[k - a] = 1.0 - up if mistake == "weights_swapped" else up
        elif k > c0:
            up = float(k - c0) / float(cp - c0)
            w[k - a] = up if mistake == "weights_swapped" else 1.0 - up
    return w


def log_gains(rows, kind, mistake=None):
    rows = np.asarray(rows, dtype=np.float64)
    if kind == LOG:
        return rows
    with np.errstate(all="ignore"):
        return np.log(rows) if mistake == "power_without_half" else np.log(rows) / 2.0


def segment_inputs(x, rows, kind, fs, fft_size, frame_period_ms, mistake=None):
    """-> (a [S], s [S, N] the weighted segments, ls [S, N/2+1] their log gains)"""
    x = np.asarray(x, dtype=np.float64)
    n, N = len(x), fft_size
    S = segments(n, frame_period_ms, fs)
    ls_all = log_gains(rows, kind, mistake)
    f_length = len(ls_all)
    a_all, s, ls = np.zeros(S, dtype=np.int64), np.zeros((S, N)), np.zeros((S, N // 2 + 1))
    for t in range(S):
        a, b, L = span(t, n, frame_period_ms, fs)
        s[t, :L] = x[a:b + 1] * weights(t, n, frame_period_ms, fs, mistake)
        a_all[t] = a + 1 if mistake == "a_off_by_one" else a
        r = t + 1 if mistake == "row_t_plus_1" else t
        ls[t] = ls_all[r % f_length if mistake == "row_not_held" else min(r, f_length - 1)]
    return a_all, s, ls


def responses(s, ls, fft_size, mistake=None):
    """r [S, N]: the circular convolution of every segment with its row's minimum-phase response; NaN where the row is bad"""
    N = fft_size
    bad = ~np.isfinite(ls).all(axis=-1)
    with np.errstate(all="ignore"):
        M = mp.minimum_phase(np.where(bad[:, None], 0.0, ls), N)
    if mistake == "m_conjugated":
        M = np.conj(M)
    R = mp.forward(s)[..., :N // 2 + 1] * M
    full = np.concatenate([R, np.conj(R[..., N // 2 - 1:0:-1])], axis=-1)
    full[..., 0] = full[..., 0].real
    full[..., N // 2] = full[..., N // 2].real
    r = np.fft.fft(full, axis=-1).real
    if mistake != "no_1_over_n":
        r = r / N
    r[bad] = np.nan
    return r, M, bad


OLA_TILE, OLA_TRIP = 1024, 4


def overlap_add_tiled(a, r, n, h, mistake=None):
    """the same sum the way filter_overlap_add_kernel decides it: tiles of OLA_TILE outputs, the first segment of a tile from an estimate
    and a walk, trips of OLA_TRIP segments until one starts behind the tile; h is the hop.  Without a mistake it is overlap_add bit for
    bit.  An output no tile writes stays 0.0."""
    S, N = r.shape
    y = np.zeros(n)
    tiles = n // OLA_TILE if mistake == "ola_tiles_rounded_down" else -(-n // OLA_TILE)
    taps = N - 1 if mistake == "ola_last_tap_dropped" else N
    for t0 in range(0, tiles * OLA_TILE, OLA_TILE):
        last, end = t0 + OLA_TILE - 1, min(n, t0 + OLA_TILE)
        q = math.floor(float(t0 - N) / h)
        if mistake == "ola_estimate_taken_as_first":
            t = max(int(q + 2.0), 0)
        elif mistake == "estimate_without_margin_or_walk":      # (no mistake: see MISTAKES)
            t = max(int(q), 0)
        else:
            est = q - 1.0
            t = int(est) if est > 0.0 else 0
            reach = t0 + 1 if mistake == "ola_last_tap_segment_skipped" else t0
            while t < S and int(a[t]) + N <= reach:
                t += 1
        acc = np.zeros(end - t0)
        while t < S:
            probe = min(t + OLA_TRIP - 1, S - 1) if mistake == "ola_trip_dropped_at_the_edge" else t
            if int(a[probe]) > last:
                break
            for tt in range(t, min(t + OLA_TRIP, S)):
                at = int(a[tt])
                lo, hi = max(at, t0), min(at + taps, end)
                if at <= last and hi > lo:
                    acc[lo - t0:hi - t0] += r[tt, lo - at:hi - at]
            t += OLA_TRIP
        y[t0:end] = acc
    return y


def overlap_add(a, r, n, mistake=None, h=None):
    """(h, the hop, is wanted with one of OVERLAP_ADD_MISTAKES only)"""
    if mistake in OVERLAP_ADD_MISTAKES:
        return overlap_add_tiled(a, r, n, h, mistake)
    y = np.zeros(n)
    N = r.shape[-1]
    for t in range(len(a)):
        lo, hi = int(a[t]), min(n, int(a[t]) + N)
        y[lo:hi] += r[t, :hi - lo]
    return y


def frame_filter(x, rows, kind, fs, fft_size, frame_period_ms, mistake=None):
    """y of THE rule (float64)"""
    a, s, ls = segment_inputs(x, rows, kind, fs, fft_size, frame_period_ms, mistake)
    if not len(a):
        return np.zeros(0)
    r, _, _ = responses(s, ls, fft_size, mistake)
    return overlap_add(a, r, len(x), mistake, hop(frame_period_ms, fs))


def unit(x, rows, kind, fs, fft_size, frame_period_ms):
    """u = 2^-52 * max_t(||s_t||_1 * max_k |M_t[k]|) over the segments whose rows are finite (0.0 if there is none)"""
    a, s, ls = segment_inputs(x, rows, kind, fs, fft_size, frame_period_ms)
    if not len(a):
        return 0.0
    _, M, bad = responses(s, ls, fft_size)
    size = np.abs(s).sum(axis=-1) * np.abs(M).max(axis=-1)
    return 2.0 ** -52 * float(size[~bad].max()) if (~bad).any() else 0.0


def parts(x, rows, kind, fs, fft_size, frame_period_ms):
    """one evaluation of the segments for a caller that wants several of y, u and u_at:
    (a [S], r [S, N], size [S] = ||s_t||_1 * max_k |M_t[k]|, bad [S])"""
    a, s, ls = segment_inputs(x, rows, kind, fs, fft_size, frame_period_ms)
    if not len(a):
        return a, np.zeros((0, fft_size)), np.zeros(0), np.zeros(0, dtype=bool)
    r, M, bad = responses(s, ls, fft_size)
    return a, r, np.abs(s).sum(axis=-1) * np.abs(M).max(axis=-1), bad


def unit_of(size, bad):
    """unit from parts"""
    return 2.0 ** -52 * float(size[~bad].max()) if (~bad).any() else 0.0


def unit_at_of(a, size, bad, n, fft_size):
    """unit_at from parts"""
    total = np.zeros(n)
    for t in range(len(a)):
        if not bad[t]:
            total[int(a[t]):min(n, int(a[t]) + fft_size)] += size[t]
    return 2.0 ** -52 * total


def unit_at(x, rows, kind, fs, fft_size, frame_period_ms):
    """u_at[k] = 2^-52 * sum of ||s_t||_1 * max_k |M_t[k]| over the segments with finite rows and a_t <= k < a_t + N: a rigorous bound on
    the magnitude that arrives at sample k, times the unit roundoff (0.0 where no such segment reaches)"""
    a, _, size, bad = parts(x, rows, kind, fs, fft_size, frame_period_ms)
    return unit_at_of(a, size, bad, len(x), fft_size)


def coded_gains(decode, to, frm=None, skip_energy=False):
    """the coded call's rows: decode(d), d = to - from (to alone without from), d[:, 0] = 0.0 with skip_energy"""
    d = np.array(to, dtype=np.float64) if frm is None else np.asarray(to, dtype=np.float64) - np.asarray(frm, dtype=np.float64)
    if skip_energy:
        d[:, 0] = 0.0
    return decode(d)


# ---- the wide rule -------------------------------------------------------------------------------------------------------------------
def _wide_dft(n, sign):
    k = np.arange(n)
    pi = 4 * np.arctan(np.longdouble(1))
    ang = (2 * pi / n) * ((k[:, None] * k[None, :]) % n).astype(np.longdouble)
    return np.cos(ang) + sign * 1j * np.sin(ang)


def wide_filter(x, rows, kind, fs, fft_size, frame_period_ms):
    """the rule with direct transforms in np.longdouble; the weighted segments and the log gains are the float64 ones (the rule's own
    roundings of x * w and of log(g) / 2 are part of the rule)"""
    N, m = fft_size, fft_size // 2
    a, s, ls = segment_inputs(x, rows, kind, fs, fft_size, frame_period_ms)
    Fp, Fm = _wide_dft(N, +1), _wide_dft(N, -1)
    r = np.zeros((len(a), N), dtype=np.longdouble)
    for t in range(len(a)):
        l = ls[t].astype(np.longdouble)
        full = np.concatenate([l, l[m - 1:0:-1]])
        cep = (Fp @ full).real
        cep[1:m] *= 2
        cep[m + 1:] = 0
        R = (Fp @ s[t].astype(np.longdouble)) * np.exp((Fp @ cep) / N)   # (bins 0 .. N/2 are the rule's; the rest is overwritten)
        R[0], R[m] = R[0].real, R[m].real
        R[m + 1:] = np.conj(R[m - 1:0:-1])
        r[t] = (Fm @ R).real / N
    y = np.zeros(len(x), dtype=np.longdouble)
    for t in range(len(a)):
        lo, hi = int(a[t]), min(len(x), int(a[t]) + N)
        y[lo:hi] += r[t, :hi - lo]
    return y


# ---- the inputs the tests share -----------------------------------------------------------------------------------------------------
ROW_KINDS = ("envelope", "notch", "noise", "zeros")


def case_rows(what, f_length, fft_size, seed=0):
    """f_length rows of log amplitude gains: minimum_phase_rule's formant envelope swung through gains of +-50 dB (5.756 nepers), its
    35-deep notch moved from row to row, 0.5 N(0, 1), or zeros (M is exactly 1)"""
    m = fft_size // 2
    rng = np.random.default_rng(77 + seed)
    out = np.zeros((f_length, m + 1))
    for t in range(f_length):
        if what == "envelope":
            out[t] = mp.fixture_input("envelope", fft_size) * (0.55 + 0.45 * math.cos(0.9 * t + seed)) + 5.756 * math.sin(1.7 * t + seed)
        elif what == "notch":
            out[t] = np.roll(mp.fixture_input("notch", fft_size), 7 * t)
        elif what == "noise":
            out[t] = 0.5 * rng.normal(size=m + 1)
        else:
            assert what == "zeros"
    return out


def as_kind(log_rows, kind):
    """log amplitude gains as rows of the kind"""
    return np.exp(2.0 * log_rows) if kind == POWER else log_rows


# ---- the long cases: tests/test_gpu_filter_long.py runs them, tests/test_filter_rule.py holds the overlap-add's mistakes against them ---
# (fs, fft_size, frame_period_ms, n).  WALK: a few tiles each, some tile's estimate floor((t0 - N) / h) - 1 is positive, n ends a few
# samples into its last tile; the last two at the largest hop.  DEEP: hop 1 from periods that are binary fractions (N rows over every
# sample, S = n), hop 1.5 (centres 0, 2, 3, 5, 6 ...) and hop 24 at 1024 (43 rows over a sample).  TIES: hop 64.49999999999999, where
# the rule's c_t lies one above the exact value at 16 of the first 80 t.
WALK = ((8000, 512, 5.0, 2051), (16000, 1024, 5.0, 3077), (44100, 2048, 5.0, 4101), (48000, 2048, 5.0, 4101), (96000, 4096, 5.0, 7171),
        (48000, 2048, 512 / 48.0, 5125), (96000, 4096, 1024 / 96.0, 8193))
DEEP = ((8000, 512, 0.125, 2051), (16000, 1024, 0.0625, 3077), (32000, 2048, 0.03125, 4101), (8000, 512, 0.1875, 2051), (24000, 1024, 1.0, 3077))
TIES = ((22050, 1024, 64.5 / 22.05, 3077), (22050, 512, 64.5 / 22.05, 3077))
ROW_MODES = ("exact", "held", "surplus")


def estimates(n, fs, fft_size, frame_period_ms):
    """floor((t0 - N) / h) - 1 of every tile of an utterance of n samples"""
    h = hop(frame_period_ms, fs)
    return [math.floor(float(t0 - fft_size) / h) - 1.0 for t0 in range(0, n, OLA_TILE)]


def mode_rows(what, mode, S, fft_size, kind, seed):
    """rows of the content for S segments: as many ("exact"), two that are held ("held"), two more than are read ("surplus")"""
    return as_kind(case_rows(what, {"exact": S, "held": min(2, S), "surplus": S + 2}[mode], fft_size, seed), kind)


def long_batch(fs, fft_size, frame_period_ms, n, kind, seed, modes=ROW_MODES):
    """the long utterance (noise rows), one of hop + 1 samples (notch rows) and one of exactly OLA_TILE samples (noise rows): the grid is
    wider than the two short ones need.  modes: how many rows each of the three gets."""
    rng = np.random.default_rng(1000 + seed)
    lengths = (n, int(hop(frame_period_ms, fs)) + 1, OLA_TILE)
    xs = [rng.normal(size=m) for m in lengths]
    rows = [mode_rows(what, mode, segments(m, frame_period_ms, fs), fft_size, kind, seed + i)
            for i, (m, what, mode) in enumerate(zip(lengths, ("noise", "notch", "noise"), modes))]
    return xs, rows


def deep_case(fs, fft_size, frame_period_ms, n, kind, seed):
    """one utterance with a row per segment: noise as POWER rows, the moving notch as LOG rows"""
    x = np.random.default_rng(2000 + seed).normal(size=n)
    return x, mode_rows("noise" if kind == POWER else "notch", "exact", segments(n, frame_period_ms, fs), fft_size, kind, seed)
