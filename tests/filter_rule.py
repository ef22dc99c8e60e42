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
"""
import math

import numpy as np

import minimum_phase_rule as mp

POWER, LOG = 0, 1
MISTAKES = ("weights_swapped", "a_off_by_one", "m_conjugated", "no_1_over_n", "power_without_half", "row_t_plus_1", "row_not_held")

# K_NP: this file against the wide rule, 0.1731 u as tests/test_filter_rule.py measures it on every run (held below K_NP).
# MEASURED_DEVICE: the largest |device - rule| / u on the MI355X over tests/test_gpu_filter.py and tests/test_gpu_filter_chain.py:
# 0.5209 (fft 512 at 8 kHz, LOG rows; 0.41 at 1024, 0.15 at 2048, 0.03 at 4096; the block form against the wavefront form 0.22 at the
# most).  It is 3 K_np, below the 16 K_np at which a step would have to be named.  K: the next power of two above twice that.
K_NP = 0.25
MEASURED_DEVICE = 0.5209
K = 2.0


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


def overlap_add(a, r, n):
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
    return overlap_add(a, r, len(x))


def unit(x, rows, kind, fs, fft_size, frame_period_ms):
    """u = 2^-52 * max_t(||s_t||_1 * max_k |M_t[k]|) over the segments whose rows are finite (0.0 if there is none)"""
    a, s, ls = segment_inputs(x, rows, kind, fs, fft_size, frame_period_ms)
    if not len(a):
        return 0.0
    _, M, bad = responses(s, ls, fft_size)
    size = np.abs(s).sum(axis=-1) * np.abs(M).max(axis=-1)
    return 2.0 ** -52 * float(size[~bad].max()) if (~bad).any() else 0.0


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
