"""The rule of include/world_class_vresample.h in numpy: the plan, the table, the positions, the counts and the summation, each
written from the header's text alone.  numpy rounds every product and every sum and never fuses them, and the taps are added in
ascending order, so `vresample_at` reproduces the library bit for bit when it is given the library's own table.  Positions and steps
are Python integers: pos = q 2^32 + f."""
import math

import numpy as np

ZEROS = 64
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492
ONE = 1 << 32
DEFAULT = (3, 5)  # phase_bits, degree


def plan(step_max, zeros=ZEROS, rolloff=ROLLOFF, phase_bits=DEFAULT[0], degree=DEFAULT[1]):
    """(K, P, D, s)"""
    s = rolloff * min(1.0, 4294967296.0 / float(step_max))
    return int(math.ceil(zeros / s)), 1 << phase_bits, degree, s


def prototype(d, s, zeros=ZEROS, beta=BETA):
    """g(d) for an array of distances"""
    d = np.asarray(d, dtype=np.float64)
    u = d * s / zeros
    inside = np.abs(u) < 1
    w = np.where(inside, np.i0(beta * np.sqrt(np.where(inside, 1 - u * u, 0.0))) / np.i0(beta), 0.0)
    v = s * d
    sinc = np.where(v == 0, 1.0, np.sin(np.pi * v) / np.where(v == 0, 1.0, np.pi * v))
    return s * sinc * w


def table(step_max, zeros=ZEROS, rolloff=ROLLOFF, beta=BETA, phase_bits=DEFAULT[0], degree=DEFAULT[1]):
    """C as a [P, 2K+1, D+1] array: for every segment and tap the polynomial through g at the segment's Chebyshev nodes"""
    half, segs, deg, s = plan(step_max, zeros, rolloff, phase_bits, degree)
    nu = -np.cos(np.pi * (np.arange(deg + 1) + 0.5) / (deg + 1))
    V = nu[:, None] ** np.arange(deg + 1)[None, :]
    k = np.arange(-half, half + 1, dtype=np.float64)
    C = np.empty((segs, 2 * half + 1, deg + 1))
    for seg in range(segs):
        phi = (seg + (nu + 1.0) / 2.0) / segs
        g = prototype(k[None, :] - phi[:, None], s, zeros, beta)  # [node, tap]
        C[seg] = np.linalg.solve(V, g).T
    return C


def out_length(step, n):
    return -(-(n * ONE) // step)


def committed(q, f, step, half, samples, flushed=False):
    """the outputs at (q, f) + i step, i >= 0, that a stream with `samples` samples commits"""
    lim = samples if flushed else max(samples - half, 0)
    room = lim * ONE - (q * ONE + f)
    return -(-room // step) if room > 0 else 0


def positions(step, count, start=0):
    """`count` positions from `start`, spaced by step"""
    return [start + i * step for i in range(count)]


def vresample_at(x, positions, C, phase_bits):
    """y at explicit positions of one utterance x (float64) on the table C:
    a_m = ((0.0 + x[q-K] C[seg][0][m]) + x[q-K+1] C[seg][1][m]) + ..., y = ((a_D nu + a_{D-1}) nu + ...) nu + a_0"""
    x = np.asarray(x, dtype=np.float64)
    taps, deg = C.shape[1], C.shape[2] - 1
    half = (taps - 1) // 2
    if len(positions) == 0:
        return np.zeros(0)
    q = np.array([p >> 32 for p in positions], dtype=np.int64)
    f = np.array([p & (ONE - 1) for p in positions], dtype=np.int64)
    seg = f >> (32 - phase_bits)
    mu = (f & ((1 << (32 - phase_bits)) - 1)).astype(np.float64) * 2.0 ** (phase_bits - 32)
    nu = 2.0 * mu - 1.0
    base = int(q.min())
    top = int(q.max())
    # xp[q - base + j] = x[q - K + j], +0.0 outside [0, N)
    idx = np.arange(base - half, top + half + 1)
    xp = np.where((idx >= 0) & (idx < len(x)), x[np.clip(idx, 0, len(x) - 1)], 0.0)
    a = np.zeros((deg + 1, len(q)))
    for j in range(taps):
        a = a + xp[q - base + j][None, :] * C[seg, j, :].T
    y = a[deg]
    for m in range(deg - 1, -1, -1):
        y = y * nu + a[m]
    return y


def vresample(x, step, C, phase_bits):
    """a whole utterance at one step"""
    return vresample_at(x, positions(step, out_length(step, len(x))), C, phase_bits)


def pcm16(y):
    """wc_double_to_pcm16_device's quantisation for finite y"""
    return np.clip(np.trunc(np.asarray(y, dtype=np.float64) * 32767), -32768, 32767).astype(np.int16)


def table_error(C, step_max, phase_bits, fractions, zeros=ZEROS, rolloff=ROLLOFF, beta=BETA):
    """(max coefficient error, worst-phase sum S) of the table against the exact prototype at the given 32-bit fractions: the
    polynomial of every tap at nu(f) against g(k - f 2^-32)"""
    half, _, deg, s = plan(step_max, zeros, rolloff, phase_bits, C.shape[2] - 1)
    f = np.asarray(fractions, dtype=np.int64)
    seg = f >> (32 - phase_bits)
    nu = 2.0 * ((f & ((1 << (32 - phase_bits)) - 1)).astype(np.float64) * 2.0 ** (phase_bits - 32)) - 1.0
    k = np.arange(-half, half + 1, dtype=np.float64)
    worst, worst_sum = 0.0, 0.0
    for a in range(0, len(f), 256):
        sl = slice(a, a + 256)
        poly = np.zeros((len(f[sl]), len(k)))
        for m in range(deg, -1, -1):
            poly = poly * nu[sl][:, None] + C[seg[sl], :, m]
        err = np.abs(poly - prototype(k[None, :] - (f[sl].astype(np.float64) * 2.0 ** -32)[:, None], s, zeros, beta))
        worst = max(worst, float(err.max()))
        worst_sum = max(worst_sum, float(err.sum(axis=1).max()))
    return worst, worst_sum
