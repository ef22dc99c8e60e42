"""The rule of include/world_class_resample.h in numpy: the plan, the table, the counts and the summation, each written from the
header's text alone.  numpy rounds every product and every sum and never fuses them, and the taps are added in ascending order, so
`resample` reproduces the library bit for bit when it is given the library's own table."""
import math

import numpy as np

ZEROS = 64
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492
# the conversions whose quality DESIGN.md section 10 quotes: (fs_in, fs_out) -> (L, M, K)
TABLE = {
    (44100, 48000): (160, 147, 68),
    (48000, 44100): (147, 160, 74),
    (44100, 24000): (80, 147, 125),
    (48000, 24000): (1, 2, 136),
    (24000, 48000): (2, 1, 68),
    (96000, 8000): (1, 12, 811),
    (22050, 16000): (320, 441, 94),
}


def plan(fs_in, fs_out, zeros=ZEROS, rolloff=ROLLOFF):
    """(L, M, K, s)"""
    g = math.gcd(fs_in, fs_out)
    up, down = fs_out // g, fs_in // g
    s = rolloff * min(1.0, float(up) / down)
    return up, down, int(math.ceil(zeros / s)), s


def table(fs_in, fs_out, zeros=ZEROS, rolloff=ROLLOFF, beta=BETA):
    """G as an [L, 2K+1] array"""
    up, _, half, s = plan(fs_in, fs_out, zeros, rolloff)
    k = np.arange(-half, half + 1, dtype=np.int64)[None, :]
    p = np.arange(up, dtype=np.int64)[:, None]
    d = (k * up - p).astype(np.float64) / float(up)
    u = d * s / zeros
    inside = np.abs(u) < 1
    w = np.where(inside, np.i0(beta * np.sqrt(np.where(inside, 1 - u * u, 0.0))) / np.i0(beta), 0.0)
    v = s * d
    sinc = np.where(v == 0, 1.0, np.sin(np.pi * v) / np.where(v == 0, 1.0, np.pi * v))
    return s * sinc * w


def out_length(up, down, n):
    return -(-(n * up) // down)


def committed(up, down, half, samples, flushed=False):
    if flushed:
        return out_length(up, down, samples)
    if samples <= half:
        return 0
    return min(out_length(up, down, samples - half), out_length(up, down, samples))


def resample(x, up, down, G):
    """y of one utterance x (float64) on the table G: ((0.0 + x[q-K] G[p][0]) + x[q-K+1] G[p][1]) + ..."""
    x = np.asarray(x, dtype=np.float64)
    half = (G.shape[1] - 1) // 2
    n = np.arange(out_length(up, down, len(x)), dtype=np.int64)
    q, p = n * down // up, n * down % up
    xp = np.concatenate([np.zeros(half), x, np.zeros(half + 1)])  # xp[q + j] = x[q - K + j], +0.0 outside
    acc = np.zeros(len(n))
    for j in range(G.shape[1]):
        acc = acc + xp[q + j] * G[p, j]
    return acc


def pcm16(y):
    """wc_double_to_pcm16_device's quantisation for finite y"""
    return np.clip(np.trunc(np.asarray(y, dtype=np.float64) * 32767), -32768, 32767).astype(np.int16)
