"""The map rule of include/world_class_warp.h in Python integers and floats, written from the header's text alone: a Python float is a
double, every operation on one is rounded and none is fused.  The rule at a position is tests/vresample_rule.py's vresample_at,
unchanged; `warp_at` only keeps it from building a signal as long as the positions reach (an output whose taps all lie outside the
signal is +0.0 by that rule)."""
import math

import numpy as np

import vresample_rule as R

NO_POSITION = -(1 << 63)
LIMIT = float(1 << 30)


def map_out_length(length, out_per_entry):
    return int(math.floor(float(length - 1) * out_per_entry)) + 1


def map_position(m, out_per_entry, in_per_unit, n):
    """output n of a map m of L >= 1 doubles"""
    L = len(m)
    t = float(n) / out_per_entry
    if t >= L - 1:
        v = float(m[L - 1])
    else:
        i = int(math.floor(t))
        w = t - i
        v = float(m[i]) if w == 0 else float(m[i]) + w * (float(m[i + 1]) - float(m[i]))
    p = v * in_per_unit
    if math.isfinite(p) and -LIMIT <= p < LIMIT:
        return int(math.floor(p * 4294967296.0))
    return NO_POSITION


def map_positions(m, out_per_entry, in_per_unit, n_out):
    return [map_position(m, out_per_entry, in_per_unit, n) for n in range(n_out)]


def live(positions, n, half):
    """which outputs have a tap inside a signal of n samples: -K <= q <= n - 1 + K"""
    return np.array([-half <= (int(p) >> 32) <= n - 1 + half for p in positions], dtype=bool)


def warp_at(x, positions, C, phase_bits):
    """vresample_at on the live outputs, +0.0 at the others"""
    half = (C.shape[1] - 1) // 2
    positions = [int(p) for p in positions]
    keep = live(positions, len(x), half)
    y = np.zeros(len(positions))
    if keep.any():
        y[keep] = R.vresample_at(x, [p for p, k in zip(positions, keep) if k], C, phase_bits)
    return y
