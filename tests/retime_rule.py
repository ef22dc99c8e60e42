"""The rule of time-scale modification (include/world_class_io.h, wc_retime_parameters_device) restated in numpy, and the time
maps the tests share.  A helper of tests/test_retime_rule.py and tests/test_gpu_retime.py, not a test module.

An utterance has n source frames; output frame k sits at pos[k] source frames from the first one:
  pos[k] not finite      F0 and both rows NaN
  p = min(max(pos[k], 0), n - 1), i = floor(p), a = p - i
  a == 0                 source frame i, bit for bit
  a > 0                  row = (1 - a) * row[i] + a * row[i + 1] (two products and one sum, each rounded);
                         F0: both neighbours voiced: the same expression; neither: 0; only i: f0[i] while a < 0.5, only i + 1:
                         f0[i + 1] while a > 0.5, else 0 -- voiced where the interpolated voicing of reference
                         src/synthesis.cpp:200-204 exceeds 0.5
then f0 *= f0_scale[k].  (The spectral stretch per output frame is the device's own arithmetic, log and exp: the GPU tests
compare it with wc_modify_parameters_frames_device and, within a tolerance, with oracle.port_io.)"""
import numpy as np


def retime(f0, sp, ap, pos, f0_scale=None):
    f0, sp, ap, pos = (np.asarray(a, dtype=np.float64) for a in (f0, sp, ap, pos))
    n, m = len(f0), len(pos)
    f0_out = np.full(m, np.nan)
    sp_out = np.full((m,) + sp.shape[1:], np.nan)
    ap_out = np.full((m,) + ap.shape[1:], np.nan)
    for k in range(m):
        if not np.isfinite(pos[k]):
            continue
        p = min(max(float(pos[k]), 0.0), float(n - 1))
        i = int(np.floor(p))
        a = p - i
        if a == 0:
            f0_out[k], sp_out[k], ap_out[k] = f0[i], sp[i], ap[i]
            continue
        j = i + 1
        sp_out[k] = (1.0 - a) * sp[i] + a * sp[j]
        ap_out[k] = (1.0 - a) * ap[i] + a * ap[j]
        vi, vj = f0[i] != 0, f0[j] != 0
        if vi and vj:
            f0_out[k] = (1.0 - a) * f0[i] + a * f0[j]
        elif vi:
            f0_out[k] = f0[i] if a < 0.5 else 0.0
        elif vj:
            f0_out[k] = f0[j] if a > 0.5 else 0.0
        else:
            f0_out[k] = 0.0
    if f0_scale is not None:
        f0_out = f0_out * np.asarray(f0_scale, dtype=np.float64)
    return f0_out, sp_out, ap_out


def retime_batch(lengths, f0, sp, ap, out_lengths, pos, f0_scale=None):
    """the packed batch: utterance by utterance"""
    outs, fi, fo = [], 0, 0
    for n, m in zip(lengths, out_lengths):
        sc = None if f0_scale is None else f0_scale[fo:fo + m]
        outs.append(retime(f0[fi:fi + n], sp[fi:fi + n], ap[fi:fi + n], pos[fo:fo + m], sc))
        fi, fo = fi + n, fo + m
    return tuple(np.concatenate([o[q] for o in outs]) for q in range(3))


def time_map(n_frames, speed):
    """what world_class_amd.io.time_map must return"""
    if np.ndim(speed) == 0:
        return np.arange(int(np.floor((n_frames - 1) / speed)) + 1) * float(speed)
    speed = np.asarray(speed, dtype=np.float64)
    pos = np.zeros(len(speed))
    for k in range(1, len(speed)):
        pos[k] = pos[k - 1] + speed[k - 1]
    return pos


MAPS = ("identity", "half_speed", "speed_1.5", "slow_1.37", "ramp", "hold_and_back", "overshoot")


def map_of(name, n):
    """the time maps of the tests for an utterance of n source frames (n > 30); with n = 120 the lengths are 120, 239, 80, 164, 144,
    188 and 142 output frames"""
    if name == "identity":
        return np.arange(n, dtype=np.float64)
    if name == "half_speed":
        return np.arange(2 * n - 1) / 2
    if name == "speed_1.5":
        return np.arange(int((n - 1) / 1.5) + 1) * 1.5
    if name == "slow_1.37":
        return np.arange(int((n - 1) * 1.37) + 1) / 1.37
    if name == "ramp":  # from speed 0.5 to 1.5 over 1.2 n output frames
        m = n + n // 5
        k = np.arange(m)
        return np.minimum(n - 1, np.cumsum(0.5 + k / m) - 0.5)
    if name == "hold_and_back":
        return np.concatenate([np.arange(30.0), np.full(20, 29.25), np.arange(29.25, 5, -0.75), np.arange(5.0, n, 1.1)])
    if name == "overshoot":
        return np.arange(-3.0, n + 4, 0.9)
    raise KeyError(name)


def ratios_of(fft):
    """the eight ratios of tests/test_gpu_modify_frames.py: none (0), six ordinary ones, the smallest valid one"""
    return [0.0, 0.37, 0.8, 0.999, 1.0, 1.2, 2.5, 2.0 / fft]


def cycled(fft, n, first=0):
    r = ratios_of(fft)
    return np.array([r[(first + i) % len(r)] for i in range(n)])
