"""The rule of voice morphing (include/world_class_io.h, wc_morph_parameters_device) restated in numpy on top of
retime_rule.retime, and the inputs the tests share.  A helper of tests/test_morph_rule.py and tests/test_gpu_morph.py, not a test
module.

Output frame k has a position in A (pa), a position in B (pb), a weight w and an F0 weight wf (None: wf = w):
  pa, pb or w not finite   F0 and both rows NaN;  only wf not finite: F0 NaN
  A_k, B_k                 retime_rule.retime of A at pa and of B at pb, without scale
  ap                       w == 0: apA, w == 1: apB, else (1 - w) * apA + w * apB (two products and one sum, each rounded)
  sp                       w == 0: spA, w == 1: spB, else exp((1 - w) * log(spA) + w * log(spB))
  F0                       wf == 0: fA, wf == 1: fB; both voiced: exp((1 - wf) * log(fA) + wf * log(fB)); neither: 0; only A: fA
                           while wf < 0.5, only B: fB while wf > 0.5, else 0
(The spectral ratios per source are the device's own arithmetic, as in retime_rule: the GPU tests compare them with
wc_retime_parameters_device.)"""
import numpy as np

import retime_rule as rr

WEIGHTS = [0.0, 1.0, 0.25, 0.5, 0.75, -0.5, 1.5, 0.5]
PAIRS = [(61, 97), (97, 74), (74, 61)]  # source frames of (A, B)
# pair 0: one map for both sources; pairs 1 and 2: the map of A, the map of B
PAIR_MAPS = [("hold_and_back", "hold_and_back"), ("ramp", "speed_1.5"), ("slow_1.37", "overshoot")]


def morph(a, b, pos_a, pos_b, weight, f0_weight=None, ratio_a=None, ratio_b=None):
    """one pair: a and b are (f0, sp, ap); (f0, sp, ap) of the blend"""
    if ratio_a is not None or ratio_b is not None:
        raise NotImplementedError("the numpy rule has no spectral ratios (the device's own log / interp1 / exp)")
    pos_a, pos_b, w = (np.asarray(v, dtype=np.float64) for v in (pos_a, pos_b, weight))
    wf = w if f0_weight is None else np.asarray(f0_weight, dtype=np.float64)
    fa, spa, apa = rr.retime(a[0], a[1], a[2], pos_a)
    fb, spb, apb = rr.retime(b[0], b[1], b[2], pos_b)
    m = len(w)
    f0 = np.full(m, np.nan)
    sp = np.full(spa.shape, np.nan)
    ap = np.full(apa.shape, np.nan)
    for k in range(m):
        if not (np.isfinite(pos_a[k]) and np.isfinite(pos_b[k]) and np.isfinite(w[k])):
            continue
        if w[k] == 0:
            sp[k], ap[k] = spa[k], apa[k]
        elif w[k] == 1:
            sp[k], ap[k] = spb[k], apb[k]
        else:
            ap[k] = (1.0 - w[k]) * apa[k] + w[k] * apb[k]
            sp[k] = np.exp((1.0 - w[k]) * np.log(spa[k]) + w[k] * np.log(spb[k]))
        v = wf[k]
        if not np.isfinite(v):
            continue
        va, vb = fa[k] != 0, fb[k] != 0
        if v == 0:
            f0[k] = fa[k]
        elif v == 1:
            f0[k] = fb[k]
        elif va and vb:
            f0[k] = np.exp((1.0 - v) * np.log(fa[k]) + v * np.log(fb[k]))
        elif va:
            f0[k] = fa[k] if v < 0.5 else 0.0
        elif vb:
            f0[k] = fb[k] if v > 0.5 else 0.0
        else:
            f0[k] = 0.0
    return f0, sp, ap


def morph_batch(a_lengths, a, b_lengths, b, out_lengths, pos_a, pos_b, weight, f0_weight=None):
    """the packed batch: pair by pair"""
    outs, ia, ib, io = [], 0, 0, 0
    for na, nb, m in zip(a_lengths, b_lengths, out_lengths):
        wf = None if f0_weight is None else f0_weight[io:io + m]
        outs.append(morph(tuple(v[ia:ia + na] for v in a), tuple(v[ib:ib + nb] for v in b), pos_a[io:io + m], pos_b[io:io + m],
                          weight[io:io + m], wf))
        ia, ib, io = ia + na, ib + nb, io + m
    return tuple(np.concatenate([o[q] for o in outs]) for q in range(3))


def cycled_weights(m, first=0):
    return np.array([WEIGHTS[(first + i) % len(WEIGHTS)] for i in range(m)])


def to_length(pos, m):
    """a map truncated, or padded by holding its last position"""
    return pos[:m].copy() if len(pos) >= m else np.concatenate([pos, np.full(m - len(pos), pos[-1])])


def voicing_cases(fa, fb):
    """how many frames are voiced in both / only A / only B / neither"""
    va, vb = fa != 0, fb != 0
    return int((va & vb).sum()), int((va & ~vb).sum()), int((~va & vb).sum()), int((~va & ~vb).sum())


def batch(fs, fft, seed, with_f0_weight=False):
    """three ragged pairs of oracle/gen_golden.synth_params utterances: the weights cycle through WEIGHTS, the F0 weights (if any)
    through the same cycle three places on.  Pair 0 takes one map for both sources: synth_params leaves frames 31-39 and 71-79 of
    every utterance unvoiced, so equal positions meet frames where neither source is voiced (two different maps hardly ever do);
    pairs 1 and 2 take two different maps, B's truncated or padded to the length of A's.  All four voicing cases occur.
    A dict: a_lengths, b_lengths, out_lengths, a, b (packed f0, sp, ap), pos_a, pos_b, weight, f0_weight (or None)."""
    from oracle.gen_golden import synth_params
    pa_, pb_ = [], []
    srcs_a = [synth_params(fs, fft, na, seed + 2 * u) for u, (na, _) in enumerate(PAIRS)]
    srcs_b = [synth_params(fs, fft, nb, seed + 2 * u + 1) for u, (_, nb) in enumerate(PAIRS)]
    for u, ((na, nb), (ma, mb)) in enumerate(zip(PAIRS, PAIR_MAPS)):
        pos = rr.map_of(ma, na)
        pa_.append(pos)
        pb_.append(pos.copy() if u == 0 else to_length(rr.map_of(mb, nb), len(pos)))
    out_lengths = [len(p) for p in pa_]
    m = sum(out_lengths)
    d = dict(a_lengths=[p[0] for p in PAIRS], b_lengths=[p[1] for p in PAIRS], out_lengths=out_lengths,
             a=tuple(np.concatenate([s[q] for s in srcs_a]) for q in range(3)), b=tuple(np.concatenate([s[q] for s in srcs_b]) for q in range(3)),
             pos_a=np.concatenate(pa_), pos_b=np.concatenate(pb_), weight=cycled_weights(m),
             f0_weight=cycled_weights(m, 3) if with_f0_weight else None)
    fa = rr.retime_batch(d["a_lengths"], *d["a"], out_lengths, d["pos_a"])[0]
    fb = rr.retime_batch(d["b_lengths"], *d["b"], out_lengths, d["pos_b"])[0]
    assert all(c > 0 for c in voicing_cases(fa, fb)), voicing_cases(fa, fb)
    return d


def rule_of(d):
    return morph_batch(d["a_lengths"], d["a"], d["b_lengths"], d["b"], d["out_lengths"], d["pos_a"], d["pos_b"], d["weight"], d["f0_weight"])
