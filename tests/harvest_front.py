"""Harvest's front half -- decimation, the int-typed DC removal, the band-pass with its four zero-crossing detectors, the raw
candidates and the detector over bands (reference src/harvest.cpp:213-248, :1005-1346, src/world_matlabfunctions.cpp:27-210) --
on signals written by hand: a high-precision rule of every stage and the tables it is checked on.  numpy only.  The signals are
written with the host's sin and cos and seeded noise: the same on every run of one host, a rounding apart between hosts whose
libm differs -- so K_ref and every figure measured on them belong to the host that measured them.

The rule.  np.longdouble except where the reference decides in integers.
 * decimate_rule: getWaveformAndSpectrum's padding (lag = ceil(140 / r) r edge samples on either side), decimate's nine
   reflected samples, FilterForDecimate's recursion forward and over the reversed output, sample by sample, from COEF (typed
   here as data, not read from the product), nout / nbeg and the copy from lag / r.  r = 1: x followed by one zero, exactly.
 * dc_rule: acc = (int)(acc + y[i]) on the float64 samples in the reference's order -- integer arithmetic, exact -- then
   mean = acc / n in float64 and the one subtraction.
 * band_rule, per band b: hl = round(fs_d / b * 2); taps Nuttall(i / 2 hl) cos(2 pi b i / fs_d); f[i] = sum_j tap[j] y[i + 1 - j],
   the reference's index bias of hl + 1 (one sample late), as a direct sum; beside it A[i] = sum_j |tap[j] y[i + 1 - j]|.  The four
   detectors (f, -f, the difference f[i+1] - f[i] and its negative; 0 < s[i] && s[i+1] <= 0), fine edges
   e - s[e-1] / (s[e] - s[e-1]), intervals fs_d / (fine[i+1] - fine[i]) at (fine[i] + fine[i+1]) / 2 / fs_d; fewer than three
   intervals of any type (the reference's checkEvent(n - 2)) is a band of zeros; interp1 onto the 1 ms grid with histc's clamping
   (the first / last segment extrapolates), the mean of the four, and the four-sided test > 1.1 b, < 0.9 b, > ceil, < floor with
   the two products formed in float64.
 * detect_rule: a function of a raw table alone, float64, the reference's order -- vuv, zeros forced at both end bands, runs of at
   least 10 bands, the run's values summed ascending and divided by the run length.  The device sums in the same order, so its
   candidates are compared bit for bit.

The units.  Nothing is fitted to the device; each unit is formed from the rule's own sums.
 * y: u_y = eps sum_k |g_k x|, g the zero-phase impulse response of the two passes.  It is evaluated as the two passes themselves
   run on |h| and |x| (h the one-pass response cut where it stays below 1e-20 of its peak), so the samples the second pass never
   sees at the far end are left out exactly as the filter leaves them out.
 * a fine edge: u_e = eps A / |s[e] - s[e-1]|, A the largest of A[e-1], A[e], A[e+1].  An interval F between two edges moves by
   (F^2 / fs_d) per sample of edge error, so a raw candidate at a frame has
   u = mean over the four types of [(|1 - s| F0^2 + |s| F1^2 + 2 |F1 - F0| max(F0, F1)) / fs_d * max u_e] + eps F
   with F0, F1 the two intervals its interpolation reads, s the interpolation weight (beyond 0..1 where histc extrapolates) and
   max u_e over the three edges that bound them.
 * K_ref: the restatement's (oracle/port.harvest_debug: a float64 recursion, an FFT convolution) largest error in these units
   against the rule over all tables, per stage, measured where it is used (k_ref below); printed, recorded in DESIGN.md, never
   written down as a tolerance.
 * the device is allowed 2 K_ref(y) units on y (K_ref(y) taken over the tables of the decimation ratio it runs: the float64
   recursion's error grows from 1 unit at r = 2 to 70 to 80 at r = 12), 2 K_ref(raw) units on raw candidates of the FIR form and 2 K_ref(raw)
   max(1, p / log2 N) on those of the sliding forms: N is the reference's FFT size for the signal and p the number of steps of
   the rotating recurrence the sliding sums have gone through when they produce the sample -- the 2 hl + 1 steps that build a
   chunk's first window and one step per output of the 2048-sample chunk since (linear accumulation against a transform's
   logarithmic one, the refinement pin's argument).  The growth multiplies the edge part of u, not eps F.
 * near-threshold set: frames whose rule value lies within the allowed error of 1.1 b, 0.9 b, floor or ceil and which no other
   of the four comparisons rejects beyond doubt, and frames within two periods of the band of a sample at which |f| (or the
   difference signal) is below the allowed error eps A of its own sum -- an edge might appear or vanish there -- unless the
   sample's neighbours lie firmly on opposite sides (then there is one crossing either way, at the same place to first order).
   Elsewhere the zero pattern must be the rule's.  At most 1 % of a table's live positions (those of bands in which all four
   series exist) may be in the set.

The tables.  Each is (signals, handle options, what it must reach); tests/test_harvest_front_rule.py proves on the CPU that each
reaches it, tests/test_gpu_harvest_front.py then holds the device to the rule on them.  Band-pass tables run at fs = 8000 with
target_fs = 8000 on signals below 1: y is the signal and one zero, bit for bit, and a sinusoid's crossings sit where the table
put them.  Every signal is at least three 1 ms frames long (a handle takes nothing shorter) and long enough for the reference's
FFT buffer to hold its lowest band's taps (Table.add).  `burst` and `level_drop` are not stationary.  Behind burst's tone lie
exact zeros, where the reference's FFT convolution leaves the roundings of the whole utterance; the restatement and the reference
are compared there under that utterance-wide unit (near_threshold(wide=True)), the device under the local one.

Level-drop tables.  The A of a unit at a sample is the largest A since the last point at which that side's sums were formed
afresh: for the reference's FFT convolution the whole utterance (wide=True); for the device's sliding sums the chunk up to the
sample, and the sample's own window -- with no growth -- where the chunk is left to direct sums.  Which chunks those are is
restated from the kernel's header (quiet_chunks: a block of 64 samples whose largest |y| is below 1e-8 of the largest before it,
anywhere in what the chunk's sums read), not read from the device.  A device is held there (1) to the rule's zero pattern on
every frame that is firm under the utterance-wide unit and (2), on those frames, to twice the restatement's error on the same
frame plus its own stationary bound in the unit just named: it may not be more than twice worse than the reference where the
reference itself is noisy.  On a chunk left to direct sums (falls to 0.5e-8 and 1e-10) that unit is tiny and the bound is in
effect twice the reference's own noise; on one that is not (2e-8, 1e-6) the unit carries the loud part of the chunk.  That a fall
to 2e-8 is NOT left to direct sums and one to 0.5e-8 is, is held bit for bit against the form that never falls back.
"""
import math

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "the rule needs a long double wider than float64"
LOG2 = 0.69314718055994529
PI_L = LD(4) * np.arctan(LD(1))
EPS = float(np.finfo(np.float64).eps)
SD_CH = 2048     # outputs per chunk of the sliding band-pass (wc_harvest.hip)
FIR_ADV = 2046   # tile advance of the FIR band-pass
DS_SPAN = 15616  # decimated samples per block of hv_decimate_scan_kernel
K_NFACT = 9

# FilterForDecimate's coefficient sets (a0, a1, a2, b0, b1) per ratio: data of the rule
COEF = {
    2: (0.041156734567757189, -0.42599112459189636, 0.041037215479961225, 0.16797464681802227, 0.50392394045406674),
    3: (0.95039378983237421, -0.67429146741526791, 0.15412211621346475, 0.071221945171178636, 0.21366583551353591),
    4: (1.4499664446880227, -0.98943497080950582, 0.24578252340690215, 0.036710750339322612, 0.11013225101796784),
    5: (1.7610939654280557, -1.2554914843859768, 0.3237186507788215, 0.021334858522387423, 0.06400457556716227),
    6: (1.9715352749512141, -1.4686795689225347, 0.3893908434965701, 0.013469181309343825, 0.040407543928031475),
    7: (2.1225239019534703, -1.6395144861046302, 0.44469707800587366, 0.0090366882681608418, 0.027110064804482525),
    8: (2.2357462340187593, -1.7780899984041358, 0.49152555365968692, 0.0063522763407111993, 0.019056829022133598),
    9: (2.3236003491759578, -1.8921545617463598, 0.53148928133729068, 0.0046331164041389372, 0.013899349212416812),
    10: (2.3936475118069387, -1.9873904075111861, 0.5658879979027055, 0.0034818622251927556, 0.010445586675578267),
    11: (2.450743295230728, -2.06794904601978, 0.59574774438332101, 0.0026822508007163792, 0.0080467524021491377),
    12: (2.4981398605924205, -2.1368928194784025, 0.62187513816221485, 0.0021097275904709001, 0.0063291827714127002),
}

# single changes to the rule that a device held to it would be caught by ("ge_upper", `>= 1.1 b`, is a seventh the rule knows: it
# differs at equality alone, out of any device's reach, and is not listed)
MUTANTS = ("bias_hl", "fine_from_e", "lt0", "run9", "coef12", "dc_round")
# the table each mutant of the rule must be caught on
MUTANT_TABLE = {"bias_hl": "seam", "fine_from_e": "late_in_chunk", "lt0": "burst", "run9": "runs_33",
                "coef12": "ratio_7", "dc_round": "dc"}


def mround(x):
    return int(x + 0.5) if x > 0 else int(x - 0.5)


def frames_1ms(n, fs):
    return int(1000.0 * n / fs) + 1


def band_list(floor, ceil, cio):
    """boundary_f0_list of reference :1388-1397, float64"""
    lo, hi = floor * 0.9, ceil * 1.1
    n = 1 + int(math.log(hi / lo) / LOG2 * cio)
    return [lo * math.pow(2.0, float(i + 1) / cio) for i in range(n)]


def slots(n_bands):
    return mround(n_bands // 10)


def half_len(fs_d, b):
    return mround(fs_d / b * 2.0)


def fft_size(y_len, fs_d, b0):
    """the reference's transform size for a signal (reference :1401-1403, GetSuitableFFTSize)"""
    n = y_len + 4 * int(1.0 + fs_d / b0 / 2.0)
    return int(math.pow(2.0, int(math.log(n) / LOG2) + 1.0))


# ------------------------------------------------------------------------------------------------------------------------
# decimation and DC removal
# ------------------------------------------------------------------------------------------------------------------------
def _iir(x, c):
    """FilterForDecimate's recursion, long double, sample by sample"""
    a0, a1, a2, b0, b1 = [LD(v) for v in c]
    y = np.empty(len(x), dtype=LD)
    w0 = w1 = w2 = LD(0)
    for i, v in enumerate(x):
        wt = v + a0 * w0 + a1 * w1 + a2 * w2
        y[i] = b0 * wt + b1 * w0 + b1 * w1 + b0 * w2
        w2, w1, w0 = w1, w0, wt
    return y


_impulse = {}


def impulse(r):
    """|h| of one pass, float64, cut behind the last sample that reaches 1e-20 of the peak"""
    if r not in _impulse:
        d = np.zeros(4096, dtype=LD)
        d[0] = 1
        h = np.abs(_iir(d, COEF[r])).astype(np.float64)
        _impulse[r] = h[:int(np.flatnonzero(h >= 1e-20 * h.max())[-1]) + 1]
    return _impulse[r]


def _padded(x, r):
    lag = int(math.ceil(140.0 / r) * r)
    x = np.asarray(x, dtype=LD)
    nx = np.concatenate([np.full(lag, x[0]), x, np.full(lag, x[-1])])
    t = np.concatenate([2 * nx[0] - nx[K_NFACT:0:-1], nx, 2 * nx[-1] - nx[-2:-2 - K_NFACT:-1]])
    return lag, len(nx), t


def _keep(v, nn, r, lag, y_len):
    """decimate's nout / nbeg walk over the twice-filtered padded signal v and the copy from lag / r"""
    nout = nn // r + 1
    nbeg = r - r * nout + nn
    out = v[np.arange(nbeg, nn + K_NFACT, r) + K_NFACT - 1]
    y = np.zeros(y_len, dtype=v.dtype)
    got = out[lag // r: lag // r + y_len]
    y[:len(got)] = got
    return y


def decimate_rule(x, r, coef=None):
    """(y before the DC removal [1 + n / r], long double; u_y per sample, float64)"""
    n = len(x)
    y_len = 1 + n // r
    if r == 1:
        return np.concatenate([np.asarray(x, dtype=LD), np.zeros(1, dtype=LD)]), np.zeros(y_len)
    c = COEF[r] if coef is None else coef
    lag, nn, t = _padded(x, r)
    v = _iir(_iir(t, c)[::-1], c)[::-1]
    h = impulse(r)
    a = np.abs(t).astype(np.float64)
    g = np.convolve(np.convolve(a, h)[:len(a)][::-1], h)[:len(a)][::-1]
    return _keep(v, nn, r, lag, y_len), EPS * _keep(g, nn, r, lag, y_len)


def dc_rule(y, mutant=None):
    """the int-typed accumulation on the float64 samples, then the subtraction in long double; returns (y, acc)"""
    acc = 0
    for v in np.asarray(y, dtype=np.float64).tolist():
        acc = int(round(acc + v)) if mutant == "dc_round" else int(acc + v)
    mean = float(acc) / len(y)
    return np.asarray(y, dtype=LD) - LD(mean), acc


# ------------------------------------------------------------------------------------------------------------------------
# one band: band-pass, detectors, raw candidates
# ------------------------------------------------------------------------------------------------------------------------
def taps(fs_d, b, hl):
    i = np.arange(-hl, hl + 1).astype(LD)
    t = (i + hl) / (2 * LD(hl))
    w = LD(0.355768) - LD(0.487396) * np.cos(2 * PI_L * t) + LD(0.144232) * np.cos(4 * PI_L * t) - LD(0.012604) * np.cos(6 * PI_L * t)
    return w * np.cos(2 * PI_L * LD(b) * i / LD(fs_d))


def bandpass(y, fs_d, b, mutant=None):
    """f[i] and A[i], i < len(y): direct sums with the reference's index bias hl + 1"""
    hl = half_len(fs_d, b)
    h = taps(fs_d, b, hl)
    bias = hl if mutant == "bias_hl" else hl + 1
    n = len(y)
    z = np.zeros(1, dtype=LD)
    f = np.concatenate([np.convolve(y, h), z])[bias:bias + n]
    A = np.concatenate([np.convolve(np.abs(y), np.abs(h)), z])[bias:bias + n]
    return f, A.astype(np.float64), hl


def _engine(s, A2, U2, grow, n, fs_d, mutant):
    """zeroCrossingEngine on s[:n]: (edges, fine, u_e in samples for the direct and for the sliding sums, intervals, locations) or
    None.  A2: the sums' own A; U2: the sliding side's A (band_rule), which grows by grow[e]"""
    lead = s[:n - 1] > 0
    fall = (s[1:n] < 0) if mutant == "lt0" else (s[1:n] <= 0)
    e = np.flatnonzero(lead & fall) + 1
    if len(e) < 2:
        return None
    den = s[e] - s[e - 1]
    fine = e.astype(LD) - (s[e] if mutant == "fine_from_e" else s[e - 1]) / den
    Ae = np.maximum(np.maximum(A2[e - 1], A2[e]), A2[np.minimum(e + 1, len(A2) - 1)])
    Ge = np.maximum(np.maximum(U2[e - 1], U2[e]), U2[np.minimum(e + 1, len(U2) - 1)]) * grow[e]
    ue = EPS * Ae / np.abs(den).astype(np.float64)
    ug = EPS * Ge / np.abs(den).astype(np.float64)
    fs = LD(fs_d)
    return dict(e=e, fine=fine, ue=ue, ug=ug, itv=fs / (fine[1:] - fine[:-1]), loc=(fine[:-1] + fine[1:]) / 2 / fs)


def _interp(z, t, fs_d):
    """interp1 of one interval series onto t (histc's clamping); returns (values, unit of the FIR form, unit of the sliding forms)"""
    loc, itv, ue = z["loc"], z["itv"], z["ue"]
    n = len(loc)
    k = np.clip(np.searchsorted(loc, t, side="right"), 1, n - 1)
    s = (t - loc[k - 1]) / (loc[k] - loc[k - 1])
    v = itv[k - 1] + s * (itv[k] - itv[k - 1])
    f0, f1, sf = itv[k - 1].astype(np.float64), itv[k].astype(np.float64), s.astype(np.float64)
    gain = (np.abs(1 - sf) * f0 * f0 + np.abs(sf) * f1 * f1 + 2 * np.abs(f1 - f0) * np.maximum(f0, f1)) / fs_d
    ug = z["ug"]
    worst = np.maximum(np.maximum(ue[k - 1], ue[k]), ue[k + 1])
    worst_g = np.maximum(np.maximum(ug[k - 1], ug[k]), ug[k + 1])
    return v, gain * worst, gain * worst_g


def quiet_chunks(y, hl_max):
    """the chunks the sliding band-pass leaves to direct sums, as its header states them: a chunk is quiet if, over the samples its
    sums ever see -- 2 hl_max + 2 in front of its first output to hl_max + 4 behind its last, in whole blocks of 64, not beyond
    the utterance -- the largest |y| of a block falls below 1e-8 of the largest of the blocks before it.  y: float64"""
    n = len(y)
    a = np.abs(np.asarray(y, dtype=np.float64))
    bm = [float(a[i:i + 64].max()) for i in range(0, n, 64)]
    out = []
    for i0 in range(0, n, SD_CH):
        b0 = max(0, i0 - 2 * hl_max - 2) // 64
        b1 = min(len(bm) - 1, (i0 + SD_CH + hl_max + 4) // 64)
        m, flag = 0.0, False
        for v in bm[b0:b1 + 1]:
            flag |= v < 1e-8 * m
            m = max(m, v)
        out.append(flag)
    return out


def band_rule(y, fs_d, b, L1, floor, ceil, n_fft, mutant=None, quiet=None):
    """one band of the raw table by the rule.  y: the decimated signal after the DC removal (long double).  Returns a dict: hl,
    f, A, counts (intervals per type), value [L1] (the mean of the four before the test, nan for a dead band), raw [L1] (after
    it), unit_fir / unit_sl [L1] (what 1 unit of K is worth, in Hz, for the direct and for the sliding forms), zero_f / zero_d
    (per sample: |f| / (eps A) and the same of the difference signal, for the near-threshold set), grow [n] and Au [n].
    quiet (level-drop tables; quiet_chunks): the sliding side's A at a sample is the largest A since that side's sums were formed
    afresh -- since the start of its chunk, or the sample's own A (and no growth) where the chunk is left to direct sums."""
    n = len(y)
    f, A, hl = bandpass(y, fs_d, b, mutant)
    d = f[1:] - f[:-1]
    Ad = A[1:] + A[:-1]
    pos = np.arange(n)
    grow = np.maximum(1.0, ((pos % SD_CH) + 2 * hl + 1) / math.log2(n_fft))
    Au = A
    if quiet is not None:
        Au = A.copy()
        for c, q in enumerate(quiet):
            seg = slice(c * SD_CH, min((c + 1) * SD_CH, n))
            if q:
                grow[seg] = 1.0
            else:
                Au[seg] = np.maximum.accumulate(A[seg])
    Ud = Au[1:] + Au[:-1]
    zs = [_engine(f, A, Au, grow, n, fs_d, mutant), _engine(-f, A, Au, grow, n, fs_d, mutant), _engine(d, Ad, Ud, grow, n - 1, fs_d, mutant),
          _engine(-d, Ad, Ud, grow, n - 1, fs_d, mutant)]
    counts = [0 if z is None else len(z["itv"]) for z in zs]
    out = dict(hl=hl, f=f, A=A, Au=Au, counts=counts, grow=grow, b=b, zs=zs)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["zero_f"] = np.where(A > 0, np.abs(f).astype(np.float64) / (EPS * A), np.inf)
        out["zero_d"] = np.where(Ad > 0, np.abs(d).astype(np.float64) / (EPS * Ad), np.inf)
    if min(counts) <= 2:
        out.update(value=np.full(L1, np.nan), raw=np.zeros(L1), unit_fir=np.zeros(L1), unit_sl=np.zeros(L1), alive=False)
        return out
    t = (np.arange(L1) * 1 / 1000.0).astype(LD)
    v = np.zeros(L1, dtype=LD)
    uf, us = np.zeros(L1), np.zeros(L1)
    for z in zs:
        vi, a, g = _interp(z, t, fs_d)
        v, uf, us = v + vi, uf + a, us + g
    v = v / 4
    vf = v.astype(np.float64)
    upper, lower = b * 1.1, b * 0.9  # (float64 products, and the comparisons are of doubles: the reference's candidate is one)
    out_of = (vf >= upper) if mutant == "ge_upper" else (vf > upper)
    dead = out_of | (vf < lower) | (vf > ceil) | (vf < floor)
    out.update(value=vf, raw=np.where(dead, 0.0, vf), unit_fir=uf / 4 + EPS * np.abs(vf), unit_sl=us / 4 + EPS * np.abs(vf), alive=True,
               upper=upper, lower=lower)
    return out


def allowed_hz(br, k, sliding):
    """what the device may be off by, in Hz, per frame of a band: 2 K units"""
    return 2.0 * k * (br["unit_sl"] if sliding else br["unit_fir"])


def _weak(s, bound):
    """samples at which an edge might appear or vanish: |s| within its bound (a sum over nothing but zeros is exact and firm),
    unless the neighbours lie firmly on opposite sides -- then there is one crossing whichever way s[i] falls, and its fine
    position is the same to first order"""
    w = (np.abs(s) <= bound) & (bound > 0)
    pos, neg = s > bound, s < -bound
    through = np.zeros(len(s), dtype=bool)
    through[1:-1] = (pos[:-2] & neg[2:]) | (neg[:-2] & pos[2:])
    return np.flatnonzero(w & ~through)


def near_threshold(br, k, sliding, floor, ceil, fs_d, wide=False):
    """frames of a band that are not compared for their zero pattern (module docstring).  wide: a sample is weak where |f| is
    below the allowed error of the LARGEST sum of the utterance -- the unit of an FFT convolution, whose roundings are those of
    the whole utterance wherever they land"""
    L1 = len(br["raw"])
    near = np.zeros(L1, dtype=bool)
    g = br["grow"] if sliding else np.ones(len(br["grow"]))
    A = br["Au"] if sliding else br["A"]
    f = br["f"].astype(np.float64)
    d = (br["f"][1:] - br["f"][:-1]).astype(np.float64)
    if wide:
        top = 2.0 * k * EPS * float(br["A"].max())
        weak = np.union1d(_weak(f, np.full(len(f), top)), _weak(d, np.full(len(d), 2 * top)))
    else:
        Ad = A[1:] + A[:-1]
        weak = np.union1d(_weak(f, 2.0 * k * g * EPS * A), _weak(d, 2.0 * k * g[:-1] * EPS * Ad))
    if len(weak):
        t = np.arange(L1) / 1000.0
        span = 2.0 / br["b"]
        ts = weak / fs_d
        lo, hi = np.searchsorted(ts, t - span), np.searchsorted(ts, t + span, side="right")
        near |= hi > lo
    if br["alive"]:  # a frame one of the four comparisons rejects beyond doubt is zero whatever the others say
        a, v = allowed_hz(br, k, sliding), br["value"]
        dead = (v - a > br["upper"]) | (v + a < br["lower"]) | (v - a > ceil) | (v + a < floor)
        unsure = np.zeros(L1, dtype=bool)
        for thr in (br["upper"], br["lower"], floor, ceil):
            unsure |= np.abs(v - thr) <= a
        near |= unsure & ~dead
    return near


# ------------------------------------------------------------------------------------------------------------------------
# detection over bands
# ------------------------------------------------------------------------------------------------------------------------
def detect_rule(raw, S, mutant=None):
    """raw [n_bands][L1] float64 -> (cand0 [L1][S], run lengths per frame as lists of (st, ed))"""
    nb, L1 = raw.shape
    need = 9 if mutant == "run9" else 10
    cand = np.zeros((L1, S))
    runs = []
    for i in range(L1):
        vuv = (raw[:, i] > 0).astype(int)
        vuv[0] = vuv[nb - 1] = 0
        d = np.diff(vuv)
        st, ed = np.flatnonzero(d == 1) + 1, np.flatnonzero(d == -1) + 1
        nc = 0
        rr = []
        for a, b in zip(st, ed):
            rr.append((int(a), int(b)))
            if b - a < need or nc >= S:
                continue
            t = 0.0
            for j in range(a, b):
                t += float(raw[j, i])
            cand[i, nc] = t / (b - a)
            nc += 1
        runs.append(rr)
    return cand, runs


# ------------------------------------------------------------------------------------------------------------------------
# tables
# ------------------------------------------------------------------------------------------------------------------------
class Table:
    """signals, handle options, the bands the rule is evaluated on (None: all) and notes on what the table reaches"""

    def __init__(self, name, fs, floor=71.0, ceil=800.0, cio=40.0, target_fs=8000.0, stage="raw", bands=None, with_ref=True, stationary=True):
        self.name, self.fs, self.floor, self.ceil, self.cio, self.target_fs = name, fs, floor, ceil, cio, target_fs
        self.stage, self.with_ref = stage, with_ref and cio == 40.0 and target_fs == 8000.0
        self.stationary = stationary
        self.r = max(min(mround(fs / target_fs), 12), 1)
        self.fs_d = fs / self.r
        self.b = band_list(floor, ceil, cio)
        self.S = slots(len(self.b))
        self.bands = list(range(len(self.b))) if bands is None else bands
        self.xs, self.notes = [], {}
        assert half_len(self.fs_d, self.b[0]) <= 1024

    def options(self):
        return dict(f0_floor=self.floor, f0_ceil=self.ceil, target_fs=float(self.target_fs), channels_in_octave=self.cio)

    def add(self, x):
        self.xs.append(np.asarray(x, dtype=np.float64))
        u = len(self.xs) - 1
        # the reference writes its 2 hl + 1 taps into a buffer of its FFT size, which it sizes by the signal: on a signal too short
        # for its lowest band it overruns the buffer.  Every table stays where the reference is defined.
        assert self.L1(u) >= 3 and self.n_fft(u) >= 2 * half_len(self.fs_d, self.b[0]) + 1, (self.name, u, len(x))
        return u

    def y_len(self, u):
        return 1 + len(self.xs[u]) // self.r

    def L1(self, u):
        return frames_1ms(len(self.xs[u]), self.fs)

    def n_fft(self, u):
        return fft_size(self.y_len(u), self.fs_d, self.b[0])


def tones(fs, n, parts, seed=0, noise=0.0):
    """sum of a sin(2 pi f t + ph) over parts (f, a, ph) plus a noise floor"""
    t = np.arange(n) / fs
    x = np.zeros(n)
    for f, a, ph in parts:
        x += a * np.sin(2 * np.pi * f * t + ph)
    if noise:
        x += noise * np.random.default_rng(seed).normal(size=n)
    return x


def _ratio(name):
    r = int(name.split("_")[1])
    fs = 8000 * r  # round(fs / 8000) = r with the stock target_fs: the real reference can run it
    if r in (5, 9):  # the same ratio reached through target_fs as well
        t = Table(name, 48000, target_fs=48000.0 / r, stage="y")
        fs = 48000
    else:
        t = Table(name, fs, stage="y")
    assert t.r == r
    n = int(0.1 * fs) + r + 1  # (not a multiple of r)
    t.add(tones(fs, n, [(183.0, 0.45, 0.3), (2710.0, 0.3, 1.1)], seed=r, noise=1e-3))
    return t


def _dec_edges(name):
    t = Table(name, 16000, stage="y")
    r = t.r
    assert r == 2
    lag = int(math.ceil(140.0 / r) * r)
    rng = np.random.default_rng(5)

    def sig(n):
        return 0.6 * np.sin(2 * np.pi * 211.0 * np.arange(n) / 16000 + 0.2) + 0.05 * rng.normal(size=n)
    # (32 samples are the shortest a handle takes at 16 kHz: three 1 ms frames; dec_short goes below)
    lens = [32, 33, lag - 1, lag, lag + 1, 2 * 30, 2 * 31, 2 * 32 + 1, 2 * (DS_SPAN - 2), 2 * (DS_SPAN - 1) + 1, 2 * DS_SPAN]
    for n in lens:
        t.add(sig(n))
    t.notes["y_lens"] = [t.y_len(u) for u in range(len(t.xs))]
    return t


def _dec_short(name):
    """inputs of 8, 9 and 10 samples -- at and around decimate's nine reflected samples, far below the padding -- at 4 kHz, where
    they are three frames long (the shortest signal a handle takes)"""
    t = Table(name, 4000, 71.0, 400.0, target_fs=2000.0, stage="y")
    rng = np.random.default_rng(9)
    for n in (8, 9, 10):
        t.add(0.5 * rng.uniform(-1, 1, size=n))
    return t


def _dc(name):
    t = Table(name, 8000, 100.0, 400.0, stage="raw", with_ref=False)  # (the real reference corrupts its heap on DC offsets)
    n = 1600
    tt = np.arange(n) / 8000.0
    base = np.sin(2 * np.pi * 200.0 * tt + 0.1)
    k = int(np.argmax(base))
    a = 0.999 * base / base[k]
    a[k] = 1.0                                   # a peak of exactly 1: the branch is taken
    b = a.copy()
    b[k] = float(np.nextafter(1.0, 0.0))         # the next double below: it is not
    t.add(a)
    t.add(b)
    t.add(2.5 + 0.4 * np.sin(2 * np.pi * 180.0 * tt))
    t.add(-2.5 + 0.4 * np.sin(2 * np.pi * 180.0 * tt))
    # halves 0.6 apart: every addition truncates, the int sum stays far from the sum of the doubles
    t.add(0.6 + 0.59 * np.sin(2 * np.pi * 220.0 * tt) + 0.45 * (np.arange(n) % 7 == 0))
    t.add(-0.6 + 0.59 * np.sin(2 * np.pi * 220.0 * tt) - 0.45 * (np.arange(n) % 7 == 0))
    return t


def tone_with_edge_at(fs, n, f, where, kind, amp=0.5):
    """a sinusoid of f Hz whose `kind` event (0 negative-going crossing, 1 positive-going, 2 peak, 3 dip) of the band-passed signal
    falls at sample position `where` (fractional: between where's floor and ceiling): the band-pass is zero-phase and one sample
    late, the difference signal half a sample early"""
    # band-passed f[i] ~ g x(i + 1): a crossing of f at position p is a crossing of x at p + 1; an extremum of f shows in the
    # difference f[i+1] - f[i] half a sample early
    phase_at = {0: np.pi, 1: 0.0, 2: np.pi / 2, 3: 3 * np.pi / 2}[kind]
    p = where + 1.0 + (0.5 if kind >= 2 else 0.0)
    ph = phase_at - 2 * np.pi * f * p / fs
    return amp * np.sin(2 * np.pi * f * np.arange(n) / fs + ph)


def near_bands(t, freqs, width=1):
    """for every frequency the band nearest to it and `width` neighbours on either side"""
    out = set()
    for f in freqs:
        j = int(np.argmin(np.abs(np.log(np.asarray(t.b) / f))))
        out.update(range(max(0, j - width), min(len(t.b), j + width + 1)))
    return sorted(out)


def _seam(name):
    fir = name.endswith("_fir")
    t = Table(name, 8000, 120.0, 330.0)
    freqs = (150.0, 233.0)
    t.bands = near_bands(t, freqs)
    adv = FIR_ADV if fir else SD_CH
    t.notes.update(fir=fir, adv=adv)
    placed = []
    k = 0
    for f in freqs:
        for kind in range(4):
            for border in (adv, 2 * adv):
                for off in (-1.5, -0.5, 0.5):  # between border-2|border-1, border-1|border, border|border+1
                    y_len = (2 * adv - 1, 2 * adv, 2 * adv + 1, adv + 500)[k % 4] if border == adv else 2 * adv + 300 + k % 3
                    t.add(tone_with_edge_at(8000, y_len - 1, f, border + off, kind))
                    placed.append((len(t.xs) - 1, f, kind, border, off))
                    k += 1
    for y_len in (adv - 1, adv, adv + 1):  # utterances that end on the first border
        t.add(tone_with_edge_at(8000, y_len - 1, 150.0, adv - 8.5, 0))
    t.notes["placed"] = placed
    return t


def _late(name):
    t = Table(name, 8000, 120.0, 330.0)
    t.bands = near_bands(t, (140.0, 260.0))
    placed = []
    for f in (140.0, 260.0):
        for pos in list(range(2040, 2048)) + list(range(2048, 2056)):
            t.add(tone_with_edge_at(8000, 2600, f, pos - 0.5, 0))
            placed.append((len(t.xs) - 1, f, pos))
    t.notes["placed"] = placed
    return t


def _few(name):
    t = Table(name, 8000, 160.0, 640.0)
    # bare tones of a few cycles of 320 Hz (25 samples a cycle), nothing around them: the edge counts of the four types differ by
    # one, so that bands with exactly two intervals of some type (zeros) stand beside bands with three of every type (alive)
    for cycles in (1.0, 3.5, 4.0, 4.25, 4.5, 4.75, 5.0, 5.5):
        m = int(round(cycles * 25))
        t.add(0.5 * np.sin(2 * np.pi * 320.0 * np.arange(m) / 8000.0 + 0.3))
    t.add(0.5 * np.sin(2 * np.pi * 200.0 * np.arange(120) / 8000.0))  # shorter than the lowest band's window (2 hl + 1 = 219)
    return t


def _burst(name):
    """a burst of a tone, then exact zeros to the end: behind the burst every band's output reaches exactly 0 (a direct sum over
    zeros), which the detector's `<= 0` meets.  The reference's FFT convolution leaves 1e-17 there instead, so the restatement is
    compared on this table only where it is firm under its own, utterance-wide unit (SCOPE_WIDE)."""
    t = Table(name, 8000, 100.0, 400.0, stationary=False)
    for cycles, ph in ((8.0, 0.3), (8.25, 0.3), (8.5, 0.3), (8.75, 0.3), (8.0, 1.9), (8.5, 1.9)):
        x = np.zeros(1400)
        m = int(round(cycles * 40))
        x[:m] = 0.5 * np.sin(2 * np.pi * 200.0 * np.arange(m) / 8000.0 + ph)
        t.add(x)
    return t


LEVELS = (1e-6, 2e-8, 0.5e-8, 1e-10)
LEVEL_FALL, LEVEL_ZEROS = 1000, 2400
LEVEL_FRAMES = slice(150, 240)  # 1 ms frames that read the quiet stretch of the first chunk alone


def _level(name):
    """a 200 Hz tone of 0.9 that falls at sample LEVEL_FALL -- inside the first chunk and inside every band's window -- to c times
    its level, c on either side of the quiet-chunk threshold 1e-8, and to exact zeros at LEVEL_ZEROS, far enough behind the first
    chunk's lookahead that the first chunk is quiet by the fall alone.  The second chunk sees the zeros and is always quiet."""
    t = Table(name, 8000, 100.0, 400.0, stationary=False)
    t.bands = near_bands(t, (200.0,))
    t.notes["level"] = True
    base = 0.9 * np.sin(2 * np.pi * 200.0 * np.arange(3000) / 8000.0 + 0.3)
    for c in LEVELS:
        x = base.copy()
        x[LEVEL_FALL:] *= c
        x[LEVEL_ZEROS:] = 0.0
        t.add(x)
    return t


BAND_TEST_FRAME = 60


def _band_test(name):
    """tones placed by the rule itself.  A sampled sinusoid's raw candidate is not its frequency (the crossings are interpolated
    linearly), so the tone whose candidate at frame BAND_TEST_FRAME of band j sits on 1.1 b or 0.9 b is found by bisection over
    the doubles: the last frequency whose rule value is at or below the product and the next double above it."""
    t = Table(name, 8000, 100.0, 400.0)
    j = 40
    b = t.b[j]
    t.notes["band"] = j
    n = 960

    def value(f):
        y = np.append(tones(8000, n, [(f, 0.5, 0.4)]), 0.0).astype(LD)
        return band_rule(y, 8000.0, b, frames_1ms(n, 8000), t.floor, t.ceil, fft_size(n + 1, 8000.0, t.b[0]))["value"][BAND_TEST_FRAME]
    close, firm = [], []
    for thr in (b * 1.1, b * 0.9):
        lo, hi = thr * 0.99, thr * 1.01
        assert value(lo) < thr < value(hi)
        while np.nextafter(lo, np.inf) < hi:
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if value(mid) < thr else (lo, mid)
        close += [lo, hi]                     # within a double of the product: in the near-threshold set on purpose
        if thr == b * 1.1:                    # a tone whose candidate, rounded to a double, IS the product: `>` keeps it, `>=` would not
            near = [hi]
            for _ in range(31):  # (the candidate moves by about a double per double of the tone: one of these lands on it)
                near.append(float(np.nextafter(near[-1], np.inf)))
            eq = [f for f in near if value(f) == thr]
            t.notes["equal"] = len(close) - 1 if eq and eq[0] == hi else None
            if eq and eq[0] != hi:
                close.append(eq[0])
                t.notes["equal"] = len(close) - 1
        firm += [lo * (1.0 + 1e-6), lo * (1.0 - 1e-6)]
    for thr in (100.0, 400.0):
        firm += [thr * (1.0 + 1e-6), thr * (1.0 - 1e-6)]
    t.notes.update(close=close, firm=firm)
    for f in close:
        t.add(tones(8000, n, [(f, 0.5, 0.4)]))
    for f in firm:
        t.add(tones(8000, 2400, [(f, 0.5, 0.4)]))
    t.add(tones(8000, 480, [(100.0, 0.5, 0.2)]))  # at floor: 80 samples a period, every interval is the floor to a rounding
    t.add(tones(8000, 480, [(400.0, 0.5, 0.2)]))  # at ceil
    return t


def lit_bands(t, f):
    """bands b with 0.9 b <= f <= 1.1 b (the products in float64, as the reference forms them) -- where a pure tone's raw
    candidate survives the band test"""
    return [j for j, b in enumerate(t.b) if b * 0.9 <= f <= b * 1.1]


def _runs(name):
    cio = float(name.split("_")[1])
    t = Table(name, 8000, 71.0, 800.0, cio=cio)
    nb = len(t.b)
    want = {33.0: (9, 10), 36.0: (10, 11)}[cio]
    found = {}
    f = 150.0
    while len(found) < 2:  # a tone whose lit bands number `want`, 1e-3 clear of either neighbour band's threshold
        lit = lit_bands(t, f)
        if len(lit) in want and len(lit) not in found and len(lit_bands(t, f * 1.001)) == len(lit) == len(lit_bands(t, f * 0.999)):
            found[len(lit)] = f
        f += 0.25
    t.notes["counted"] = found
    for n_lit in want:
        t.add(tones(8000, 1600, [(found[n_lit], 0.5, 0.3)]))
    lo = 0.5 * (71.0 + 1.1 * t.b[0])          # lights band 0: the run starts at band 1 and is one shorter
    hi = 0.5 * (800.0 + 0.9 * t.b[nb - 1])    # lights the last band (at 36 bands an octave 0.9 b of the last band is above the ceiling)
    assert 0 in lit_bands(t, lo) and (cio == 36.0 or nb - 1 in lit_bands(t, hi))
    t.add(tones(8000, 1600, [(lo, 0.5, 0.3)]))
    t.add(tones(8000, 1600, [(hi if cio == 33.0 else 0.999 * 800.0, 0.5, 0.3)]))
    f2 = 4.5 * found[want[1]]
    while not (len(lit_bands(t, f2)) >= 10 and len(lit_bands(t, f2 * 1.001)) == len(lit_bands(t, f2)) == len(lit_bands(t, f2 * 0.999))):
        f2 += 0.25
    # two runs of at least 10 in every frame.  A band's main lobe is as wide as the band is high, so the upper bands see the lower
    # tone 40 dB down and no further: it is written 42 dB below the upper one, which then wobbles by less than its margin
    t.add(tones(8000, 1600, [(found[want[1]], 0.004, 0.3), (f2, 0.5, 1.0)]))
    t.notes.update(lo=lo, hi=hi)
    return t


BUILDERS = {}
for _r in range(2, 13):
    BUILDERS["ratio_%d" % _r] = _ratio
BUILDERS.update(dec_edges=_dec_edges, dec_short=_dec_short, burst=_burst, dc=_dc, seam=_seam, seam_fir=_seam, late_in_chunk=_late, few_edges=_few, band_test=_band_test, level_drop=_level,
                runs_33=_runs, runs_36=_runs)
NAMES = sorted(BUILDERS)
Y_TABLES = [n for n in NAMES if n.startswith("ratio_") or n.startswith("dec_")]
RAW_TABLES = [n for n in NAMES if n not in Y_TABLES]
LEVEL_TABLES = ["level_drop"]
PLAIN_RAW_TABLES = [n for n in RAW_TABLES if n not in LEVEL_TABLES]  # held frame by frame to the stationary bound alone
_tables, _rules, _ports = {}, {}, {}


def table(name):
    if name not in _tables:
        _tables[name] = BUILDERS[name](name)
    return _tables[name]


def rule(name, mutant=None):
    """per utterance a dict: y0 (before the DC removal), u_y, acc, y (long double), and for raw tables `bands`: {band index:
    band_rule}.  Computed once per (table, mutant)."""
    key = (name, mutant)
    if key in _rules:
        return _rules[key]
    t = table(name)
    out = []
    for u, x in enumerate(t.xs):
        c = None
        if mutant == "coef12":  # a0 of the ratio changed in its 12th significant digit
            c = list(COEF[t.r])
            c[0] = c[0] * (1.0 + 1e-11)
        y0, uy = decimate_rule(x, t.r, c)
        y, acc = dc_rule(y0, mutant)
        if acc != 0:  # the subtraction rounds once more: eps |y - mean| on top of the decimator's unit
            uy = uy + EPS * np.abs(y).astype(np.float64)
        r = dict(y0=y0, u_y=uy, acc=acc, y=y)
        if t.stage == "raw":
            quiet = quiet_chunks(y.astype(np.float64), half_len(t.fs_d, t.b[0])) if t.notes.get("level") else None
            r["quiet"] = quiet
            r["bands"] = {j: band_rule(y, t.fs_d, t.b[j], t.L1(u), t.floor, t.ceil, t.n_fft(u), mutant, quiet) for j in t.bands}
        out.append(r)
    _rules[key] = out
    return out


def rule_raw(t, r):
    """the rule's raw table [n_bands][L1] of one utterance (float64)"""
    return np.stack([r["bands"][j]["raw"] for j in range(len(t.b))])


def restatement(port, name):
    """oracle/port.harvest_debug on a table: per utterance dict(y, raw); computed once"""
    if name not in _ports:
        t = table(name)
        port.set_harvest_options(float(t.target_fs), t.cio, False)
        try:
            _ports[name] = [port.harvest_debug(x, t.fs, f0_floor=t.floor, f0_ceil=t.ceil) for x in t.xs]
        finally:
            port.set_harvest_options()
    return _ports[name]


def y_errors(r, y):
    """|y - rule| in units u_y, per sample (0 where the unit is 0: decimation 1 must be exact)"""
    d = np.abs(np.asarray(y, dtype=LD) - r["y"]).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(r["u_y"] > 0, d / r["u_y"], np.where(d == 0, 0.0, np.inf))


def raw_errors(br, row, sliding):
    """|raw - rule| of one band in units, on the frames where both are non-zero"""
    both = (row != 0) & (br["raw"] != 0)
    e = np.zeros(len(row))
    unit = br["unit_sl"] if sliding else br["unit_fir"]
    e[both] = np.abs(row[both] - br["raw"][both]) / unit[both]
    return e


def same_zero_pattern(t, u, r, raw, k, sliding, wide=False):
    """outside the near-threshold set a raw table is zero exactly where the rule's is; returns (near, live) counts"""
    near_n = live_n = 0
    for j in t.bands:
        br = r["bands"][j]
        near = near_threshold(br, k, sliding, t.floor, t.ceil, t.fs_d, wide)
        if br["alive"]:
            live_n += len(near)
            near_n += int(near.sum())
        bad = np.flatnonzero(~near & ((raw[j] != 0) != (br["raw"] != 0)))
        assert len(bad) == 0, (t.name, u, "band", j, "zero pattern differs at frames", bad[:8].tolist())
    return near_n, live_n


_k_ref = {}


def k_ref(port):
    """{"y": .., "raw": .., "y_r": {ratio: ..}}: the restatement's largest error against the rule in units, over all stationary
    tables; y_r: the same over the tables of one decimation ratio (the float64 recursion's error grows with the ratio: a device
    is held to the figure of the ratio it runs)"""
    if not _k_ref:
        ky = kr = 0.0
        kyr = {}
        for name in NAMES:
            t = table(name)
            if not t.stationary:
                continue
            for r, d in zip(rule(name), restatement(port, name)):
                e = float(y_errors(r, d["y"]).max())
                ky, kyr[t.r] = max(ky, e), max(kyr.get(t.r, 0.0), e)
                if t.stage == "raw":
                    for j in t.bands:
                        kr = max(kr, float(raw_errors(r["bands"][j], d["raw"][j], False).max()))
        _k_ref.update(y=ky, raw=kr, y_r=kyr)
    return _k_ref
