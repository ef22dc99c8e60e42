"""Harvest's refinement (overlapF0Candidates + refineF0Candidates, reference src/harvest.cpp:750-1000) on candidates written by
hand: a high-precision rule of the operation and the tables it is checked on.  numpy only; everything is deterministic.

The rule.  A raw candidate f refined at frame i (pos = i ms) is cut into integers first -- the half window length hw, the
transform size N, the first sample `basic`, the harmonic count nh, the six bins and, with use_cos_table, the table indices of
every window sample.  Those are evaluated in float64 with the reference's own expressions in the reference's order: they are part
of the definition.  Everything behind them -- the Blackman window, its difference, the DFT sums taken directly at the bins, the
instantaneous frequencies, the three sums over harmonics and the two quotients -- is evaluated in np.longdouble.

The unit.  One rounding in the instantaneous frequency ni / pw * fs / 2 pi of harmonic h is worth, to first order,
eps (fs / 2 pi) (sum |mw y|) (sum |dw y|) / pw_h, and one rounding of the result eps f:
    u(c) = eps (fs / 2 pi) max_h [(sum |mw y|) (sum |dw y|) / pw_h] + eps f,
computed by the rule from its own sums.  Errors of the refined F0 are counted in u, errors of 1 / score in u / f.  K_ref is the
largest error of the CPU oracle (a radix-2 FFT of log2 N stages) in these units over all tables, measured where it is used
(k_ref below; tests/test_harvest_refine_rule.py prints it); a device that advances window and twiddles by rotation recurrences over q = ceil((2 hw + 1) / 8)
steps per lane is allowed 2 K_ref max(1, q / log2 N) units.

The tables.  Each is (signals, handle options, raw candidate rows).  All handles run at decimation 1 (target_fs = fs) on signals
below 1 in magnitude, so the decimated signal is the signal itself with one zero appended (the reference's integer-typed DC
accumulator stays 0) and stretches of exact zeros survive.  tests/test_harvest_refine_rule.py proves on the CPU that every table
reaches what it is named for; tests/test_gpu_harvest_refine.py then compares the device with the oracle and the rule on them.
"""
import math
from fractions import Fraction

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "the rule needs a long double wider than float64"
K_PI = 3.1415926535897932384   # the reference's world::kPi as a double
LOG2 = 0.69314718055994529     # world::kLog2
SAFE = 0.000000000001          # world_common's safe-guard minimum
PI_L = LD(4) * np.arctan(LD(1))
EPS = float(np.finfo(np.float64).eps)
PAD = 2048                     # samples kept on either side of an utterance for the mutants that read past its ends

MUTANTS = ("hw+1", "bin+1", "nh-1", "basic+1", "noclamp", "neighbour", "overlap_swapped", "fused_bin")


def mround(x):
    return int(x + 0.5) if x > 0 else int(x - 0.5)


def up(v):
    return float(np.nextafter(v, np.inf))


def down(v):
    return float(np.nextafter(v, -np.inf))


def frames_1ms(n, fs):
    return int(1000.0 * n / fs) + 1


def slots(floor, ceil, cio):
    """candidate slots per frame before the overlap (reference :1388-1397, :1418-1419)"""
    adj_floor, adj_ceil = floor * 0.9, ceil * 1.1
    n_bands = 1 + int(math.log(adj_ceil / adj_floor) / LOG2 * cio)
    return mround(n_bands // 10)


def lowest_floor(fs, cio=40.0):
    """the lowest multiple of 0.1 Hz whose first band-pass is within the supported half length of 1024 samples"""
    f = 10.0
    while mround(fs / (f * 0.9 * math.pow(2.0, 1.0 / cio)) * 2.0) > 1024:
        f = round(f + 0.1, 1)
    return f


def block_source(i, b):
    """frame whose slots block b of frame i's row holds (reference :987-1000)"""
    return i if b == 0 else (i - b if b <= 3 else i + (b - 3))


# ------------------------------------------------------------------------------------------------------------------------
# the integer decisions, float64, the reference's expressions in the reference's order
# ------------------------------------------------------------------------------------------------------------------------
def decisions(fs, i, f, mutant=None):
    pos = i * 1 / 1000.0
    hw = int(1.5 * fs / f + 1.0)
    if mutant == "hw+1":
        hw += 1
    bt = hw * 2 + 1
    fft_index = 2 + int(math.log(hw * 2 + 1.0) / LOG2)
    N = int(math.pow(2.0, fft_index))
    bt0 = (-hw) / fs
    basic = mround((pos + bt0) * fs + 0.001)
    if mutant == "basic+1":
        basic += 1
    nh = min(int(fs / 2.0 / f), 6)
    if mutant == "nh-1":
        nh = max(nh - 1, 1)
    if mutant == "fused_bin":  # bin_unit * (h + 1) + 0.5 rounded once
        unit = Fraction(f * N / fs)
        bins = [int(float(unit * (h + 1) + Fraction(1, 2))) for h in range(nh)]
    else:
        bins = [mround(f * N / fs * (h + 1)) for h in range(nh)]
    if mutant == "bin+1":
        bins[0] += 1
    return dict(pos=pos, hw=hw, bt=bt, N=N, basic=basic, nh=nh, bins=bins)


_cos_table = []


def cos_table():
    """reference :152-170, built in float64 as the reference builds it"""
    if not _cos_table:
        n = 2000
        t = np.zeros(4 * n + 1)
        interval = K_PI / 2. / n
        for i in range(n + 1):
            t[i] = math.cos(interval * i)
        for i in range(n):
            t[i + n + 1] = -t[n - 1 - i]
        for i in range(n):
            t[i + n * 2 + 1] = -t[i + 1]
        for i in range(n):
            t[i + n * 3 + 1] = t[n - 1 - i]
        _cos_table.append(t)
    return _cos_table[0]


def table_indices(fs, d):
    """the two table indices of every window sample (reference :779-787): float64"""
    n = np.arange(d["bt"], dtype=np.float64)
    wlt = (2.0 * d["hw"] + 1.0) / fs
    two_pi = 2.0 * K_PI
    tmp = (d["basic"] + n - 1.0) / fs - d["pos"]
    tmp2 = two_pi * (tmp / wlt + 1)
    dindex = np.fmod(tmp2, two_pi) / two_pi * 8000
    dindex2 = np.fmod(dindex * 2, 8000.0)

    def c_round(x):  # std::round on non-negative values
        t = np.trunc(x)
        return (t + (x - t >= 0.5)).astype(np.int64)
    return c_round(dindex), c_round(dindex2)


_twiddles = {}


def twiddles(N):
    if N not in _twiddles:
        ang = 2 * PI_L * np.arange(N, dtype=LD) / LD(N)
        _twiddles[N] = (np.cos(ang), np.sin(ang))
    return _twiddles[N]


# ------------------------------------------------------------------------------------------------------------------------
# one candidate
# ------------------------------------------------------------------------------------------------------------------------
def refine_one(ybuf, y_len, fs, i, f, table=False, mutant=None):
    """ybuf: PAD samples, the utterance's y_len samples, PAD samples.  Returns the decisions plus rf, inv (= 1 / score), the unit u,
    the clamps met and `zero` (a harmonic of exactly no power)."""
    d = decisions(fs, i, f, mutant)
    hw, bt, N, basic, nh = d["hw"], d["bt"], d["N"], d["basic"], d["nh"]
    n = np.arange(bt)
    src = basic + n - 1
    d["clamp_lo"], d["clamp_hi"] = bool(src[0] < 0), bool(src[-1] > y_len - 1)
    if mutant in ("noclamp", "neighbour"):
        ys = ybuf[np.clip(src, -PAD, y_len - 1 + PAD) + PAD]
    else:
        ys = ybuf[np.clip(src, 0, y_len - 1) + PAD]
    fs_l = LD(fs)
    if table:
        i1, i2 = table_indices(fs, d)
        tab = cos_table().astype(LD)
        mw = LD(0.42) + LD(0.5) * tab[i1] + LD(0.08) * tab[i2]
    else:
        tmp = (LD(basic) + n.astype(LD) - 1) / fs_l - LD(d["pos"])
        th = 2 * PI_L * tmp / ((2 * LD(hw) + 1) / fs_l)
        mw = LD(0.42) + LD(0.5) * np.cos(th) + LD(0.08) * np.cos(2 * th)
    dw = np.empty(bt, dtype=LD)
    dw[0] = -mw[1] / 2
    dw[-1] = mw[-2] / 2
    dw[1:-1] = -(mw[2:] - mw[:-2]) / 2
    a, b = mw * ys, dw * ys
    A, B = np.abs(a).sum(), np.abs(b).sum()
    tc, ts = twiddles(N)
    num = den = sc = LD(0)
    worst = LD(0)
    zero = False
    for h in range(nh):
        k = d["bins"][h]
        ph = (k * n) % N
        c, s = tc[ph], ts[ph]
        mr, mi, dr, di = (a * c).sum(), -(a * s).sum(), (b * c).sum(), -(b * s).sum()  # the conjugate of the e^{+i} transform (:831, :840)
        pw = mr * mr + mi * mi
        ni = mr * di - mi * dr
        if pw == 0:
            inst = LD(0)
            zero = True
        else:
            inst = LD(k) * fs_l / N + ni / pw * fs_l / 2 / PI_L
            worst = max(worst, A * B / pw)
        amp = np.sqrt(pw)
        num += amp * inst
        den += amp * (h + 1)
        sc += abs((inst / (h + 1) - LD(f)) / LD(f))
    d["rf"] = float(num / (den + LD(SAFE)))
    d["inv"] = float(sc / nh + LD(SAFE))
    d["unit"] = float(LD(EPS) * fs_l / (2 * PI_L) * worst + LD(EPS) * LD(f))
    d["zero"] = zero
    return d


# ------------------------------------------------------------------------------------------------------------------------
# tables
# ------------------------------------------------------------------------------------------------------------------------
class Table:
    def __init__(self, name, fs, floor, ceil, cio=40.0, cos=False):
        self.name, self.fs, self.floor, self.ceil, self.cio, self.cos = name, fs, floor, ceil, cio, cos
        self.S = slots(floor, ceil, cio)
        self.xs, self.cand0, self.f_true = [], [], []
        self.notes = {}
        self.rng = np.random.default_rng(sum(ord(c) for c in name.replace("_cos", "")))

    def options(self):
        """keyword arguments of world_class_amd.Harvest"""
        return dict(f0_floor=self.floor, f0_ceil=self.ceil, target_fs=float(self.fs), channels_in_octave=self.cio, use_cos_table=self.cos)

    def add(self, x, f_true=None):
        x = np.asarray(x, dtype=np.float64)
        assert np.abs(x).max() < 1.0  # the reference's integer DC accumulator stays at 0: y is x itself
        L1 = frames_1ms(len(x), self.fs)
        self.xs.append(x)
        self.cand0.append(np.zeros((L1, self.S)))
        self.f_true.append(f_true)
        return len(self.xs) - 1

    def L1(self, u):
        return len(self.cand0[u])

    def put(self, u, i, j, f):
        assert self.floor <= f <= self.ceil and self.cand0[u][i, j] == 0.0, (self.name, u, i, j, f)
        self.cand0[u][i, j] = f

    def near(self, u, i, j, spread=0.02):
        """a candidate within 2 % of the true F0 at frame i"""
        f = float(self.f_true[u][i]) * (1.0 + self.rng.uniform(-spread, spread))
        self.put(u, i, j, min(max(f, self.floor), self.ceil))

    def anywhere(self, u, i, j):
        self.put(u, i, j, float(math.exp(self.rng.uniform(math.log(self.floor), math.log(self.ceil)))))

    def y(self, u):
        """the decimated signal at decimation 1: the signal and one zero (reference :217-219, y_length = x_length + 1)"""
        return np.append(self.xs[u], 0.0)

    def rows(self):
        """the batch's raw candidate rows, utterance after utterance"""
        return np.concatenate(self.cand0)


def voice(fs, n, f_a, f_b, seed, noise=1e-3, level=0.5, flat=False):
    """harmonics of an F0 gliding from f_a to f_b over n samples (1 / k amplitudes, all of them below 0.45 fs) plus a noise floor;
    returns the signal and the true F0 at every 1 ms frame"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    f = f_a * (f_b / f_a) ** (t / t[-1])
    phase = 2 * np.pi * np.cumsum(f) / fs
    x = np.zeros(n)
    k = 1
    while k * max(f_a, f_b) < 0.45 * fs and k <= 60:
        x += (1.0 if flat else 1.0 / k) * np.sin(k * phase + rng.uniform(0, 2 * np.pi))
        k += 1
    x = level * x / np.abs(x).max() + noise * rng.normal(size=n)
    L1 = frames_1ms(n, fs)
    at = np.minimum(np.round(np.arange(L1) * fs / 1000.0).astype(int), n - 1)
    return x, f[at]


def _cut_triples(t, u, frame, fc):
    """fc, the next double above and the next below, in the first free slots of `frame`"""
    for v in (fc, up(fc), down(fc)):
        if t.floor <= v <= t.ceil:
            j = int(np.argmax(t.cand0[u][frame] == 0.0))
            t.put(u, frame, j, v)
            t.notes.setdefault("cut_candidates", []).append((u, frame, j))


def _half_bin_frequencies(fs, f_near, h):
    """a frequency near f_near whose bin of harmonic h is a half-integer (exactly where (h + 1) divides into the rate's factors)"""
    for shift in (1.0, 1.01, 0.99, 1.02, 0.98):  # (a span that holds a cut of N: stay on one side of it)
        d = decisions(fs, 0, f_near * shift)
        m = int(f_near * shift * d["N"] / fs * (h + 1))
        f = (m + 0.5) * fs / (d["N"] * (h + 1))
        if decisions(fs, 0, f)["N"] == d["N"]:
            return f
    raise AssertionError("no half-integer bin near %g" % f_near)


def _cuts(name, cos):
    low = "low" in name
    fs = 8000
    t = Table(name, fs, 17.5, 260.0) if low else Table(name, fs, 71.0, 1400.0)
    # hw cuts where 2 hw + 1 crosses a power of two (N doubles): 1.5 fs / f + 1 = 2^k, and hw cuts that are exact in float64
    hw_cuts = [1.5 * fs / (2 ** k - 1) for k in range(4, 10)] + [100.0, 800.0, 125.0, 250.0]
    nh_cuts = [fs / (2.0 * k) for k in range(3, 7)]
    spans = [(22.5, 24.5), (46.0, 48.0), (93.0, 102.0), (186.0, 195.0)] if low else \
            [(93.0, 102.0), (186.0, 195.0), (380.0, 394.0), (655.0, 680.0), (785.0, 815.0), (985.0, 1015.0), (1315.0, 1350.0), (120.0, 130.0), (245.0, 255.0)]
    for k, (fa, fb) in enumerate(spans):
        n = 2400 if fa < 60 else 800
        x, ft = voice(fs, n, fa, fb, 100 + k)
        u = t.add(x, ft)
        L1, mid = t.L1(u), t.L1(u) // 2
        for fc in hw_cuts + nh_cuts:
            if fa <= fc <= fb:
                fr = int(np.argmin(np.abs(ft[L1 // 4: 3 * L1 // 4] - fc))) + L1 // 4
                _cut_triples(t, u, fr, fc)
        if 93.0 <= fa and fb <= 1015.0:
            for h in range(6):
                if (h + 1) * fb < fs / 2:
                    _cut_triples(t, u, mid + 5 + h, _half_bin_frequencies(fs, 0.5 * (fa + fb), h))
        for i in range(mid - 8, mid - 2):
            t.near(u, i, t.S - 1)
        t.anywhere(u, mid - 10, 3)
    return t


def _longest(name, cos):
    fs = 16000 if "16k" in name else 8000
    floor = lowest_floor(fs)
    ceil = 800.0 if "wide" in name else floor * 14.6
    t = Table(name, fs, floor, ceil)
    fa, fb = (floor * 1.03, floor * 1.32)
    x, ft = voice(fs, int(0.4 * fs), fa, fb, 7)
    u = t.add(x, ft)
    for i in range(150, 251, 10):
        for j in (0, t.S // 2, t.S - 1):
            t.near(u, i, j)
    t.anywhere(u, 200, 1)
    return t


SLOT_HANDLES = {16: (1000.0, 40.0), 17: (1190.0, 40.0), 18: (1400.0, 40.0), 19: (1680.0, 40.0), 32: (1000.0, 80.0)}


def _slots(name, cos):
    S = int(name.split("_")[1])
    ceil, cio = SLOT_HANDLES[S]
    t = Table(name, 8000, 71.0, ceil, cio)
    assert t.S == S
    x, ft = voice(8000, 800, 150.0, 400.0, 20 + S)
    u = t.add(x, ft)
    for i in (49, 50, 51):
        for j in range(S):
            t.near(u, i, j)
    for i in (10, 30, 70, 90):
        t.near(u, i, S - 1)
        t.anywhere(u, i, 0)
    return t


def _edges(name, cos):
    t = Table(name, 8000, 40.0, 800.0)
    for k, n in enumerate((1600, 1608, 1616, 400, 1592)):  # 201, 202, 203, 51 and 200 frames; 401 samples are shorter than a 42 Hz window
        x, ft = voice(8000, n, 41.0, 45.0, 40 + k)
        u = t.add(x, ft)
        L1 = t.L1(u)
        for i in list(range(4)) + list(range(L1 - 4, L1)):
            t.near(u, i, 0)
            t.near(u, i, t.S - 1)
        if n == 400:  # frames whose windows leave the utterance on both sides at once
            for i in range(22, 29):
                t.near(u, i, 1)
    return t


def _ragged(name, cos):
    t = Table(name, 8000, 71.0, 800.0)
    for k, (n, level) in enumerate(((800, 0.5), (120, 1e-3), (808, 0.7), (640, 0.5))):
        x, ft = voice(8000, n, 180.0, 240.0, 60 + k, noise=1e-3 * level, level=level)
        t.add(x, ft)
    for u, frames in ((0, range(t.L1(0) - 3, t.L1(0))), (2, range(3)), (2, range(t.L1(2) - 3, t.L1(2))), (3, range(3))):
        for i in frames:
            for j in range(t.S):
                t.near(u, i, j)
    for i in (0, 1, 2, t.L1(1) - 3, t.L1(1) - 2, t.L1(1) - 1):
        t.near(1, i, 0)
        t.near(1, i, t.S - 1)
    return t


def _one_live(name, cos):
    t = Table(name, 8000, 71.0, 800.0)
    for k, (frame, slot) in enumerate(((50, 7), (0, 0), (-1, 14))):
        x, ft = voice(8000, 800, 200.0, 220.0, 70 + k)
        u = t.add(x, ft)
        i = frame % t.L1(u)
        t.near(u, i, slot)
        t.notes.setdefault("live", []).append((u, i, slot))
    return t


def _silence(name, cos):
    t = Table(name, 8000, 71.0, 800.0)
    x, ft = voice(8000, 1600, 150.0, 150.0, 80)
    x[400:1000] = 0.0  # frames 50 .. 125; a 150 Hz window is 163 samples: frames 61 .. 114 see nothing but zeros
    u = t.add(x, ft)
    for i in (70, 80, 90, 100):
        t.near(u, i, 0)
    for i in list(range(42, 54)) + list(range(122, 134)):
        t.near(u, i, 1)
        t.near(u, i, 14)
    return t


def _crowded(name, cos):
    S = int(name.split("_")[1])
    t = Table(name, 8000, 71.0, 800.0) if S == 15 else Table(name, 8000, 71.0, 1000.0, 80.0)
    assert t.S == S
    x, ft = voice(8000, 800, 75.0, 75.0, 90 + S, flat=True)  # a flat comb 75 Hz apart: a harmonic of any candidate finds a partial nearby
    u = t.add(x, ft)
    lo, hi = math.log(t.floor * 1.02), math.log(t.ceil * 0.98)
    for i in range(44, 51):
        for j in range(S):
            if j < 4:
                f = 150.0 + 75.0 * j  # the same value in every frame: stretches of equal keys
            else:
                f = math.exp(lo + (hi - lo) * ((j - 4) * 7 + (i - 44) + 0.5) / ((S - 4) * 7))
            t.put(u, i, j, f)
    return t


BUILDERS = dict(cuts_low=_cuts, cuts_high=_cuts, longest_8k=_longest, longest_16k=_longest, longest_wide=_longest,
                slots_16=_slots, slots_17=_slots, slots_18=_slots, slots_19=_slots, slots_32=_slots, edges=_edges, ragged=_ragged,
                one_live=_one_live, silence=_silence, crowded_15=_crowded, crowded_32=_crowded)
WITH_COS_TABLE = ("cuts_low", "cuts_high", "edges", "crowded_15", "crowded_32")
NAMES = sorted(BUILDERS) + [n + "_cos" for n in WITH_COS_TABLE]
# the table each mutant of the rule must be caught on
MUTANT_TABLE = {"hw+1": "cuts_low", "bin+1": "cuts_high", "nh-1": "cuts_high", "basic+1": "edges", "noclamp": "edges",
                "neighbour": "ragged", "overlap_swapped": "one_live", "fused_bin": "cuts_high"}

_tables, _rules = {}, {}


def table(name):
    if name not in _tables:
        cos = name.endswith("_cos")
        base = name[:-4] if cos else name
        t = BUILDERS[base](name, cos)
        t.cos = cos
        _tables[name] = t
    return _tables[name]


# ------------------------------------------------------------------------------------------------------------------------
# the rule on a table
# ------------------------------------------------------------------------------------------------------------------------
FIELDS = ("f", "rf", "inv", "unit", "growth", "hw", "N", "nh", "basic")


def rule(name, mutant=None):
    """per utterance a dict of [L1][7 S] arrays: live, f (the raw candidate), rf and inv = 1 / score before the thresholds, unit,
    growth = max(1, q / log2 N), hw, N, nh, basic, clamp_lo, clamp_hi, zero, survive, and bins [L1][7 S][6].  Computed once."""
    if (name, mutant) in _rules:
        return _rules[(name, mutant)]
    t = table(name)
    out = []
    for u in range(len(t.xs)):
        y = t.y(u)
        ybuf = np.zeros(len(y) + 2 * PAD, dtype=LD)
        ybuf[PAD:PAD + len(y)] = y
        if mutant == "neighbour":
            if u > 0:
                p = t.y(u - 1)[-PAD:]
                ybuf[PAD - len(p):PAD] = p
            if u + 1 < len(t.xs):
                q = t.y(u + 1)[:PAD]
                ybuf[PAD + len(y):PAD + len(y) + len(q)] = q
        L1, S = t.L1(u), t.S
        r = {k: np.zeros((L1, 7 * S)) for k in FIELDS}
        for k in ("live", "clamp_lo", "clamp_hi", "zero", "survive"):
            r[k] = np.zeros((L1, 7 * S), dtype=bool)
        r["bins"] = np.zeros((L1, 7 * S, 6), dtype=np.int64)
        done = {}
        for i in range(L1):
            for b in range(7):
                bb = b if mutant != "overlap_swapped" or b == 0 else (b + 3 if b <= 3 else b - 3)
                src = block_source(i, bb)
                if src < 0 or src >= L1:
                    continue
                for j in np.flatnonzero(t.cand0[u][src] > 0.0):
                    f = float(t.cand0[u][src, j])
                    if (i, f) not in done:
                        done[(i, f)] = refine_one(ybuf, len(y), float(t.fs), i, f, t.cos, mutant)
                    d = done[(i, f)]
                    p = j + S * b
                    r["live"][i, p] = True
                    r["f"][i, p] = f
                    for k in ("rf", "inv", "unit", "hw", "N", "nh", "basic", "clamp_lo", "clamp_hi", "zero"):
                        r[k][i, p] = d[k]
                    r["bins"][i, p, :d["nh"]] = d["bins"]
                    r["growth"][i, p] = max(1.0, math.ceil(d["bt"] / 8) / math.log2(d["N"]))
                    r["survive"][i, p] = not (d["rf"] < t.floor or d["rf"] > t.ceil or 1.0 / d["inv"] < 2.5)
        out.append(r)
    _rules[(name, mutant)] = out
    return out


def allowed(r, k):
    """units the device may be off by, per position: 2 K_ref max(1, q / log2 N)"""
    return 2.0 * k * r["growth"]


def near_threshold(t, r, k):
    """candidates whose rule value lies within the comparison bound of the floor, the ceiling or score 2.5"""
    b = allowed(r, k) * r["unit"]
    bs = np.where(r["live"], b / np.where(r["f"] > 0, r["f"], 1.0), 0.0)
    return r["live"] & ((np.abs(r["rf"] - t.floor) <= b) | (np.abs(r["rf"] - t.ceil) <= b) | (np.abs(r["inv"] - 0.4) <= bs))


def errors(r, cand1, score1):
    """errors of a refinement's rows [L1][7 S] against the rule of one utterance, position by position, in units: of the refined
    F0 and of 1 / score, where the candidate survives on both sides (0 elsewhere)"""
    assert cand1.shape == r["rf"].shape and score1.shape == r["rf"].shape
    both = r["live"] & (cand1 != 0) & (score1 != 0) & r["survive"]
    err_f, err_s = np.zeros(cand1.shape), np.zeros(cand1.shape)
    err_f[both] = np.abs(cand1[both] - r["rf"][both]) / r["unit"][both]
    err_s[both] = np.abs(1.0 / score1[both] - r["inv"][both]) / (r["unit"][both] / r["f"][both])
    return err_f, err_s


def same_zero_pattern(t, r, cand1, score1, k):
    """outside the near-threshold set a refinement's rows are zero exactly where the rule's are"""
    assert np.array_equal(cand1 != 0, score1 != 0), t.name
    assert not (cand1 != 0)[~r["live"]].any(), (t.name, "a value where no candidate was written")
    firm = r["live"] & ~near_threshold(t, r, k)
    bad = np.argwhere(firm & ((cand1 != 0) != r["survive"]))
    assert len(bad) == 0, (t.name, "zero pattern differs at (frame, position)", bad[:8].tolist())


_oracle, _k_ref = {}, []


def oracle(port, name):
    """the CPU oracle on a table: per utterance (cand1, score1, decisions), computed once"""
    if name not in _oracle:
        t = table(name)
        _oracle[name] = [port.harvest_refine(t.y(u), float(t.fs), t.cand0[u], t.floor, t.ceil, t.cos, decisions=True)
                         for u in range(len(t.xs))]
    return _oracle[name]


def k_ref(port):
    """K_ref: the largest error of the CPU oracle against the rule, in units, over all tables (F0 and 1 / score alike)"""
    if not _k_ref:
        k = 0.0
        for name in NAMES:
            for r, (c1, s1, _) in zip(rule(name), oracle(port, name)):
                ef, es = errors(r, c1, s1)
                k = max(k, float(ef.max()), float(es.max()))
        _k_ref.append(k)
    return _k_ref[0]


# the device's key of a candidate and the hash of its 256-entry table (hv_refine_packed_kernel), for the claims of `crowded`
def key_of(fs, f):
    """(hw, six bins) as the kernels pack them, and the table entry the key hashes to"""
    hw = int(1.5 * fs / f + 1.0)
    N = 1 << (2 + (2 * hw + 1).bit_length() - 1)
    unit = f * N / fs
    b0 = mround(unit)
    kk = hw | (b0 << 32)
    for h in range(1, 6):
        dlt = mround(unit * (h + 1)) - (h + 1) * b0 + 8
        kk |= (dlt & 15) << (11 + 4 * (h - 1))
    lo, hi = kk & 0xFFFFFFFF, kk >> 32
    entry = ((((lo * 2654435761) & 0xFFFFFFFF) ^ ((((hi * 40503) & 0xFFFFFFFF) * 65537) & 0xFFFFFFFF)) >> 24)
    return kk, entry
