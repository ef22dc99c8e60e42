"""CPU tests of the variable-ratio resampler's host functions against the rule in numpy (tests/vresample_rule.py): plan, table, counts,
refusals, the table's error against the exact prototype, and the quality the tables buy, recomputed from the library's table through
the rule's summation under the rational converter's own bound (QUALITY_BOUND of tests/test_resample_rule.py)."""
import ctypes as C

import numpy as np
import pytest

import vresample_rule as R
from test_resample_rule import QUALITY_BOUND
from world_class_amd import WorldClassError, vresample as vr

ONE = R.ONE
UP = vr.step_of(48000 / 44100 * 1.0003)   # a capture clock 300 ppm off: no fraction a table of rows could hold
DOWN = vr.step_of(0.7071)
DOWN_MAX = vr.step_of(0.70)
# (phase_bits, degree): the default first
PLANS = [(3, 5), (4, 5), (2, 7), (8, 3)]
# (step_min, step_max) -> the step the tones run at
QUALITY_CASES = [(UP, UP, UP), (DOWN, DOWN_MAX, DOWN), (ONE, ONE, ONE)]


def kw(bits, degree):
    return {} if (bits, degree) == R.DEFAULT else {"phase_bits": bits, "degree": degree}


@pytest.fixture(scope="module")
def tables():
    return {(b, d, hi): vr.filter_table(lo, hi, **kw(b, d)) for b, d in PLANS for lo, hi, _ in QUALITY_CASES}


def test_step_of_is_the_rounded_quotient():
    assert vr.step_of(1) == ONE and vr.step_of(2) == 1 << 31 and vr.step_of(0.5) == 1 << 33 and vr.step_of(4 / 3) == 3 << 30
    assert vr.step_of(0.8) == round(ONE / 0.8) and isinstance(vr.step_of(48000 / 44100), int)
    assert abs(UP * 48000 * 1.0003 - ONE * 44100) < 48000 * 1.0003


@pytest.mark.parametrize("step_max", [1 << 28, ONE - 1, ONE, ONE + 1, UP, DOWN_MAX, 1 << 33, 1 << 36])
def test_plan_is_the_rules(step_max):
    lo = 1 << 28
    assert vr.plan(lo, step_max) == R.plan(step_max)
    assert vr.plan(lo, step_max)[1:3] == (8, 5)   # 0, 0 select the default pair
    for zeros in (1, 4):
        assert vr.plan(lo, step_max, zeros=zeros) == R.plan(step_max, zeros=zeros)
    for bits, degree in ((0, 3), (0, 7), (8, 3), (3, 5), (5, 7)):
        assert vr.plan(lo, step_max, zeros=4, phase_bits=bits, degree=degree) == R.plan(step_max, zeros=4, phase_bits=bits, degree=degree)
    assert vr.plan(lo, step_max, zeros=64, rolloff=R.ROLLOFF, beta=R.BETA) == vr.plan(lo, step_max)
    if step_max <= ONE:
        assert vr.plan(lo, step_max)[0] == 68 and vr.plan(step_max, step_max) == vr.plan(lo, step_max)   # the rational converter's K; step_min plays no part


@pytest.mark.parametrize("bits,degree", PLANS + [(0, 7), (0, 3), (8, 7)])
def test_table_is_the_rules_within_1e_12(bits, degree):
    """two solves of the node system differ by 2.2e-14 at degree 7, and the coefficients are below 1: 1e-12 is 50 times that"""
    for step_max, zeros, rolloff, beta in ((ONE, 64, R.ROLLOFF, R.BETA), (1 << 33, 64, R.ROLLOFF, R.BETA), (UP, 4, 0.8, 6.0)):
        Cl = vr.filter_table(1 << 28, step_max, zeros, rolloff, beta, bits, degree)
        half, segs, deg, _ = vr.plan(1 << 28, step_max, zeros, rolloff, beta, bits, degree)
        assert Cl.shape == (segs, 2 * half + 1, deg + 1) == (1 << bits, 2 * half + 1, degree + 1)
        diff = np.abs(Cl - R.table(step_max, zeros, rolloff, beta, bits, degree)).max()
        print("(%d, %d) step_max %d zeros %d: max |library - numpy| %.2e" % (bits, degree, step_max, zeros, diff))
        assert diff <= 1e-12
        assert np.abs(Cl).max() <= 1.0


def test_the_default_table_is_the_default_pair():
    assert np.array_equal(vr.filter_table(ONE, ONE), vr.filter_table(ONE, ONE, phase_bits=3, degree=5))
    assert vr.filter_table(ONE, ONE).size == 6576


@pytest.mark.parametrize("bits,degree", PLANS)
def test_table_error_against_the_exact_prototype(bits, degree, tables):
    """the polynomials at 4096 random fractions (and the segments' ends) against g itself.  S, the worst sum over a phase's taps,
    bounds what the table adds to an output of samples within [-1, 1]: it has to leave room under the quality bound"""
    rng = np.random.default_rng(bits * 8 + degree)
    f = np.concatenate([rng.integers(0, ONE, 4096), [0, ONE - 1, (1 << (32 - bits)) - 1, ONE >> 1]])
    for _, hi, _ in QUALITY_CASES:
        worst, S = R.table_error(tables[(bits, degree, hi)], hi, bits, f)
        print("(%d, %d) step_max %d: max coefficient error %.2e, worst-phase sum S %.2e" % (bits, degree, hi, worst, S))
        assert worst <= S < QUALITY_BOUND


def _tone_error(C, bits, step, step_max, freq, stop_band=False, fs_in=48000.0):
    """max |y - the same tone at the outputs' own times| over the outputs whose q lies 2K inputs inside a 0.2 s tone; in the stop
    band the tone should vanish, so the error is max |y|"""
    half = (C.shape[1] - 1) // 2
    n_in = int(0.2 * fs_in)
    x = np.sin(2 * np.pi * freq * np.arange(n_in) / fs_in)
    pos = R.positions(step, R.out_length(step, n_in))
    y = R.vresample_at(x, pos, C, bits)
    t = np.array(pos, dtype=np.float64) / ONE   # (below 2^53: exact)
    keep = (t >= 2 * half) & (t < n_in - 2 * half)
    assert keep.sum() > 100
    want = 0.0 if stop_band else np.sin(2 * np.pi * freq * t / fs_in)
    return np.abs(y - want)[keep].max()


@pytest.mark.parametrize("bits,degree", PLANS)
def test_quality_under_the_rational_converters_bound(bits, degree, tables):
    """tones through the rule on the library's table: 1 kHz, 0.9 x rolloff x the lower Nyquist rate, and 1.06 x that rate where the
    conversion goes down.  The lower Nyquist rate is the one step_max designs the cut-off for, fs_in / 2 x min(1, 2^32 / step_max):
    at DOWN the handle is made for 0.70 and run at 0.7071, as a varispeed range is"""
    fs_in = 48000.0
    for lo, hi, step in QUALITY_CASES:
        Cl = tables[(bits, degree, hi)]
        nyquist = fs_in / 2 * min(1.0, ONE / hi)
        e1 = _tone_error(Cl, bits, step, hi, 1000.0)
        e2 = _tone_error(Cl, bits, step, hi, 0.9 * R.ROLLOFF * nyquist)
        print("(%d, %d) step %d: 1 kHz %.2e, 0.9 x rolloff x Nyquist %.2e" % (bits, degree, step, e1, e2))
        assert e1 < QUALITY_BOUND and e2 < QUALITY_BOUND
        if hi > ONE:
            e3 = _tone_error(Cl, bits, step, hi, 1.06 * nyquist, stop_band=True)
            print("(%d, %d) step %d: stop band %.2e" % (bits, degree, step, e3))
            assert e3 < QUALITY_BOUND


STEPS = [1 << 28, ONE - 1, ONE, ONE + 1, UP, DOWN, 3 << 30, (1 << 36) - 12345, 1 << 36]


@pytest.mark.parametrize("step", STEPS)
def test_counts_are_python_integers(step):
    half = 68
    for n in (0, 1, half, half + 1, 2 ** 31 + 7, 2 ** 40 + 12345, 2 ** 58 + 3):
        assert vr.out_length(step, n) == R.out_length(step, n)
    big = 1 << 62
    cases = [(0, 0, 0), (0, 0, half), (0, 0, half + 1), (0, 0, 100000), (5, 123456789, 4), (5, 123456789, 5 + half), (5, 123456789, 6 + half),
             (1000, ONE - 1, 2000), (big - 50, 7, big + 100), (big - 50, ONE - 1, big - 50 + half), (big - 50, ONE - 1, big - 49 + half),
             (big, 0, big + (1 << 20)), (big + 12345, 99, big)]
    for q, f, T in cases:
        for flushed in (False, True):
            assert vr.committed(q, f, step, half, T, flushed) == R.committed(q, f, step, half, T, flushed), (q, f, T, flushed)
    assert vr.committed(0, 0, step, 0, 1000) == vr.committed(0, 0, step, 5, 1000, True) == R.out_length(step, 1000)
    assert vr.committed(0, 0, step, half, half) == 0 and vr.committed(0, 0, step, half, half, True) == vr.out_length(step, half)


def test_counts_that_leave_63_bits_are_refused():
    L = vr._L()
    assert L.wc_vresample_out_length(1 << 28, 1 << 62) < 0 and L.wc_vresample_committed(0, 0, 1 << 28, 0, 1 << 62, 1) < 0
    assert vr.out_length(1 << 36, 1 << 62) == 1 << 58
    for args in ((-1, 0, ONE, 68, 10, 0), (0, 0, ONE, -1, 10, 0), (0, 0, ONE, 68, -1, 0), (0, 0, (1 << 28) - 1, 68, 10, 0), (0, 0, (1 << 36) + 1, 68, 10, 0)):
        assert L.wc_vresample_committed(*args) < 0
    assert L.wc_vresample_out_length(ONE, -1) < 0 and L.wc_vresample_out_length((1 << 28) - 1, 5) < 0 and L.wc_vresample_out_length((1 << 36) + 1, 5) < 0


@pytest.mark.parametrize("half", [2, 68])
def test_any_split_commits_every_output_once(half):
    """a stream's bookkeeping replayed with the library's count: the position moves on by count x step, so every output is committed
    once and in order exactly when the counts add up -- to out_length at a constant step, and to the rule's own replay where the step
    changes between pushes"""
    rng = np.random.default_rng(half)
    for step in (UP, DOWN, ONE, ONE + 1, 1 << 28, 1 << 36):
        for total in (1, half - 1, half, half + 1, 5000):
            for _ in range(4):
                cuts = np.sort(rng.integers(0, total + 1, size=rng.integers(0, 6)))
                marks = [int(c) for c in cuts] + [total]
                pos, n_out = 0, 0
                for T in marks + [None]:
                    c = vr.committed(pos >> 32, pos & (ONE - 1), step, half, total if T is None else T, T is None)
                    assert c >= 0
                    pos, n_out = pos + c * step, n_out + c
                assert n_out == vr.out_length(step, total) and pos >= total * ONE > pos - step
    for total in (300, 5000):
        pos = rpos = 0
        T = 0
        while T < total:
            T = min(total, T + int(rng.integers(0, 400)))
            step = int(rng.integers(1 << 28, (1 << 36) + 1))
            c = vr.committed(pos >> 32, pos & (ONE - 1), step, half, T)
            assert c == R.committed(rpos >> 32, rpos & (ONE - 1), step, half, T)
            pos, rpos = pos + c * step, rpos + c * step
            assert (pos >> 32) + half > T - 1 and (c == 0 or ((pos - step) >> 32) + half <= T - 1)   # the first uncommitted and the last committed
            assert (pos >> 32) >= T - half
        c = vr.committed(pos >> 32, pos & (ONE - 1), step, half, total, True)
        assert (pos + c * step) >> 32 >= total and (c == 0 or (pos + (c - 1) * step) >> 32 <= total - 1)


LO, HI = 1 << 28, 1 << 36


@pytest.mark.parametrize("args", [
    (LO - 1, ONE, 0, 0.0, 0.0, 0, 0), (ONE, HI + 1, 0, 0.0, 0.0, 0, 0), (0, ONE, 0, 0.0, 0.0, 0, 0), (ONE, 1 << 63, 0, 0.0, 0.0, 0, 0),   # a step outside [2^28, 2^36]
    (ONE + 1, ONE, 0, 0.0, 0.0, 0, 0),   # step_min > step_max
    (ONE, ONE, 0, 0.0, 0.0, -1, 5), (ONE, ONE, 0, 0.0, 0.0, 9, 5),   # phase_bits
    (ONE, ONE, 0, 0.0, 0.0, 3, 4), (ONE, ONE, 0, 0.0, 0.0, 3, 1), (ONE, ONE, 0, 0.0, 0.0, 3, 9), (ONE, ONE, 0, 0.0, 0.0, 3, -5),   # degree
    (ONE, ONE, 0, 0.0, 0.0, 3, 0),   # degree 0 is the default PAIR
    (ONE, ONE, -1, 0.0, 0.0, 0, 0),   # zeros < 1 (0 is the default)
    (ONE, ONE, 0, -0.5, 0.0, 0, 0), (ONE, ONE, 0, 1.0000001, 0.0, 0, 0), (ONE, ONE, 0, float("nan"), 0.0, 0, 0),   # rolloff outside (0, 1]
    (ONE, ONE, 0, 0.0, float("inf"), 0, 0), (ONE, ONE, 0, 0.0, float("nan"), 0, 0), (ONE, ONE, 0, 0.0, -1.0, 0, 0), (ONE, ONE, 0, 0.0, 701.0, 0, 0),   # beta
    (ONE, HI, 0, 0.0, 0.0, 8, 7), (ONE, ONE, 50000, 0.0, 0.0, 0, 0),   # a table above 2^21 doubles
])
def test_refusals(args):
    with pytest.raises(WorldClassError) as e:
        vr.plan(*args)
    assert "vresample" in str(e.value)
    with pytest.raises(WorldClassError):
        vr.filter_table(*args)
    if args[4] == 0.0:  # (the tiling takes no beta)
        with pytest.raises(WorldClassError):
            vr.tiling(args[0], args[1], args[2], args[3], args[5], args[6])


def test_the_cap_keeps_the_useful_tables_in_and_a_short_array_is_refused():
    assert vr.plan(LO, HI)[0] == 1081 and vr.plan(LO, 1 << 35, phase_bits=8, degree=3)[:2] == (541, 256)   # 1/16 at the default, 1/8 at 256 segments
    half, segs, deg, _ = vr.plan(ONE, ONE)
    c = np.empty(segs * (2 * half + 1) * (deg + 1) - 1)
    assert vr._L().wc_vresample_filter(ONE, ONE, 0, 0.0, 0.0, 0, 0, c.ctypes.data_as(C.POINTER(C.c_double)), c.size) < 0
    assert vr._L().wc_vresample_filter(ONE, ONE, 0, 0.0, 0.0, 0, 0, None, 1 << 21) < 0


def test_tiling_query():
    tile, seg_min, plain = vr.tiling(ONE, vr.step_of(0.9))
    assert tile > 0 and tile % vr.WAVE == 0 and seg_min >= vr.WAVE and plain > 0
    assert vr.tiling(LO, HI, zeros=512)[0] == 0   # 17293 taps and 16 inputs per output: no tile fits the local memory
    assert vr.tiling(ONE, ONE, phase_bits=8, degree=3)[1] > seg_min   # more segments want more outputs before a wavefront fills
