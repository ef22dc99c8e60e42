"""CPU tests of the warp's host functions (include/world_class_warp.h) against the map rule in Python (tests/warp_rule.py): the
positions of a time map, exactly; the output length; refusals; the tiling query beside the converter's; and the quality of a warp
along a vibrato curve, on the rule alone under the rational converter's bound."""
import ctypes as C
import math

import numpy as np
import pytest

import vresample_rule as R
import warp_rule as W
from test_gpu_vresample import PLANS, plan_args
from test_resample_rule import QUALITY_BOUND
from world_class_amd import WorldClassError, vresample as vr, warp

NAN = float("nan")
TWO30 = float(1 << 30)


def b_on_a(rng, length):
    """what d_b_on_a looks like: half-integer, non-decreasing, with flat runs and steps of 2"""
    return np.cumsum(rng.choice([0.0, 0.5, 1.0, 2.0], size=length)) + 3.0


# name -> (map, out_per_entry, in_per_unit)
def map_cases():
    rng = np.random.default_rng(5)
    m9 = b_on_a(rng, 9)
    holed = b_on_a(rng, 9)
    holed[4] = NAN   # entries 3 and 5 stay finite exactly at n = 3 x 240 and 5 x 240; everything strictly between 3 and 5 is lost
    below = math.nextafter(-TWO30, -math.inf)
    return {
        "one_entry": (np.array([7.5]), 240.0, 240.0),
        "two_entries": (np.array([0.5, 2.5]), 240.0, 80.0),
        "b_on_a_240": (m9, 240.0, 220.5),
        "b_on_a_220_5": (m9, 220.5, 240.0),
        "b_on_a_80": (m9, 80.0, 240.0),
        "nan_entry": (holed, 240.0, 240.0),
        "falling": (m9[::-1].copy(), 80.0, 13.25),
        "long": (b_on_a(rng, 257), 80.0, 220.5),
        "range_ends": (np.array([-TWO30, below, TWO30, math.nextafter(TWO30, 0.0), math.inf, -math.inf, -0.0]), 1.0, 1.0),
        "range_ends_scaled": (np.array([-TWO30 / 4, below / 4, TWO30 / 4, 1.0]), 3.0, 4.0),
    }


MAPS = map_cases()


@pytest.mark.parametrize("name", sorted(MAPS))
def test_map_positions_are_the_rule_exactly(name):
    m, ope, ipu = MAPS[name]
    n_out = W.map_out_length(len(m), ope) + 5   # past the last entry: t >= L - 1, the end is held
    assert warp.map_out_length(len(m), ope) == n_out - 5
    got = warp.map_positions(m, ope, ipu, n_out)
    want = W.map_positions(m, ope, ipu, n_out)
    assert got.dtype == np.int64 and [int(p) for p in got] == want
    assert np.array_equal(warp.map_positions(m, ope, ipu), got[:n_out - 5])   # (n_out defaults to map_out_length)
    assert want[-1] == want[-5] == W.map_position(m, ope, ipu, 10 ** 9)


def test_the_cases_reach_what_they_are_for():
    m, ope, ipu = MAPS["nan_entry"]
    pos = W.map_positions(m, ope, ipu, W.map_out_length(len(m), ope))
    lost = [n for n, p in enumerate(pos) if p == W.NO_POSITION]
    assert lost == list(range(3 * 240 + 1, 5 * 240))   # the entries beside the NaN stay, on their own outputs (w == 0)
    assert pos[3 * 240] == int(m[3] * 240) << 32 and pos[5 * 240] == int(m[5] * 240) << 32
    m, ope, ipu = MAPS["range_ends"]
    pos = W.map_positions(m, ope, ipu, len(m))
    assert pos[0] == -(1 << 62) and pos[1] == W.NO_POSITION and pos[2] == W.NO_POSITION and pos[3] == (1 << 62) - (1 << 9)
    assert pos[4] == pos[5] == W.NO_POSITION and pos[6] == 0
    m, ope, ipu = MAPS["b_on_a_220_5"]
    ts = [n / ope for n in range(W.map_out_length(len(m), ope))]
    assert sum(t == math.floor(t) for t in ts) >= 4 and sum(t != math.floor(t) for t in ts) > 1000
    assert W.NO_POSITION == warp.NO_POSITION == -(1 << 63)


def test_an_identity_map_with_equal_hops():
    """positions n 2^32 wherever (n / hop) x hop rounds back to n: at 80 and at a power of two always, at 240 and 220.5 some come out
    one unit of 2^-32 lower -- the rule's arithmetic, and the library's"""
    m = np.arange(40.0)
    for hop, exact in ((80.0, True), (256.0, True), (240.0, False), (220.5, False)):
        pos = warp.map_positions(m, hop, hop)
        off = pos.astype(object) - np.arange(len(pos)).astype(object) * R.ONE
        assert [int(p) for p in pos] == W.map_positions(m, hop, hop, len(pos))
        assert set(off) == ({0} if exact else {0, -1})


@pytest.mark.parametrize("length,ope", [(1, 240.0), (2, 240.0), (9, 220.5), (9, 0.3), (257, 80.0), (2 ** 31 - 1, 1e-3), (100, 2.0 ** 40)])
def test_map_out_length_is_its_formula(length, ope):
    assert warp.map_out_length(length, ope) == W.map_out_length(length, ope) == int(math.floor((length - 1) * ope)) + 1


def test_refusals():
    L = warp._L()
    for length, ope in ((0, 240.0), (-1, 240.0), (9, 0.0), (9, -1.0), (9, NAN), (9, math.inf), (2 ** 31 - 1, 1e300)):
        assert L.wc_warp_map_out_length(length, ope) < 0
        with pytest.raises(WorldClassError):
            warp.map_out_length(length, ope)
    m = np.arange(4.0)
    pos = np.zeros(8, dtype=np.int64)
    mp, pp = m.ctypes.data_as(C.POINTER(C.c_double)), pos.ctypes.data_as(C.POINTER(C.c_longlong))
    assert L.wc_warp_map_positions(mp, 4, 2.0, 1.0, 8, pp) == 0
    for args in ((None, 4, 2.0, 1.0, 8, pp), (mp, 4, 2.0, 1.0, 8, None), (mp, 0, 2.0, 1.0, 8, pp), (mp, 4, 2.0, 1.0, -1, pp),
                 (mp, 4, 0.0, 1.0, 8, pp), (mp, 4, NAN, 1.0, 8, pp), (mp, 4, math.inf, 1.0, 8, pp), (mp, 4, -2.0, 1.0, 8, pp),
                 (mp, 4, 2.0, 0.0, 8, pp), (mp, 4, 2.0, NAN, 8, pp), (mp, 4, 2.0, math.inf, 8, pp), (mp, 4, 2.0, -1.0, 8, pp)):
        before = pos.copy()
        assert L.wc_warp_map_positions(*args) < 0
        assert np.array_equal(pos, before)
    with pytest.raises(WorldClassError) as e:
        warp.map_positions(m, 0.0, 1.0)
    assert "warp" in str(e.value)
    with pytest.raises(WorldClassError):   # the plan's refusals are the converter's
        warp.tiling(R.ONE + 1, R.ONE)


@pytest.mark.parametrize("name", sorted(PLANS))
def test_tiling_is_the_converters_with_a_span(name):
    a = plan_args(name)
    half = vr.plan(**a)[0]
    tile_outputs, segment_min, plain_block = vr.tiling(**a)
    got = warp.tiling(**a)
    assert (got[0], got[2], got[3]) == (tile_outputs, segment_min, plain_block)
    assert (got[0] == 0) == (tile_outputs == 0) == (name == "no_tile")
    taps = 2 * half + 1
    assert got[1] >= taps + 1
    if tile_outputs:   # the span of a tile at step_max, which the converter's own tiles need
        assert got[1] >= (tile_outputs * a["step_max"] >> 32) + taps


def test_dead_outputs_are_plus_zero_by_the_rule_itself():
    """warp_rule.warp_at leaves the outputs without a tap inside the signal to a constant: the rule gives the same, sign and all"""
    C_, bits = vr.filter_table(R.ONE, 1 << 33, zeros=4), R.DEFAULT[0]
    half = (C_.shape[1] - 1) // 2
    x = 1e6 * np.random.default_rng(2).uniform(-1, 1, 50)
    for q in (-half - 1, -half - 7, len(x) + half, len(x) + half + 9):
        for f in (0, 1, R.ONE - 1, R.ONE >> 1):
            y = R.vresample_at(x, [q * R.ONE + f], C_, bits)
            assert y[0] == 0.0 and not np.signbit(y[0])
    edge = [(-half) * R.ONE, (-half) * R.ONE + R.ONE - 1, (len(x) - 1 + half) * R.ONE + 5, W.NO_POSITION, (1 << 63) - 1, 17 * R.ONE + 99]
    y = W.warp_at(x, edge, C_, bits)
    assert np.array_equal(y[[0, 1, 2, 5]], R.vresample_at(x, [edge[i] for i in (0, 1, 2, 5)], C_, bits))
    assert np.array_equal(W.live(edge, len(x), half), [True, True, True, False, False, True]) and not np.signbit(y).any() and y[1] != 0.0


def test_quality_of_a_warp_along_a_vibrato_curve():
    """a 3 kHz sine of 6000 samples at 48 kHz along n + 40 sin(2 pi n / 600), on the default table made for step_max = 2^33: the
    curve advances by at most 1 + 80 pi / 600 = 1.42 samples per output, inside the handle's cut-off"""
    fs, freq, n_in = 48000.0, 3000.0, 6000
    C_ = vr.filter_table(R.ONE, 1 << 33)
    half = (C_.shape[1] - 1) // 2
    x = np.sin(2 * np.pi * freq * np.arange(n_in) / fs)
    n = np.arange(half + 50, n_in - half - 50)
    p = n + 40.0 * np.sin(2 * np.pi * n / 600.0)
    assert p.min() >= half and p.max() < n_in - half
    pos = [int(math.floor(v * 4294967296.0)) for v in p]
    y = R.vresample_at(x, pos, C_, R.DEFAULT[0])
    t = np.array(pos, dtype=np.float64) / R.ONE   # (below 2^53: exact)
    err = np.abs(y - np.sin(2 * np.pi * freq * t / fs)).max()
    print("warp along a vibrato curve: max error %.2e (bound %.0e)" % (err, QUALITY_BOUND))
    assert err < QUALITY_BOUND
