"""GPU tests of wc_warp_device (include/world_class_warp.h): bit for bit against wc_vresample_device at arithmetic positions and
against the rule in numpy (tests/vresample_rule.py: vresample_at) on the library's own table everywhere else -- at the span where a
tile stops holding its inputs in local memory, at positions that fall, repeat and jump, at the ends of a signal and beyond them, in
a ragged batch with empty utterances, in every sample format.  Every batch is guarded as tests/test_gpu_vresample.py's are."""
import numpy as np
import pytest

import vresample_rule as R
import warp_rule as W
from test_gpu_vresample import GUARD, PATTERN, PLANS as VR_PLANS, UPR, WIDE, batch_of, check, lengths_of, run_guarded as vr_run_guarded
from world_class_amd import DeviceArray, WorldClassError, io as wio, lib, vresample as vr, warp

pytestmark = pytest.mark.gpu

ONE = R.ONE
LLONG_MAX = (1 << 63) - 1
# name -> (step_min, step_max, zeros, phase_bits, degree): the converter's test plans and a small one (K = 9, tiles of 2048)
PLANS = {name: p[:5] for name, p in VR_PLANS.items()}
PLANS["small"] = WIDE + (4, 0, 0)
ARITHMETIC = {"default": UPR, "one_segment": UPR, "256_segments": ONE + 1, "zeros_1": 3 << 30, "no_tile": 1 << 35, "small": 1 << 33}
TILED = ["small", "default", "one_segment", "256_segments"]


def plan_args(name):
    lo, hi, zeros, bits, degree = PLANS[name]
    return dict(step_min=lo, step_max=hi, zeros=zeros, phase_bits=bits, degree=degree)


class Plan:
    def __init__(self, name):
        a = plan_args(name)
        self.half, segs, _, _ = vr.plan(**a)
        self.bits = segs.bit_length() - 1
        self.taps = 2 * self.half + 1
        self.C = vr.filter_table(**a)
        self.tile, self.span_max, self.segment_min, self.plain_block = warp.tiling(**a)
        self.r = vr.VResampler(**a)


@pytest.fixture(scope="module")
def plans():
    """name -> the plan's numbers, the library's table and a handle, made on first use"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = Plan(name)
        return made[name]

    yield get
    for p in made.values():
        p.r.close()


def run_guarded(r, xs, poss, in_dtype=np.float64, in_format="f64", out_format="f64"):
    """wc_warp_device on a packed batch with d_y GUARD samples too long and pre-filled; the guard must come back untouched"""
    outs = [len(p) for p in poss]
    total = sum(outs)
    odt = vr.OUT_FORMATS[out_format][1]
    fill = np.full(total + GUARD, PATTERN, dtype=np.uint64).view(np.float64) if odt == np.float64 else np.full(total + GUARD, 0x5A5A, dtype=np.int16)
    flat = np.array([int(v) for p in poss for v in p] + [0], dtype=np.int64)   # (Python integers of any size below 2^63)
    d_x = DeviceArray.from_host(np.concatenate(xs), dtype=in_dtype)
    d_pos = DeviceArray.from_host(flat, dtype=np.int64)
    d_y = DeviceArray.from_host(fill, dtype=odt)
    try:
        warp.warp_device(r, d_x, [len(x) for x in xs], d_pos, outs, d_y, in_format, out_format)
        y = d_y.to_host()
    finally:
        d_x.free()
        d_pos.free()
        d_y.free()
    assert np.array_equal(y[total:].view(np.uint8), fill[total:].view(np.uint8)), "the guard behind the output was written"
    return np.split(y[:total], np.cumsum(outs)[:-1])


def between_neighbours(xs, poss, seed=3):
    """every utterance between neighbours of amplitude 1e6 that take no output: a read across an utterance's end shows"""
    rng = np.random.default_rng(seed)
    loud = lambda: 1e6 * rng.uniform(-1, 1, 300)
    all_x, all_p = [loud()], [[]]
    for x, p in zip(xs, poss):
        all_x += [x, loud()]
        all_p += [p, []]
    return all_x, all_p


def run_and_check(p, xs, poss):
    """the guarded batch against the rule, utterance by utterance; an output with no tap inside its signal is +0.0, sign and all"""
    all_x, all_p = between_neighbours(xs, poss)
    ys = run_guarded(p.r, all_x, all_p)
    for u, (x, pos, y) in enumerate(zip(all_x, all_p, ys)):
        want = W.warp_at(x, pos, p.C, p.bits)
        assert len(y) == len(want)
        assert np.array_equal(y, want), "utterance %d (%d samples, %d outputs): %d differ, first at %d" % (
            u, len(x), len(y), int((y != want).sum()), int(np.argmax(y != want)))
        dead = ~W.live(pos, len(x), p.half) if len(pos) else np.zeros(0, dtype=bool)
        assert not y[dead].view(np.uint64).any()
    return ys[1::2]


# ---- 1. arithmetic positions ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PLANS))
def test_arithmetic_positions_are_the_converters_bits(name, plans):
    p, step = plans(name), ARITHMETIC[name]
    if name in VR_PLANS:
        ns = lengths_of(name, step)[0]
    else:   # the same lengths for the plan of this file
        ns = [1, 2, p.half, 2 * p.half + 1, 20011]
        for edge in (p.tile, p.segment_min, p.plain_block):
            for t in (edge - 1, edge, edge + 1):
                ns += [max(1, t * step >> 32), (t * step >> 32) + 1]
        ns = list(dict.fromkeys(ns))
    if name == "no_tile":
        assert p.tile == 0
        ns = [n for n in ns if n != 20011] + [1500 * step >> 32]
    outs = [vr.out_length(step, n) for n in ns]
    if p.tile:
        assert min(outs) < p.segment_min <= max(outs) and max(outs) > p.tile   # both mappings, more than one tile
    xs = batch_of(ns, seed=step % 1000 + len(name))
    poss = [R.positions(step, vr.out_length(step, len(x))) for x in xs]
    got = run_guarded(p.r, xs, poss)
    want = vr_run_guarded(p.r, xs, step)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    check(xs, got, [step] * len(xs), p.C, p.bits)


# ---- 2. the span edge -------------------------------------------------------------------------------------------------------------
def spread_tile(rng, count, q0, width):
    """count positions with q from q0 to q0 + width, both reached, in random order with random fractions"""
    q = rng.integers(q0, q0 + width + 1, count)
    if count >= 2:
        a, b = rng.choice(count, 2, replace=False)
        q[a], q[b] = q0, q0 + width
    else:
        q[:] = q0 + width
    return [int(v) * ONE + int(f) for v, f in zip(q, rng.integers(0, ONE, count))]


@pytest.mark.parametrize("name", TILED)
def test_the_last_near_tile_and_the_first_far_tile(name, plans):
    p = plans(name)
    rng = np.random.default_rng(len(name))
    near, n_in = p.span_max - p.taps, 9000
    assert p.tile > 0 and near + 1 + 300 < n_in
    mid = lambda: R.positions(ONE, p.tile, start=1000 * ONE + 77)
    fill = -(-p.segment_min // p.tile)   # whole tiles in front of a partial one, so that the utterance is tiled
    xs, poss = [], []
    # the first and the last tile of a three-tile utterance, each way round; q0 = -K reads the zeros in front, the other the zeros behind
    for first, last in ((near, near + 1), (near + 1, near)):
        xs.append(rng.uniform(-1, 1, n_in))
        poss.append(spread_tile(rng, p.tile, -p.half, first) + mid() + spread_tile(rng, p.tile, n_in - 1 + p.half - last, last))
    # a partial last tile of tile_outputs - 1 outputs and of 1 output
    for count in (p.tile - 1, 1):
        for width in (near, near + 1):
            xs.append(rng.uniform(-1, 1, n_in))
            poss.append(mid() * fill + spread_tile(rng, count, 200, width))
    for pos in poss:   # the tiles are what they are meant to be
        assert len(pos) >= p.segment_min
        for k in range(0, len(pos), p.tile):
            q = [v >> 32 for v in pos[k:k + p.tile]]
            assert max(q) - min(q) in (near, near + 1, p.tile - 1, 0)
    run_and_check(p, xs, poss)


# ---- 3. order and repeats -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["default", "256_segments", "small"])
def test_positions_that_fall_repeat_and_jump(name, plans):
    p, step = plans(name), ARITHMETIC[name]
    rng = np.random.default_rng(17)
    n_in = 20011
    forward = R.positions(step, vr.out_length(step, n_in))
    assert len(forward) > 2 * p.tile
    shuffled = [forward[i] for i in rng.permutation(len(forward))]
    last_segment = ONE - (ONE >> p.bits)
    xs = [rng.uniform(-1, 1, n_in) for _ in range(5)]
    assert 2 * p.tile >= p.segment_min
    poss = [forward[::-1],                                                              # reverse playback
            shuffled,                                                                   # every tile far
            forward[:p.tile] + [1234 * ONE + 0x9abcdef1] * p.tile + forward[:77],       # one bucket of tile_outputs equal positions
            forward[:p.tile] + [int(q) * ONE + int(f) for q, f in zip(rng.integers(100, 900, p.tile), rng.integers(last_segment, ONE, p.tile))],
            [777 * ONE + 5] * (p.segment_min - 1)]                                      # and repeats on the plain mapping
    ys = run_and_check(p, xs, poss)
    back = run_guarded(p.r, [xs[0]], [forward])[0]
    assert np.array_equal(ys[0], back[::-1])   # an output depends on its position alone


# ---- 4. the ends ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "zeros_1"])
def test_the_ends_of_a_signal_and_beyond(name, plans):
    p = plans(name)
    rng = np.random.default_rng(23)
    n_in, K = 700, p.half
    live = lambda count: [int(q) * ONE + int(f) for q, f in zip(rng.integers(-K, n_in + K, count), rng.integers(0, ONE, count))]
    edges = [q * ONE + f for q in (-K - 1, -K, -K + 1, n_in - 1 + K - 1, n_in - 1 + K, n_in + K) for f in (0, 0xffffffff)]
    far_off = [W.NO_POSITION, LLONG_MAX, -ONE * (1 << 30), ONE * (1 << 30), W.NO_POSITION + 1, LLONG_MAX - ONE]
    tile = p.tile
    one_hole = live(tile)
    one_hole[tile // 3] = W.NO_POSITION
    only_last = [W.NO_POSITION] * (tile - 1) + [3 * ONE + 7]
    poss = [live(tile - len(edges)) + edges + far_off + live(100),      # the edges inside a tile of live ones, the far ones in the next
            one_hole + [W.NO_POSITION] * tile + live(tile),               # NO_POSITION alone; a whole tile of it; live ones behind it
            only_last + [LLONG_MAX] * 5,                                  # a tile whose only live output is its last; a dead partial tile
            edges + far_off,                                              # the same on the plain mapping
            [W.NO_POSITION] * 3]
    assert len(poss[3]) < p.segment_min <= len(poss[2])
    xs = [1e6 * rng.uniform(-1, 1, n_in) for _ in poss]
    ys = run_and_check(p, xs, poss)
    assert not ys[1][tile:2 * tile].view(np.uint64).any() and ys[1][2 * tile:].any()   # +0.0 with the sign bit clear
    assert not ys[2][:tile - 1].view(np.uint64).any() and ys[2][tile - 1] != 0.0
    assert ys[3][:len(edges)].any() and ys[0][tile - len(edges):tile].any()   # the live edges are no zeros


# ---- 5. a ragged batch --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["default", "small"])
def test_a_ragged_batch_with_empty_utterances(name, plans):
    p, step = plans(name), ARITHMETIC[name]
    rng = np.random.default_rng(29)
    outs = [0, 1, p.segment_min - 1, 0, p.segment_min, 2 * p.tile + 1, 0]
    ns = [1, 2, 300, 20011, 5000, 20011, 7]
    xs = [rng.uniform(-1, 1, n) * (1.0 if u % 2 else 1e6) for u, n in enumerate(ns)]
    poss = []
    for u, (n, count) in enumerate(zip(ns, outs)):
        if u == 5:   # tiles of its own kind: arithmetic, then anywhere around the signal
            poss.append(R.positions(step, p.tile, start=50 * ONE) + [int(q) * ONE + int(f) for q, f in zip(
                rng.integers(-p.half - 2, n + p.half + 2, count - p.tile), rng.integers(0, ONE, count - p.tile))])
        else:
            poss.append([int(q) * ONE + int(f) for q, f in zip(rng.integers(-p.half - 2, n + p.half + 2, count), rng.integers(0, ONE, count))])
    ys = run_guarded(p.r, xs, poss)   # (the batch as it is: the empty utterances are its first, its last and one between)
    assert [len(y) for y in ys] == outs
    for x, pos, y in zip(xs, poss, ys):
        assert np.array_equal(y, W.warp_at(x, pos, p.C, p.bits))


# ---- 6. formats -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def format_case(plans):
    """a small batch on both mappings, near and far tiles, in int16 (some samples at the ends of the range), and its double results"""
    p = plans("default")
    rng = np.random.default_rng(11)
    xs16 = [rng.integers(-32768, 32768, n).astype(np.int16) for n in (5, 137, 6000)]
    xs16[1][:4] = [-32768, 32767, 0, -1]
    glide = np.cumsum(rng.integers(ONE >> 1, ONE + (ONE >> 1), p.tile + 300))   # a speed glide: near tiles
    poss = [[int(q) * ONE + int(f) for q, f in zip(rng.integers(-3, 9, 40), rng.integers(0, ONE, 40))],
            [W.NO_POSITION] + R.positions(UPR, 100) + [LLONG_MAX],
            [int(v) for v in glide] + [int(q) * ONE + int(f) for q, f in zip(rng.integers(0, 6000, 500), rng.integers(0, ONE, 500))]]
    wide = [x.astype(np.float64) / 32768.0 for x in xs16]
    want = run_guarded(p.r, wide, poss)
    for x, pos, y in zip(wide, poss, want):
        assert np.array_equal(y, W.warp_at(x, pos, p.C, p.bits))
    return p.r, xs16, wide, poss, want


def test_int16_and_float32_inputs_are_the_double_call_on_the_widened_samples(format_case):
    r, xs16, wide, poss, want = format_case
    got = run_guarded(r, xs16, poss, np.int16, "i16")
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    xs32 = [(3.0 * x).astype(np.float32) for x in wide]
    got = run_guarded(r, xs32, poss, np.float32, "f32")
    want32 = run_guarded(r, [x.astype(np.float64) for x in xs32], poss)
    assert all(np.array_equal(a, b) for a, b in zip(got, want32))


def test_int16_output_is_double_to_pcm16_of_the_double_output(format_case):
    r, xs16, wide, poss, _ = format_case
    loud = [1.7 * x for x in wide]   # (some outputs beyond the range: the clamp)
    y = np.concatenate(run_guarded(r, loud, poss))
    d_y, d_p = DeviceArray.from_host(y), DeviceArray(len(y), dtype=np.int16)
    try:
        wio.double_to_pcm16_device(d_y, len(y), d_p)
        want = d_p.to_host()
    finally:
        d_y.free()
        d_p.free()
    got = np.concatenate(run_guarded(r, loud, poss, out_format="i16"))
    assert got.dtype == np.int16 and np.array_equal(got, want)
    assert np.array_equal(want, R.pcm16(y)) and want.min() == -32768 and want.max() == 32767
    got = np.concatenate(run_guarded(r, xs16, poss, np.int16, "i16", "i16"))
    assert np.array_equal(got, R.pcm16(np.concatenate(format_case[4])))


def test_warp_on_host_arrays_returns_the_same(format_case):
    r, xs16, wide, poss, want = format_case
    for xs in (wide, xs16, [x.astype(np.float32) for x in wide]):   # (an int16 sample over 32768 is exact in float32)
        got = warp.warp(r, xs, poss)
        assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))
    got = warp.warp(r, xs16, poss, out_format="i16")
    assert all(np.array_equal(a, R.pcm16(b)) for a, b in zip(got, want))
    got = warp.warp(r, [wide[2], wide[0]], [[], poss[0]])   # an utterance without outputs
    assert len(got[0]) == 0 and np.array_equal(got[1], want[0])


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched(format_case):
    r, xs16, wide, poss, want = format_case
    L = warp._L()
    fill = np.full(64, PATTERN, dtype=np.uint64).view(np.float64)
    d_x, d_pos, d_y = DeviceArray.from_host(np.ones(64)), DeviceArray.from_host(np.zeros(64, dtype=np.int64), dtype=np.int64), DeviceArray.from_host(fill)
    untouched = lambda: np.array_equal(d_y.to_host().view(np.uint8), fill.view(np.uint8))
    try:
        for x_lengths, out_lengths in (([5, 0], [4, 4]), ([-1], [4]), ([], []), ([5, 5], [4, -1])):
            with pytest.raises(WorldClassError):
                warp.warp_device(r, d_x, x_lengths, d_pos, out_lengths, d_y)
            assert untouched()
        with pytest.raises(WorldClassError) as e:   # 2^31 packed outputs: refused on the host, nothing is enqueued
            warp.warp_device(r, d_x, [5, 5], d_pos, [2 ** 31 - 1, 1], d_y)
        assert "2^31" in str(e.value) and untouched()
        for in_format, out_format in ((3, 0), (-1, 0), (0, 2), (0, -1)):
            assert L.wc_warp_device(r._h, 1, d_x.ptr, in_format, warp._ints([4]), d_pos.ptr, warp._ints([4]), d_y.ptr, out_format) < 0
            assert untouched()
        four = warp._ints([4])
        for args in ((None, 1, d_x.ptr, 0, four, d_pos.ptr, four, d_y.ptr, 0), (r._h, 1, None, 0, four, d_pos.ptr, four, d_y.ptr, 0),
                     (r._h, 1, d_x.ptr, 0, None, d_pos.ptr, four, d_y.ptr, 0), (r._h, 1, d_x.ptr, 0, four, None, four, d_y.ptr, 0),
                     (r._h, 1, d_x.ptr, 0, four, d_pos.ptr, None, d_y.ptr, 0), (r._h, 1, d_x.ptr, 0, four, d_pos.ptr, four, None, 0),
                     (r._h, 0, d_x.ptr, 0, four, d_pos.ptr, four, d_y.ptr, 0)):
            assert L.wc_warp_device(*args) < 0
            assert untouched()
        with pytest.raises(ValueError):
            warp.warp_device(r, d_x, [4, 4], d_pos, [4], d_y)
        assert lib().wc_synchronize() == 0 and untouched()
        assert L.wc_warp_device(r._h, 1, d_x.ptr, 0, four, d_pos.ptr, four, d_y.ptr, 0) == 0   # and the call itself goes through
        assert not np.array_equal(d_y.to_host()[:4].view(np.uint8), fill[:4].view(np.uint8)) and np.array_equal(d_y.to_host()[4:].view(np.uint8), fill[4:].view(np.uint8))
    finally:
        d_x.free()
        d_pos.free()
        d_y.free()
    assert all(np.array_equal(a, b) for a, b in zip(run_guarded(r, wide, poss), want))   # the handle is as it was
