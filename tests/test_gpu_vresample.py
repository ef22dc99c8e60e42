"""GPU tests of the variable-ratio batch resampler (include/world_class_vresample.h): wc_vresample_device bit for bit against the rule
in numpy (tests/vresample_rule.py) on the library's own table, at the steps where every output of a tile falls into one segment, at
the ends of the handle's range, at the lengths where the kernels change mapping or tile, in every sample format, with guards behind
the output; and against the rational converter where the step is an exact fraction."""
import numpy as np
import pytest

import vresample_rule as R
from world_class_amd import DeviceArray, WorldClassError, io as wio, lib, resample as rs, vresample as vr

pytestmark = pytest.mark.gpu

ONE = R.ONE
UPR = vr.step_of(48000 / 44100)
WIDE = (3 << 30, 1 << 33)      # 4/3 down to 1/2
NEAR_ONE = (UPR, ONE + 1)
# name -> (step_min, step_max, zeros, phase_bits, degree, the steps that run)
PLANS = {
    "default": WIDE + (0, 0, 0, [ONE, ONE + 1, ONE - 1, 3 << 30, 1 << 33, UPR]),   # (3 x 2^30 and 2^33 are step_min and step_max themselves)
    "one_segment": NEAR_ONE + (0, 0, 7, [UPR, ONE - 1, ONE, ONE + 1]),
    "256_segments": NEAR_ONE + (0, 8, 3, [UPR, ONE, ONE + 1]),   # the widest bucket array
    "zeros_1": WIDE + (1, 0, 0, [3 << 30, ONE + 1, 1 << 33]),      # K = 3
    "no_tile": (1 << 35, 1 << 36, 512, 0, 0, [1 << 35, 1 << 36]),  # 17293 taps, 16 inputs per output: the plain mapping alone
}
CASES = [(name, step) for name, p in PLANS.items() for step in p[5]]
GUARD = 64
PATTERN = 0xA5A5A5A5A5A5A5A5


def plan_args(name):
    lo, hi, zeros, bits, degree, _ = PLANS[name]
    return dict(step_min=lo, step_max=hi, zeros=zeros, phase_bits=bits, degree=degree)


@pytest.fixture(scope="module")
def tables():
    """name -> (the library's table, phase_bits, K), built once"""
    out = {}
    for name in PLANS:
        a = plan_args(name)
        half, segs, _, _ = vr.plan(**a)
        out[name] = (vr.filter_table(**a), segs.bit_length() - 1, half)
    return out


def lengths_of(name, step):
    """the ragged batch: lengths around the table's half width K, a long one, and the input lengths whose outputs straddle the
    kernels' own edges -- a tile of the segment mapping, the length from which it is used, and a block of the plain mapping"""
    a = plan_args(name)
    half = vr.plan(**a)[0]
    a.pop("step_min"), a.pop("step_max")
    tile_outputs, segment_min, plain_block = vr.tiling(*PLANS[name][:2], **a)
    ns = [1, 2, half, 2 * half, 2 * half + 1, 20011]
    for edge in (tile_outputs, segment_min, plain_block):
        if edge > 0:
            for t in (edge - 1, edge, edge + 1):
                n = t * step >> 32   # out_length(n) <= t < out_length(n + 1)
                ns += [max(1, n), n + 1]
    return list(dict.fromkeys(ns)), (tile_outputs, segment_min, plain_block)


def batch_of(ns, seed):
    """every utterance of the list between neighbours of amplitude 1e6: a read across an utterance's end shows"""
    rng = np.random.default_rng(seed)
    xs = [1e6 * rng.uniform(-1, 1, 300)]
    for n in ns:
        xs += [rng.uniform(-1, 1, n), 1e6 * rng.uniform(-1, 1, 300)]
    return xs


def run_guarded(r, xs, steps, in_dtype=np.float64, in_format="f64", out_format="f64"):
    """wc_vresample_device on a packed batch with d_y GUARD samples too long and pre-filled; the guard must come back untouched"""
    steps = [steps] * len(xs) if isinstance(steps, int) else steps
    outs = [vr.out_length(s, len(x)) for s, x in zip(steps, xs)]
    total = sum(outs)
    odt = vr.OUT_FORMATS[out_format][1]
    fill = np.full(total + GUARD, PATTERN, dtype=np.uint64).view(np.float64) if odt == np.float64 else np.full(total + GUARD, 0x5A5A, dtype=np.int16)
    d_x = DeviceArray.from_host(np.concatenate(xs), dtype=in_dtype)
    d_y = DeviceArray.from_host(fill, dtype=odt)
    try:
        r.run_device(d_x, [len(x) for x in xs], steps, d_y, in_format, out_format)
        y = d_y.to_host()
    finally:
        d_x.free()
        d_y.free()
    assert np.array_equal(y[total:].view(np.uint8), fill[total:].view(np.uint8)), "the guard behind the output was written"
    return np.split(y[:total], np.cumsum(outs)[:-1])


def check(xs, ys, steps, C, bits):
    for u, (x, y, step) in enumerate(zip(xs, ys, steps)):
        want = R.vresample(x, step, C, bits)
        assert len(y) == len(want) == R.out_length(step, len(x))
        assert np.array_equal(y, want), "utterance %d (%d samples, step %d): %d of %d outputs differ, first at %d" % (
            u, len(x), step, int((y != want).sum()), len(y), int(np.argmax(y != want)))


@pytest.mark.parametrize("name,step", CASES)
def test_batch_is_the_rule_bit_for_bit(name, step, tables):
    C, bits, half = tables[name]
    ns, (tile_outputs, segment_min, _) = lengths_of(name, step)
    if name == "no_tile":
        assert tile_outputs == 0
        ns = [n for n in ns if n != 20011] + [1500 * step >> 32]   # (1500 outputs of 17293 taps are long enough here)
    outs = [vr.out_length(step, n) for n in ns]
    if tile_outputs:
        assert min(outs) < segment_min <= max(outs) and max(outs) > tile_outputs  # both mappings, more than one tile
    xs = batch_of(ns, seed=step % 1000 + len(name))
    r = vr.VResampler(**plan_args(name))
    try:
        ys = run_guarded(r, xs, step)
    finally:
        r.close()
    check(xs, ys, [step] * len(xs), C, bits)


def test_a_step_of_its_own_per_utterance(tables):
    C, bits, half = tables["default"]
    steps = PLANS["default"][5] + [WIDE[0] + 12345, WIDE[1] - 1, vr.step_of(48000 / 44100 * 1.0003)]
    ns = [1, 2 * half + 1, 700, 6000]
    rng = np.random.default_rng(8)
    xs, each = [], []
    for n in ns:
        for step in steps:
            xs.append(rng.uniform(-1, 1, n) * (1.0 if len(xs) % 2 else 1e6))
            each.append(step)
    r = vr.VResampler(**plan_args("default"))
    try:
        ys = run_guarded(r, xs, each)
        again = r.run(xs, each)
    finally:
        r.close()
    check(xs, ys, each, C, bits)
    assert all(np.array_equal(a, b) for a, b in zip(again, ys))


@pytest.fixture(scope="module")
def format_case():
    """a small batch on both mappings at two steps, in int16 (some samples at the ends of the range), and its double results"""
    rng = np.random.default_rng(11)
    xs16 = [rng.integers(-32768, 32768, n).astype(np.int16) for n in (5, 137, 6000)]
    xs16[1][:4] = [-32768, 32767, 0, -1]
    steps = [UPR, ONE + 1, vr.step_of(48000 / 44100 * 1.0003)]
    r = vr.VResampler(**plan_args("default"))
    wide = [x.astype(np.float64) / 32768.0 for x in xs16]
    yield r, xs16, wide, steps, run_guarded(r, wide, steps)
    r.close()


def test_int16_and_float32_inputs_are_the_double_call_on_the_widened_samples(format_case):
    r, xs16, wide, steps, want = format_case
    got = run_guarded(r, xs16, steps, np.int16, "i16")
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    xs32 = [(3.0 * x).astype(np.float32) for x in wide]
    got = run_guarded(r, xs32, steps, np.float32, "f32")
    want32 = run_guarded(r, [x.astype(np.float64) for x in xs32], steps)
    assert all(np.array_equal(a, b) for a, b in zip(got, want32))


def test_int16_output_is_double_to_pcm16_of_the_double_output(format_case):
    r, xs16, wide, steps, _ = format_case
    loud = [1.7 * x for x in wide]  # (some outputs beyond the range: the clamp)
    y = np.concatenate(run_guarded(r, loud, steps))
    d_y, d_p = DeviceArray.from_host(y), DeviceArray(len(y), dtype=np.int16)
    try:
        wio.double_to_pcm16_device(d_y, len(y), d_p)
        want = d_p.to_host()
    finally:
        d_y.free()
        d_p.free()
    got = np.concatenate(run_guarded(r, loud, steps, out_format="i16"))
    assert got.dtype == np.int16 and np.array_equal(got, want)
    assert np.array_equal(want, R.pcm16(y)) and want.min() == -32768 and want.max() == 32767
    got = np.concatenate(run_guarded(r, xs16, steps, np.int16, "i16", "i16"))
    assert np.array_equal(got, R.pcm16(np.concatenate(format_case[4])))


def test_run_on_host_arrays_returns_the_same(format_case):
    r, xs16, wide, steps, want = format_case
    for xs in (wide, xs16, [x.astype(np.float32) for x in wide]):  # (an int16 sample over 32768 is exact in float32)
        got = r.run(xs, steps)
        assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))
    got = r.run(xs16, steps, out_format="i16")
    assert all(np.array_equal(a, R.pcm16(b)) for a, b in zip(got, want))
    one = r.run(wide, UPR)   # (one step for all)
    assert np.array_equal(one[0], want[0]) and len(one[2]) == vr.out_length(UPR, 6000)


def test_batch_refusals(format_case):
    r, xs16, wide, steps, want = format_case
    d = DeviceArray(16)
    try:
        for lengths in ([5, 0], [-1], []):
            with pytest.raises(WorldClassError):
                r.run_device(d, lengths, [ONE] * len(lengths), d)
        with pytest.raises(WorldClassError) as e:   # 2 x ceil((2^31 - 1) 4 / 3) outputs: refused on the host, nothing is enqueued
            r.run_device(d, [2 ** 31 - 1, 2 ** 31 - 1], [3 << 30, 3 << 30], d)
        assert "2^31" in str(e.value)
        for step in (WIDE[0] - 1, WIDE[1] + 1, 0, 1 << 28, 1 << 36):   # outside the handle's range, inside the rule's or not
            with pytest.raises(WorldClassError) as e:
                r.run_device(d, [4, 4], [ONE, step], d)
            assert "step" in str(e.value)
        u64 = vr._u64
        for in_format, out_format in ((3, 0), (-1, 0), (0, 2)):
            assert vr._L().wc_vresample_device(r._h, 1, d.ptr, in_format, vr._ints([4]), (u64 * 1)(ONE), d.ptr, out_format) < 0
        assert vr._L().wc_vresample_device(r._h, 1, d.ptr, 0, vr._ints([4]), None, d.ptr, 0) < 0
        with pytest.raises(WorldClassError):
            r.run_device(None, [4], [ONE], d)
    finally:
        d.free()
    assert lib().wc_synchronize() == 0
    assert all(np.array_equal(a, b) for a, b in zip(run_guarded(r, wide, steps), want))  # the handle is as it was


# (fs_in, fs_out) -> the step that is exact in 2^-32
RATIONAL = {(24000, 48000): 1 << 31, (48000, 24000): 1 << 33, (36000, 48000): 3 << 30, (40000, 32000): 5 << 30}


@pytest.mark.parametrize("conv", sorted(RATIONAL))
def test_the_rational_converter_agrees_within_the_tables_error(conv):
    """with step_max the step itself, s and K are the rational plan's and output n sits at the same place, so the two differ by the
    table's error and the rounding of two summations: |y_v - y_r| <= max|x| (S + 64 taps 2^-53), S the worst sum over a phase's taps
    of the library's polynomials' errors against the exact prototype -- at the phases this ratio visits and at 2048 random ones"""
    step = RATIONAL[conv]
    up, down, half = rs.plan(*conv)
    assert step * up == down << 32 and vr.plan(step, step)[0] == half
    C = vr.filter_table(step, step)
    bits = R.DEFAULT[0]
    rng = np.random.default_rng(conv[0])
    visited = [(p << 32) // up for p in range(up)]
    _, S = R.table_error(C, step, bits, np.concatenate([rng.integers(0, ONE, 2048), visited]))
    x = rng.uniform(-1, 1, 9000)
    v, r = vr.VResampler(step, step), rs.Resampler(*conv)
    try:
        y_v, y_r = v.run([x], step)[0], r.run([x])[0]
    finally:
        v.close()
        r.close()
    bound = np.abs(x).max() * (S + 64 * (2 * half + 1) * 2.0 ** -53)
    diff = np.abs(y_v - y_r).max()
    print("%s: S %.2e, bound %.2e, max |y_v - y_r| %.2e" % (conv, S, bound, diff))
    assert len(y_v) == len(y_r) == rs.out_length(*conv, len(x)) and diff <= bound
