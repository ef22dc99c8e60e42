"""GPU tests of the batch resampler (include/world_class_resample.h): wc_resample_device bit for bit against the rule in numpy
(tests/resample_rule.py) on the library's own table, at the ratios where the kernels take different paths and at the lengths where
they change mapping or tile, in every sample format, with guards behind the output."""
import numpy as np
import pytest

import resample_rule as R
from world_class_amd import DeviceArray, WorldClassError, io as wio, lib, resample as rs

pytestmark = pytest.mark.gpu

# (fs_in, fs_out, zeros)
CASES = [
    (44100, 48000, 0),
    (48000, 44100, 0),   # M = 160: the lane stride that needs the padded tile
    (48000, 24000, 0),   # L = 1
    (24000, 48000, 0),   # M = 1
    (8000, 44100, 0),    # L = 441
    (96000, 8000, 0),    # 1623 taps
    (44100, 48000, 1),   # K = 2
]
GUARD = 64
PATTERN = 0xA5A5A5A5A5A5A5A5


def lengths_of(fs_in, fs_out, zeros):
    """the ragged batch: lengths around the table's half width K, a long one, and the input lengths whose outputs straddle the kernels' own edges -- the first tile of
    the phase mapping, the length from which it is used, and one wavefront row of every phase (WAVE x L)"""
    up, down, half = rs.plan(fs_in, fs_out, zeros)
    tile_outputs, phase_min, plain_block = rs.tiling(fs_in, fs_out, zeros)
    ns = [1, 2, half, 2 * half, 2 * half + 1, 2 * half + 2, 7, 20011]
    for edge in (tile_outputs, phase_min, rs.WAVE * up, plain_block):
        if edge > 0:
            for t in (edge - 1, edge, edge + 1):
                ns += [max(1, t * down // up), t * down // up + 1]   # out_length of the two: the last count <= t and the first above
    return list(dict.fromkeys(ns))  # (each once, in this order)


def batch_of(ns, seed):
    """every utterance of the list between neighbours of amplitude 1e6: a read across an utterance's end shows"""
    rng = np.random.default_rng(seed)
    xs = [1e6 * rng.uniform(-1, 1, 300)]
    for n in ns:
        xs += [rng.uniform(-1, 1, n), 1e6 * rng.uniform(-1, 1, 300)]
    return xs


def run_guarded(r, xs, in_dtype=np.float64, in_format="f64", out_format="f64"):
    """wc_resample_device on a packed batch with d_y GUARD samples too long and pre-filled; the guard must come back untouched"""
    outs = [r.out_length(len(x)) for x in xs]
    total = sum(outs)
    odt = rs.OUT_FORMATS[out_format][1]
    fill = np.full(total + GUARD, PATTERN, dtype=np.uint64).view(np.float64) if odt == np.float64 else np.full(total + GUARD, 0x5A5A, dtype=np.int16)
    d_x = DeviceArray.from_host(np.concatenate(xs), dtype=in_dtype)
    d_y = DeviceArray.from_host(fill, dtype=odt)
    try:
        r.run_device(d_x, [len(x) for x in xs], d_y, in_format, out_format)
        y = d_y.to_host()
    finally:
        d_x.free()
        d_y.free()
    assert np.array_equal(y[total:].view(np.uint8), fill[total:].view(np.uint8)), "the guard behind the output was written"
    return np.split(y[:total], np.cumsum(outs)[:-1])


@pytest.mark.parametrize("fs_in,fs_out,zeros", CASES)
def test_batch_is_the_rule_bit_for_bit(fs_in, fs_out, zeros):
    up, down, half = rs.plan(fs_in, fs_out, zeros)
    G = rs.filter_taps(fs_in, fs_out, zeros)
    ns = lengths_of(fs_in, fs_out, zeros)
    tile_outputs, phase_min, _ = rs.tiling(fs_in, fs_out, zeros)
    outs = [rs.out_length(fs_in, fs_out, n) for n in ns]
    assert tile_outputs > 0 and min(outs) < phase_min <= max(outs) and max(outs) > tile_outputs  # both mappings, more than one tile
    xs = batch_of(ns, seed=fs_in + zeros)
    r = rs.Resampler(fs_in, fs_out, zeros)
    try:
        ys = run_guarded(r, xs)
    finally:
        r.close()
    for u, (x, y) in enumerate(zip(xs, ys)):
        want = R.resample(x, up, down, G)
        assert len(y) == len(want) == R.out_length(up, down, len(x))
        assert np.array_equal(y, want), "utterance %d (%d samples): %d of %d outputs differ, first at %d" % (
            u, len(x), int((y != want).sum()), len(y), int(np.argmax(y != want)))


def test_a_plan_without_a_tile_goes_output_by_output():
    """22.05 -> 16 kHz (M = 441): the input tile of one wavefront row would not fit the local memory"""
    conv = (22050, 16000)
    assert rs.tiling(*conv)[0] == 0
    up, down, half = rs.plan(*conv)
    G = rs.filter_taps(*conv)
    xs = batch_of([1, half, 2 * half + 1, 9001], seed=3)
    r = rs.Resampler(*conv)
    try:
        ys = run_guarded(r, xs)
    finally:
        r.close()
    for x, y in zip(xs, ys):
        assert np.array_equal(y, R.resample(x, up, down, G))


@pytest.fixture(scope="module")
def format_case():
    """a small batch on both mappings at 44.1 -> 48 kHz, in int16 (some samples at the ends of the range), and its double results"""
    conv = (44100, 48000)
    rng = np.random.default_rng(11)
    xs16 = [rng.integers(-32768, 32768, n).astype(np.int16) for n in (5, 137, 6000)]
    xs16[1][:4] = [-32768, 32767, 0, -1]
    r = rs.Resampler(*conv)
    wide = [x.astype(np.float64) / 32768.0 for x in xs16]
    yield r, xs16, wide, run_guarded(r, wide)
    r.close()


def test_int16_and_float32_inputs_are_the_double_call_on_the_widened_samples(format_case):
    r, xs16, wide, want = format_case
    got = run_guarded(r, xs16, np.int16, "i16")
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    xs32 = [(3.0 * x).astype(np.float32) for x in wide]
    got = run_guarded(r, xs32, np.float32, "f32")
    want32 = run_guarded(r, [x.astype(np.float64) for x in xs32])
    assert all(np.array_equal(a, b) for a, b in zip(got, want32))


def test_int16_output_is_double_to_pcm16_of_the_double_output(format_case):
    r, xs16, wide, _ = format_case
    loud = [1.7 * x for x in wide]  # (some outputs beyond the range: the clamp)
    y = np.concatenate(run_guarded(r, loud))
    d_y, d_p = DeviceArray.from_host(y), DeviceArray(len(y), dtype=np.int16)
    try:
        wio.double_to_pcm16_device(d_y, len(y), d_p)
        want = d_p.to_host()
    finally:
        d_y.free()
        d_p.free()
    got = np.concatenate(run_guarded(r, loud, out_format="i16"))
    assert got.dtype == np.int16 and np.array_equal(got, want)
    assert np.array_equal(want, R.pcm16(y)) and want.min() == -32768 and want.max() == 32767
    got = np.concatenate(run_guarded(r, xs16, np.int16, "i16", "i16"))
    assert np.array_equal(got, R.pcm16(np.concatenate(format_case[3])))


def test_run_on_host_arrays_returns_the_same(format_case):
    r, xs16, wide, want = format_case
    for xs in (wide, xs16, [x.astype(np.float32) for x in wide]):  # (an int16 sample over 32768 is exact in float32)
        got = r.run(xs)
        assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))
    got = r.run(xs16, out_format="i16")
    assert all(np.array_equal(a, R.pcm16(b)) for a, b in zip(got, want))


def test_batch_refusals(format_case):
    r, xs16, wide, want = format_case
    d = DeviceArray(16)
    try:
        for lengths in ([5, 0], [-1], []):
            with pytest.raises(WorldClassError):
                r.run_device(d, lengths, d)
        with pytest.raises(WorldClassError) as e:   # 2 x ceil((2^31 - 1) 160 / 147) outputs: refused on the host, nothing is enqueued
            r.run_device(d, [2 ** 31 - 1, 2 ** 31 - 1], d)
        assert "2^31" in str(e.value)
        for in_format, out_format in ((3, 0), (-1, 0), (0, 2)):
            assert rs._L().wc_resample_device(r._h, 1, d.ptr, in_format, rs._ints([4]), d.ptr, out_format) < 0
        with pytest.raises(WorldClassError):
            r.run_device(None, [4], d)
    finally:
        d.free()
    assert lib().wc_synchronize() == 0
    assert all(np.array_equal(a, b) for a, b in zip(run_guarded(r, wide), want))  # the handle is as it was
