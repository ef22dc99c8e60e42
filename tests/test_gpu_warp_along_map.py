"""GPU tests of wc_warp_along_map_device (include/world_class_warp_stream.h): bit for bit the chain wc_warp_map_positions_device ->
wc_warp_device, and the rule in Python (tests/warp_rule.py) on the short maps, on the two handles of tests/test_gpu_warp_map.py; a
batch with records in both groups, an utterance without outputs between its neighbours and outputs past the map's end; a map with one
jump across the whole signal (a far tile inside near ones); every sample format; every refusal.  Every output is guarded."""
import math

import numpy as np
import pytest

import vresample_rule as R
import warp_rule as W
from test_gpu_vresample import GUARD, PATTERN
from test_gpu_warp_map import hand_made_b_on_a
from test_warp_rule import MAPS
from world_class_amd import DeviceArray, WorldClassError, lib, vresample as vr, warp, warp_stream as ws

pytestmark = pytest.mark.gpu

PAIRS = [(240.0, 220.5), (220.5, 240.0), (80.0, 240.0)]
SHORT = ["one_entry", "two_entries", "nan_entry", "falling", "range_ends"]
NAMES = ["one_entry", "two_entries", "long", "nan_entry", "falling", "range_ends"]


class Handle:
    def __init__(self, **plan):
        self.r = vr.VResampler(**plan)
        self.C = vr.filter_table(**plan)
        self.half, segs, _, _ = vr.plan(**plan)
        self.bits = segs.bit_length() - 1
        self.tile, self.span_max, self.segment_min, _ = warp.tiling(plan["step_min"], plan["step_max"], zeros=plan.get("zeros", 0))


@pytest.fixture(scope="module")
def handles():
    """tiles of 2048 outputs; the default with tiles of 4096, K = 68 and segment_min 256"""
    hs = [Handle(step_min=R.ONE, step_max=1 << 33, zeros=4), Handle(step_min=R.ONE, step_max=R.ONE)]
    assert (hs[0].tile, hs[1].tile, hs[1].half, hs[1].segment_min) == (2048, 4096, 68, 256)
    yield hs
    for h in hs:
        h.r.close()


def guard_fill(total, out_format):
    if out_format == "f64":
        return np.full(total + GUARD, PATTERN, dtype=np.uint64).view(np.float64)
    return np.full(total + GUARD, 0x5A5A, dtype=np.int16)


def run(r, xs, maps, ope, ipu, outs, in_format="f64", out_format="f64", chain=False):
    """the fused call, or the chain of the two calls it replaces, on a packed batch with a guard behind the outputs"""
    total = sum(outs)
    fill = guard_fill(total, out_format)
    idt, odt = vr.IN_FORMATS[in_format][1], vr.OUT_FORMATS[out_format][1]
    held = [DeviceArray.from_host(np.concatenate(xs).astype(idt), dtype=idt), DeviceArray.from_host(np.concatenate(maps)),
            DeviceArray.from_host(fill, dtype=odt)]
    try:
        if chain:
            held.append(DeviceArray(max(total, 1), dtype=np.int64))
            warp.map_positions_device(r, held[1], [len(m) for m in maps], ope, ipu, outs, held[3])
            warp.warp_device(r, held[0], [len(x) for x in xs], held[3], outs, held[2], in_format, out_format)
        else:
            ws.warp_along_map_device(r, held[0], [len(x) for x in xs], held[1], [len(m) for m in maps], ope, ipu, outs, held[2], in_format, out_format)
        y = held[2].to_host()
    finally:
        for d in held:
            d.free()
    assert np.array_equal(y[total:].view(np.uint8), fill[total:].view(np.uint8)), "the guard behind the output was written"
    return np.split(y[:total], np.cumsum(outs)[:-1])


def same_bits(got, want):
    return len(got) == len(want) and all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, want))


def the_batch(ope):
    """the CPU test's maps and a hand-made d_b_on_a (40 entries onto 60 frames of 240 samples), each on a signal of its own; an
    utterance without outputs between its neighbours; out_lengths a few past the map's end, where the end is held"""
    rng = np.random.default_rng(97)
    maps = [MAPS[name][0] for name in NAMES] + [hand_made_b_on_a(40, 60, 1)]
    xs = [rng.uniform(-1, 1, n) for n in (3000, 700, 14400, 3001, 2999, 333, 60 * 240)]
    outs = [warp.map_out_length(len(m), ope) + 5 for m in maps]
    maps.insert(3, MAPS["long"][0])
    xs.insert(3, 1e6 * rng.uniform(-1, 1, 300))
    outs.insert(3, 0)
    return xs, maps, outs


@pytest.mark.parametrize("ope,ipu", PAIRS)
def test_the_batch_is_the_chain_and_the_rule(ope, ipu, handles):
    xs, maps, outs = the_batch(ope)
    for h in handles:
        assert outs[0] < h.segment_min <= outs[2] and outs[3] == 0 and outs[2] > h.tile   # the plain group, the tiled one, more than one tile
        got = run(h.r, xs, maps, ope, ipu, outs)
        assert same_bits(got, run(h.r, xs, maps, ope, ipu, outs, chain=True))
        for u, (x, m, n, y) in enumerate(zip(xs, maps, outs, got)):
            if len(m) <= 9:   # the rule in Python on the short maps
                assert np.array_equal(y, W.warp_at(x, W.map_positions(m, ope, ipu, n), h.C, h.bits)), u
        nan = NAMES.index("nan_entry") + 1
        hole = np.array([p == W.NO_POSITION for p in W.map_positions(maps[nan], ope, ipu, outs[nan])])
        assert hole.any() and not got[nan][hole].view(np.uint64).any() and got[nan][~hole].any()   # a NaN entry is silence, +0.0


def test_the_maps_of_the_cpu_test_at_their_own_parameters(handles):
    rng = np.random.default_rng(5)
    for h in handles:
        for name in SHORT + ["b_on_a_220_5", "range_ends_scaled"]:
            m, ope, ipu = MAPS[name]
            xs = [rng.uniform(-1, 1, 2500), rng.uniform(-1, 1, 17)]
            maps, outs = [m, m[:1]], [warp.map_out_length(len(m), ope) + 3, 7]
            got = run(h.r, xs, maps, ope, ipu, outs)
            assert same_bits(got, run(h.r, xs, maps, ope, ipu, outs, chain=True)), name
            for x, mm, n, y in zip(xs, maps, outs, got):
                assert np.array_equal(y, W.warp_at(x, W.map_positions(mm, ope, ipu, n), h.C, h.bits)), name


def test_one_jump_across_the_whole_signal(handles):
    """30 entries that walk through the first frames, then one step to the signal's far end: the tile that holds the step is a far
    tile, its neighbours are near ones"""
    rng = np.random.default_rng(13)
    hop = 240.0
    m = np.concatenate([np.arange(30.0), 1900.0 + np.arange(30.0)])
    x = rng.uniform(-1, 1, 1930 * 240)
    n_out = warp.map_out_length(len(m), hop)
    pos = warp.map_positions(m, hop, hop, n_out)
    for k, h in enumerate(handles):
        spans = [int(q.max() - q.min()) + 2 * h.half + 1 for q in (pos[i:i + h.tile] >> 32 for i in range(0, n_out, h.tile))]
        far = [s > h.span_max for s in spans]
        assert sum(far) == 1 and not far[0] and not far[-1] and len(spans) >= 3
        got = run(h.r, [x], [m], hop, hop, [n_out])
        assert same_bits(got, run(h.r, [x], [m], hop, hop, [n_out], chain=True))
        if k == 0:   # (K = 9: the rule in Python on every output)
            assert np.array_equal(got[0], W.warp_at(x, [int(p) for p in pos], h.C, h.bits))


@pytest.mark.parametrize("in_format", ["f64", "i16", "f32"])
@pytest.mark.parametrize("out_format", ["f64", "i16"])
def test_every_format_is_the_chain_in_that_format(in_format, out_format, handles):
    ope, ipu = PAIRS[0]
    xs, maps, outs = the_batch(ope)
    if in_format == "i16":
        xs = [np.random.default_rng(3 + len(x)).integers(-32768, 32768, len(x)).astype(np.int16) for x in xs]
    elif out_format == "i16":
        xs = [1.7 * x for x in xs]   # (some outputs beyond the range: the clamp)
    for h in handles:
        got = run(h.r, xs, maps, ope, ipu, outs, in_format, out_format)
        assert same_bits(got, run(h.r, xs, maps, ope, ipu, outs, in_format, out_format, chain=True))
        assert got[2].any() and got[0].dtype == vr.OUT_FORMATS[out_format][1]


def test_refusals_leave_the_output_untouched(handles):
    r = handles[0].r
    L = ws._L()
    fill = np.full(64, PATTERN, dtype=np.uint64).view(np.float64)
    d_x, d_map, d_y = DeviceArray.from_host(np.ones(64)), DeviceArray.from_host(np.arange(16.0)), DeviceArray.from_host(fill)
    untouched = lambda: np.array_equal(d_y.to_host().view(np.uint8), fill.view(np.uint8))
    four, i = ws._ints([4]), ws._ints
    good = (r._h, 1, d_x.ptr, 0, four, d_map.ptr, four, 2.0, 1.0, four, d_y.ptr, 0)

    def but(**changed):
        names = ["r", "n_utt", "d_x", "in_format", "x_length", "d_map", "map_length", "ope", "ipu", "out_length", "d_y", "out_format"]
        return tuple(changed.get(name, v) for name, v in zip(names, good))

    try:
        cases = [but(r=None), but(n_utt=0), but(n_utt=-1), but(d_x=None), but(x_length=None), but(d_map=None), but(map_length=None),
                 but(out_length=None), but(d_y=None),                                              # both calls' NULL arrays
                 but(x_length=i([0])), but(map_length=i([0])), but(map_length=i([-3])), but(out_length=i([-1])),
                 but(n_utt=2, x_length=i([4, 4]), map_length=i([4, 4]), out_length=i([2 ** 31 - 1, 1])),
                 but(n_utt=2, x_length=i([4, 0]), map_length=i([4, 4]), out_length=i([4, 4])),
                 but(n_utt=2, x_length=i([4, 4]), map_length=i([4, 0]), out_length=i([4, 4])),
                 but(in_format=3), but(in_format=-1), but(out_format=2), but(out_format=-1),
                 but(ope=0.0), but(ope=-2.0), but(ope=math.nan), but(ope=math.inf), but(ipu=0.0), but(ipu=-1.0), but(ipu=math.nan), but(ipu=math.inf)]
        for args in cases:
            assert L.wc_warp_along_map_device(*args) < 0
            assert untouched()
        with pytest.raises(WorldClassError) as e:
            ws.warp_along_map_device(r, d_x, [5, 5], d_map, [4, 4], 2.0, 1.0, [2 ** 31 - 1, 1], d_y)
        assert "2^31" in str(e.value)
        with pytest.raises(ValueError):
            ws.warp_along_map_device(r, d_x, [4, 4], d_map, [4], 2.0, 1.0, [4, 4], d_y)
        assert lib().wc_synchronize() == 0 and untouched()
        assert L.wc_warp_along_map_device(*good) == 0   # and a good call follows
        y = d_y.to_host()
        assert np.array_equal(y[4:].view(np.uint8), fill[4:].view(np.uint8))
        assert np.array_equal(y[:4], W.warp_at(np.ones(4), W.map_positions(np.arange(4.0), 2.0, 1.0, 4), handles[0].C, handles[0].bits))
    finally:
        for d in (d_x, d_map, d_y):
            d.free()
