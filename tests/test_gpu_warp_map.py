"""GPU tests of wc_warp_map_positions_device (include/world_class_warp.h): the map rule on the device equals the host function, and so
the rule in Python (tests/warp_rule.py), on the CPU test's maps, with guards behind the positions; and the chain map -> positions ->
warp stays on the device and equals the rule at the rule's positions bit for bit."""
import numpy as np
import pytest

import vresample_rule as R
import warp_rule as W
from test_gpu_vresample import PATTERN
from test_warp_rule import MAPS
from world_class_amd import DeviceArray, WorldClassError, lib, vresample as vr, warp

pytestmark = pytest.mark.gpu

GUARD = 64
GUARD_FILL = np.int64(0x5A5A5A5A5A5A5A5A)


@pytest.fixture(scope="module")
def handles():
    """a handle with tiles of 2048 outputs and one with tiles of 4096: the map kernel counts a long map's blocks in tiles"""
    hs = [vr.VResampler(R.ONE, 1 << 33, zeros=4), vr.VResampler(R.ONE, R.ONE)]
    yield hs
    for h in hs:
        h.close()


def run_guarded(r, maps, ope, ipu, outs):
    total = sum(outs)
    fill = np.full(total + GUARD, GUARD_FILL, dtype=np.int64)
    d_map = DeviceArray.from_host(np.concatenate(maps))
    d_pos = DeviceArray.from_host(fill, dtype=np.int64)
    try:
        warp.map_positions_device(r, d_map, [len(m) for m in maps], ope, ipu, outs, d_pos)
        pos = d_pos.to_host()
    finally:
        d_map.free()
        d_pos.free()
    assert np.array_equal(pos[total:], fill[total:]), "the guard behind the positions was written"
    return np.split(pos[:total], np.cumsum(outs)[:-1])


def check(maps, ope, ipu, outs, got):
    for m, n, pos in zip(maps, outs, got):
        host = warp.map_positions(m, ope, ipu, n)
        assert len(pos) == n and np.array_equal(pos, host)
        assert [int(v) for v in pos] == W.map_positions(m, ope, ipu, n)


@pytest.mark.parametrize("ope,ipu", [(240.0, 220.5), (220.5, 240.0), (80.0, 240.0)])
def test_three_maps_are_the_host_function_and_the_rule(ope, ipu, handles):
    maps = [MAPS["one_entry"][0], MAPS["two_entries"][0], MAPS["long"][0]]
    assert [len(m) for m in maps] == [1, 2, 257]
    outs = [warp.map_out_length(len(m), ope) + 5 for m in maps]   # (past the last entry: the end is held)
    for r in handles:
        segment_min = warp.tiling(r.step_min, r.step_max, zeros=4 if r is handles[0] else 0)[2]
        assert outs[1] < segment_min <= outs[2]   # the plain group of records and the tiled one
        check(maps, ope, ipu, outs, run_guarded(r, maps, ope, ipu, outs))


def test_special_entries_empty_outputs_and_every_other_map(handles):
    r = handles[0]
    for name in ("nan_entry", "range_ends", "range_ends_scaled", "falling", "b_on_a_240"):
        m, ope, ipu = MAPS[name]
        maps = [m, MAPS["long"][0], m[:1], m]
        outs = [warp.map_out_length(len(m), ope) + 3, 0, 7, 1]   # (a map without outputs between its neighbours)
        got = run_guarded(r, maps, ope, ipu, outs)
        check(maps, ope, ipu, outs, got)
    m, ope, ipu = MAPS["nan_entry"]
    pos = run_guarded(r, [m], ope, ipu, [warp.map_out_length(len(m), ope)])[0]
    assert (pos == warp.NO_POSITION).sum() == 2 * 240 - 1 and pos[3 * 240] != warp.NO_POSITION != pos[5 * 240]


def test_refusals_leave_the_positions_untouched(handles):
    r = handles[0]
    L = warp._L()
    fill = np.full(64, GUARD_FILL, dtype=np.int64)
    d_map, d_pos = DeviceArray.from_host(np.arange(16.0)), DeviceArray.from_host(fill, dtype=np.int64)
    four = warp._ints([4])
    try:
        for args in ((None, 1, d_map.ptr, four, 2.0, 1.0, four, d_pos.ptr), (r._h, 0, d_map.ptr, four, 2.0, 1.0, four, d_pos.ptr),
                     (r._h, 1, None, four, 2.0, 1.0, four, d_pos.ptr), (r._h, 1, d_map.ptr, None, 2.0, 1.0, four, d_pos.ptr),
                     (r._h, 1, d_map.ptr, four, 2.0, 1.0, None, d_pos.ptr), (r._h, 1, d_map.ptr, four, 2.0, 1.0, four, None),
                     (r._h, 1, d_map.ptr, warp._ints([0]), 2.0, 1.0, four, d_pos.ptr), (r._h, 1, d_map.ptr, four, 2.0, 1.0, warp._ints([-1]), d_pos.ptr),
                     (r._h, 2, d_map.ptr, warp._ints([4, 4]), 2.0, 1.0, warp._ints([2 ** 31 - 1, 1]), d_pos.ptr),
                     (r._h, 1, d_map.ptr, four, 0.0, 1.0, four, d_pos.ptr), (r._h, 1, d_map.ptr, four, float("nan"), 1.0, four, d_pos.ptr),
                     (r._h, 1, d_map.ptr, four, 2.0, float("inf"), four, d_pos.ptr), (r._h, 1, d_map.ptr, four, 2.0, -1.0, four, d_pos.ptr)):
            assert L.wc_warp_map_positions_device(*args) < 0
            assert np.array_equal(d_pos.to_host(), fill)
        with pytest.raises(WorldClassError):
            warp.map_positions_device(r, d_map, [4], 2.0, 0.0, [4], d_pos)
        assert lib().wc_synchronize() == 0
        warp.map_positions_device(r, d_map, [4], 2.0, 1.0, [4], d_pos)
        assert [int(v) for v in d_pos.to_host()[:5]] == W.map_positions(np.arange(4.0), 2.0, 1.0, 4) + [int(GUARD_FILL)]
    finally:
        d_map.free()
        d_pos.free()


def hand_made_b_on_a(frames_a, frames_b, seed):
    """a time map as wc_align_features_device writes it: half-integer, non-decreasing, flat runs and steps of 2, from B's first frame
    to its last"""
    rng = np.random.default_rng(seed)
    m = np.cumsum(rng.choice([0.0, 1.0, 1.5, 2.0, 3.0], size=frames_a))
    m = np.round(m * (frames_b - 1) / m[-1] * 2) / 2
    assert m[-1] == frames_b - 1 and (np.diff(m) >= 0).all() and (np.diff(m) == 0).any() and (np.diff(m) >= 2).any()
    return m


def test_map_to_positions_to_warp_on_the_device(handles):
    """B's 60 frames of 240 samples on A's 40 frames: nothing comes back to the host between the two calls"""
    r = handles[1]
    C_, bits = vr.filter_table(R.ONE, R.ONE), R.DEFAULT[0]
    hop, frames_a, frames_b = 240.0, 40, 60
    rng = np.random.default_rng(41)
    b = rng.uniform(-1, 1, frames_b * int(hop))
    maps = [hand_made_b_on_a(frames_a, frames_b, 1), np.arange(float(frames_a))]
    xs = [b, b[:frames_a * int(hop)]]
    outs = [warp.map_out_length(frames_a, hop)] * 2
    assert outs[0] == (frames_a - 1) * int(hop) + 1
    total = sum(outs)
    fill = np.full(total + GUARD, PATTERN, dtype=np.uint64).view(np.float64)
    d_map, d_x = DeviceArray.from_host(np.concatenate(maps)), DeviceArray.from_host(np.concatenate(xs))
    d_pos, d_y = DeviceArray(total, dtype=np.int64), DeviceArray.from_host(fill)
    try:
        warp.map_positions_device(r, d_map, [frames_a] * 2, hop, hop, outs, d_pos)
        warp.warp_device(r, d_x, [len(x) for x in xs], d_pos, outs, d_y)
        y, pos = d_y.to_host(), d_pos.to_host()
    finally:
        for d in (d_map, d_x, d_pos, d_y):
            d.free()
    assert np.array_equal(y[total:].view(np.uint8), fill[total:].view(np.uint8))
    for u, (m, x) in enumerate(zip(maps, xs)):
        want = W.map_positions(m, hop, hop, outs[u])
        assert [int(v) for v in pos[u * outs[0]:(u + 1) * outs[0]]] == want
        assert np.array_equal(y[u * outs[0]:(u + 1) * outs[0]], W.warp_at(x, want, C_, bits))
    # the identity map: positions n 2^32 wherever (n / hop) x hop rounds back to n -- at a hop of 240 within one unit of 2^-32
    # below it, at 80 and at every power of two exactly
    ident = pos[outs[0]:].astype(object) - np.arange(outs[0]).astype(object) * R.ONE
    assert set(ident) <= {0, -1}
    same = run_guarded(r, [np.arange(float(frames_a))], 80.0, 80.0, [warp.map_out_length(frames_a, 80.0)])[0]
    assert np.array_equal(same, np.arange(len(same), dtype=np.int64) << 32)
    assert np.array_equal(warp.warp(r, [b], [same])[0], r.run([b], R.ONE)[0][:len(same)])   # and there the warp is the converter at ratio 1
