"""GPU tests of the warp streams (include/world_class_warp_stream.h): 8 streams on 3 tracks of 14 400 samples, one handle with int16
tracks and one with double ones, maps of 40 entries.  For every cut into pushes, at every delay, flush included, a stream's
concatenated outputs are wc_warp_along_map_device's on its consumed entries, bit for bit, and samples_out are the rule's counts
(tests/warp_stream_rule.py); a NaN entry that is carried from one push to the next; two streams on one slot; a reset mid-way; every
refusal.  Every output buffer carries a guard pattern behind it."""
import ctypes as C
import math

import numpy as np
import pytest

import vresample_rule as R
import warp_stream_rule as S
from test_gpu_vresample import GUARD, PATTERN
from world_class_amd import DeviceArray, WorldClassError, last_error, lib, vresample as vr, warp, warp_stream as ws

pytestmark = pytest.mark.gpu

N, TRACKS, TRACK_LEN, ENTRIES, MAX_DELAY = 8, 3, 14400, 40, 3
PLANS = {"small_i16": (dict(step_min=R.ONE, step_max=1 << 33, zeros=4), "i16"), "default_f64": (dict(step_min=R.ONE, step_max=R.ONE), "f64")}
TRACK_OF = [0, 1, 2, 0, 1, 2, 0, 1]
OPE = [240.0, 220.5, 240.0, 240.0, 220.5, 80.0, 220.5, 240.0]   # (220.5: push boundaries fall between whole samples)
IPU = [240.0, 240.0, 220.5, 120.0, 240.0, 240.0, 200.0, 240.0]   # streams 0 and 3 share slot 0 at different in_per_unit


def make_maps():
    """d_b_on_a-like: half-integers onto 60 frames with flat runs and steps; one that falls; one that leaves the track"""
    rng = np.random.default_rng(77)
    maps = [np.minimum(np.cumsum(rng.choice([0.0, 0.5, 1.0, 1.5, 2.0, 3.0], size=ENTRIES)), 59.0) for _ in range(N)]
    maps[5] = maps[5][::-1].copy()
    maps[6] = maps[6] + 35.0
    return maps


MAPS = make_maps()   # made once and left unchanged


class Env:
    def __init__(self, name):
        plan, fmt = PLANS[name]
        self.fmt = fmt
        self.r = vr.VResampler(**plan)
        self.h = ws.WarpStream(plan["step_min"], plan["step_max"], N, TRACKS, TRACK_LEN, ENTRIES, MAX_DELAY, 240.0, track_format=fmt,
                               zeros=plan.get("zeros", 0))
        self.segment_min = warp.tiling(plan["step_min"], plan["step_max"], zeros=plan.get("zeros", 0))[2]
        rng = np.random.default_rng(len(name))
        self.tracks = [rng.integers(-32768, 32768, TRACK_LEN).astype(np.int16) if fmt == "i16" else rng.uniform(-1, 1, TRACK_LEN) for _ in range(TRACKS)]
        for t, x in enumerate(self.tracks):
            self.h.set_track(t, x)
        self.cap = N * self.h.max_out_per_push
        self._refs = {}

    def along_map(self, xs, maps, opes, ipus):
        """wc_warp_along_map_device for (a track, a map, out_length = c(entries)) each; one call per (out_per_entry, in_per_unit)"""
        out = []
        for x, m, ope, ipu in zip(xs, maps, opes, ipus):
            n = S.committed(len(m), ope)
            if n == 0:
                out.append(np.zeros(0))
                continue
            held = [DeviceArray.from_host(x, dtype=x.dtype), DeviceArray.from_host(np.asarray(m, dtype=np.float64)), DeviceArray(n)]
            try:
                ws.warp_along_map_device(self.r, held[0], [len(x)], held[1], [len(m)], ope, ipu, [n], held[2], self.fmt)
                out.append(held[2].to_host())
            finally:
                for d in held:
                    d.free()
        return out

    def refs(self, entries):
        """every stream's whole call on its first `entries` entries: computed once"""
        if entries not in self._refs:
            self._refs[entries] = self.along_map([self.tracks[t] for t in TRACK_OF], [m[:entries] for m in MAPS], OPE, IPU)
        return self._refs[entries]

    def close(self):
        self.h.close()
        self.r.close()


@pytest.fixture(scope="module")
def envs():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Env(name)
        return made[name]

    yield get
    for e in made.values():
        e.close()


def enqueue(env, call, slices, cap):
    """one push or flush: the streams' doubles packed, the outputs into a pre-filled buffer with a guard; per stream its outputs"""
    flat = np.array([float(v) for s in slices for v in s] + [0.0])
    fill = np.full(cap + GUARD, PATTERN, dtype=np.uint64).view(np.float64)
    d_in, d_y = DeviceArray.from_host(flat), DeviceArray.from_host(fill)
    try:
        counts = call(d_in, d_y)
        y = d_y.to_host()
    finally:
        d_in.free()
        d_y.free()
    total = sum(counts)
    assert total <= cap and np.array_equal(y[total:].view(np.uint8), fill[total:].view(np.uint8)), "an output beyond samples_out was written"
    return counts, np.split(y[:total], np.cumsum(counts)[:-1])


def drive(env, delays, pushes, maps=MAPS, opes=OPE, reset=True):
    """the maps as an alignment stream with these lags hands them over, pushes[k][u] rows of stream u in push k.  Returns (per
    stream the concatenated outputs, the tails, per push the outputs per stream)"""
    h = env.h
    if reset:
        for u in range(N):
            h.reset(u, TRACK_OF[u], delays[u], opes[u], IPU[u])
    handed = [S.settled_rows(maps[u], delays[u]) for u in range(N)]
    taken, got, per_push = [h.rows_received(u) for u in range(N)], [[] for _ in range(N)], []
    for counts in pushes:
        slices = [handed[u][0][taken[u]:taken[u] + c] for u, c in enumerate(counts)]
        before = [h.entries_consumed(u) for u in range(N)]
        out_counts, ys = enqueue(env, lambda d_in, d_y: h.push_device(counts, d_in, d_y), slices, env.cap)
        want = []
        for u, c in enumerate(counts):   # the rule's counts, from the counts alone
            consumed = S.push_split(taken[u], c, delays[u])[1]
            want.append(S.committed(before[u] + consumed, opes[u]) - S.committed(before[u], opes[u]))
            taken[u] += c
        assert out_counts == want
        for u, y in enumerate(ys):
            got[u].append(y)
        per_push.append(out_counts)
    assert [h.rows_received(u) for u in range(N)] == taken
    return [np.concatenate(g + [np.zeros(0)]) for g in got], [t for _, t in handed], per_push


def cuts(name):
    if name == "at_once":
        return [[ENTRIES] * N]
    if name == "one_each":   # 240 outputs and fewer: the plain group
        return [[1] * N] * ENTRIES
    if name == "tiled":      # two entries and more
        return [[k] * N for k in (2, 3, 5, 8, 22)]
    pattern, left, pushes = [1, 3, 0, 2, 5], [ENTRIES] * N, []   # pushes without rows for some streams, both groups in one launch
    while any(left):
        counts = [min(pattern[(len(pushes) + u) % 5], left[u]) for u in range(N)]
        left = [a - c for a, c in zip(left, counts)]
        pushes.append(counts)
    return pushes


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("cut", ["at_once", "one_each", "tiled", "mixed"])
@pytest.mark.parametrize("delay", [0, 1, 3])
@pytest.mark.parametrize("name", sorted(PLANS))
def test_every_cut_is_the_whole_call(name, delay, cut, envs):
    env, h = envs(name), envs(name).h
    pushes = cuts(cut)
    got, tails, per_push = drive(env, [delay] * N, pushes)
    consumed = ENTRIES - delay
    for u in range(N):
        assert same_bits(got[u], env.refs(consumed)[u]), (u, "pushes")
        assert (h.entries_consumed(u), h.samples_committed(u), h.get_delay(u)) == (consumed, S.committed(consumed, OPE[u]), delay)
    seen = [0] * N
    for counts, outs in zip(pushes, per_push):   # a push that ends inside the first `delay` rows forms nothing
        seen = [s + c for s, c in zip(seen, counts)]
        assert all(s > delay or n == 0 for s, n in zip(seen, outs))
    if cut == "mixed":   # both groups in one launch, and streams without rows beside them
        assert any(0 in counts and any(0 < n < env.segment_min for n in outs) and max(outs) >= env.segment_min for counts, outs in zip(pushes, per_push))
    if cut == "one_each":
        assert max(max(outs) for outs in per_push) < env.segment_min
    if delay == 0:
        return
    counts, ys = enqueue(env, lambda d_in, d_y: h.flush_device([1] * N, d_in, d_y), tails, N * h.max_out_per_flush)
    assert counts == [S.committed(ENTRIES, OPE[u]) - S.committed(consumed, OPE[u]) for u in range(N)]
    for u in range(N):
        assert same_bits(np.concatenate([got[u], ys[u]]), env.refs(ENTRIES)[u]), (u, "flush")
        assert (h.rows_received(u), h.entries_consumed(u), h.samples_committed(u)) == (ENTRIES, ENTRIES, S.committed(ENTRIES, OPE[u]))
    assert same_bits(env.refs(ENTRIES)[0][:len(got[0])], got[0])   # (the prefix property on the device)


def test_two_streams_on_one_slot_with_different_in_per_unit(envs):
    """streams 0 and 3 share slot 0 and out_per_entry; test_every_cut_is_the_whole_call holds each to its own whole call, and here
    those two whole calls differ by more than their maps: stream 3's map at stream 0's in_per_unit is another signal"""
    env = envs("small_i16")
    assert TRACK_OF[0] == TRACK_OF[3] and OPE[0] == OPE[3] and IPU[0] != IPU[3]
    other = env.along_map([env.tracks[0]], [MAPS[3]], [OPE[3]], [IPU[0]])[0]
    assert other.shape == env.refs(ENTRIES)[3].shape and not same_bits(other, env.refs(ENTRIES)[3])
    got, _, _ = drive(env, [0] * N, [[ENTRIES if u in (0, 3) else 0 for u in range(N)]])
    assert same_bits(got[0], env.refs(ENTRIES)[0]) and same_bits(got[3], env.refs(ENTRIES)[3]) and all(len(got[u]) == 0 for u in (1, 2, 4, 5, 6, 7))


@pytest.mark.parametrize("name", sorted(PLANS))
def test_a_nan_entry_that_is_carried(name, envs):
    """entry 4 is NaN and the last of its push: the outputs that read it are silence on both sides of the push boundary"""
    env = envs(name)
    maps = [m.copy() for m in MAPS]
    maps[0][4] = math.nan
    rest = [0] * (N - 1)
    got, _, per_push = drive(env, [0] * N, [[5] + rest, [ENTRIES - 5] + rest], maps=maps)
    assert OPE[0] == 240.0 and per_push[0][0] == 4 * 240 + 1 and per_push[1][0] == (ENTRIES - 5) * 240
    y = got[0]
    assert not y[3 * 240 + 1:5 * 240].view(np.uint64).any()                 # +0.0 from behind entry 3 up to entry 5, across the boundary at 961
    assert y[3 * 240] != 0.0 and y[5 * 240] != 0.0 and y[:3 * 240].any()    # and no other output is touched
    want = env.along_map([env.tracks[0]], [maps[0]], [OPE[0]], [IPU[0]])[0]
    assert same_bits(y, want)
    assert same_bits(y[5 * 240:], env.refs(ENTRIES)[0][5 * 240:])           # behind the hole the map is the unbroken one's
    assert all(len(g) == 0 for g in got[1:])


def test_a_reset_mid_way_restarts_at_the_first_output(envs):
    env, h = envs("default_f64"), envs("default_f64").h
    first = [[10] * N]
    got, _, _ = drive(env, [0] * N, first)
    h.reset(2, 1, 0, 220.5, 80.0)   # another slot, other parameters
    assert (h.rows_received(2), h.entries_consumed(2), h.samples_committed(2)) == (0, 0, 0)
    maps = list(MAPS)
    maps[2] = MAPS[4]
    opes = list(OPE)
    opes[2] = 220.5
    counts = [ENTRIES - 10] * N
    counts[2] = ENTRIES
    rest, _, _ = drive(env, [0] * N, [counts], maps=maps, opes=opes, reset=False)
    for u in range(N):
        if u != 2:
            assert same_bits(np.concatenate([got[u], rest[u]]), env.refs(ENTRIES)[u]), u
    assert same_bits(rest[2], env.along_map([env.tracks[1]], [MAPS[4]], [220.5], [80.0])[0])
    assert same_bits(got[2], env.refs(10)[2])


def test_refusals_leave_everything_as_it_was():
    L = ws._L()
    plan = dict(step_min=R.ONE, step_max=1 << 33, zeros=4)
    r = vr.VResampler(**plan)
    h = ws.WarpStream(R.ONE, 1 << 33, 3, 2, 2000, 8, 2, 100.0, zeros=4)
    rng = np.random.default_rng(19)
    x = rng.uniform(-1, 1, 2000)
    maps = [np.cumsum(rng.choice([0.5, 1.0, 2.0], size=8)), np.cumsum(rng.choice([0.5, 1.0, 2.0], size=8))]
    opes, ipus, delays = [100.0, 60.5], [50.0, 30.0], [0, 2]
    handed = [S.settled_rows(m, d) for m, d in zip(maps, delays)]
    cap = 3 * h.max_out_per_push
    fill = np.full(cap + GUARD, PATTERN, dtype=np.uint64).view(np.float64)
    d_x, d_in, d_y = DeviceArray.from_host(x), DeviceArray.from_host(np.zeros(64)), DeviceArray.from_host(fill)
    got = (C.c_int * 3)()
    ints = ws._ints
    state = lambda: [(h.rows_received(u), h.entries_consumed(u), h.samples_committed(u), h.get_delay(u)) for u in range(3)] + [h.track_length(0), h.track_length(1)]
    untouched = lambda: np.array_equal(d_y.to_host().view(np.uint8), fill.view(np.uint8))

    def refused(calls):
        before = state()
        for k, call in enumerate(calls):
            assert call() < 0, k
            assert state() == before and untouched(), k

    def push(counts, out):
        """a good push through buffers of its own"""
        assert counts[2] == 0
        flat = np.array([v for u in range(2) for v in handed[u][0][h.rows_received(u):h.rows_received(u) + counts[u]]] + [0.0])
        d_m, d_o = DeviceArray.from_host(flat), DeviceArray(cap)
        try:
            n = h.push_device(counts, d_m, d_o)
            y = d_o.to_host()
        finally:
            d_m.free()
            d_o.free()
        for u, part in enumerate(np.split(y[:sum(n)], np.cumsum(n)[:-1])):
            out[u].append(part)

    try:
        # ---- before anything is attached ----
        assert (h.track_length(0), h.track_length(1), h.track_length(2), h.track_length(-1)) == (0, 0, -1, -1)
        refused([lambda: L.wc_warp_stream_reset(h._h, 0, 0, 0, 100.0, 50.0),                       # a slot that has not been set
                 lambda: L.wc_warp_stream_push_device(h._h, ints([1, 0, 0]), d_in.ptr, d_y.ptr, 0, got),   # rows for a stream that is not attached
                 lambda: L.wc_warp_stream_set_track_device(h._h, 0, 0, d_x.ptr), lambda: L.wc_warp_stream_set_track_device(h._h, 0, 2001, d_x.ptr),
                 lambda: L.wc_warp_stream_set_track_device(h._h, 0, 2000, None), lambda: L.wc_warp_stream_set_track_device(h._h, -1, 2000, d_x.ptr),
                 lambda: L.wc_warp_stream_set_track_device(h._h, 2, 2000, d_x.ptr), lambda: L.wc_warp_stream_set_track_device(None, 0, 2000, d_x.ptr)])
        h.set_track_device(0, 2000, d_x)
        for u in range(2):
            h.reset(u, 0, delays[u], opes[u], ipus[u])
        out = [[], [], []]
        push([3, 3, 0], out)
        assert state()[:2] == [(3, 3, S.committed(3, 100.0), 0), (3, 1, S.committed(1, 60.5), 2)]
        # ---- with rows in two streams ----
        bad_reset = lambda *a: (lambda: L.wc_warp_stream_reset(h._h, *a))
        bad_push = lambda counts, m=d_in.ptr, y=d_y.ptr, fmt=0, out_=got, hh=h._h: (lambda: L.wc_warp_stream_push_device(hh, counts, m, y, fmt, out_))
        bad_flush = lambda want, t=d_in.ptr, y=d_y.ptr, fmt=0, out_=got, hh=h._h: (lambda: L.wc_warp_stream_flush_device(hh, want, t, y, fmt, out_))
        refused([bad_push(ints([1, 0, 0]), hh=None), bad_push(None), bad_push(ints([1, 0, 0]), out_=None),
                 bad_push(ints([-1, 0, 0])), bad_push(ints([0, 9, 0])), bad_push(ints([1, 1, 1])),     # a count out of range; a stream that is not attached
                 bad_push(ints([1, 0, 0]), m=None), bad_push(ints([0, 1, 0]), m=None), bad_push(ints([1, 0, 0]), y=None),
                 bad_push(ints([1, 0, 0]), fmt=2), bad_push(ints([1, 0, 0]), fmt=-1),
                 bad_reset(-1, 0, 0, 100.0, 50.0), bad_reset(3, 0, 0, 100.0, 50.0), bad_reset(0, -1, 0, 100.0, 50.0), bad_reset(0, 2, 0, 100.0, 50.0),
                 bad_reset(0, 1, 0, 100.0, 50.0),                                                       # slot 1 has not been set
                 bad_reset(0, 0, -1, 100.0, 50.0), bad_reset(0, 0, 3, 100.0, 50.0),
                 bad_reset(0, 0, 0, 0.0, 50.0), bad_reset(0, 0, 0, -1.0, 50.0), bad_reset(0, 0, 0, math.nan, 50.0), bad_reset(0, 0, 0, math.inf, 50.0),
                 bad_reset(0, 0, 0, 100.5, 50.0),                                                       # above max_out_per_entry
                 bad_reset(0, 0, 0, 100.0, 0.0), bad_reset(0, 0, 0, 100.0, -1.0), bad_reset(0, 0, 0, 100.0, math.nan), bad_reset(0, 0, 0, 100.0, math.inf),
                 lambda: L.wc_warp_stream_set_track_device(h._h, 0, 1000, d_x.ptr),                     # under attached streams that have rows
                 bad_flush(None), bad_flush(ints([0, 1, 0]), out_=None), bad_flush(ints([0, 1, 0]), hh=None),
                 bad_flush(ints([1, 0, 0])), bad_flush(ints([0, 0, 1])),                                # delay 0; not attached
                 bad_flush(ints([0, 1, 0]), t=None), bad_flush(ints([0, 1, 0]), y=None), bad_flush(ints([0, 1, 0]), fmt=2)])
        h.set_track_device(1, 1500, d_x)   # (a slot nobody is attached to may be set at any time)
        h.reset(2, 1, 1, 100.0, 50.0)
        refused([bad_flush(ints([0, 0, 1]))])                                                           # attached, a delay, but no rows
        assert h.push_device([0, 0, 0], None, None) == [0, 0, 0]   # no rows: nothing to read or to write
        with pytest.raises(WorldClassError) as e:
            h.push_device([9, 0, 0], d_in, d_y)
        assert "warp stream" in str(e.value)
        with pytest.raises(ValueError):
            h.push_device([1, 1], d_in, d_y)
        # ---- the next push and the flush are what they would have been ----
        push([5, 5, 0], out)
        tail = DeviceArray.from_host(np.array(handed[1][1]))
        d_o = DeviceArray(3 * h.max_out_per_flush)
        try:
            n = h.flush_device([0, 1, 0], tail, d_o)
            assert n == [0, S.committed(8, 60.5) - S.committed(6, 60.5), 0] and len(handed[1][1]) == 3
            out[1].append(d_o.to_host()[:n[1]])
        finally:
            tail.free()
            d_o.free()
        assert state()[:2] == [(8, 8, S.committed(8, 100.0), 0), (8, 8, S.committed(8, 60.5), 2)]
        refused([bad_push(ints([0, 1, 0])), bad_flush(ints([0, 1, 0]))])                                # the stream has ended
        for u in range(2):
            n = S.committed(8, opes[u])
            held = [DeviceArray.from_host(maps[u]), DeviceArray(n)]
            try:
                ws.warp_along_map_device(r, d_x, [2000], held[0], [8], opes[u], ipus[u], [n], held[1])
                assert same_bits(np.concatenate(out[u]), held[1].to_host()), u
            finally:
                for d in held:
                    d.free()
        h.reset(1, 0, 0, 60.5, 30.0)   # a reset revives an ended stream
        assert h.push_device([1, 1, 0], d_in, d_y)[1] == 1
        assert lib().wc_synchronize() == 0
    finally:
        for d in (d_x, d_in, d_y):
            d.free()
        h.close()
        r.close()


def test_create_refusals():
    L = ws._L()
    good = [R.ONE, 1 << 33, 4, 0.0, 0.0, 0, 0, 3, 2, 2000, 0, 8, 2, 100.0]
    names = ["step_min", "step_max", "zeros", "rolloff", "beta", "phase_bits", "degree", "n_streams", "n_tracks", "max_track_samples", "track_format",
             "max_entries_per_push", "max_delay", "max_out_per_entry"]
    for changed in (dict(step_min=(1 << 33) + 1), dict(degree=4), dict(n_streams=0), dict(n_tracks=0), dict(max_track_samples=0), dict(max_entries_per_push=0),
                    dict(max_delay=-1), dict(max_out_per_entry=0.0), dict(max_out_per_entry=math.nan), dict(max_out_per_entry=math.inf),
                    dict(track_format=3), dict(track_format=-1),
                    dict(max_entries_per_push=1 << 24, max_out_per_entry=240.0),                       # max_out_per_push leaves 31 bits
                    dict(n_streams=1 << 20, max_entries_per_push=1 << 10, max_out_per_entry=240.0),   # the packed output does
                    dict(max_delay=1 << 24, max_out_per_entry=240.0)):
        args = [changed.get(n, v) for n, v in zip(names, good)]
        assert not L.wc_warp_stream_create(*args), changed
        assert last_error()
    with pytest.raises(WorldClassError):
        ws.WarpStream(R.ONE, 1 << 33, 0, 2, 2000, 8, 2, 100.0, zeros=4)
    h = ws.WarpStream(R.ONE, 1 << 33, 3, 2, 2000, 8, 0, 100.0, zeros=4)   # max_delay 0: nothing can be flushed
    assert h.max_out_per_flush == 0 and h.max_out_per_push >= S.committed(9, 100.0) - S.committed(1, 100.0)
    h.close()
