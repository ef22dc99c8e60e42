"""GPU tests of the variable-ratio resample streams (include/world_class_vresample.h): three streams on one handle, each at a step of
its own, pushed in pieces of every kind, give bit for bit what the batch call gives on the whole signals, with the counts of
wc_vresample_committed; a stream whose step moves between pushes gives the rule at the positions that accumulate; refused pushes and
refused steps change nothing; and the chain the streams exist for -- a capture clock that is 20 ppm off, resampled into an analysis
stream -- equals the whole-signal chain."""
import numpy as np
import pytest

import vresample_rule as R
from world_class_amd import WorldClassError, vresample as vr

pytestmark = pytest.mark.gpu

ONE = R.ONE
MAX = 9000
LO, HI = 3 << 30, 1 << 33   # 4/3 down to 1/2
UPR = vr.step_of(48000 / 44100)
MASK = ONE - 1


def whole(xs, steps, out_format="f64", lo=LO, hi=HI):
    r = vr.VResampler(lo, hi)
    try:
        return r.run(xs, steps, out_format)
    finally:
        r.close()


def test_three_streams_are_the_batch_call_bit_for_bit():
    half = vr.plan(LO, HI)[0]
    rng = np.random.default_rng(44)
    sizes = [0, 1, half - 1, half, half + 1, 300, 8820, MAX]
    steps = [UPR, HI, ONE + 1]              # (stream 1 keeps the step every stream starts with: step_max)
    x0 = rng.uniform(-1, 1, 40000)          # stream 0: pushes of every size
    x1 = rng.uniform(-1, 1, 21000)          # stream 1: idle for whole pushes
    x2 = rng.uniform(-1, 1, half - 3)       # stream 2: fewer than K samples in all, then flushed with n_new = 0
    x2b = rng.uniform(-1, 1, 3 * half + 5)  # and after its reset a new signal
    s = vr.VResampleStream(LO, HI, 3, MAX)
    assert s.max_out_per_push == vr.out_length(LO, MAX + half)
    s.set_step(0, steps[0])
    s.set_step(2, steps[2])
    got = [[], [], [], []]  # (the last: stream 2 after its reset)
    at = [0, 0, 0]    # samples pushed
    pos = [0, 0, 0]   # the next output's position
    second_life = False

    def push(chunks, flush=None):
        before = [s.samples_received(u) for u in range(3)]
        done = [s.samples_committed(u) for u in range(3)]
        out = s.push(chunks, flush)
        for u in range(3):
            n = 0 if chunks[u] is None else len(chunks[u])
            assert s.samples_received(u) == before[u] + n
            now_flushed = flushed[u] or bool(flush and flush[u])
            want = vr.committed(pos[u] >> 32, pos[u] & MASK, steps[u], half, before[u] + n, now_flushed)
            assert len(out[u]) == want and s.samples_committed(u) == done[u] + want
            pos[u] += want * steps[u]
            flushed[u] = now_flushed
            got[3 if (u == 2 and second_life) else u].append(out[u])
        return out

    flushed = [False, False, False]
    step = 0
    try:
        while at[0] < len(x0) or at[1] < len(x1):
            n0 = min(int(rng.choice(sizes)), len(x0) - at[0])
            n1 = 0 if step % 3 else min(int(rng.choice(sizes)), len(x1) - at[1])
            if at[0] == len(x0):
                n1 = min(MAX, len(x1) - at[1])  # (stream 0 has ended: stream 1 finishes alone)
            c2 = None
            if step == 1:
                c2 = x2[:5]
            elif step == 2:
                c2 = x2[5:]
            if step == 4:
                push([None, None, None], [0, 0, 1])   # stream 2 ends with n_new = 0: its outputs are all zero tail
                # a push after the flush, a count above the maximum and a step outside the handle's range are refused, and nothing moves
                state = [(s.samples_received(u), s.samples_committed(u)) for u in range(3)]
                with pytest.raises(WorldClassError):
                    s.push([x0[at[0]:at[0] + 10], None, np.zeros(1)])
                with pytest.raises(WorldClassError):
                    s.push([np.zeros(MAX + 1), None, None])
                for bad in (LO - 1, HI + 1, 0, 1 << 28, 1 << 36, 1 << 64):
                    with pytest.raises(WorldClassError):
                        s.set_step(0, bad)
                with pytest.raises(WorldClassError):
                    s.set_step(3, ONE)
                assert state == [(s.samples_received(u), s.samples_committed(u)) for u in range(3)]
            if step == 6:
                s.reset(2)   # a new signal on stream 2 while the others go on: the position rewinds, the step stays
                flushed[2], second_life, pos[2] = False, True, 0
                c2 = x2b[:half + 1]
            elif step == 7:
                c2 = x2b[half + 1:]
            push([x0[at[0]:at[0] + n0], x1[at[1]:at[1] + n1], c2])
            at[0] += n0
            at[1] += n1
            step += 1
        assert step > 8
        push([None, None, None], [1, 1, 1])
        assert [len(p) for p in s.push([None, None, None])] == [0, 0, 0]  # a flushed stream commits nothing more
        want = whole([x0, x1, x2, x2b], steps + [steps[2]])
        for k in range(4):
            y = np.concatenate(got[k])
            assert len(y) == len(want[k]) and np.array_equal(y, want[k]), "signal %d" % k
        assert s.samples_committed(0) == vr.out_length(steps[0], len(x0)) and s.samples_received(2) == len(x2b)
        assert s.samples_received(3) == -1
        with pytest.raises(WorldClassError):
            s.reset(3)
    finally:
        s.close()


def test_a_step_that_moves_between_pushes_is_the_rule_at_the_accumulated_positions():
    """stream 0's step goes up, down, to step_min and to step_max between pushes, with refused steps and a refused push in between;
    its outputs are vresample_at at the positions that (position += count x step) gives, the counts the rule's own.  Stream 1 takes
    the same samples at a constant step and stays the batch call's"""
    half, _, _, _ = vr.plan(LO, HI)
    C = vr.filter_table(LO, HI)
    bits = R.DEFAULT[0]
    rng = np.random.default_rng(6)
    x = rng.uniform(-1, 1, 30000)
    # (samples, the step set in front of the push; None: the step stays)
    schedule = [(500, UPR), (3000, None), (0, HI), (137, None), (2000, ONE), (MAX, LO), (1, HI), (4000, vr.step_of(48000 / 44100 * 1.0003)),
                (half, LO + 777), (2500, HI - 1), (half + 1, ONE - 1), (3000, ONE + 1), (5000, LO)]
    assert sum(n for n, _ in schedule) <= len(x)
    s = vr.VResampleStream(LO, HI, 2, MAX)
    s.set_step(1, UPR)
    positions, parts, parts1 = [], [], []
    pos, at, step = 0, 0, HI
    try:
        for k, (n, new_step) in enumerate(schedule + [(len(x) - sum(n for n, _ in schedule), None)]):
            if new_step is not None:
                s.set_step(0, new_step)
                step = new_step
            if k == 5:
                with pytest.raises(WorldClassError):
                    s.set_step(0, HI + 1)
                with pytest.raises(WorldClassError):
                    s.push([np.zeros(MAX + 1), np.zeros(3)])
            last = at + n == len(x)
            out = s.push([x[at:at + n], x[at:at + n]], [last, last])
            at += n
            count = R.committed(pos >> 32, pos & MASK, step, half, at, last)
            assert len(out[0]) == count
            positions += R.positions(step, count, pos)
            pos += count * step
            parts.append(out[0])
            parts1.append(out[1])
        assert at == len(x) and positions[-1] >> 32 <= len(x) - 1 < pos >> 32   # the flush commits up to the last sample's outputs
        assert len(set(b - a for a, b in zip(positions[:-1], positions[1:]))) >= 5   # the spacing did move
    finally:
        s.close()
    y = np.concatenate(parts)
    want = R.vresample_at(x, positions, C, bits)
    assert len(y) == len(want) and np.array_equal(y, want), "%d of %d outputs differ, first at %d" % (int((y != want).sum()), len(y), int(np.argmax(y != want)))
    assert np.array_equal(np.concatenate(parts1), whole([x], UPR)[0])


def test_int16_in_and_int16_out_on_one_stream():
    rng = np.random.default_rng(2)
    x = rng.integers(-32768, 32768, 12000).astype(np.int16)
    s = vr.VResampleStream(LO, HI, 1, 4410)
    s.set_step(0, UPR)
    try:
        parts = [s.push([x[a:a + 4410]], [a + 4410 >= len(x)], out_format="i16")[0] for a in range(0, len(x), 4410)]
    finally:
        s.close()
    y = np.concatenate(parts)
    assert y.dtype == np.int16 and np.array_equal(y, whole([x], UPR, "i16")[0])


def test_float32_in_on_one_stream_through_the_segment_mapping():
    """float32 samples, the third input format a push widens: four pushes of 600 at step 2^32 + 1 on the default table, each of at
    least segment_min = 256 outputs, so the pushes take the segment mapping (the batch tests hold the plain one in float32)"""
    step = ONE + 1
    tile_outputs, segment_min, _ = vr.tiling(step, step)
    x = np.random.default_rng(3).uniform(-1, 1, 2400).astype(np.float32)
    s = vr.VResampleStream(step, step, 1, 600)
    try:
        parts = [s.push([x[a:a + 600]], [a + 600 >= len(x)])[0] for a in range(0, len(x), 600)]
    finally:
        s.close()
    assert tile_outputs > 0 and segment_min == 256 and len(parts) == 4 and all(len(p) >= segment_min for p in parts)
    y = np.concatenate(parts)
    assert y.dtype == np.float64 and np.array_equal(y, whole([x], step, lo=step, hi=step)[0])


def test_create_refusals():
    for args in ((LO, HI, 0, 100), (LO, HI, 1, 0), (HI, LO, 1, 100), ((1 << 28) - 1, HI, 1, 100)):
        with pytest.raises(WorldClassError):
            vr.VResampleStream(*args)
    with pytest.raises(WorldClassError) as e:   # max_out leaves 31 bits
        vr.VResampleStream(1 << 28, ONE, 1, 2 ** 28)
    assert "31 bits" in str(e.value)
    with pytest.raises(WorldClassError):
        vr.VResampleStream(LO, HI, 1, 100, phase_bits=9, degree=5)


def test_vresample_stream_into_analysis_stream_is_the_whole_signal_chain():
    """44.1 kHz from a device whose clock is 20 ppm off, in 200 ms pushes -> 24 kHz -> an analysis stream's fixed chunks: the samples
    are the whole call's bit for bit, so the frames are too"""
    from world_class_amd.stream import StreamAnalyzer
    from world_class_amd.synth import make_utterance
    fs_in, fs_out = 44100, 24000
    step = vr.step_of(fs_out / fs_in * 1.00002)
    x = make_utterance(fs_in, 1.3, 7)

    def analyze(pieces):
        """the 24 kHz samples as they arrive -> the analyzer's chunks (the last one, shorter, with the flush) -> all frames"""
        an = StreamAnalyzer(fs_out, 1, frame_period=5.0, chunk_ms=200, lookback_ms=400, lookahead_ms=400)
        cs, buf, res = an.chunk_samples, np.zeros(0), []
        for piece in pieces:
            buf = np.concatenate([buf, piece])
            while len(buf) > cs:
                res.append(an.push([buf[:cs]])[0])
                buf = buf[cs:]
        res.append(an.push([buf], [1])[0])
        return {k: np.concatenate([r[k] for r in res]) for k in ("tpos", "f0", "sp")}

    s = vr.VResampleStream(step, step, 1, 8820)
    try:
        pieces = [s.push([x[a:a + 8820]], [a + 8820 >= len(x)])[0] for a in range(0, len(x), 8820)]
    finally:
        s.close()
    y = whole([x], step, lo=step, hi=step)[0]
    assert len(y) == vr.out_length(step, len(x)) and np.array_equal(np.concatenate(pieces), y)
    streamed, direct = analyze(pieces), analyze([y])
    assert len(direct["f0"]) > 200 and (direct["f0"] > 0).any()
    for k in ("tpos", "f0", "sp"):
        assert np.array_equal(streamed[k], direct[k]), k
