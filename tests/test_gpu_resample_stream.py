"""GPU tests of the resample streams (include/world_class_resample.h): three streams on one handle, pushed in pieces of every kind,
give bit for bit what the batch call gives on the whole signals, with the counts of wc_resample_committed; refused pushes change
nothing; and the chain the streams exist for -- resample stream into an analysis stream -- equals the whole-signal chain."""
import numpy as np
import pytest

from world_class_amd import WorldClassError, resample as rs

pytestmark = pytest.mark.gpu

MAX = 9000


def whole(conv, xs, out_format="f64"):
    r = rs.Resampler(*conv)
    try:
        return r.run(xs, out_format)
    finally:
        r.close()


@pytest.mark.parametrize("conv", [(44100, 48000), (48000, 24000)])
def test_three_streams_are_the_batch_call_bit_for_bit(conv):
    up, down, half = rs.plan(*conv)
    rng = np.random.default_rng(conv[0])
    sizes = [0, 1, half - 1, half, half + 1, 147, 8820, MAX]
    x0 = rng.uniform(-1, 1, 40000)          # stream 0: pushes of every size
    x1 = rng.uniform(-1, 1, 21000)          # stream 1: idle for whole pushes
    x2 = rng.uniform(-1, 1, half - 3)       # stream 2: fewer than K samples in all, then flushed with n_new = 0
    x2b = rng.uniform(-1, 1, 3 * half + 5)  # and after its reset a new signal
    s = rs.ResampleStream(*conv, 3, MAX)
    assert s.max_out_per_push == rs.out_length(*conv, MAX + half)
    got = [[], [], [], []]  # (the last: stream 2 after its reset)
    pos = [0, 0, 0]
    second_life = False

    def push(chunks, flush=None):
        before = [s.samples_received(u) for u in range(3)]
        was_flushed = list(flushed)
        out = s.push(chunks, flush)
        for u in range(3):
            n = 0 if chunks[u] is None else len(chunks[u])
            assert s.samples_received(u) == before[u] + n
            now_flushed = was_flushed[u] or bool(flush and flush[u])
            want = rs.committed(*conv, before[u] + n, now_flushed) - rs.committed(*conv, before[u], was_flushed[u])
            assert len(out[u]) == want and s.samples_committed(u) == rs.committed(*conv, before[u] + n, now_flushed)
            flushed[u] = now_flushed
            got[3 if (u == 2 and second_life) else u].append(out[u])
        return out

    flushed = [False, False, False]
    step = 0
    try:
        while pos[0] < len(x0) or pos[1] < len(x1):
            n0 = min(int(rng.choice(sizes)), len(x0) - pos[0])
            n1 = 0 if step % 3 else min(int(rng.choice(sizes)), len(x1) - pos[1])
            if pos[0] == len(x0):
                n1 = min(MAX, len(x1) - pos[1])  # (stream 0 has ended: stream 1 finishes alone)
            c2 = None
            if step == 1:
                c2 = x2[:5]
            elif step == 2:
                c2 = x2[5:]
            if step == 4:
                push([None, None, None], [0, 0, 1])   # stream 2 ends with n_new = 0: its outputs are all zero tail
                # a push after the flush and a count above the maximum are refused, and nothing moves
                state = [(s.samples_received(u), s.samples_committed(u)) for u in range(3)]
                with pytest.raises(WorldClassError):
                    s.push([x0[pos[0]:pos[0] + 10], None, np.zeros(1)])
                with pytest.raises(WorldClassError):
                    s.push([np.zeros(MAX + 1), None, None])
                assert state == [(s.samples_received(u), s.samples_committed(u)) for u in range(3)]
            if step == 6:
                s.reset(2)   # a new signal on stream 2 while the others go on
                flushed[2], second_life = False, True
                c2 = x2b[:half + 1]
            elif step == 7:
                c2 = x2b[half + 1:]
            push([x0[pos[0]:pos[0] + n0], x1[pos[1]:pos[1] + n1], c2])
            pos[0] += n0
            pos[1] += n1
            step += 1
        assert step > 8
        push([None, None, None], [1, 1, 1])
        assert [len(p) for p in s.push([None, None, None])] == [0, 0, 0]  # a flushed stream commits nothing more
        want = whole(conv, [x0, x1, x2, x2b])
        for k in range(4):
            y = np.concatenate(got[k])
            assert len(y) == len(want[k]) and np.array_equal(y, want[k]), "signal %d" % k
        assert s.samples_committed(0) == rs.out_length(*conv, len(x0)) and s.samples_received(2) == len(x2b)
        assert s.samples_received(3) == -1
        with pytest.raises(WorldClassError):
            s.reset(3)
    finally:
        s.close()


def test_int16_in_and_int16_out_on_one_stream():
    conv = (44100, 48000)
    rng = np.random.default_rng(2)
    x = rng.integers(-32768, 32768, 12000).astype(np.int16)
    s = rs.ResampleStream(*conv, 1, 4410)
    try:
        parts = [s.push([x[a:a + 4410]], [a + 4410 >= len(x)], out_format="i16")[0] for a in range(0, len(x), 4410)]
    finally:
        s.close()
    y = np.concatenate(parts)
    assert y.dtype == np.int16 and np.array_equal(y, whole(conv, [x], "i16")[0])


def test_float32_in_on_one_stream_through_the_phase_mapping():
    """float32 samples, the third input format a push widens: four pushes of 400 at 48 -> 24 kHz (L = 1, K = 136), each of at least
    phase_min = 32 outputs, so the pushes take the phase mapping (the batch tests hold the plain one in float32)"""
    conv = (48000, 24000)
    tile_outputs, phase_min, _ = rs.tiling(*conv)
    x = np.random.default_rng(3).uniform(-1, 1, 1600).astype(np.float32)
    s = rs.ResampleStream(*conv, 1, 400)
    try:
        parts = [s.push([x[a:a + 400]], [a + 400 >= len(x)])[0] for a in range(0, len(x), 400)]
    finally:
        s.close()
    assert tile_outputs > 0 and phase_min == 32 and len(parts) == 4 and all(len(p) >= phase_min for p in parts)
    y = np.concatenate(parts)
    assert y.dtype == np.float64 and np.array_equal(y, whole(conv, [x])[0])


def test_create_refusals():
    for args in ((44100, 48000, 0, 100), (44100, 48000, 1, 0), (44100, 44100, 1, 100), (24000, 48000, 1, 2 ** 30)):
        with pytest.raises(WorldClassError):
            rs.ResampleStream(*args)
    with pytest.raises(WorldClassError) as e:   # max_out x M leaves 31 bits
        rs.ResampleStream(48000, 44100, 1, 2 ** 24)
    assert "31 bits" in str(e.value)


def test_resample_stream_into_analysis_stream_is_the_whole_signal_chain():
    """22.05 kHz in 200 ms pushes -> 16 kHz -> an analysis stream's fixed chunks: the samples are the whole call's bit for bit, so the
    frames are too"""
    from world_class_amd.stream import StreamAnalyzer
    from world_class_amd.synth import make_utterance
    conv = (22050, 16000)
    x = make_utterance(conv[0], 1.3, 7)

    def analyze(pieces):
        """the 16 kHz samples as they arrive -> the analyzer's chunks (the last one, shorter, with the flush) -> all frames"""
        an = StreamAnalyzer(conv[1], 1, frame_period=5.0, chunk_ms=200, lookback_ms=400, lookahead_ms=400)
        cs, buf, res = an.chunk_samples, np.zeros(0), []
        for piece in pieces:
            buf = np.concatenate([buf, piece])
            while len(buf) > cs:
                res.append(an.push([buf[:cs]])[0])
                buf = buf[cs:]
        res.append(an.push([buf], [1])[0])
        return {k: np.concatenate([r[k] for r in res]) for k in ("tpos", "f0", "sp")}

    s = rs.ResampleStream(*conv, 1, 4410)
    try:
        pieces = [s.push([x[a:a + 4410]], [a + 4410 >= len(x)])[0] for a in range(0, len(x), 4410)]
    finally:
        s.close()
    y = whole(conv, [x])[0]
    assert np.array_equal(np.concatenate(pieces), y)
    streamed, direct = analyze(pieces), analyze([y])
    assert len(direct["f0"]) > 200 and (direct["f0"] > 0).any()
    for k in ("tpos", "f0", "sp"):
        assert np.array_equal(streamed[k], direct[k]), k
