"""-m gpu: a speed per synthesis stream (include/world_class_stream.h, wc_synth_stream_set_speed).  The streams are driven push by
push with source frames; the samples of each are compared with ONE whole-utterance call over all of its source frames at the
positions tests/stream_speed_rule.py gives: Synthesis.compute_coded_retimed_device for coded pushes, io.retime_parameters followed
by Synthesis.compute_batch for full rows -- bit for bit at fft 1024 / 2048, within 1e-12 at 512 / 4096 (FP64 atomics) -- and with
the reference's Synthesis on tests/retime_rule.py's frames within 1e-8.  Every driven stream also checks frames_for_push before each
push, the accounting after it and the header's latency bound in synthesis frames."""
import math

import numpy as np
import pytest

import retime_rule as rr
import stream_speed_rule as sr

pytestmark = pytest.mark.gpu
Y_ABS = 1e-8        # the project's waveform tolerance
ATOMIC_ABS = 1e-12  # fft 512 / 4096: the bound of tests/test_gpu_synth_stream.py
ND = 40


@pytest.fixture(scope="module")
def env():
    import torch
    import world_class_amd as w
    from world_class_amd import codec, io as wio
    w.lib().wc_set_device(0)
    return w, codec, wio, torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).ravel()).cuda()


def _params(fs, fft, frames, seed, unvoiced=None, end_unvoiced=False):
    from oracle.gen_golden import synth_params
    f0, sp, ap = synth_params(fs, fft, frames, seed)
    if unvoiced is not None:
        f0[unvoiced] = 0.0
        ap[unvoiced] = 1.0 - 1e-12
    if end_unvoiced:
        f0[-2] = 140.0
        f0[-1] = 0.0
        ap[-1] = 1.0 - 1e-12
    return f0, sp, ap


def _code(env, fs, fft, p):
    """(f0, sp, ap) -> (f0, coded sp, coded ap), coded on the device"""
    w, codec, wio, torch = env
    f0, sp, ap = p
    n, n_ap = len(f0), codec.number_of_aperiodicities(fs)
    d_csp = torch.empty(n * ND, dtype=torch.float64, device="cuda")
    d_cap = torch.empty(n * n_ap, dtype=torch.float64, device="cuda")
    codec.code_spectral_envelope_device(fs, fft, n, ND, _dev(torch, sp), d_csp)
    codec.code_aperiodicity_device(fs, fft, n, _dev(torch, ap), d_cap)
    w.lib().wc_synchronize()
    return f0, d_csp.cpu().numpy().reshape(n, ND), d_cap.cpu().numpy().reshape(n, n_ap)


def refused():
    """the project's error with WC_ERR_INVALID (-1): no other exception passes"""
    import world_class_amd as w
    return pytest.raises(w.WorldClassError, match=r"error -1:")


def _gap(fs, fft):
    lowest = fs // fft + 1.0
    return int(np.ceil(max(2.0 * fs / lowest, fs / 500.0))) + 4


def drive(st, srcs, patterns, speed_at=None, coded=False, mods=None):
    """Pushes srcs[u] = (f0, rows, rows) into stream u in patterns[u] frames per push (cycled; 0 = idle), the last push of a stream
    flushing it.  speed_at(u, k): the speed to set before push k, or None to leave it.  Returns per stream the samples, the push
    sizes and the speeds in effect, having checked frames_for_push, the accounting and the latency bound at every push."""
    n = st.n_streams
    fs, fft, fp = st.fs, st.fft_size, st.frame_period
    for u, m in enumerate(mods or []):
        st.set_modification(u, *m)
    pos, k, done = [0] * n, 0, [False] * n
    ys, pushes, speeds = [[] for _ in range(n)], [[] for _ in range(n)], [[] for _ in range(n)]
    speed = [1.0] * n
    while not all(done):
        cols, flush, want = ([], [], []), [], []
        for u, src in enumerate(srcs):
            s_new = speed_at(u, k) if speed_at else None
            if s_new is not None and not done[u]:
                st.set_speed(u, s_new)
                speed[u] = s_new
            total = len(src[0])
            c = 0 if done[u] else min(patterns[u][k % len(patterns[u])], total - pos[u])
            for q in range(3):
                cols[q].append(src[q][pos[u]:pos[u] + c])
            flush.append(1 if not done[u] and pos[u] + c >= total else 0)
            want.append(st.frames_for_push(u, c))
            if not done[u]:
                pushes[u].append(c)
                speeds[u].append(speed[u])
            pos[u] += c
        before = [st.frames_synthesised(u) for u in range(n)]
        out = st.push_coded(*cols, flush) if coded else st.push(*cols, flush)
        for u in range(n):
            ys[u].append(out[u])
            if done[u]:
                continue
            p_rule, c_rule = sr.positions(pushes[u], speeds[u])
            G = st.frames_synthesised(u)
            assert G - before[u] == want[u] == c_rule[-1], (u, k, G - before[u], want[u], c_rule[-1])
            assert G == len(p_rule) and st.frames_received(u) == pos[u]
            assert (math.isnan(st.source_position(u)) if not p_rule else st.source_position(u) == p_rule[-1]), (u, k)
            got = sum(len(a) for a in ys[u])
            assert st.samples_committed(u) == got
            if not flush[u] and G >= 2:  # the header's latency bound, in synthesis frames
                assert got >= (G - 2) * fp / 1000.0 * fs - _gap(fs, fft) - fft // 2, (u, k, G, got)
            done[u] = bool(flush[u])
        k += 1
    return [np.concatenate(a) for a in ys], pushes, speeds


def whole_coded(env, fs, fft, fp, src, pos, scale, ratio, rng=0):
    """one compute_coded_retimed_device call over all source frames: samples and final noise position"""
    w, codec, wio, torch = env
    f0, csp, cap = src
    n, m = len(f0), len(pos)
    syn = w.Synthesis(fs, fft, fp)
    ol = syn.out_length(m)
    y = torch.full((ol + 1,), np.nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    end = syn.compute_coded_retimed_device(_dev(torch, f0), [n], _dev(torch, csp), ND, _dev(torch, cap), [m], _dev(torch, pos),
                                           _dev(torch, np.full(m, scale)), _dev(torch, np.full(m, ratio)), [ol], y, rng_pos=[rng])
    w.lib().wc_synchronize()
    y = y.cpu().numpy()
    assert np.isnan(y[-1])
    return y[:-1], end[0]


def whole_rows(env, fs, fft, fp, src, pos, rng=0):
    """io.retime_parameters (no scale, no ratio) followed by one batch Synthesis call"""
    w, codec, wio, torch = env
    f0, sp, ap = wio.retime_parameters(src[0], src[1], src[2], np.asarray(pos), fs, fft)
    ys, end = w.Synthesis(fs, fft, fp).compute_batch([f0], [sp], [ap], rng_pos=[rng])
    return ys[0], end[0]


SPEEDS = [0.5, 1.5, 1 / 1.37, 2.75, 1.25]
PATTERNS = [[3, 0, 11, 1], [1, 2, 0, 17], [7, 0, 0, 1, 20], [20, 1, 0], [1]]  # the last: one frame at a time
MODS = [(1.0, 0.0), (1.1, 0.8), (0.9, 1.2), (1.0, 1.2), (1.2, 0.0)]


def _sources(fs, fft, frames, seed):
    return [_params(fs, fft, frames, seed), _params(fs, fft, frames + 5, seed + 1, unvoiced=slice(frames // 5, frames // 2), end_unvoiced=True),
            _params(fs, fft, frames - 7, seed + 2), _params(fs, fft, frames + 11, seed + 3), _params(fs, fft, frames // 2, seed + 4)]


@pytest.mark.parametrize("fs,fft,fp", [(16000, 1024, 5.0), (24000, 1024, 1.0), (48000, 2048, 5.0)])
def test_retimed_coded_streams_equal_the_whole_utterance_call(env, fs, fft, fp):
    """1. five streams at speeds 0.5, 1.5, 1 / 1.37, 2.75 and 1.25 set before the first push, ragged pushes with idle and
    one-frame pushes, a long unvoiced stretch and a voiced -> unvoiced end; ratios 0, 0.8 and 1.2"""
    from world_class_amd.stream import StreamSynthesizer
    srcs = [_code(env, fs, fft, p) for p in _sources(fs, fft, int(round(600 / fp)), 300)]
    st = StreamSynthesizer(fs, fft, fp, len(srcs), 64)
    ys, pushes, speeds = drive(st, srcs, PATTERNS, lambda u, k: SPEEDS[u] if k == 0 else None, coded=True, mods=MODS)
    for u, src in enumerate(srcs):
        pos, _ = sr.positions(pushes[u], speeds[u])
        assert pos[-1] <= len(src[0]) - 1 < pos[-1] + SPEEDS[u]
        want, end = whole_coded(env, fs, fft, fp, src, pos, *MODS[u])
        assert np.isfinite(want).all() and np.array_equal(ys[u], want), (u, len(ys[u]), len(want))
        assert st.rng_position(u) == end
        assert st.frames_synthesised(u) == len(pos) and st.source_position(u) == pos[-1] and st.frames_received(u) == len(src[0])


@pytest.mark.parametrize("fs,fft,fp", [(16000, 1024, 5.0), (48000, 2048, 5.0)])
def test_full_rows_are_retimed_without_scale_or_ratio(env, fs, fft, fp):
    """2. the same through push (full rows, no setting): io.retime_parameters_device followed by Synthesis"""
    from world_class_amd.stream import StreamSynthesizer
    srcs = _sources(fs, fft, 120, 320)
    st = StreamSynthesizer(fs, fft, fp, len(srcs), 64)
    ys, pushes, speeds = drive(st, srcs, PATTERNS, lambda u, k: SPEEDS[u] if k == 0 else None)
    for u, src in enumerate(srcs):
        pos, _ = sr.positions(pushes[u], speeds[u])
        want, end = whole_rows(env, fs, fft, fp, src, pos)
        assert np.array_equal(ys[u], want), u
        assert st.rng_position(u) == end


@pytest.mark.parametrize("fs,fft,coded", [(8000, 512, False), (96000, 4096, False), (96000, 4096, True)])
def test_sizes_with_fp64_atomics(env, fs, fft, coded):
    """3. fft 512 (8 kHz: full rows only, the codec needs 12 kHz) and 4096: within 1e-12"""
    from world_class_amd.stream import StreamSynthesizer
    fp = 5.0
    raw = [_params(fs, fft, 90, 340), _params(fs, fft, 90, 341, unvoiced=slice(10, 40), end_unvoiced=True)]
    srcs = [_code(env, fs, fft, p) for p in raw] if coded else raw
    mods = [(1.1, 0.8), (1.0, 1.2)] if coded else None
    st = StreamSynthesizer(fs, fft, fp, 2, 40)
    ys, pushes, speeds = drive(st, srcs, [[1, 4, 0], [9, 2]], lambda u, k: (0.5, 1.5)[u] if k == 0 else None, coded=coded, mods=mods)
    for u, src in enumerate(srcs):
        pos, _ = sr.positions(pushes[u], speeds[u])
        want, _ = whole_coded(env, fs, fft, fp, src, pos, *mods[u]) if coded else whole_rows(env, fs, fft, fp, src, pos)
        assert len(ys[u]) == len(want) and np.abs(ys[u] - want).max() <= ATOMIC_ABS, (u, np.abs(ys[u] - want).max())


@pytest.mark.parametrize("fs,fft", [(16000, 1024), (48000, 2048)])
def test_stream_matches_the_reference_chain(env, port, fs, fft):
    """4. the reference's Synthesis (oracle/port.py) on the numpy restatement's frames of the whole utterance, from noise
    position 0, against the stream on full rows: within 1e-8"""
    from world_class_amd.stream import StreamSynthesizer
    fp = 5.0
    srcs = [_params(fs, fft, 120, 350), _params(fs, fft, 120, 351, unvoiced=slice(30, 60), end_unvoiced=True)]
    st = StreamSynthesizer(fs, fft, fp, 2, 64)
    ys, pushes, speeds = drive(st, srcs, [[3, 0, 11, 1], [7, 20, 1]], lambda u, k: (1 / 1.37, 1.5)[u] if k == 0 else None)
    for u, src in enumerate(srcs):
        pos, _ = sr.positions(pushes[u], speeds[u])
        f0, sp, ap = rr.retime(src[0], src[1], src[2], pos)
        port.rng_seek(0)
        want = port.synthesis(f0, sp, ap, fs, fp)
        err = np.abs(ys[u] - want).max()
        print("stream against the reference chain, fs %d, stream %d: %.3e (peak %.2f)" % (fs, u, err, np.abs(want).max()))
        assert len(ys[u]) == len(want) and err < Y_ABS
    port.rng_reset()


def _ramp(u, k):
    """stream 0: a ramp 0.5 -> 1.5 set push by push; stream 1: 1.0, then 0.75 from push 4, 1.0 again from push 9"""
    if u == 0:
        return min(1.5, 0.5 + 0.05 * k)
    return 0.75 if 4 <= k < 9 else 1.0


@pytest.mark.parametrize("fs,fft,scale,ratio", [(16000, 1024, 1.0, 0.0), (48000, 2048, 1.0, 0.0), (48000, 2048, 1.0, 1.2), (16000, 1024, 1.3, 0.0)])
def test_speed_changes_between_pushes(env, fs, fft, scale, ratio):
    """5. bit for bit the retimed call on the rule's positions -- with an F0 scale too (stream 1 then takes its carried row from its
    kept coded frame: its window row is scaled) -- but for stream 1 with ratio 1.2: the frames formed before it became retimed were
    stretched inside the decoder (1e-12 relative on rows, the header's statement), so its waveform is held to 1e-8.  Stream 0 is
    retimed from its first push: exact with every setting"""
    from world_class_amd.stream import StreamSynthesizer
    fp = 5.0
    srcs = [_code(env, fs, fft, p) for p in (_params(fs, fft, 130, 360), _params(fs, fft, 110, 361, unvoiced=slice(40, 55)))]
    st = StreamSynthesizer(fs, fft, fp, 2, 64)
    mods = [(scale, ratio), (scale, ratio)]
    ys, pushes, speeds = drive(st, srcs, [[5, 7, 0, 6], [6, 1, 9]], _ramp, coded=True, mods=mods)
    assert len(set(speeds[0])) > 10 and set(speeds[1]) == {1.0, 0.75}
    for u, src in enumerate(srcs):
        pos, _ = sr.positions(pushes[u], speeds[u])
        want, end = whole_coded(env, fs, fft, fp, src, pos, *mods[u])
        assert st.rng_position(u) == end
        if ratio == 0.0 or u == 0:
            assert np.array_equal(ys[u], want), u
        else:
            err = np.abs(ys[u] - want).max()
            print("speed changes, ratio %.1f, stream %d: %.3e" % (ratio, u, err))
            assert len(ys[u]) == len(want) and err < Y_ABS


def test_streams_are_independent(env):
    """6. a never-retimed stream with a ratio and a retimed one make the same samples alone and beside retimed neighbours"""
    from world_class_amd.stream import StreamSynthesizer
    fs, fft, fp = 48000, 2048, 5.0
    srcs = [_code(env, fs, fft, p) for p in _sources(fs, fft, 100, 370)[:4]]
    mods = [(1.1, 1.2), (0.9, 0.8), (1.0, 1.2), (1.2, 0.0)]
    speeds = [1.0, 0.5, 2.75, 1 / 1.37]
    st = StreamSynthesizer(fs, fft, fp, 4, 64)
    ys, _, _ = drive(st, srcs, PATTERNS[:4], lambda u, k: speeds[u] if k == 0 and u else None, coded=True, mods=mods)
    for u in (0, 1):
        alone = StreamSynthesizer(fs, fft, fp, 1, 64)
        y1, _, _ = drive(alone, [srcs[u]], [PATTERNS[u]], lambda v, k: speeds[u] if k == 0 and u else None, coded=True, mods=[mods[u]])
        assert np.array_equal(ys[u], y1[0]), u
    # the never-retimed stream is the batch call with its ratio in the decoder
    w, codec, wio, torch = env
    f0, csp, cap = srcs[0]
    syn = w.Synthesis(fs, fft, fp)
    ol = syn.out_length(len(f0))
    y = torch.empty(ol, dtype=torch.float64, device="cuda")
    syn.compute_coded_modified_device(_dev(torch, f0 * mods[0][0]), [len(f0)], _dev(torch, csp), ND, _dev(torch, cap),
                                      _dev(torch, np.full(len(f0), mods[0][1])), [ol], y, rng_pos=[0])
    w.lib().wc_synchronize()
    assert np.array_equal(ys[0], y.cpu().numpy())
    assert st.frames_synthesised(0) == st.frames_received(0) == len(f0) and st.source_position(0) == len(f0) - 1


@pytest.mark.parametrize("explicit", [False, True])
def test_a_neutral_stream_is_todays_stream(env, explicit):
    """7. with set_speed(u, 1.0) or without any call: the batch call's samples, and the retiming kernel is never launched"""
    from world_class_amd.stream import StreamSynthesizer
    w, codec, wio, torch = env
    fs, fft, fp = 16000, 1024, 5.0
    srcs = [_params(fs, fft, 80, 380), _params(fs, fft, 90, 381)]
    L = w.lib()
    L.wc_set_kernel_timing(0)
    L.wc_set_kernel_timing(1)  # a fresh window: no event of an earlier test
    try:
        for coded in (False, True):
            use = [_code(env, fs, fft, p) for p in srcs] if coded else srcs
            st = StreamSynthesizer(fs, fft, fp, 2, 32)
            ys, _, _ = drive(st, use, [[3, 0, 11], [1]], (lambda u, k: 1.0) if explicit else None, coded=coded)
            for u, src in enumerate(use):
                n = len(src[0])
                want = (whole_coded(env, fs, fft, fp, src, np.arange(n, dtype=np.float64), 1.0, 0.0) if coded
                        else w.Synthesis(fs, fft, fp).compute_batch([src[0]], [src[1]], [src[2]], rng_pos=[0]))[0]
                want = want[0] if isinstance(want, list) else want
                assert np.array_equal(ys[u], want), (coded, u)
                assert st.frames_synthesised(u) == st.frames_received(u) == n
        assert L.wc_last_kernel_ms(b"retime_stream_kernel") < 0, "the retiming kernel ran for neutral streams"
        st = StreamSynthesizer(fs, fft, fp, 1, 32)  # (the check does see the kernel when it runs)
        drive(st, [srcs[0]], [[9]], lambda u, k: 0.5 if k == 0 else None)
        assert L.wc_last_kernel_ms(b"retime_stream_kernel") >= 0
    finally:
        L.wc_set_kernel_timing(0)


@pytest.mark.parametrize("coded", [True, False])
def test_refusals_leave_every_stream_as_it_was(env, coded):
    """8. bad speeds, a push that would form max_frames + 1 frames, a flush with one synthesis frame, a refusal for stream 1 that
    leaves stream 0 untouched; the streams then continue to the whole call's samples -- through push_coded and through push (full
    rows); reset returns the speed to 1.0"""
    from world_class_amd.stream import StreamSynthesizer
    fs, fft, fp, mf = 16000, 1024, 5.0, 16
    srcs = [_params(fs, fft, 40, 390), _params(fs, fft, 40, 391)]
    if coded:
        srcs = [_code(env, fs, fft, p) for p in srcs]
    st = StreamSynthesizer(fs, fft, fp, 2, mf)
    state = lambda: [(st.samples_committed(u), st.frames_received(u), st.frames_synthesised(u), repr(st.source_position(u)), st.rng_position(u))
                     for u in range(2)]
    e = [np.zeros(0), np.zeros((0, srcs[0][1].shape[1])), np.zeros((0, srcs[0][2].shape[1]))]  # (full rows: fft // 2 + 1 columns)
    cut = lambda u, a, b: [srcs[u][q][a:b] for q in range(3)]

    def push(a, b, flush=None):
        return (st.push_coded if coded else st.push)(*[[a[q], b[q]] for q in range(3)], flush)

    st.set_speed(0, 0.5)
    st.set_speed(1, 3.0)
    acc = [[], []]
    r = push(cut(0, 0, 6), cut(1, 0, 2))
    acc[0].append(r[0]); acc[1].append(r[1])
    assert st.frames_synthesised(0) == 11 and st.frames_synthesised(1) == 1 and st.source_position(1) == 0.0
    s0 = state()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with refused():
            st.set_speed(0, bad)
    assert state() == s0
    assert st.frames_for_push(0, 9) == mf + 1  # 18 frames at half speed: one more than the bound, and the count stops there
    with refused():
        push(cut(0, 6, 15), e)
    assert state() == s0
    st.set_speed(0, 1e-300)
    assert st.frames_for_push(0, 1) == mf + 1
    st.set_speed(0, 0.5)
    with refused():  # F = 2 at speed 3: one synthesis frame, flushed
        push(e, e, flush=[0, 1])
    assert state() == s0
    with refused():  # stream 0 is fine, stream 1 is refused: neither moves
        push(cut(0, 6, 10), e, flush=[0, 1])
    assert state() == s0
    for a in range(6, 40, 8):
        last = a + 8 >= 40
        r = push(cut(0, a, a + 8), cut(1, a - 4, a + 4) if not last else cut(1, a - 4, 40), flush=[1, 1] if last else None)
        acc[0].append(r[0]); acc[1].append(r[1])
    for u, speed in enumerate((0.5, 3.0)):
        pos = list(np.arange(int(39 / speed) + 1) * speed)
        want, end = whole_coded(env, fs, fft, fp, srcs[u], pos, 1.0, 0.0) if coded else whole_rows(env, fs, fft, fp, srcs[u], pos)
        assert np.array_equal(np.concatenate(acc[u]), want), u
        assert st.rng_position(u) == end and st.frames_synthesised(u) == len(pos) and st.frames_received(u) == 40
    if not coded:
        return  # (the reset below is the handle's, the same for both kinds of rows)
    st.reset(0)
    assert st.frames_for_push(0, 5) == 5 and math.isnan(st.source_position(0)) and st.frames_received(0) == 0
    one = StreamSynthesizer(fs, fft, fp, 1, 40)
    y = one.push_coded([srcs[0][0]], [srcs[0][1]], [srcs[0][2]], [1])[0]
    st2 = StreamSynthesizer(fs, fft, fp, 2, 40)
    st2.set_speed(0, 0.5)
    st2.push_coded(*[[cut(0, 0, 4)[q], e[q]] for q in range(3)])
    st2.reset(0)  # not retimed any more, speed 1.0
    got = st2.push_coded(*[[srcs[0][q], e[q]] for q in range(3)], [1, 0])[0]
    assert np.array_equal(got, y) and st2.frames_synthesised(0) == 40


def test_a_speed_that_falls_behind_the_carried_row_is_refused(env):
    """one source row is carried, frame F - 1: set_speed refuses a speed with floor(last + speed) < F - 1 and keeps the setting.  After
    8 frames at speed 2.75 (last = 5.5) a speed of 0.5 asks for frame 6, which is gone; 1.6 asks for frames 7 and 8 and goes on to the
    whole call's samples"""
    from world_class_amd.stream import StreamSynthesizer
    fs, fft, fp = 16000, 1024, 5.0
    src = _params(fs, fft, 40, 395)
    st = StreamSynthesizer(fs, fft, fp, 1, 32)
    cut = lambda a, b: [[src[q][a:b]] for q in range(3)]
    st.set_speed(0, 2.75)
    ys = [st.push(*cut(0, 8))[0]]
    assert st.source_position(0) == 5.5 and st.frames_synthesised(0) == 3
    with refused():
        st.set_speed(0, 0.5)
    assert st.frames_for_push(0, 12) == sr.positions([8, 12], [2.75, 2.75])[1][1]  # the speed is still 2.75
    st.set_speed(0, 1.6)
    ys.append(st.push(*cut(8, 20))[0])
    ys.append(st.push(*cut(20, 40), [1])[0])
    pos, counts = sr.positions([8, 12, 20], [2.75, 1.6, 1.6])
    assert st.frames_synthesised(0) == len(pos) and counts[0] == 3
    want, end = whole_rows(env, fs, fft, fp, src, pos)
    assert np.array_equal(np.concatenate(ys), want) and st.rng_position(0) == end


def test_a_decelerating_stream(env):
    """a speed lowered push by push beside a neighbour that is idle or fed: set_speed takes a lower speed exactly when
    floor(last + speed) >= F - 1 (both cases occur), a refused one leaves the speed, the neighbour and every later push alone, and
    the stream ends at the whole call's samples on the positions of the speeds that were taken"""
    from world_class_amd.stream import StreamSynthesizer
    fs, fft, fp = 16000, 1024, 5.0
    srcs = [_params(fs, fft, 60, 396), _params(fs, fft, 30, 397)]
    st = StreamSynthesizer(fs, fft, fp, 2, 64)
    e = [np.zeros(0), np.zeros((0, fft // 2 + 1)), np.zeros((0, fft // 2 + 1))]
    speed, taken, refusals, acc, other = 1.75, [], 0, [], []
    st.set_speed(0, speed)
    for k in range(12):
        a, b = 5 * k, 5 * k + 5
        if k:
            lower = speed * 0.8
            ok = math.floor(st.source_position(0) + lower) >= a - 1
            if ok:
                st.set_speed(0, lower)
                speed = lower
            else:
                refusals += 1
                with refused():
                    st.set_speed(0, lower)
        taken.append(speed)
        nb = [srcs[1][q][a // 2:a // 2 + 5] for q in range(3)] if k % 2 == 0 else e  # the neighbour: fed every other push
        r = st.push(*[[srcs[0][q][a:b], nb[q]] for q in range(3)], [1 if k == 11 else 0, 1 if k == 10 else 0])
        acc.append(r[0]); other.append(r[1])
    assert refusals > 0 and len(set(taken)) > 3, (refusals, taken)
    pos, _ = sr.positions([5] * 12, taken)
    want, end = whole_rows(env, fs, fft, fp, srcs[0], pos)
    assert st.frames_synthesised(0) == len(pos) and np.array_equal(np.concatenate(acc), want) and st.rng_position(0) == end
    w = env[0]
    nbr = np.concatenate([srcs[1][0][a // 2:a // 2 + 5] for a in range(0, 60, 10)])
    idx = np.concatenate([np.arange(a // 2, a // 2 + 5) for a in range(0, 60, 10)])
    want1 = w.Synthesis(fs, fft, fp).compute_batch([nbr], [srcs[1][1][idx]], [srcs[1][2][idx]], rng_pos=[0])[0][0]
    assert np.array_equal(np.concatenate(other), want1)


def _until_retimed(env, fs, fft, fp, src, mods, declare):
    """stream 0 with a modification setting at speed 1.0 (declare: set_speed(0, 1.0) before the first frame), two coded pushes;
    stream 1 is flushed by the first push, so a later push that gives it a frame is refused.  cut(a, b): frames a .. b for stream 0"""
    from world_class_amd.stream import StreamSynthesizer
    st = StreamSynthesizer(fs, fft, fp, 2, 32)
    st.set_modification(0, *mods)
    if declare:
        st.set_speed(0, 1.0)
    cut = lambda a, b, fl=0, nb=0: ([src[0][a:b], src[0][:nb]], [src[1][a:b], src[1][:nb]], [src[2][a:b], src[2][:nb]], [fl, 0])
    first = cut(0, 6, nb=3)
    ys = [st.push_coded(*first[:3], [0, 1])[0], st.push_coded(*cut(6, 13))[0]]
    return st, cut, ys


@pytest.mark.parametrize("mods", [(1.3, 0.0), (1.0, 1.2), (0.9, 0.8)])
def test_a_refused_coded_push_leaves_the_kept_coded_frame(env, mods):
    """a stream with a setting at speed 1.0 keeps its newest coded frame (its window row is scaled and stretched); coded pushes
    that are refused (here: a frame for a neighbour that was flushed) must not replace it.  The stream is then given speed 0.5: its first interpolated frames take source
    frame 12 from the kept frame, and the samples are the whole call's (bit for bit without a ratio, 1e-8 with one: test 5)"""
    fs, fft, fp = 48000, 2048, 5.0
    src = _code(env, fs, fft, _params(fs, fft, 40, 398))
    st, cut, ys = _until_retimed(env, fs, fft, fp, src, mods, True)
    s0 = (st.samples_committed(0), st.frames_received(0), st.frames_synthesised(0), st.source_position(0), st.rng_position(0))
    with refused():  # stream 1 was flushed: refused by the push on full rows, behind the stages that take stream 0's frames
        st.push_coded(*cut(20, 27, nb=1))
    assert s0 == (st.samples_committed(0), st.frames_received(0), st.frames_synthesised(0), st.source_position(0), st.rng_position(0))
    st.set_speed(0, 0.5)
    ys.append(st.push_coded(*cut(13, 25))[0])
    ys.append(st.push_coded(*cut(25, 40, 1))[0])
    pos, _ = sr.positions([6, 7, 12, 15], [1.0, 1.0, 0.5, 0.5])
    want, end = whole_coded(env, fs, fft, fp, src, pos, *mods)
    got = np.concatenate(ys)
    assert st.rng_position(0) == end and len(got) == len(want)
    if mods[1] == 0.0:
        assert np.array_equal(got, want)
    else:
        err = np.abs(got - want).max()
        print("kept coded frame after a refused push, mods %s: %.3e" % (mods, err))
        assert err < Y_ABS


def test_a_modified_stream_declares_its_speed_before_it_changes_it(env):
    """without set_speed before its newest frame, a stream with a setting has no unmodified source row to carry: becoming retimed is
    refused by frames_for_push and by the push, nothing moves, and once set_speed(0, 1.0) was in effect for a push the change goes"""
    fs, fft, fp = 16000, 1024, 5.0
    src = _code(env, fs, fft, _params(fs, fft, 30, 399))
    st, cut, ys = _until_retimed(env, fs, fft, fp, src, (1.1, 0.8), False)
    s0 = (st.samples_committed(0), st.frames_received(0), st.frames_synthesised(0), st.source_position(0), st.rng_position(0))
    st.set_speed(0, 0.5)
    with refused():
        st.frames_for_push(0, 3)
    with refused():
        st.push_coded(*cut(13, 16))
    assert s0 == (st.samples_committed(0), st.frames_received(0), st.frames_synthesised(0), st.source_position(0), st.rng_position(0))
    st.set_speed(0, 1.0)
    ys.append(st.push_coded(*cut(13, 16))[0])
    st.set_speed(0, 0.5)
    assert st.frames_for_push(0, 4) == 8
    ys.append(st.push_coded(*cut(16, 30, 1))[0])
    pos, _ = sr.positions([6, 7, 3, 14], [1.0, 1.0, 1.0, 0.5])
    want, end = whole_coded(env, fs, fft, fp, src, pos, 1.1, 0.8)
    got = np.concatenate(ys)
    assert st.rng_position(0) == end and len(got) == len(want) and np.abs(got - want).max() < Y_ABS
