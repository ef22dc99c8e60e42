"""The preconditions of tests/test_gpu_stage_edges.py, on the CPU: every input of that file reaches the edge it is named after.  A
device test that compares two runs passes just as well on an input that misses its target -- a frame that LoveTrain gates out never
reaches the kernel under test, a glide whose pulse intervals skip a value never takes the other side of a noise class -- so what
the inputs hit is held here, against the reference's own formulas (tests/stage_edges.py) and the CPU restatement (oracle/port.py)."""
import numpy as np
import pytest

import stage_edges as se

RATES = [(48000, 2048), (16000, 1024), (24000, 1024)]
SENTINEL = 1.0 - 1e-12


@pytest.mark.parametrize("kind,fs", [(k, fs) for k in ("ct", "d4c", "lovetrain") for fs in (16000, 24000, 48000)])
def test_the_helper_hands_out_an_f0_of_the_intended_length(kind, fs):
    # (a floor bounds the lengths D4C's windows can have: the helper refuses what lies beyond)
    longest = {"ct": 1 << 20, "d4c": se.d4c_half_length(fs, 0.0), "lovetrain": se.lovetrain_half_length(fs, 0.0)}[kind]
    for hl in (127, 128, 255, 256, 511, 512, 767, 768, 1023, 1024):
        if hl <= longest:
            assert se.half_length(kind, fs, se.f0_for_half_length(kind, fs, hl)) == hl
        else:
            with pytest.raises(AssertionError):
                se.f0_for_half_length(kind, fs, hl)
    for last in (255, 511, 1023, 2047):
        if (last + 1) // 2 <= longest:
            a, b = se.edge_pair(kind, fs, last)
            assert a > b
            assert 2 * se.half_length(kind, fs, a) + 1 == last and 2 * se.half_length(kind, fs, b) + 1 == last + 2


@pytest.mark.parametrize("fs,fft", RATES)
def test_cheaptrick_cases_lie_on_both_sides_of_every_edge(port, fs, fft):
    floor = se.ct_f0_floor(fs, fft)
    assert floor == port.cheaptrick_f0_floor(fs, fft) and fft == port.cheaptrick_fft_size(fs)
    f = se.ct_f0s(fs, fft, lambda v: se.ct_wave_takes(fft, v, fs))
    wl = {k: 2 * se.ct_half_length(fs, v, floor) + 1 for k, v in f.items()}
    for last in (fft // 4 - 1, fft // 2 - 1):
        assert wl["wl%d" % last] == last and wl["wl%d" % (last + 2)] == last + 2
        assert se.ct_prune_class(fft, last) * 2 == se.ct_prune_class(fft, last + 2)
    # the longest window: 1.5 fs / floor is (fft - 3) / 2, half way between two lengths; whichever way the next double above the floor
    # rounds, the window fits the transform and no F0 has a longer one
    assert wl["longest"] in (fft - 3, fft - 1) and se.ct_prune_class(fft, wl["longest"]) == 4
    assert wl["below_floor"] == 2 * se.matlab_round(1.5 * fs / se.DEFAULT_F0) + 1
    # the hand-over: adjacent doubles on the two sides, at the capacity of the smoothing's half width and one below it
    assert np.nextafter(f["last_inside"], np.inf) == f["first_outside"]
    assert se.ct_wave_takes(fft, f["last_inside"], fs) and not se.ct_wave_takes(fft, f["first_outside"], fs)
    cap = se.ct_half_width(fft, f["last_inside"], fs)
    assert se.ct_half_width(fft, f["first_outside"], fs) == cap + 1
    assert se.ct_half_width(fft, f["one_below_capacity"], fs) == cap - 1 and se.ct_wave_takes(fft, f["one_below_capacity"], fs)
    # first and last frame of every utterance carry the longest window, which hangs over both ends of the signal
    names, xs, tps, cs = se.ct_case(fs, fft, f, se.CT_FIRST_SEED[fs])
    for x, t, c in zip(xs, tps, cs):
        assert c[0] == c[-1] == f["longest"]
        assert t[0] * fs - wl["longest"] // 2 < 0 and t[-1] * fs + wl["longest"] // 2 > len(x) - 1
    assert names.index("first_outside") > 0  # (a listed frame's index lies beyond the first utterance)
    # the reference's own error on these inputs stays under the bound between two kernels (tests/test_gpu_cheaptrick.py: 1e-10)
    for nm, x, t, c in zip(names, xs, tps, cs):
        r = se.one_ulp_response(port, x, fs, t, c)
        print(fs, nm, "one ulp of the input moves the restatement's envelope by %.1e" % r)
        assert r < 1e-10, (nm, r)


@pytest.fixture(scope="module")
def d4c_oracle(port):
    """the CPU restatement's aperiodicity of every D4C utterance, once"""
    out = {}
    for fs, fft in RATES:
        n = se.d4c_fft_size(fs)
        f = se.d4c_f0s(fs, lambda v: se.d4c_wave_takes(n, v, fs))
        names, xs, tps, cs = se.d4c_case(fs, f, se.D4C_FIRST_SEED)
        aps = []
        for x, t, c in zip(xs, tps, cs):
            port.rng_reset()
            aps.append(port.d4c(x, fs, t, c, fft))
        port.rng_reset()
        out[fs] = (f, names, aps)
    return out


@pytest.mark.parametrize("fs,fft", RATES)
def test_d4c_cases_lie_on_both_sides_of_every_edge(fs, fft):
    n = se.d4c_fft_size(fs)
    assert n == (4096 if fs == 48000 else 2048)
    f = se.d4c_f0s(fs, lambda v: se.d4c_wave_takes(n, v, fs))
    longest = 2 * se.d4c_half_length(fs, se.D4C_FLOOR) + 1
    reached = [last for last in (511, 1023, 1535, 2047) if last + 2 <= longest]
    assert reached == {48000: [511, 1023, 1535, 2047], 24000: [511, 1023, 1535], 16000: [511, 1023]}[fs]
    for last in reached:
        a, b = f["wl%d" % last], f["wl%d" % (last + 2)]
        assert min(a, b) > se.D4C_FLOOR
        assert 2 * se.d4c_half_length(fs, a) + 1 == last and 2 * se.d4c_half_length(fs, b) + 1 == last + 2
        if last < 2047:
            assert se.d4c_groups(last) + 1 == se.d4c_groups(last + 2)
        else:
            assert not se.d4c_is_long(last) and se.d4c_is_long(last + 2)
    if fs == 48000:
        a, b = f["lt2047"], f["lt2049"]
        assert min(a, b) > se.LOVETRAIN_FLOOR
        assert 2 * se.lovetrain_half_length(fs, a) + 1 == 2047 and 2 * se.lovetrain_half_length(fs, b) + 1 == 2049
    else:
        assert 2 * se.lovetrain_half_length(fs, se.LOVETRAIN_FLOOR) + 1 <= 2048 and "lt2047" not in f
    assert se.d4c_half_length(fs, f["floored"]) == se.d4c_half_length(fs, f["floor"]) == (longest - 1) // 2
    assert se.lovetrain_half_length(fs, f["floored"]) == se.lovetrain_half_length(fs, se.LOVETRAIN_FLOOR)
    assert np.nextafter(f["last_inside"], np.inf) == f["first_outside"]
    assert se.d4c_wave_takes(n, f["last_inside"], fs) and not se.d4c_wave_takes(n, f["first_outside"], fs)
    assert se.d4c_half_width(n, f["first_outside"], fs) == se.d4c_half_width(n, f["last_inside"], fs) + 1


@pytest.mark.parametrize("fs,fft", RATES)
def test_every_d4c_frame_under_test_is_gated_in_and_lies_between_the_clamps(d4c_oracle, fs, fft):
    f, names, aps = d4c_oracle[fs]
    for nm, ap in zip(names, aps):
        gated_out = np.nonzero((ap == SENTINEL).all(axis=1))[0]
        assert len(ap) >= 50 and len(gated_out) == 0, (nm, f[nm], gated_out)
        inside = float(((ap > 0.001) & (ap < 0.999)).mean())
        print(fs, nm, "%.4f Hz: %d frames gated in, %.1f %% of the bins between the clamps" % (f[nm], len(ap), 100.0 * inside))
        assert inside >= 0.9, (nm, inside)


@pytest.mark.parametrize("fs,fft", RATES)
def test_synthesis_contours_hold_both_values_of_every_noise_class_edge(port, fs, fft):
    names, params, start = se.syn_case(fs, fft)
    got = {nm: se.pulse_intervals(port, p[0], fft, fs) for nm, p in zip(names, params)}
    for b, nfr in se.SYN_GLIDES[(fs, fft)]:
        d, v = got["glide%d" % b]
        assert nfr <= 121 and v.all()
        assert b in d and b + 1 in d, (b, sorted(set(d.tolist())))
        assert se.syn_noise_class(fft, b) * 2 == se.syn_noise_class(fft, b + 1)
    assert [b for b, _ in se.SYN_GLIDES[(fs, fft)]] == [fft // 4, fft // 2]
    if fft == 2048:
        for size in (128, 129):
            d, v = got["onset%d" % size]
            assert v.any() and not v.all()
            last_unvoiced = np.nonzero(~v)[0][-1]
            assert d[last_unvoiced] == size and d[~v].max() == size  # the last unvoiced pulse reaches up to the first voiced one
            assert (d[~v] < 128).sum() > 10                          # (the ordinary unvoiced pulses: 500 Hz)
    d, v = got["longest"]
    lowest = se.syn_lowest_f0(fs, fft)
    assert v.all() and len(d) >= 4 and d.max() == int(fs / lowest) and se.syn_noise_class(fft, int(d.max())) == 4 and d.max() <= fft
    d, v = got["below_lowest"]
    assert not v.any() and len(d) > 100
    assert start[names.index("glide%d" % (fft // 2))] == 0
