"""CPU, no device: the inputs of tests/frame_periods.py reach the edges they are made for, and the CPU restatement (oracle/port.py)
holds against the real reference at those frame periods -- against tests/golden/frame_periods.npz (made from the real reference by
oracle/gen_golden_frame_periods.py) everywhere, and against the live reference where oracle/_ref is built.  The pin is
tests/test_oracle_golden.py's: 1e-9 on the waveform and on F0 with the same voicing.  Measured when the fixture was made: at most
2.4e-16 on the waveform of the plain contours (1.8e-14 on the steep ones, whose samples reach 40) and 1.6e-12 Hz on F0.

tests/test_gpu_frame_periods.py then uses the restatement and the fixture as the checkers of the product."""
import hashlib

import numpy as np
import pytest

import frame_periods as fpm
from test_oracle_golden import F0_ABS, Y_ABS


@pytest.fixture(scope="module")
def fixture():
    return np.load(fpm.fixture_path())


def against_fixture(z, name, kind, y, tol):
    """a waveform against what the fixture holds of the reference's: returns the worst difference seen on stored samples"""
    k = "%s/%s/" % (name, kind)
    assert len(y) == int(z[k + "y_len"][0])
    if k + "y" in z:
        worst = float(np.abs(y - z[k + "y"]).max())
    else:
        worst = 0.0
        for st, w in zip(z[k + "y_win_start"], z[k + "y_win"]):
            worst = max(worst, float(np.abs(y[st:st + fpm.WIN] - w).max()))
        nb = len(y) // fpm.BLOCK
        assert np.abs(y[:nb * fpm.BLOCK].reshape(nb, fpm.BLOCK).sum(1) - z[k + "y_blocksum"]).max() < tol * fpm.BLOCK
    assert worst < tol, (name, kind, worst)
    return worst


def check_params(z, name, kind, p):
    """the regenerated parameters are the ones the fixture was made from"""
    assert np.allclose([p[0].sum(), p[1].sum(), p[2].sum()], z["%s/%s/param_sums" % (name, kind)], rtol=1e-12, atol=0)


# ---- the inputs reach the edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fpm.MUST_REACH))
def test_boundary_contours_put_pulses_of_both_kinds_on_frame_boundaries(port, name):
    """pulses ON the sample k fp fs, with the quotient's floor at k - 1 and at k: at least three of each at 16 kHz / 12.5 ms, one of
    each at the other cases whose sample grid has boundaries of both kinds"""
    fs, fft, fp, _, n_frames = fpm.CASES[name]
    f0 = fpm.contour(name, "boundary")[0]
    below, at = fpm.boundary_pulses(port, f0, fs, fft, fp)
    print(name, "boundary pulses with floor k - 1:", len(below), "with floor k:", len(at))
    assert len(below) >= fpm.MUST_REACH[name] and len(at) >= fpm.MUST_REACH[name]
    # (the steep contour is the same F0 over rows stepped at the boundaries of the first kind: its pulses are the same)
    f0s, sps, _ = fpm.contour(name, "steep")
    assert np.array_equal(f0s, f0)
    k = (np.array(below) / (fp / 1000.0 * fs)).round().astype(int)
    assert set(fpm.STEPS[name]) <= set(k) and set(k) <= set(fpm.STEPS[name]) | {j + 1 for j in fpm.STEPS[name]}
    assert set(fpm.STEPS[name]) <= set(fpm.below_boundaries(fs, fp, n_frames))
    j = np.array(fpm.STEPS[name])
    assert (sps[j - 1].max(axis=1) > 1e12 * sps[j].max(axis=1)).all()


@pytest.mark.parametrize("name", fpm.NAMES)
def test_contours_have_the_shapes_they_are_named_after(port, name):
    fs, fft, fp, _, _ = fpm.CASES[name]
    lowest = fs // fft + 1.0
    for kind in fpm.contours(name):
        f0, sp, ap = fpm.contour(name, kind)
        assert 2 <= len(f0) <= 120 and sp.shape == ap.shape == (len(f0), fft // 2 + 1)
        v = f0[f0 > 0]
        d = fs / v
        assert (np.abs(d - d.round()) < 1e-9).all() and (v > lowest).all()  # fs / d, none below the stage's lowest F0
        assert (ap[f0 == 0] == fpm.SENTINEL).all() and (ap[f0 > 0][:, 0] < 0.5).all()
        n, cap = port.synthesis_pulses(f0, fft, fs, fp)
        assert n <= cap  # (the reference's pulse arrays hold it: the fixture could be made)
    f0 = fpm.contour(name, "end_unvoiced")[0]
    assert f0[-2] > 0 and f0[-1] == 0
    assert len(fpm.contour(name, "two")[0]) == 2
    f0 = fpm.contour(name, "gap")[0]
    gap = np.flatnonzero(f0 == 0)
    assert (np.diff(gap) == 1).all() and len(gap) * fp / 1000.0 * fs > 512 and f0[gap[-1] + 1] > 0
    if fft >= 1024:  # and the voiced stretch behind the gap has pulse intervals beyond 512 samples
        assert fs / f0[-1] > 512
    if name == "48k_0.7ms":  # more frames than pulses
        assert port.synthesis_pulses(fpm.contour(name, "boundary")[0], fft, fs, fp)[0] < 120


# ---- the restatement holds at these frame periods ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fpm.NAMES)
def test_restatement_synthesis_against_the_fixture(port, fixture, name):
    fs, fft, fp, _, _ = fpm.CASES[name]
    for kind in fpm.contours(name):
        p = fpm.contour(name, kind)
        check_params(fixture, name, kind, p)
        port.rng_reset()
        y = port.synthesis(*p, fs, fp)
        assert len(y) == fpm.out_length(len(p[0]), fp, fs)
        print(name, kind, "restatement against the fixture: %.2e" % against_fixture(fixture, name, kind, y, Y_ABS))
    port.rng_reset()


@pytest.mark.parametrize("name,fs,fp", fpm.HARVEST_PERIODS)
def test_restatement_harvest_against_the_fixture(port, fixture, name, fs, fp):
    x = fpm.harvest_signal(fs)
    assert hashlib.sha256(x.tobytes()).digest() == fixture["harvest/%s/x_sha256" % name].tobytes(), "synthetic generator drifted"
    want = fixture["harvest/%s/f0" % name]
    tpos, f0 = port.harvest(x, fs, frame_period=fp)
    assert len(f0) == len(want) == fpm.get_samples(fs, len(x), fp)
    assert np.array_equal(tpos, np.arange(len(f0)) * fp / 1000.0)
    assert np.array_equal(f0 == 0, want == 0)
    print(name, "restatement F0 against the fixture: %.2e Hz" % np.abs(f0 - want).max())
    assert np.abs(f0 - want).max() < F0_ABS
    assert (want > 0).sum() > 40


@pytest.mark.parametrize("name", fpm.NAMES)
def test_restatement_against_the_live_reference(port, name):
    """where oracle/_ref is built: Synthesis from noise position 0 on every contour, and Harvest on the case's own signal at the
    case's frame period -- no fallback, none of these stage calls crashes the reference"""
    from oracle import ref
    if not ref.available():
        pytest.skip("oracle/_ref not built in this environment")
    fs, fft, fp, _, _ = fpm.CASES[name]
    for kind in fpm.contours(name):
        p = fpm.contour(name, kind)
        want = ref.run_fresh("at", 0, "synthesis", *p, fs, fp)
        port.rng_reset()
        y = port.synthesis(*p, fs, fp)
        assert len(y) == len(want)
        print(name, kind, "restatement against the live reference: %.2e" % np.abs(y - want).max())
        assert np.abs(y - want).max() < Y_ABS
    port.rng_reset()
    x = fpm.harvest_signal(fs)
    tr, fr = ref.run_fresh("harvest", x, fs, frame_period=fp)
    tp, f0 = port.harvest(x, fs, frame_period=fp)
    assert np.array_equal(tp, tr) and np.array_equal(f0 == 0, fr == 0)
    print(name, "restatement F0 against the live reference: %.2e Hz" % np.abs(f0 - fr).max())
    assert np.abs(f0 - fr).max() < F0_ABS


# ---- lengths ----------------------------------------------------------------------------------------------------------------------
def test_lengths_truncate_as_the_reference_does(port):
    """get_samples and the out-length formula on sample and frame counts around exact multiples of the hop: the truncation of a
    product that is nominally a whole number drops a frame or a sample at some of them, as in the reference (24 kHz, hop 256: 57
    frames give 14336 samples, not 14337)"""
    from oracle import ref
    R = ref.Ref() if ref.available() else None
    dropped = 0
    for fs, fp, ns in fpm.length_grid():
        hop = fp / 1000.0 * fs
        for n in ns:
            want = fpm.get_samples(fs, n, fp)
            assert port.get_samples(fs, n, fp) == want
            if R is not None:
                assert R.get_samples(fs, n, fp) == want
            if abs(n / hop - round(n / hop)) < 1e-9 and want == round(n / hop):
                dropped += 1  # n is k hops and the quotient fell below k: k frames, not k + 1
        for frames in list(range(2, 122)) + [998, 4002]:
            ol = fpm.out_length(frames, fp, fs)
            exact = (frames - 1) * hop
            assert ol in (int(round(exact)) + 1, int(round(exact))) if abs(exact - round(exact)) < 1e-6 else ol == int(exact) + 1
            # (the restatement's Synthesis takes its default length from the same formula)
    assert dropped > 0
    assert fpm.out_length(57, 256 / 24000 * 1000, 24000) == 14336
