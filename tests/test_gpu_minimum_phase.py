"""-m gpu: the device's minimum-phase analyses on their own (wc_debug_minimum_phase, wc_synthesis.hip) against the numpy rule of
tests/minimum_phase_rule.py, which tests/test_minimum_phase_rule.py holds to the real reference at 1e-13 (measured 7.7e-15).

  form 0  minimum_phase_lds<n, T>, a workgroup of the pulse kernel's T threads: n = 512 (T = 64), 1024 (128), 2048, 4096 (256)
  form 1  one wavefront: minimum_phase_wave8 (n = 1024) and minimum_phase_wave (n = 2048)

The device forms take the cepstrum as real, use a real second transform, hold the bins in the paired layout with lane 0's special
pairs, and (form 1) the lean exp and sin / cos: a log spectrum that is non-zero in ONE bin finds a bin mapped wrongly in one lane or
slot whatever the goldens of the stage tests happen to carry there.  Bound, per bin: |device - rule| <= 1e-12 |rule|, the project's
minimum-phase bound (tests/test_helpers.py) made relative.

Measured on an MI355X, worst max |device - rule| / |rule| over the six spectra (the notch or the floor; every test prints its own):
  n =  512 form 0  1.53e-14       n = 1024 form 0  1.60e-14       n = 1024 form 1  1.52e-14
  n = 2048 form 0  1.77e-14       n = 2048 form 1  1.46e-14       n = 4096 form 0  1.93e-14
one bin at a time at most 1.8e-15; form 0 against form 1 1.59e-14 (n = 1024) and 1.66e-14 (n = 2048); flat and zeros exact."""
import ctypes as C

import numpy as np
import pytest

import minimum_phase_rule as rule

pytestmark = pytest.mark.gpu

BOUND = 1e-12
FORMS = {512: (0,), 1024: (0, 1), 2048: (0, 1), 4096: (0,)}
THREADS = {512: 64, 1024: 128, 2048: 256, 4096: 256}  # (launch_pulses of wc_synthesis.hip)


@pytest.fixture(scope="module")
def mp():
    import world_class_amd as w
    L = w.lib()
    dp = C.POINTER(C.c_double)
    L.wc_debug_minimum_phase.restype = C.c_int
    L.wc_debug_minimum_phase.argtypes = [C.c_int, C.c_int, C.c_int, dp, dp]

    def run(form, n, ls, rc_only=False):
        ls = np.ascontiguousarray(np.atleast_2d(ls), dtype=np.float64)
        batch = ls.shape[0]
        out = np.full((batch, n // 2 + 1, 2), np.nan)
        rc = L.wc_debug_minimum_phase(form, n, batch, ls.ctypes.data_as(dp), out.ctypes.data_as(dp))
        if rc_only:
            return rc
        assert rc == 0, w.last_error()
        return out[..., 0] + 1j * out[..., 1]
    return run


def worst(got, want):
    return (np.abs(got - want) / np.abs(want)).max()


def check(got, want, what):
    print("%s: max |device - rule| / |rule| = %.3g" % (what, worst(got, want)))
    bad = np.argwhere(~(np.abs(got - want) <= BOUND * np.abs(want)))
    assert len(bad) == 0, "%s: %d bins beyond the bound, first (spectrum, bin) %s" % (what, len(bad), bad[0])


def one_bin_indices(n, form):
    m, t = n // 2, THREADS[n]
    if form == 1:
        return np.arange(m + 1)
    rng = np.random.default_rng(n)
    named = [0, 1, 2, t - 1, t, t + 1, m // 2 - 1, m // 2, m // 2 + 1, m - 2, m - 1, m]
    rest = np.setdiff1d(np.arange(m + 1), named)
    return np.concatenate([named, rng.choice(rest, 64, replace=False)])


@pytest.mark.parametrize("a", [3.0, -3.0])
@pytest.mark.parametrize("n", rule.SIZES)
def test_one_bin_at_a_time(mp, n, a):
    m = n // 2
    for form in FORMS[n]:
        ks = one_bin_indices(n, form)
        ls = np.zeros((len(ks), m + 1))
        ls[np.arange(len(ks)), ks] = a
        got = mp(form, n, ls)
        check(got, rule.minimum_phase(ls, n), "n = %d form %d, %+.0f in one bin (%d spectra)" % (n, form, a, len(ks)))
        assert (got[:, 0].imag == 0.0).all() and (got[:, m].imag == 0.0).all()


def spectra(n):
    names = ["%s" % k for k in rule.KINDS] + ["flat", "floor", "zeros"]
    ls = np.stack([rule.fixture_input(k, n) for k in rule.KINDS] + [rule.extra_input(k, n) for k in ("flat", "floor", "zeros")])
    return names, ls


@pytest.mark.parametrize("n", rule.SIZES)
def test_spectra_against_the_rule_and_between_forms(mp, n):
    m = n // 2
    names, ls = spectra(n)
    z = np.load(rule.FIXTURE)
    for i, k in enumerate(rule.KINDS):
        assert np.array_equal(ls[i], z[f"{k}/in_{n}"])
    assert ls[4].min() < -18.0 and ls[4].max() == 2.0 and np.abs(rule.log_minimum_phase(ls[4], n).imag).max() > 16.0  # (the floor)
    want = rule.minimum_phase(ls, n)
    got = {}
    for form in FORMS[n]:
        got[form] = mp(form, n, ls)
        for i, name in enumerate(names):
            check(got[form][i:i + 1], want[i:i + 1], "n = %d form %d, %s" % (n, form, name))
        assert (got[form][:, 0].imag == 0.0).all() and (got[form][:, m].imag == 0.0).all()
        print("n = %d form %d: worst of the six spectra %.3g" % (n, form, worst(got[form], want)))
    if len(got) == 2:
        d = np.abs(got[0] - got[1])
        print("n = %d: max |form 0 - form 1| / |.| = %.3g" % (n, (d / np.abs(want)).max()))
        assert (d <= BOUND * np.minimum(np.abs(got[0]), np.abs(got[1]))).all()


@pytest.mark.parametrize("n", rule.SIZES)
def test_a_batch_equals_its_spectra_one_at_a_time(mp, n):
    m = n // 2
    _, ls = spectra(n)
    delta = np.zeros((2, m + 1))
    delta[0, m // 2 + 1] = 3.0
    delta[1, m] = -3.0
    ls = np.concatenate([ls, delta])
    for form in FORMS[n]:
        together = mp(form, n, ls)
        for i in range(len(ls)):
            alone = mp(form, n, ls[i])
            assert np.array_equal(alone.view(np.float64), together[i:i + 1].view(np.float64)), (n, form, i)


def test_other_forms_and_sizes_are_refused(mp):
    WC_ERR_UNSUPPORTED = -3  # include/world_class_c.h
    for form, n in ((0, 256), (0, 8192), (0, 1000), (1, 512), (1, 4096), (2, 1024), (-1, 2048)):
        assert mp(form, n, np.zeros(n // 2 + 1), rc_only=True) == WC_ERR_UNSUPPORTED, (form, n)
