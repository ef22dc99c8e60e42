"""The lean sin / cos of wc_wavefft.hpp (wf_sincos: 44 call sites in CheapTrick, 3 in D4C, 6 in Synthesis; wf_sincospi: the window
phases) through their HOST twins -- the same bodies, __host__ __device__, run by wc_debug_lean_math kinds 4 and 5 -- against a wide
reference (tests/lean_math.py).  Needs no device; tests/test_gpu_lean_math.py holds the device to the twins bit for bit.

Bounds, and what the twins measure on the seeded sets (2^20 uniform samples per range, the doubles next to n pi/2 for |n| <= 70000,
every k/2 and k/4 for |k| <= 8192):
  wf_sincos    absolute error <= 2^-52 = 2.22e-16 on every input        measured 1.70e-16
  wf_sincos    <= 2 ulp for |x| <= pi/4                                  measured 1.24 ulp
  wf_sincospi  <= 2 ulp everywhere                                       measured 1.80 ulp
  wf_sincospi  exactly 0 and +-1 at every half integer                   holds
No set exceeds its bound on the twin, so the bounds stand as set.

What does NOT hold, and is printed instead of asserted:
  wf_sincos next to a multiple of pi/2: the reduction carries about 107 bits of pi/2, so the small one of the two results is off by
  up to 1781 ulp OF ITSELF there (at x = -92133.48775182787; under 4e-27 in absolute terms on that whole set).
  wf_sincospi at odd quarter integers: sin and cos come from two polynomials at |r| = 1/4 and differ in the last bit at every one of
  the 8192 odd quarters tried (both within the 2 ulp bound), so "sin = cos bit for bit" holds nowhere on the twin and is not asserted."""
import numpy as np
import pytest

import lean_math as lm

ABS_BOUND = 2.0 ** -52
ULP_BOUND = 2.0


@pytest.fixture(scope="module")
def hooks():
    return lm.Hooks()


@pytest.fixture(scope="module")
def sincos_results(hooks):
    """{set: (x, |sin error|, |cos error|, sin ulp, cos ulp)}, computed once"""
    out = {}
    for name, x in lm.sincos_sets().items():
        s, c = hooks.lean(4, x)
        out[name] = (x,) + lm.sincos_errors(x, s, c)
    return out


def test_sincos_absolute_error(sincos_results):
    for name, (x, es, ec, us, uc) in sincos_results.items():
        worst = max(es.max(), ec.max())
        print("wf_sincos %-8s %7d points: max absolute error %.3g" % (name, len(x), worst))
        assert (es <= ABS_BOUND).all() and (ec <= ABS_BOUND).all(), name


def test_sincos_ulp_error_within_the_first_octant(sincos_results):
    seen = 0
    for name, (x, es, ec, us, uc) in sincos_results.items():
        small = np.abs(x) <= np.pi / 4
        if not small.any():
            continue
        seen += int(small.sum())
        print("wf_sincos %-8s %7d points in |x| <= pi/4: max %.3g ulp" % (name, small.sum(), max(us[small].max(), uc[small].max())))
        assert (us[small] <= ULP_BOUND).all() and (uc[small] <= ULP_BOUND).all(), name
    assert seen > 1 << 20


def test_sincos_relative_error_next_to_multiples_of_half_pi_is_recorded(sincos_results):
    """a printed number, not a bound: see the module's docstring"""
    x, es, ec, us, uc = sincos_results["n pi/2"]
    worst = np.maximum(us, uc)
    i = int(np.argmax(worst))
    print("wf_sincos next to n pi/2, |n| <= %d: worst relative error %.0f ulp at x = %r (absolute %.3g)"
          % (lm.N_PI2, worst[i], x[i], max(es[i], ec[i])))
    for name, (x, es, ec, us, uc) in sincos_results.items():
        print("wf_sincos %-8s max relative error %.3g ulp" % (name, max(us.max(), uc.max())))


def test_sincospi_ulp_error(hooks):
    for name, x in lm.sincospi_sets().items():
        s, c = hooks.lean(5, x)
        _, _, us, uc = lm.sincospi_errors(x, s, c)
        print("wf_sincospi %-8s %7d points: max %.3g ulp" % (name, len(x), max(us.max(), uc.max())))
        assert (us <= ULP_BOUND).all() and (uc <= ULP_BOUND).all(), name


def test_sincospi_is_exact_at_half_integers_and_recorded_at_odd_quarters(hooks):
    k = np.arange(-8192, 8193)
    s, c = hooks.lean(5, k / 2.0)
    assert np.array_equal(s, np.where(k % 2 == 0, 0.0, np.where(k % 4 == 1, 1.0, -1.0)))
    assert np.array_equal(c, np.where(k % 2 != 0, 0.0, np.where(k % 4 == 0, 1.0, -1.0)))
    ko = k[k % 2 != 0]
    s, c = hooks.lean(5, ko / 4.0)
    same = np.abs(s) == np.abs(c)
    print("wf_sincospi at odd quarter integers: |sin| == |cos| bit for bit at %d of %d" % (same.sum(), len(ko)))
    # (asserted only where it holds on the twin: nowhere; the values are within an ulp of each other and have the right signs)
    assert (np.abs(np.abs(s) - np.abs(c)) <= np.spacing(0.5)).all()
    assert np.array_equal(np.sign(s), np.where((ko % 8) < 4, 1.0, -1.0)) and np.array_equal(np.sign(c), np.where(((ko + 2) % 8) < 4, 1.0, -1.0))


def test_twins_pass_nan_and_zero(hooks):
    for kind in (4, 5):
        s, c = hooks.lean(kind, np.array([np.nan, 0.0, -0.0]))
        assert np.isnan(s[0]) and np.isnan(c[0])
        assert s[1] == 0.0 and c[1] == 1.0 and s[2] == 0.0 and c[2] == 1.0
