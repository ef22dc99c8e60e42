"""The numpy rule of MinimumPhaseAnalysis (tests/minimum_phase_rule.py) against the real reference: the fixture
tests/golden/minphase_sizes.npz (oracle/gen_golden_minphase.py: 512 .. 4096 points, an envelope, a deep notch, noise) and the
1024-point golden minphase/*.  Per bin |rule - ref| <= 1e-13 |ref|; measured against the built reference on these inputs and a flat
spectrum: worst 7.7e-15 (the notch at 1024 points; flat is exact), the rounding of two transforms of a few thousand points and one
exp; an earlier measurement on other draws of the same three kinds found 1.42e-14, a margin of 7.  Needs no device: the
-m gpu tests (tests/test_gpu_minimum_phase.py) hold the device forms to this rule."""
import numpy as np
import pytest

import minimum_phase_rule as rule

BOUND = 1e-13


@pytest.fixture(scope="module")
def fixture():
    return np.load(rule.FIXTURE)


def rel(got, want):
    return (np.abs(got - want) / np.abs(want)).max()


@pytest.mark.parametrize("n", rule.SIZES)
def test_rule_matches_the_reference_fixture(fixture, n):
    for kind in rule.KINDS:
        ls = fixture[f"{kind}/in_{n}"]
        assert np.array_equal(ls, rule.fixture_input(kind, n)), "the input generator drifted from the fixture"
        want = fixture[f"{kind}/out_{n}"]
        want = want[:, 0] + 1j * want[:, 1]
        assert want.shape == (n // 2 + 1,) and np.isfinite(want).all() and (np.abs(want) > 0).all()
        got = rule.minimum_phase(ls, n)
        d = rel(got, want)
        print("n = %d %s: max |rule - ref| / |ref| = %.3g" % (n, kind, d))
        assert (np.abs(got - want) <= BOUND * np.abs(want)).all()


def test_rule_matches_the_1024_point_golden(golden):
    want = golden["minphase/out_1024"][:513]
    want = want[:, 0] + 1j * want[:, 1]
    got = rule.minimum_phase(golden["minphase/in_1024"][:513], 1024)
    print("golden 1024: max |rule - ref| / |ref| = %.3g" % rel(got, want))
    assert (np.abs(got - want) <= BOUND * np.abs(want)).all()


@pytest.mark.parametrize("n", rule.SIZES)
def test_rule_properties(n):
    """a flat log spectrum c gives exp(c) + 0i in every bin, zeros give exactly 1; bins 0 and M are real; batches are row by row"""
    m = n // 2
    flat = rule.minimum_phase(rule.extra_input("flat", n), n)
    assert np.abs(flat - np.exp(-2.5)).max() <= 4e-16 * np.exp(-2.5)
    assert np.array_equal(rule.minimum_phase(np.zeros(m + 1), n), np.ones(m + 1, dtype=complex))
    ls = np.stack([rule.fixture_input(k, n) for k in rule.KINDS] + [rule.extra_input("floor", n)])
    got = rule.minimum_phase(ls, n)
    assert np.abs(got[:, [0, m]].imag).max() <= 1e-15 * np.abs(got[:, [0, m]]).min()
    for i in range(len(ls)):
        assert np.array_equal(got[i], rule.minimum_phase(ls[i], n))
    # the magnitude of a minimum-phase spectrum is the exponential of the log spectrum it came from
    assert (np.abs(np.log(np.abs(got)) - ls) <= 1e-13 * np.maximum(1.0, np.abs(ls))).all()
