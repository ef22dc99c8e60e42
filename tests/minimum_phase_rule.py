"""MinimumPhaseAnalysis (reference src/world_common.cpp:196-233) as a rule in numpy float64, written from the reference's description
and held to the compiled reference by tests/test_minimum_phase_rule.py; the -m gpu tests hold the device forms to it:

    mirror the log spectrum ls[0 .. M] to N = 2 M points          (reference :199-200)
    transform with e^{+i} (the reference's forward transform)     (:205)
    take the real part: the cepstrum of a real even sequence is real; what the reference carries in the imaginary parts is its
        transform's rounding noise, which it conjugates and doubles (:207-213) -- 1e-16 of the real parts
    keep bins 0 and M, double bins 1 .. M-1, zero the upper half  (:207-217)
    transform with e^{+i} again                                   (:219)
    exp(. / N) of the complex values on bins 0 .. M               (:224-232)

Also the inputs the tests and the fixture share (oracle/gen_golden_minphase.py writes what the real reference returns for them to
tests/golden/minphase_sizes.npz)."""
import os

import numpy as np

SIZES = (512, 1024, 2048, 4096)
KINDS = ("envelope", "notch", "noise")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "minphase_sizes.npz")


def forward(x):
    """X[k] = sum_n x[n] e^{+2 pi i k n / N}, unnormalised, along the last axis"""
    return np.fft.ifft(x, axis=-1) * x.shape[-1]


def log_minimum_phase(ls, n):
    """ls: (..., n/2+1) log spectra; returns the (..., n/2+1) complex logarithms of their minimum-phase spectra: ls + i phase"""
    ls = np.asarray(ls, dtype=np.float64)
    m = n // 2
    assert ls.shape[-1] == m + 1
    full = np.concatenate([ls, ls[..., m - 1:0:-1]], axis=-1)
    cep = forward(full).real
    cep[..., 1:m] *= 2.0
    cep[..., m + 1:] = 0.0
    return forward(cep)[..., :m + 1] / n


def minimum_phase(ls, n):
    """ls: (..., n/2+1) log spectra; returns (..., n/2+1) complex minimum-phase spectra"""
    return np.exp(log_minimum_phase(ls, n))


def fixture_input(kind, n):
    """the fixture's three log spectra per size: a log envelope with formants, a -6 tilt and noise; a notch of depth 35 (-1 down to
    -36) five bins wide; 0.5 N(0, 1)"""
    m = n // 2
    rng = np.random.default_rng(1000 * KINDS.index(kind) + n)
    k = np.arange(m + 1) / m
    if kind == "envelope":
        ls = -6.0 * k + 0.05 * rng.normal(size=m + 1)
        for c, w, a in ((0.04, 0.012, 3.0), (0.11, 0.02, 2.2), (0.23, 0.03, 1.6), (0.62, 0.05, 1.0)):
            ls = ls + a * np.exp(-((k - c) / w) ** 2)
        return ls
    if kind == "notch":
        ls = np.full(m + 1, -1.0)
        c = m // 3
        ls[c - 2:c + 3] = -36.0
        return ls
    return 0.5 * rng.normal(size=m + 1)


def extra_input(kind, n):
    """further inputs of the GPU test: a flat spectrum; one with a 1e-16 power floor, ls from -18 to +2, where the phases pass
    16 radians; all zeros, whose minimum-phase spectrum is exactly 1 + 0i"""
    m = n // 2
    k = np.arange(m + 1) / m
    if kind == "flat":
        return np.full(m + 1, -2.5)
    if kind == "floor":
        # log(sqrt(power)) of a resonance of height 2 over a floor of 1e-16 in power (0.5 log 1e-16 = -18.4): phases up to 16.5 radians
        power = 1e-16 + np.exp(2.0 * 2.0) * np.exp(-((k - 0.25) / 0.05) ** 2)
        return 0.5 * np.log(power)
    assert kind == "zeros"
    return np.zeros(m + 1)
