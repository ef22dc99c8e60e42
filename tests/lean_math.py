"""What tests/test_lean_math.py (host twins, no device) and tests/test_gpu_lean_math.py (-m gpu) share: the seeded inputs of the lean
sin / cos of wc_wavefft.hpp, a wide reference for them, and the binding of the development hooks wc_debug_lean_math and
wc_debug_interp1q (wc_testhooks.hip).

The reference is numpy's longdouble where it carries at least 63 mantissa bits (x87 extended: 2^-64 relative, a two-thousandth of a
double's ulp); elsewhere mpmath at 50 digits on a seeded subset of 1e5 points."""
import ctypes as C
import functools

import numpy as np

LD = np.longdouble
WIDE = np.finfo(LD).nmant >= 63
SUBSET = 100000  # points per set without a wide longdouble
N_PI2 = 70000  # the doubles next to n pi/2 for |n| <= N_PI2
PI_LD = LD("3.14159265358979323846264338327950288")


def _subset(x, seed):
    if WIDE or len(x) <= SUBSET:
        return x
    return x[np.sort(np.random.default_rng(seed).choice(len(x), SUBSET, replace=False))]


def neighbours(x, k=3):
    """x with its k nearest doubles on each side"""
    out, lo, hi = [x], x, x
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def sincos_sets():
    """{name: float64 inputs} of wf_sincos: 2^20 uniform samples in each of +-0.78, +-10, +-1e3, +-1e5 and the doubles nearest n pi/2,
    |n| <= 70000, with three neighbours on each side"""
    rng = np.random.default_rng(20240)
    sets = {"+-%g" % r: rng.uniform(-r, r, 1 << 20) for r in (0.78, 10.0, 1e3, 1e5)}
    n = np.arange(-N_PI2, N_PI2 + 1)
    if WIDE:
        near = (n.astype(LD) * (PI_LD / 2)).astype(np.float64)
    else:
        import mpmath
        mpmath.mp.dps = 50
        near = np.array([float(int(k) * mpmath.pi / 2) for k in n])
    sets["n pi/2"] = neighbours(near)
    return {k: _subset(v, i) for i, (k, v) in enumerate(sets.items())}


@functools.lru_cache(maxsize=None)
def sincospi_sets():
    """{name: float64 inputs} of wf_sincospi: 2^20 uniform samples in each of +-0.25, +-4, +-2048, +-1e6 and every k/2 and k/4,
    |k| <= 8192"""
    rng = np.random.default_rng(20241)
    sets = {"+-%g" % r: rng.uniform(-r, r, 1 << 20) for r in (0.25, 4.0, 2048.0, 1e6)}
    k = np.arange(-8192, 8193, dtype=np.float64)
    sets["k/2, k/4"] = np.concatenate([k / 2, k / 4])
    return {k_: _subset(v, 10 + i) for i, (k_, v) in enumerate(sets.items())}


def _wide_sincos(x, pi):
    """(sin, cos) of x, or of pi x, as longdouble (WIDE only).  For pi x the reduction n = rint(2 x), r = x - n / 2 is exact in double;
    then the wide sin / cos of pi r, |r| <= 1/4, and the quadrant"""
    if not pi:
        x = np.asarray(x, dtype=LD)
        return np.sin(x), np.cos(x)
    x = np.asarray(x, dtype=np.float64)
    n = np.rint(2 * x)
    r = x - n / 2
    assert np.array_equal(r + n / 2, x) and (np.abs(r) <= 0.25).all()
    r = r.astype(LD) * PI_LD
    s, c = np.sin(r), np.cos(r)
    q = np.mod(n, 4).astype(np.int64)
    return np.choose(q, [s, c, -s, -c]), np.choose(q, [c, -s, -c, s])


def _errors(x, s, c, pi):
    """|s - sin|, |c - cos|, and the same in units of the spacing of doubles at the true values; float64 arrays"""
    x, s, c = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, s, c))
    if WIDE:
        want = _wide_sincos(x, pi)
        err = [np.abs(got.astype(LD) - w) for got, w in zip((s, c), want)]
        ulp = [np.spacing(np.abs(w.astype(np.float64))).astype(LD) for w in want]
        return (err[0].astype(np.float64), err[1].astype(np.float64),
                (err[0] / ulp[0]).astype(np.float64), (err[1] / ulp[1]).astype(np.float64))
    import mpmath
    mpmath.mp.dps = 50
    fs, fc = (mpmath.sinpi, mpmath.cospi) if pi else (mpmath.sin, mpmath.cos)
    res = np.empty((4, len(x)))
    for i in range(len(x)):
        v = mpmath.mpf(float(x[i]))
        for j, (f, got) in enumerate(((fs, s[i]), (fc, c[i]))):
            want = f(v)
            e = abs(mpmath.mpf(float(got)) - want)
            res[j, i] = float(e)
            res[2 + j, i] = float(e / mpmath.mpf(float(np.spacing(abs(float(want))))))
    return res[0], res[1], res[2], res[3]


def sincos_errors(x, s, c):
    return _errors(x, s, c, False)


def sincospi_errors(x, s, c):
    return _errors(x, s, c, True)


class Hooks:
    def __init__(self):
        import world_class_amd as w
        self.w = w
        self.L = w.lib()
        self.dp = C.POINTER(C.c_double)
        self.L.wc_debug_lean_math.restype = C.c_int
        self.L.wc_debug_lean_math.argtypes = [C.c_int, C.c_longlong, self.dp, self.dp]
        self.L.wc_debug_interp1q.restype = C.c_int
        self.L.wc_debug_interp1q.argtypes = [C.c_int, C.c_double, C.c_double, self.dp, C.c_int, C.c_longlong, self.dp, self.dp]

    def lean(self, kind, x):
        """kinds 0 / 1 (device) and 4 / 5 (host twins): (sin, cos) of wf_sincos / wf_sincospi; 2 / 3: wf_log_l / wf_exp_l"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        two = kind in (0, 1, 4, 5)
        out = np.full((2 if two else 1, x.size), np.nan)
        rc = self.L.wc_debug_lean_math(kind, x.size, x.ctypes.data_as(self.dp), out.ctypes.data_as(self.dp))
        assert rc == 0, self.w.last_error()
        return (out[0], out[1]) if two else out[0]

    def interp1q(self, kind, x0, dx, y, xi):
        y = np.ascontiguousarray(y, dtype=np.float64)
        xi = np.ascontiguousarray(xi, dtype=np.float64)
        out = np.full(xi.size, np.nan)
        rc = self.L.wc_debug_interp1q(kind, x0, dx, y.ctypes.data_as(self.dp), y.size, xi.size, xi.ctypes.data_as(self.dp),
                                      out.ctypes.data_as(self.dp))
        assert rc == 0, self.w.last_error()
        return out
