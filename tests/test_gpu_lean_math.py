"""-m gpu: the hand-written numerics every CheapTrick, D4C and Synthesis frame passes through, on their own
(wc_debug_lean_math, wc_debug_interp1q of wc_testhooks.hip):

  wf_sincos, wf_sincospi   the device equals the host twin BIT FOR BIT on the inputs of tests/test_lean_math.py, which holds the twin to
                           a wide reference (2^-52 absolute, 2 ulp): the bodies use only fma, rint, products and sums, the library is
                           compiled without contraction, so any difference is a different fma or a contraction -- a finding, not a
                           tolerance
  wf_log_l, wf_exp_l       the forms the hot path uses, on the copy of the tables wf_tables_to_lds makes in LDS (160 double2 entries:
                           the exp table has to follow the log table), equal the global-table forms wf_log / wf_exp bit for bit on the
                           inputs of test_lean_log_and_exp (tests/test_gpu_wavefft.py), special values included
  interp1q_rcp, wf_interp1q  equal each other bit for bit everywhere, the last knot included (one tests b == n - 1, the other clamps
                           the index), and lie within rounding noise of interp1q, the reference's division, which itself equals the
                           real reference's interp1Q bit for bit on the golden's inputs."""
import ctypes as C

import numpy as np
import pytest

import lean_math as lm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hooks():
    h = lm.Hooks()
    dp = C.POINTER(C.c_double)
    h.L.wc_debug_logexp.restype = C.c_int
    h.L.wc_debug_logexp.argtypes = [C.c_int, C.c_longlong, dp, dp]

    def logexp(kind, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.full(x.size, np.nan)
        assert h.L.wc_debug_logexp(kind, x.size, x.ctypes.data_as(dp), out.ctypes.data_as(dp)) == 0, h.w.last_error()
        return out
    h.logexp = logexp
    return h


def same_bits(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def differing(a, b):
    return np.flatnonzero(a.view(np.uint64) != b.view(np.uint64))


@pytest.mark.parametrize("kind,sets", [(0, "sincos_sets"), (1, "sincospi_sets")])
def test_device_sincos_equals_the_host_twin_bit_for_bit(hooks, kind, sets):
    name = ("wf_sincos", "wf_sincospi")[kind]
    for label, x in getattr(lm, sets)().items():
        ds, dc = hooks.lean(kind, x)
        hs, hc = hooks.lean(kind + 4, x)
        bad = np.union1d(differing(ds, hs), differing(dc, hc))
        print("%s %-8s %7d points: device differs from the host twin at %d" % (name, label, len(x), len(bad)))
        assert len(bad) == 0, "%s %s: first difference at x = %r: device (%r, %r), twin (%r, %r)" % (
            name, label, x[bad[0]], ds[bad[0]], dc[bad[0]], hs[bad[0]], hc[bad[0]])


def test_device_sincos_passes_nan(hooks):
    for kind in (0, 1):
        s, c = hooks.lean(kind, np.array([np.nan, 0.0, 1.0, -np.nan]))
        assert np.isnan(s[0]) and np.isnan(c[0]) and np.isnan(s[3]) and np.isnan(c[3])
        assert s[1] == 0.0 and c[1] == 1.0 and np.isfinite(s[2]) and np.isfinite(c[2])


def test_lds_table_log_and_exp_equal_the_global_table_forms(hooks):
    # (the inputs of test_lean_log_and_exp, tests/test_gpu_wavefft.py)
    rng = np.random.default_rng(11)
    x = np.concatenate([10.0 ** rng.uniform(-300, 300, 200000), rng.uniform(0.5, 2.0, 200000), 1.0 + rng.uniform(-1e-3, 1e-3, 50000),
                        [1.0, 0.5, 2.0, 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308],
                        [0.0, -1.0, np.inf, np.nan]])
    # every one of the 128 table entries, at both ends of its interval of mantissas
    i = np.arange(128)
    x = np.concatenate([x, 0.5 + i / 256.0, np.nextafter(0.5 + (i + 1) / 256.0, 0.0)])
    a, b = hooks.lean(2, x), hooks.logexp(0, x)
    bad = differing(a[~np.isnan(b)], b[~np.isnan(b)])
    assert len(bad) == 0 and np.array_equal(np.isnan(a), np.isnan(b)), "wf_log_l differs from wf_log at %d of %d" % (len(bad), len(x))
    special = a[-260:-256]
    assert special[0] == -np.inf and np.isnan(special[1]) and special[2] == np.inf and np.isnan(special[3])
    y = np.concatenate([rng.uniform(-700, 700, 300000), rng.uniform(-1, 1, 100000), [0.0, -745.0, 709.7, -800.0, 800.0], [np.nan],
                        np.arange(-64, 65) * (np.log(2.0) / 64)])  # (every one of the 64 table entries)
    a, b = hooks.lean(3, y), hooks.logexp(1, y)
    ok = ~np.isnan(b)
    bad = differing(a[ok], b[ok])
    assert len(bad) == 0 and np.array_equal(np.isnan(a), np.isnan(b)), "wf_exp_l differs from wf_exp at %d of %d" % (len(bad), len(y))
    assert np.isnan(a[400005]) and a[400004] == np.inf and a[400003] == 0.0 and a[400000] == 1.0
    # an odd count: the last wavefront is partly idle behind its table copy
    assert same_bits(hooks.lean(2, x[:997]), hooks.logexp(0, x[:997]))


# ---- the interpolators -----------------------------------------------------------------------------------------------------------

def tables(golden):
    """(n, x0, dx, y, further abscissae): the golden's table (40 knots) and seeded ones of 2, 128 (a descending axis, as the spectral
    smoothing stages have it: dx = -fs / N) and 1025 knots"""
    rng = np.random.default_rng(77)
    return [(2, 100.0, 0.375, rng.normal(size=2), None),
            (40, 0.5, 0.25, golden["interp1Q/y"], golden["interp1Q/xi"]),
            (128, 3000.0, -44100.0 / 4096.0, rng.normal(size=128), None),
            (1025, -71.5, 48000.0 / 2048.0 / 3.0, np.exp(rng.normal(size=1025) * 3.0), None)]


def abscissae(n, x0, dx, extra, seed):
    knots = x0 + np.arange(n) * dx
    last = x0 + (n - 1) * dx
    lo, hi = min(x0, last), max(x0, last)
    near = np.concatenate([np.nextafter(knots, -np.inf), np.nextafter(knots, np.inf)])
    near = near[(near >= lo) & (near <= hi)]
    xi = [knots, near, [last], np.random.default_rng(seed).uniform(lo, hi, 100000)]
    if extra is not None:
        xi.append(extra)
    xi = np.concatenate(xi)
    assert ((xi >= lo) & (xi <= hi)).all()  # nothing outside the table: the device forms read it unchecked
    return xi


def test_interp1q_division_form_equals_the_reference_golden(hooks, golden):
    got = hooks.interp1q(0, 0.5, 0.25, golden["interp1Q/y"], golden["interp1Q/xi"])
    assert same_bits(got, golden["interp1Q/yi"])


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_reciprocal_interpolators_agree_and_stay_within_rounding_of_the_division(hooks, golden, which):
    n, x0, dx, y, extra = tables(golden)[which]
    assert len(y) == n
    xi = abscissae(n, x0, dx, extra, 100 + n)
    by_div, by_rcp, in_lds = (hooks.interp1q(kind, x0, dx, y, xi) for kind in (0, 1, 2))
    bad = differing(by_rcp, in_lds)
    assert len(bad) == 0, "n = %d: interp1q_rcp and wf_interp1q differ at %d abscissae, first xi = %r" % (n, len(bad), xi[bad[0]])
    # (the last knot: the one form tests b == n - 1, the other clamps the index)
    last = xi == x0 + (n - 1) * dx
    assert last.any()
    q = (xi - x0) / dx
    b = q.astype(np.int64)
    assert b.min() == 0 and b.max() == n - 1  # (the last knot reaches the entry that has no right neighbour)
    b1 = np.minimum(b + 1, n - 1)
    bound = 4.0 * np.spacing(np.maximum(np.abs(y[b]), np.abs(y[b1]))) + np.abs(y[b1] - y[b]) * np.abs(q) * 2.0 ** -51
    d = np.abs(by_rcp - by_div)
    print("n = %d, %d abscissae: max |interp1q_rcp - interp1q| = %.3g, at most %.3g of the bound; equal bits at %d"
          % (n, len(xi), d.max(), (d / bound).max(), (d == 0).sum()))
    assert (d <= bound).all()
    # the division form against the interpolant in wide arithmetic, where there is one: 2.5 ulp of the larger neighbour (the difference,
    # the product and the sum each round once) and the quotient's rounding
    if lm.WIDE:
        w = (xi.astype(lm.LD) - lm.LD(x0)) / lm.LD(dx) - b
        want = y[b].astype(lm.LD) + (y[b1].astype(lm.LD) - y[b].astype(lm.LD)) * w
        assert (np.abs(by_div - want).astype(np.float64) <= bound).all()
