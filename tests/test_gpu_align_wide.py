"""-m gpu: extended feature alignment where a lane's strip is wider than one round of eight cells (AL_CHUNK), against the rule
(tests/align_ex_rule.py) bit for bit and against the device's own outputs (tests/align_checks.py): strips of 8, 9, 10 and 17
columns under step pattern 1 and of 8, 9, 17 and 65 under pattern 0, free and under bands whose edge falls inside a strip, open
ends at those widths, ties of the open-end scan that are certain (the same phrase twice in one track), and dimension windows of
exactly 32, 33, 64 and 96 coefficients.  The band cases run behind a call that leaves NaN in the whole scratch."""
import numpy as np
import pytest

import align_checks as ac
import align_ex_rule as ax
from test_gpu_align_ex import _align, _random_batch, env  # noqa: F401 (env is the module's fixture)

pytestmark = pytest.mark.gpu
# strips under pattern 1 are max(2, ceil(m / 64)) columns: 8 (one full round), 2, 9 (one cell into the second round, the last lane's
# strip not full), 2, 10 and 10; n as small as m - 1 <= 2 * (n - 1) allows, and the small pairs between the wide ones make the offsets odd
SLOPE_WIDE = [(257, 512), (3, 4), (258, 513), (1, 1), (300, 577), (450, 600)]
# strips under pattern 0 are ceil(m / 64) columns: 8, 9, 1, 17 and 65 (eight rounds and one cell)
PLAIN_WIDE = [(40, 512), (40, 513), (5, 3), (24, 1025), (9, 4097)]
BATCHES = {"slope": (SLOPE_WIDE, 20270), "plain": (PLAIN_WIDE, 20271), "one": ([(520, 1025)], 20272)}
_batches, _rules = {}, {}


def _batch(name):
    """a ragged batch of random rows at dims = 60, made once and left unchanged"""
    if name not in _batches:
        _batches[name] = _random_batch(BATCHES[name][0], 60, BATCHES[name][1])
    return _batches[name]


def _rule(name, band, pattern, flags):
    """the rule's answer for a batch, worked out once per setting"""
    key = (name, band, pattern, flags)
    if key not in _rules:
        a_lens, fa, b_lens, fb = _batch(name)
        _rules[key] = ax.align_batch(a_lens, fa, b_lens, fb, 1, 60, band, pattern, flags)
    return _rules[key]


def _strip(m, pattern):
    return max(2, -(-m // 64)) if pattern else -(-m // 64)


def test_the_shapes_have_the_strips_they_are_here_for():
    assert [_strip(m, 1) for _, m in SLOPE_WIDE] == [8, 2, 9, 2, 10, 10] and _strip(1025, 1) == 17
    assert [_strip(m, 0) for _, m in PLAIN_WIDE] == [8, 9, 1, 17, 65]
    assert all(max(n, m) - 1 <= 2 * (min(n, m) - 1) for n, m in SLOPE_WIDE + [(520, 1025)])
    assert -(-513 // 9) == 57 and 513 - 56 * 9 == 9 and -(-577 // 10) == 58 and 577 - 57 * 10 == 7  # (the last strip of m = 577 is not full)


@pytest.mark.parametrize("band", [0, 1, 7])
def test_pattern_1_wide_strips_in_one_ragged_batch_equal_the_rule(env, band):
    want = _rule("slope", band, 1, 0)
    got = ac.checked_align(env, _batch("slope"), 60, (1, 60), band, 1, 0, want, poison=band > 0)
    assert all(np.isfinite(r["cost"]) for r in want) and np.isfinite(got[0][:len(want)]).all()
    if band:  # the band binds: it is not the free case under another name
        free = _rule("slope", 0, 1, 0)
        wide = [u for u, (_, m) in enumerate(SLOPE_WIDE) if m > 64]
        assert any(not np.array_equal(want[u]["path"], free[u]["path"]) for u in wide)
        assert all(r["cost"] >= f["cost"] for r, f in zip(want, free))


@pytest.mark.parametrize("band", [0, 1])
def test_pattern_1_a_strip_of_two_rounds_and_one_cell(env, band):
    want = _rule("one", band, 1, 0)
    ac.checked_align(env, _batch("one"), 60, (1, 60), band, 1, 0, want, poison=band > 0)
    assert np.isfinite(want[0]["cost"])
    if band:
        assert not np.array_equal(want[0]["path"], _rule("one", 0, 1, 0)[0]["path"])


@pytest.mark.parametrize("band", [0, 3, 50])
def test_pattern_0_wide_strips_in_one_ragged_batch_equal_the_rule(env, band):
    want = _rule("plain", band, 0, 0)
    ac.checked_align(env, _batch("plain"), 60, (1, 60), band, 0, 0, want, poison=band > 0)
    assert all(np.isfinite(r["cost"]) for r in want)
    if band == 3:
        free = _rule("plain", 0, 0, 0)
        assert any(not np.array_equal(r["path"], f["path"]) for r, f in zip(want, free))


@pytest.mark.parametrize("name,pattern,flags", [(("plain", "slope")[p], p, f) for p in (0, 1) for f in (1, 2, 3)])
def test_open_ends_at_width_equal_the_rule(env, name, pattern, flags):
    """(open ends make no pair of the pattern 1 batch infeasible: all six stay)"""
    want = _rule(name, 0, pattern, flags)
    got = ac.checked_align(env, _batch(name), 60, (1, 60), 0, pattern, flags, want, poison=False)
    assert all(np.isfinite(r["cost"]) and len(r["path"]) for r in want)
    shapes, fb0, found = BATCHES[name][0], 0, []
    for (n, m), r in zip(shapes, want):
        aob = got[4][fb0:fb0 + m]
        fb0 += m
        j0, j1 = r["span"]
        assert (j0 == 0 or flags & ax.OPEN_BEGIN) and (j1 == m - 1 or flags & ax.OPEN_END)
        assert (aob[:j0] == 0.0).all() and (aob[j1 + 1:] == n - 1).all()
        found.append((m, j0, j1))
    assert any(j0 > 0 for _, j0, _ in found) == bool(flags & ax.OPEN_BEGIN)
    assert any(j1 < m - 1 for m, _, j1 in found) == bool(flags & ax.OPEN_END)


# pre, gap, post around the two copies of a query of 40 rows.  The first copy ends at column pre + 39, the second 40 + gap further.
#   (23, 450, 30): columns 62 and 552, 552 % 64 = 40 < 62: the lane with the lower number holds the higher column, and the
#                  cross-lane rounds must prefer the lower column
#   (300, 152, 50): columns 339 and 531 = 339 + 3 * 64: one lane meets both, and only a strict < in its stride loop keeps the first
TWICE = [(23, 450, 30), (300, 152, 50)]


@pytest.mark.parametrize("pattern", [0, 1])
@pytest.mark.parametrize("pre,gap,post", TWICE)
def test_the_same_phrase_twice_ends_at_the_first(env, pre, gap, post, pattern):
    n = 40
    e1, e2 = pre + n - 1, pre + n + gap + n - 1
    assert (e2 % 64 < e1 % 64) if gap == 450 else (e2 == e1 + 3 * 64)
    rng = np.random.default_rng(4000 + pre)
    q = rng.standard_normal((n, 60))
    track = np.concatenate([rng.standard_normal((pre, 60)), q, rng.standard_normal((gap, 60)), q, rng.standard_normal((post, 60))])
    m = len(track)
    assert m > 512 and len(np.unique(q, axis=0)) == n
    got = _align(env, [n], q, [m], track, 60, 1, 60, 0, pattern, 3)
    ac.check_batch([n], q, [m], track, (1, 60), 0, pattern, 3, got)
    cost, plen, path, boa, aob, span, tla, tlb = got
    assert cost[0] == 0.0 and plen[0] == n and span[:2].tolist() == [pre, e1]
    assert np.array_equal(path.reshape(-1, 2)[:n], np.stack([np.arange(n), pre + np.arange(n)], axis=1))
    assert np.array_equal(boa[:n], pre + np.arange(n, dtype=np.float64))
    assert np.array_equal(aob[:m], np.concatenate([np.zeros(pre), np.arange(n, dtype=np.float64), np.full(m - pre - n, n - 1.0)]))
    assert np.array_equal(tla[:n], np.arange(n, dtype=np.float64)) and np.array_equal(tlb[:n], pre + np.arange(n, dtype=np.float64))


LDS_SHAPES = [(33, 65), (64, 31), (2, 2)]
_lds = {}


@pytest.mark.parametrize("band", [0, 2])
@pytest.mark.parametrize("dims,lo,hi", [(40, 3, 35), (40, 3, 36), (64, 0, 64), (97, 1, 97)])
def test_dimension_windows_of_whole_lds_trips(env, dims, lo, hi, band):
    """windows of 32, 33, 64 and 96 coefficients (the cost pass takes 32 per trip through LDS); every column outside the window is
    NaN, so that reading one is seen"""
    assert hi - lo in (32, 33, 64, 96)
    if dims not in _lds:
        a_lens, fa, b_lens, fb = _random_batch(LDS_SHAPES, dims, 20280 + dims)
        _lds[dims] = (a_lens, fa, b_lens, fb)
    a_lens, fa, b_lens, fb = _lds[dims]
    fa, fb = fa.copy(), fb.copy()
    for f in (fa, fb):
        f[:, :lo] = np.nan
        f[:, hi:] = np.nan
    want = ax.align_batch(a_lens, fa, b_lens, fb, lo, hi, band, 1, 0)
    ac.checked_align(env, (a_lens, fa, b_lens, fb), dims, (lo, hi), band, 1, 0, want, poison=band > 0)
    assert [bool(np.isfinite(r["cost"])) for r in want] == [True, False, True]  # (63 > 2 * 30: the rule says so, and the device must)
