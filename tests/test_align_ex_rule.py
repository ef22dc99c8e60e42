"""CPU tests that pin the rule of extended feature alignment (tests/align_ex_rule.py, the checker of tests/test_gpu_align_ex.py):
it is the old rule at pattern 0 and flags 0, it finds the minimum over every path an exhaustive recursion walks, its paths and maps
are monotone, and the slope limit of pattern 1 is feasible exactly where it should be."""
import itertools

import numpy as np
import pytest

import align_ex_rule as ax
import align_rule as ar

INF = float("inf")


def _feats(n, dims, seed):
    return np.random.default_rng(seed).standard_normal((n, dims))


@pytest.mark.parametrize("band", [0, 2])
@pytest.mark.parametrize("n,m", [(1, 1), (1, 7), (7, 1), (12, 19), (23, 9)])
def test_pattern_0_without_flags_is_the_old_rule(n, m, band):
    a, b = _feats(n, 5, 3 * n + m), _feats(m, 5, 3 * m + n)
    old, new = ar.align(a, b, 1, 5, band), ax.align(a, b, 1, 5, band, 0, 0)
    assert old["cost"] == new["cost"] and np.array_equal(old["path"], new["path"])
    assert old["b_on_a"].tobytes() == new["b_on_a"].tobytes() and old["a_on_b"].tobytes() == new["a_on_b"].tobytes()
    assert new["span"].tolist() == [0, m - 1]
    assert np.array_equal(new["timeline_a"], new["path"][:, 0]) and np.array_equal(new["timeline_b"], new["path"][:, 1])


def _moves(step_pattern):
    """a step forward as the cells it adds, relative to the cell it leaves"""
    if step_pattern == 0:
        return [[(1, 1)], [(1, 0)], [(0, 1)]]
    return [[(1, 1)], [(1, 1), (2, 1)], [(1, 1), (1, 2)]]


def _every_path(n, m, step_pattern, flags):
    """every path of the rule as a list of cells, by plain recursion"""
    def walk(cells):
        i, j = cells[-1]
        if i == n - 1 and (j == m - 1 or flags & ax.OPEN_END):
            yield cells
        for mv in _moves(step_pattern):
            nxt = [(i + di, j + dj) for di, dj in mv]
            if nxt[-1][0] < n and nxt[-1][1] < m:
                yield from walk(cells + nxt)
    for j0 in range(m if flags & ax.OPEN_BEGIN else 1):
        yield from walk([(0, j0)])


@pytest.mark.parametrize("step_pattern", [0, 1])
def test_the_cost_is_the_minimum_over_every_path(step_pattern):
    """all shapes from 1 x 1 to 6 x 8, all four flag values, integer-valued costs (sums are exact): 192 cases per pattern"""
    rng = np.random.default_rng(68 + step_pattern)
    cases = 0
    for n, m, flags in itertools.product(range(1, 7), range(1, 9), range(4)):
        d = rng.integers(0, 10, (n, m)).astype(np.float64)
        r = ax.align(None, None, 0, 0, 0, step_pattern, flags, costs=d)
        least = min((sum(d[c] for c in p) for p in _every_path(n, m, step_pattern, flags)), default=INF)
        assert r["cost"] == least, (n, m, flags)
        cases += 1
        if least == INF:
            assert len(r["path"]) == 0 and r["span"].tolist() == [-1, -1] and np.isnan(r["b_on_a"]).all() and np.isnan(r["a_on_b"]).all()
            continue
        path = r["path"]
        assert sum(d[i, j] for i, j in path) == least
        assert max(n, path[-1, 1] - path[0, 1] + 1) <= len(path) <= n + m - 1
        assert path[0, 0] == 0 and path[-1, 0] == n - 1
        assert path[0, 1] == 0 or flags & ax.OPEN_BEGIN
        assert path[-1, 1] == m - 1 or flags & ax.OPEN_END
        assert r["span"].tolist() == [path[0, 1], path[-1, 1]]
        assert (np.diff(r["b_on_a"]) >= 0).all() and (np.diff(r["a_on_b"]) >= 0).all()
    assert cases == 192


@pytest.mark.parametrize("step_pattern,flags", [(0, 0), (0, 3), (1, 0), (1, 1), (1, 2), (1, 3)])
@pytest.mark.parametrize("n,m", [(1, 1), (9, 1), (1, 9), (21, 30), (30, 21), (12, 40)])
def test_paths_step_by_one_and_maps_do_not_decrease(n, m, step_pattern, flags):
    r = ax.align(_feats(n, 6, 10 * n + m), _feats(m, 6, 10 * m + n), 1, 6, 0, step_pattern, flags)
    if not np.isfinite(r["cost"]):
        assert step_pattern == 1 and len(r["path"]) == 0
        return
    path = r["path"]
    steps = np.diff(path, axis=0)
    assert ((steps >= 0) & (steps <= 1)).all() and (steps.sum(axis=1) >= 1).all()
    assert len(path) <= n + m - 1
    j0, j1 = r["span"]
    assert (r["a_on_b"][:j0] == 0.0).all() and (r["a_on_b"][j1 + 1:] == n - 1).all()
    for mp in (r["b_on_a"], r["a_on_b"]):
        assert np.array_equal(mp * 2, np.round(mp * 2)) and (np.diff(mp) >= 0).all()
    if step_pattern == 1:  # no row and no column holds more than two cells of the path
        assert np.bincount(path[:, 0]).max() <= 2 and np.bincount(path[:, 1]).max() <= 2


@pytest.mark.parametrize("n,m,finite", [(10, 19, True), (10, 20, False), (1, 2, False), (3, 5, True), (3, 6, False),
                                        (19, 10, True), (20, 10, False)])
def test_pattern_1_closed_is_finite_exactly_within_slope_2(n, m, finite):
    assert finite == (max(n, m) - 1 <= 2 * (min(n, m) - 1))
    r = ax.align(_feats(n, 4, n), _feats(m, 4, m), 0, 4, 0, 1, 0)
    if finite:
        assert np.isfinite(r["cost"]) and r["path"][0].tolist() == [0, 0] and r["path"][-1].tolist() == [n - 1, m - 1]
    else:
        assert r["cost"] == INF and len(r["path"]) == 0 and np.isnan(r["b_on_a"]).all() and np.isnan(r["a_on_b"]).all()
        assert r["span"].tolist() == [-1, -1] and len(r["timeline_a"]) == 0 and len(r["timeline_b"]) == 0


def test_open_ends_find_a_phrase_inside_a_track():
    """B holds A between other rows: with both ends open the cost is 0 and the span is where A lies; closed it is not"""
    q, pre, post = _feats(11, 4, 1), _feats(6, 4, 2), _feats(8, 4, 3)
    track = np.concatenate([pre, q, post])
    for step_pattern in (0, 1):
        r = ax.align(q, track, 0, 4, 0, step_pattern, 3)
        assert r["cost"] == 0.0 and r["span"].tolist() == [6, 16]
        assert np.array_equal(r["path"], np.stack([np.arange(11), np.arange(6, 17)], axis=1))
        assert r["a_on_b"].tolist() == [0.0] * 6 + list(range(11)) + [10.0] * 8
        assert ax.align(q, track, 0, 4, 0, step_pattern, 0)["cost"] > 0.0


@pytest.mark.parametrize("step_pattern,band,flags", [(0, 0, 0), (0, 2, 0), (0, 0, 3), (1, 0, 0), (1, 3, 0), (1, 0, 1), (1, 0, 2), (1, 0, 3)])
def test_the_invariants_helper_accepts_the_rule_and_refuses_what_is_wrong(step_pattern, band, flags):
    """tests/align_checks.py judges the device's outputs against each other; here it judges the rule's, which are right, and a few
    results that are wrong in one respect each"""
    import align_checks as ac
    refused = 0
    for n, m in [(1, 1), (2, 2), (2, 3), (3, 2), (1, 6), (6, 1), (9, 14), (14, 9), (21, 40), (33, 65)]:
        a, b = _feats(n, 7, 100 * n + m), _feats(m, 7, 100 * m + n)
        r = ac.rule_outputs(ax.align(a, b, 1, 6, band, step_pattern, flags))
        ac.check_alignment_outputs(a, b, (1, 6), band, step_pattern, flags, r)
        if r["K"] < 4:
            continue
        wrong = [dict(r, cost=np.nextafter(r["cost"], INF)), dict(r, path=r["path"][1:], K=r["K"] - 1),
                 dict(r, span=r["span"] + np.array([0, 1], dtype=np.int32)), dict(r, b_on_a=r["b_on_a"] + 0.5),
                 dict(r, timeline_b=r["timeline_b"] + 1.0)]
        k = r["K"] // 2  # a cell of the path moved off it: an illegal step, or a sum and maps that are another path's
        moved = r["path"].copy()
        moved[k, 1] += 1 if moved[k, 1] + 1 < m else -1
        wrong.append(dict(r, path=moved))
        for w in wrong:
            with pytest.raises(AssertionError):
                ac.check_alignment_outputs(a, b, (1, 6), band, step_pattern, flags, w)
            refused += 1
    assert refused >= 12
    if step_pattern == 1 and flags == 0 and band == 0:  # a path of pattern 0 with two straight steps in a row is no path of pattern 1
        a, b = _feats(9, 7, 1), _feats(14, 7, 2)
        r0 = ac.rule_outputs(ax.align(a, b, 1, 6, 0, 0, 0))
        steps = np.diff(r0["path"], axis=0)
        assert ((steps.sum(axis=1) == 1)[1:] & (steps.sum(axis=1) == 1)[:-1]).any()
        ac.check_alignment_outputs(a, b, (1, 6), 0, 0, 0, r0)
        with pytest.raises(AssertionError):
            ac.check_alignment_outputs(a, b, (1, 6), 0, 1, 0, r0)


def test_the_batch_form_walks_the_packed_arrays():
    a, b = _feats(10 + 4, 3, 1), _feats(6 + 9, 3, 2)
    both = ax.align_batch([10, 4], a, [6, 9], b, 0, 3, 0, 1, 3)
    one = ax.align(a[10:], b[6:], 0, 3, 0, 1, 3)
    assert both[1]["cost"] == one["cost"] and np.array_equal(both[1]["path"], one["path"])
