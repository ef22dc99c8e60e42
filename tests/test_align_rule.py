"""CPU tests that pin the rule of feature alignment itself (tests/align_rule.py, the checker of tests/test_gpu_align.py): the
diagonal for identical sequences, the path the tie-break dictates, the band, the maps, the bounds of K and what a NaN frame does."""
import numpy as np
import pytest

import align_rule as ar


def _feats(n, dims, seed):
    return np.random.default_rng(seed).standard_normal((n, dims))


def test_identical_sequences_give_the_diagonal():
    a = _feats(23, 5, 1)
    r = ar.align(a, a.copy(), 0, 5)
    assert r["cost"] == 0.0
    assert np.array_equal(r["path"], np.stack([np.arange(23), np.arange(23)], axis=1))
    assert np.array_equal(r["b_on_a"], np.arange(23.0)) and np.array_equal(r["a_on_b"], np.arange(23.0))


def test_all_equal_features_give_the_path_of_the_tie_break():
    """every D along a row or column ties, and a tie takes the diagonal: back from the end corner diagonally until an edge is met,
    then along that edge to (0, 0)"""
    r = ar.align(np.ones((3, 2)), np.ones((5, 2)), 0, 2)
    assert r["cost"] == 0.0
    assert r["path"].tolist() == [[0, 0], [0, 1], [0, 2], [1, 3], [2, 4]]
    assert r["b_on_a"].tolist() == [1.0, 3.0, 4.0] and r["a_on_b"].tolist() == [0.0, 0.0, 0.0, 1.0, 2.0]
    r = ar.align(np.ones((5, 2)), np.ones((3, 2)), 0, 2)
    assert r["path"].tolist() == [[0, 0], [1, 0], [2, 0], [3, 1], [4, 2]]
    assert r["a_on_b"].tolist() == [1.0, 3.0, 4.0] and r["b_on_a"].tolist() == [0.0, 0.0, 0.0, 1.0, 2.0]


@pytest.mark.parametrize("n,m", [(31, 18), (9, 26)])
def test_a_band_of_the_longer_length_is_no_band(n, m):
    a, b = _feats(n, 4, n), _feats(m, 4, m)
    free, wide = ar.align(a, b, 1, 4, 0), ar.align(a, b, 1, 4, max(n, m))
    assert free["cost"] == wide["cost"] and np.array_equal(free["path"], wide["path"])
    assert np.array_equal(free["b_on_a"], wide["b_on_a"]) and np.array_equal(free["a_on_b"], wide["a_on_b"])
    assert all(ar.allowed(i, j, n, m, max(n, m)) for i in range(n) for j in range(m))


@pytest.mark.parametrize("n,m", [(40, 7), (7, 40)])
def test_the_narrowest_band_still_reaches_the_corner(n, m):
    a, b = _feats(n, 3, 5), _feats(m, 3, 6)
    r = ar.align(a, b, 0, 3, 1)
    assert np.isfinite(r["cost"])
    assert r["path"][0].tolist() == [0, 0] and r["path"][-1].tolist() == [n - 1, m - 1]
    assert all(ar.allowed(i, j, n, m, 1) for i, j in r["path"])
    assert not all(ar.allowed(i, j, n, m, 1) for i in range(n) for j in range(m))
    assert r["cost"] >= ar.align(a, b, 0, 3, 0)["cost"]


@pytest.mark.parametrize("n,m,band", [(1, 1, 0), (1, 9, 0), (9, 1, 0), (2, 2, 0), (37, 52, 0), (52, 37, 3), (20, 20, 1)])
def test_maps_are_non_decreasing_half_integers_and_k_stays_within_its_bounds(n, m, band):
    r = ar.align(_feats(n, 6, 10 * n + m), _feats(m, 6, 10 * m + n), 1, 6, band)
    path, K = r["path"], len(r["path"])
    assert max(n, m) <= K <= n + m - 1
    steps = np.diff(path, axis=0)
    assert ((steps >= 0) & (steps <= 1)).all() and (steps.sum(axis=1) >= 1).all()
    for mp, other in ((r["b_on_a"], m), (r["a_on_b"], n)):
        assert np.array_equal(mp * 2, np.round(mp * 2)) and (np.diff(mp) >= 0).all()
        assert mp[0] >= 0 and mp[-1] <= other - 1
    assert r["b_on_a"][-1] >= (m - 1) / 2 and r["a_on_b"][-1] >= (n - 1) / 2


@pytest.mark.parametrize("row", [0, 6, 11])
def test_a_frame_of_nan_makes_the_pair_nan(row):
    """the last row of A carries NaN into the corner itself; a NaN row before it leaves +inf there (NaN fails every comparison, so
    the row behind it takes its left neighbour, +inf at column 0): either way the total is not finite"""
    a, b = _feats(12, 4, 3), _feats(15, 4, 4)
    a[row] = np.nan
    r = ar.align(a, b, 0, 4)
    assert np.isnan(r["cost"]) if row == 11 else r["cost"] == np.inf
    assert len(r["path"]) == 0 and r["path"].shape == (0, 2)
    assert np.isnan(r["b_on_a"]).all() and np.isnan(r["a_on_b"]).all()
    assert r["b_on_a"].shape == (12,) and r["a_on_b"].shape == (15,)


def test_the_window_of_coefficients_is_what_is_compared():
    a, b = _feats(14, 8, 7), _feats(11, 8, 8)
    r = ar.align(a, b, 2, 5)
    assert r["cost"] == ar.align(a[:, 2:5], b[:, 2:5], 0, 3)["cost"]
    d = ar.local_costs(a, b, 2, 5)
    assert d[3, 4] == np.sqrt(((a[3, 2] - b[4, 2]) ** 2 + (a[3, 3] - b[4, 3]) ** 2) + (a[3, 4] - b[4, 4]) ** 2)


def test_the_batch_form_walks_the_packed_arrays():
    a, b = _feats(10 + 4, 3, 1), _feats(6 + 9, 3, 2)
    both = ar.align_batch([10, 4], a, [6, 9], b, 0, 3)
    one = ar.align(a[10:], b[6:], 0, 3)
    assert both[1]["cost"] == one["cost"] and np.array_equal(both[1]["path"], one["path"])
