"""What tests/test_gpu_align_wide.py and tests/test_gpu_align_scratch.py share; a helper, not a test module.

check_alignment_outputs holds one pair's outputs of wc_align_features_ex_device against each other.  It takes the local cost and the
band from tests/align_rule.py (local_costs, allowed) and nothing of the recursion, so a misreading that the header, the rule and
the kernels share does not pass it: the path must be legal for the step pattern, the cost must be the sum along the returned
path, and the maps, the span and the timelines must be that path's.  tests/test_align_ex_rule.py runs it on the rule's own
results, so it is known to accept what is right before it judges the device.

The device side (checked_align, poison_scratch) goes through the sentinel discipline of tests/test_gpu_align_ex.py: every output
pre-filled, room behind the last pair, and what the call has no business writing keeps the sentinel."""
import numpy as np

from align_rule import allowed, local_costs

OPEN_BEGIN, OPEN_END = 1, 2


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def split_outputs(got, a_lens, b_lens):
    """the eight packed arrays of a call, pair by pair: dicts of cost, K, path (K x 2), b_on_a, a_on_b, span, timeline_a, timeline_b"""
    cost, plen, path, boa, aob, span, tla, tlb = got
    path, span = path.reshape(-1, 2), span.reshape(-1, 2)
    out, fa, fb, po = [], 0, 0, 0
    for u, (n, m) in enumerate(zip(a_lens, b_lens)):
        K = int(plen[u])
        assert 0 <= K <= n + m - 1, (u, K)
        out.append({"cost": cost[u], "K": K, "path": path[po:po + K], "b_on_a": boa[fa:fa + n], "a_on_b": aob[fb:fb + m], "span": span[u],
                    "timeline_a": tla[po:po + K], "timeline_b": tlb[po:po + K]})
        fa, fb, po = fa + n, fb + m, po + n + m - 1
    return out


def rule_outputs(r):
    """one dict of align_ex_rule.align in the form of split_outputs"""
    return dict(r, K=len(r["path"]))


def check_alignment_outputs(a, b, window, band, pattern, flags, outputs):
    """a (n x dims), b (m x dims), window = (dim_begin, dim_end), outputs: one dict of split_outputs"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n, m, o = len(a), len(b), outputs
    K, cost = o["K"], float(o["cost"])
    if K == 0:
        assert not np.isfinite(cost), cost
        assert np.isnan(o["b_on_a"]).all() and np.isnan(o["a_on_b"]).all() and len(o["b_on_a"]) == n and len(o["a_on_b"]) == m
        assert list(o["span"]) == [-1, -1]
        return
    assert np.isfinite(cost)
    path = np.asarray(o["path"]).astype(np.int64)
    assert path.shape == (K, 2) and K <= n + m - 1
    pi, pj = path[:, 0], path[:, 1]
    # strictly inside the matrix and the band, from the first row to the last
    assert (pi >= 0).all() and (pi < n).all() and (pj >= 0).all() and (pj < m).all()
    assert all(allowed(i, j, n, m, band) for i, j in path), "a cell of the path lies outside the band"
    assert pi[0] == 0 and pi[-1] == n - 1
    assert pj[0] == 0 or flags & OPEN_BEGIN
    assert pj[-1] == m - 1 or flags & OPEN_END
    if flags & OPEN_BEGIN:  # the backtrack stops at the first cell it meets in row 0
        assert (pi == 0).sum() == 1
    # legal steps
    steps = np.diff(path, axis=0)
    diag = (steps[:, 0] == 1) & (steps[:, 1] == 1)
    straight = ((steps[:, 0] == 1) & (steps[:, 1] == 0)) | ((steps[:, 0] == 0) & (steps[:, 1] == 1))
    assert (diag | straight).all(), "a step that is none of (1, 1), (1, 0), (0, 1)"
    if pattern == 1:
        # a two-cell step is (i - 2, j - 1), (i - 1, j), (i, j) or its mirror image: in path order the straight step comes from the
        # intermediate cell, which a diagonal step has just reached (walking back from the end, as the backtrack does, the straight
        # step is the one that a diagonal step follows).  So the path neither begins nor turns on an intermediate cell
        where = np.flatnonzero(straight)
        assert (where >= 1).all() and diag[where - 1].all(), "pattern 1: a straight step that no diagonal step leads to"
        assert np.bincount(pi).max() <= 2 and np.bincount(pj).max() <= 2
    # the cost is the sum along this very path, in path order
    with np.errstate(invalid="ignore", over="ignore"):
        d = local_costs(a, b, window[0], window[1])
    acc = float(d[pi[0], pj[0]])
    for k in range(1, K):
        acc = float(d[pi[k], pj[k]]) + acc
    assert _bits(cost) == _bits(acc), (cost, acc)
    # the maps, the span and the timelines are this path's
    j_first, j_last = int(pj[0]), int(pj[-1])
    assert list(o["span"]) == [j_first, j_last]
    jmin, jmax = np.full(n, m, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    np.minimum.at(jmin, pi, pj)
    np.maximum.at(jmax, pi, pj)
    assert np.array_equal(o["b_on_a"], (jmin + jmax) * 0.5)
    imin, imax = np.full(m, n, dtype=np.int64), np.full(m, -1, dtype=np.int64)
    np.minimum.at(imin, pj, pi)
    np.maximum.at(imax, pj, pi)
    want = (imin + imax) * 0.5
    want[:j_first], want[j_last + 1:] = 0.0, float(n - 1)
    assert np.array_equal(o["a_on_b"], want)
    assert np.array_equal(o["timeline_a"], pi.astype(np.float64)) and np.array_equal(o["timeline_b"], pj.astype(np.float64))


def check_batch(a_lens, fa, b_lens, fb, window, band, pattern, flags, got):
    """check_alignment_outputs on every pair of one device result"""
    a0 = b0 = 0
    for (n, m), o in zip(zip(a_lens, b_lens), split_outputs(got, a_lens, b_lens)):
        check_alignment_outputs(fa[a0:a0 + n], fb[b0:b0 + m], window, band, pattern, flags, o)
        a0, b0 = a0 + n, b0 + m


def poison_scratch(env, a_lens, b_lens, dims, window, band, pattern, flags):
    """a call on these lengths and settings with every feature NaN: it leaves NaN in every d and D that a call of the same layout is
    about to use, so a cell which that call then fails to write cannot find the right value left over from an earlier one.  The
    poison proves nothing unless it took: every pair must report a NaN total and K = 0"""
    import test_gpu_align_ex as tx
    fa, fb = np.full((sum(a_lens), dims), np.nan), np.full((sum(b_lens), dims), np.nan)
    got = tx._align(env, a_lens, fa, b_lens, fb, dims, window[0], window[1], band, pattern, flags)
    P = len(a_lens)
    assert np.isnan(got[0][:P]).all() and (got[1][:P] == 0).all(), "the poison call did not end every pair at NaN"
    assert (got[5][:2 * P] == -1).all() and np.isnan(got[3][:sum(a_lens)]).all() and np.isnan(got[4][:sum(b_lens)]).all()


def checked_align(env, batch, dims, window, band, pattern, flags, want, poison=True):
    """the device call (behind a poison call where asked) held against the rule's `want` through _assert_equals_rule -- d_cost
    bitwise, everything else exact, sentinels intact -- and against itself through check_alignment_outputs.  Returns the arrays"""
    import test_gpu_align_ex as tx
    a_lens, fa, b_lens, fb = batch
    if poison:
        poison_scratch(env, a_lens, b_lens, dims, window, band, pattern, flags)
    got = tx._align(env, a_lens, fa, b_lens, fb, dims, window[0], window[1], band, pattern, flags)
    check_batch(a_lens, fa, b_lens, fb, window, band, pattern, flags, got)
    tx._assert_equals_rule(got, want, a_lens, b_lens)
    return got
