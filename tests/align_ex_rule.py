"""The rule of extended feature alignment (include/world_class_io.h, wc_align_features_ex_device) restated in plain Python / numpy.
A helper of tests/test_align_ex_rule.py and tests/test_gpu_align_ex.py, not a test module.

Local cost d(i, j), packing and the band predicate are those of tests/align_rule.py.  ok(i, j): inside the matrix and inside the
band; a term whose cells are not all ok is +inf.
  step_pattern 0  Dd = D(i - 1, j - 1), Du = D(i - 1, j), Dl = D(i, j - 1)
  step_pattern 1  Dd = D(i - 1, j - 1), Du = D(i - 2, j - 1) + d(i - 1, j), Dl = D(i - 1, j - 2) + d(i, j - 1): one rounded sum each,
                  the D operand first; the path holds the intermediate cell (choice up at (i, j): (i - 1, j), then (i - 2, j - 1);
                  choice left: (i, j - 1), then (i - 1, j - 2))
  accumulation    D(i, j) = d(i, j) + best: the diagonal if Dd <= Du and Dd <= Dl, else up if Du <= Dl, else left
  start           D(0, 0) = d(0, 0); with OPEN_BEGIN D(0, j) = d(0, j) for every ok (0, j) and the backtrack stops at the first cell
                  it meets in row 0, else at (0, 0)
  end             with OPEN_END the ok cells of row n - 1 by ascending j from best = +inf, j taken when D(n - 1, j) < best; no
                  winner: (n - 1, m - 1).  The cost is D there and the backtrack starts there
  maps            b_on_a as in align_rule; a_on_b as in align_rule for j_first <= j <= j_last, 0.0 before, n - 1 behind
  span            (j_first, j_last), the columns of the path's first and last cell; timelines: (double) i_k and j_k of the K cells
  a total cost that is not finite: K = 0, no path, both maps NaN, span (-1, -1), empty timelines"""
import numpy as np

from align_rule import DIAG, LEFT, UP, allowed, local_costs

OPEN_BEGIN, OPEN_END = 1, 2


def align(a, b, dim_begin, dim_end, band=0, step_pattern=0, flags=0, costs=None):
    """dict of cost, path (K x 2 int32), b_on_a (n), a_on_b (m), span (2 int32), timeline_a (K), timeline_b (K).  costs: an (n, m)
    matrix that stands for d (the tests of the rule itself use integer-valued ones)"""
    assert step_pattern in (0, 1) and 0 <= flags <= 3 and (flags == 0 or band == 0)
    if costs is None:
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            d = local_costs(a, b, dim_begin, dim_end)
    else:
        d = np.asarray(costs, dtype=np.float64)
    n, m = d.shape
    inf = float("inf")
    ok = lambda i, j: 0 <= i < n and 0 <= j < m and allowed(i, j, n, m, band)
    D = [[inf] * m for _ in range(n)]
    choice = [[DIAG] * m for _ in range(n)]
    for i in range(n):
        for j in range(m):
            if not ok(i, j):
                continue
            if i == 0 and (j == 0 or flags & OPEN_BEGIN):
                D[0][j] = float(d[0, j])
                continue
            Dd = D[i - 1][j - 1] if ok(i - 1, j - 1) else inf
            if step_pattern == 0:
                Du = D[i - 1][j] if ok(i - 1, j) else inf
                Dl = D[i][j - 1] if ok(i, j - 1) else inf
            else:
                Du = D[i - 2][j - 1] + float(d[i - 1, j]) if ok(i - 2, j - 1) and ok(i - 1, j) else inf
                Dl = D[i - 1][j - 2] + float(d[i, j - 1]) if ok(i - 1, j - 2) and ok(i, j - 1) else inf
            if Dd <= Du and Dd <= Dl:
                best, choice[i][j] = Dd, DIAG
            elif Du <= Dl:
                best, choice[i][j] = Du, UP
            else:
                best, choice[i][j] = Dl, LEFT
            D[i][j] = float(d[i, j]) + best
    j_end = m - 1
    if flags & OPEN_END:
        best = inf
        for j in range(m):
            if ok(n - 1, j) and D[n - 1][j] < best:
                best, j_end = D[n - 1][j], j
    cost = D[n - 1][j_end]
    if not np.isfinite(cost):
        return {"cost": cost, "path": np.zeros((0, 2), dtype=np.int32), "b_on_a": np.full(n, np.nan), "a_on_b": np.full(m, np.nan),
                "span": np.array([-1, -1], dtype=np.int32), "timeline_a": np.zeros(0), "timeline_b": np.zeros(0)}
    cells = []
    i, j = n - 1, j_end
    while True:
        cells.append((i, j))
        if i == 0 and (j == 0 or flags & OPEN_BEGIN):
            break
        c = choice[i][j]
        if step_pattern == 1 and c != DIAG:
            i, j = (i - 1, j) if c == UP else (i, j - 1)
            cells.append((i, j))
            i, j = i - 1, j - 1
        else:
            if c != LEFT:
                i -= 1
            if c != UP:
                j -= 1
    path = np.array(cells[::-1], dtype=np.int32)
    j_first, j_last = int(path[0, 1]), int(path[-1, 1])
    b_on_a, a_on_b = np.empty(n), np.empty(m)
    for i in range(n):
        js = path[path[:, 0] == i, 1]
        b_on_a[i] = (int(js.min()) + int(js.max())) * 0.5
    for j in range(m):
        if j < j_first:
            a_on_b[j] = 0.0
        elif j > j_last:
            a_on_b[j] = float(n - 1)
        else:
            is_ = path[path[:, 1] == j, 0]
            a_on_b[j] = (int(is_.min()) + int(is_.max())) * 0.5
    return {"cost": cost, "path": path, "b_on_a": b_on_a, "a_on_b": a_on_b, "span": np.array([j_first, j_last], dtype=np.int32),
            "timeline_a": path[:, 0].astype(np.float64), "timeline_b": path[:, 1].astype(np.float64)}


def align_batch(a_lengths, feat_a, b_lengths, feat_b, dim_begin, dim_end, band=0, step_pattern=0, flags=0):
    """the packed batch, pair by pair: a list of align()'s dicts"""
    out, fa, fb = [], 0, 0
    for n, m in zip(a_lengths, b_lengths):
        out.append(align(feat_a[fa:fa + n], feat_b[fb:fb + m], dim_begin, dim_end, band, step_pattern, flags))
        fa, fb = fa + n, fb + m
    return out
