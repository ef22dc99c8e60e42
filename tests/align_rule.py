"""The rule of feature alignment (include/world_class_io.h, wc_align_features_device) restated in plain Python / numpy.  A helper of
tests/test_align_rule.py and tests/test_gpu_align.py, not a test module.

A has n rows, B has m rows of dims doubles; only coefficients dim_begin <= c < dim_end are compared.
  local cost      d(i, j) = sqrt(sum_c (a[i][c] - b[j][c])**2): the sum over ascending c from 0.0, every difference, product and sum
                  rounded on its own, the root correctly rounded
  band            0: every cell; >= 1: with L = max(n, m) - 1 cell (i, j) is allowed iff |i * (m - 1) - j * (n - 1)| <= band * L
                  (Python integers)
  accumulation    D(0, 0) = d(0, 0); D(i, j) = d(i, j) + best of Dd = D(i - 1, j - 1), Du = D(i - 1, j), Dl = D(i, j - 1); a
                  predecessor outside the matrix or the band is +inf; the diagonal if Dd <= Du and Dd <= Dl, else up if Du <= Dl,
                  else left -- exactly these comparisons
  path            the choices followed back from (n - 1, m - 1) to (0, 0), K cells
  maps            b_on_a[i] = (jmin(i) + jmax(i)) * 0.5 over the path's cells in row i, a_on_b[j] the mirror image
  a total cost that is not finite: K = 0, no path, both maps NaN"""
import numpy as np

DIAG, UP, LEFT = 0, 1, 2


def local_costs(a, b, dim_begin, dim_end):
    """(n, m) matrix of d(i, j): one vectorised difference, product and sum per coefficient, in ascending c"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    acc = np.zeros((a.shape[0], b.shape[0]))
    for c in range(dim_begin, dim_end):
        diff = a[:, c][:, None] - b[:, c][None, :]
        acc = acc + diff * diff
    return np.sqrt(acc)


def allowed(i, j, n, m, band):
    if band == 0:
        return True
    L = max(n, m) - 1
    return abs(int(i) * (m - 1) - int(j) * (n - 1)) <= int(band) * L


def align(a, b, dim_begin, dim_end, band=0):
    """dict of cost, path (K x 2 int32), b_on_a (n) and a_on_b (m)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n, m = a.shape[0], b.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        d = local_costs(a, b, dim_begin, dim_end)
    inf = float("inf")
    D = [[inf] * m for _ in range(n)]
    choice = [[DIAG] * m for _ in range(n)]
    for i in range(n):
        for j in range(m):
            if not allowed(i, j, n, m, band):
                continue
            if i == 0 and j == 0:
                D[0][0] = float(d[0, 0])
                continue
            Dd = D[i - 1][j - 1] if i > 0 and j > 0 and allowed(i - 1, j - 1, n, m, band) else inf
            Du = D[i - 1][j] if i > 0 and allowed(i - 1, j, n, m, band) else inf
            Dl = D[i][j - 1] if j > 0 and allowed(i, j - 1, n, m, band) else inf
            if Dd <= Du and Dd <= Dl:
                best, choice[i][j] = Dd, DIAG
            elif Du <= Dl:
                best, choice[i][j] = Du, UP
            else:
                best, choice[i][j] = Dl, LEFT
            D[i][j] = float(d[i, j]) + best
    cost = D[n - 1][m - 1]
    if not np.isfinite(cost):
        return {"cost": cost, "path": np.zeros((0, 2), dtype=np.int32), "b_on_a": np.full(n, np.nan), "a_on_b": np.full(m, np.nan)}
    cells = []
    i, j = n - 1, m - 1
    while True:
        cells.append((i, j))
        if i == 0 and j == 0:
            break
        c = choice[i][j]
        if c != LEFT:
            i -= 1
        if c != UP:
            j -= 1
    path = np.array(cells[::-1], dtype=np.int32)
    b_on_a, a_on_b = np.empty(n), np.empty(m)
    for i in range(n):
        js = path[path[:, 0] == i, 1]
        b_on_a[i] = (int(js.min()) + int(js.max())) * 0.5
    for j in range(m):
        is_ = path[path[:, 1] == j, 0]
        a_on_b[j] = (int(is_.min()) + int(is_.max())) * 0.5
    return {"cost": cost, "path": path, "b_on_a": b_on_a, "a_on_b": a_on_b}


def align_batch(a_lengths, feat_a, b_lengths, feat_b, dim_begin, dim_end, band=0):
    """the packed batch, pair by pair: a list of align()'s dicts"""
    out, fa, fb = [], 0, 0
    for n, m in zip(a_lengths, b_lengths):
        out.append(align(feat_a[fa:fa + n], feat_b[fb:fb + m], dim_begin, dim_end, band))
        fa, fb = fa + n, fb + m
    return out
