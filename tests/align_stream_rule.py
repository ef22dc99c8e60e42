"""The rule of the alignment streams (include/world_class_align_stream.h, wc_align_stream_push_device) restated row by row in plain
Python / numpy.  A helper of tests/test_align_stream_rule.py and tests/test_gpu_align_stream.py, not a test module.

A stream follows a track B of m rows; only coefficients dim_begin <= c < dim_end are compared.  The stream keeps ONE row of D, the
row of the last pushed row, and its row count; a push of k rows costs O(k * m).
  local cost      d(i, j) of tests/align_rule.py (local_costs)
  row 0           D(0, 0) = d(0, 0); with open_begin D(0, j) = d(0, j) for every j
  otherwise       D(i, j) = d(i, j) + best of Dd = D(i - 1, j - 1), Du = D(i - 1, j), Dl = D(i, j - 1); a predecessor outside the
                  matrix is +inf; the diagonal if Dd <= Du and Dd <= Dl, else up if Du <= Dl, else left -- exactly these comparisons
  per row         the open-end scan by ascending j from best = +inf, j taken when D(i, j) < best: cost = D(i, j*), position =
                  float(j*); no winner (NaN or +inf throughout): cost = D(i, m - 1), position = NaN"""
import numpy as np

from align_rule import local_costs


class Follower:
    """one stream after its reset onto the track b (or onto a track of m columns whose local costs the caller supplies)"""

    def __init__(self, b=None, dim_begin=0, dim_end=None, open_begin=False, m=None):
        self.b = None if b is None else np.asarray(b, dtype=np.float64)
        self.m = int(m) if self.b is None else self.b.shape[0]
        self.dim_begin, self.dim_end = dim_begin, dim_end
        self.open_begin = bool(open_begin)
        self.rows = 0
        self.state = None  # D of the last row

    def push(self, rows):
        """rows: (k, dims).  Returns (position, cost), k doubles each"""
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, self.b.shape[1])
        if len(rows) == 0:
            return np.zeros(0), np.zeros(0)
        with np.errstate(invalid="ignore", over="ignore"):
            d = local_costs(rows, self.b, self.dim_begin, self.b.shape[1] if self.dim_end is None else self.dim_end)
        return self.push_costs(d)

    def push_costs(self, d):
        """d: (k, m) local costs of the next k rows"""
        d = np.asarray(d, dtype=np.float64)
        assert d.ndim == 2 and d.shape[1] == self.m
        inf = float("inf")
        pos, cost = np.empty(len(d)), np.empty(len(d))
        for r in range(len(d)):
            prev, row = self.state, [inf] * self.m
            for j in range(self.m):
                dij = float(d[r, j])
                if self.rows == 0 and (j == 0 or self.open_begin):
                    row[j] = dij
                    continue
                Dd = prev[j - 1] if prev is not None and j > 0 else inf
                Du = prev[j] if prev is not None else inf
                Dl = row[j - 1] if j > 0 else inf
                if Dd <= Du and Dd <= Dl:
                    best = Dd
                elif Du <= Dl:
                    best = Du
                else:
                    best = Dl
                row[j] = dij + best
            best, at = inf, None
            for j in range(self.m):
                if row[j] < best:
                    best, at = row[j], j
            cost[r] = row[self.m - 1] if at is None else best
            pos[r] = np.nan if at is None else float(at)
            self.state = row
            self.rows += 1
        return pos, cost


def follow(a, b, dim_begin, dim_end, open_begin=False, cuts=None):
    """all rows of a through one stream, cut into pushes of the sizes in cuts (None: one push): (position, cost) over all rows"""
    a = np.asarray(a, dtype=np.float64)
    f = Follower(b, dim_begin, dim_end, open_begin)
    cuts = [len(a)] if cuts is None else list(cuts)
    assert sum(cuts) == len(a)
    out, o = [], 0
    for c in cuts:
        out.append(f.push(a[o:o + c]))
        o += c
    return np.concatenate([p for p, _ in out]), np.concatenate([c for _, c in out])
