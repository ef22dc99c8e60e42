"""The rule of an alignment stream with a search window (include/world_class_align_window.h, wc_align_stream_set_window) restated row
by row in plain Python / numpy.  A helper of tests/test_align_window_rule.py and tests/test_gpu_align_window.py, not a test module.

A stream with window (width, back, hop, monotone) follows a track B of m rows; W = min(width, m).  Row i (counted since the reset)
belongs to epoch e = i // hop, and every row of an epoch uses the columns [lo_e, lo_e + w_e):
  epoch 0         lo = 0, w = W; with open_begin w = m (the first hop rows search the whole track)
  epoch e >= 1    w = W; p = the position written for row e * hop - 1; lo stays if p is NaN, else lo = min(max(lo, int(p) - back), m - W)
  local cost      d(i, j) of tests/align_rule.py (local_costs)
  row 0           D(0, 0) = d(0, 0); with open_begin D(0, j) = d(0, j) for every j of the window
  otherwise       D(i, j) = d(i, j) + best of Dd = D(i - 1, j - 1), Du = D(i - 1, j), Dl = D(i, j - 1) by the comparisons of
                  tests/align_stream_rule.py; a predecessor outside the matrix, outside row i's window (Dl) or outside row i - 1's
                  window (Du, Dd) is +inf
  per row         the scan by ascending j over the row's window from best = +inf, j taken when D(i, j) < best; with monotone only
                  columns j >= q can win, q the last position written that is not NaN (0: none); cost = D(i, j*), position =
                  float(j*); no winner: cost = D(i, lo + w - 1), position = NaN"""
import numpy as np

from align_rule import local_costs
from align_stream_rule import follow as _unwindowed

_followable = {}


class WindowFollower:
    """one stream after its reset onto the track b (or onto a track of m columns whose local costs the caller supplies) and its
    set_window(width, back, hop, monotone)"""

    def __init__(self, b=None, dim_begin=0, dim_end=None, open_begin=False, width=1, back=0, hop=1, monotone=False, m=None):
        self.b = None if b is None else np.asarray(b, dtype=np.float64)
        self.m = int(m) if self.b is None else self.b.shape[0]
        assert width >= 1 and 0 <= back < width and 1 <= hop <= 64
        self.dim_begin, self.dim_end = dim_begin, dim_end
        self.open_begin, self.monotone = bool(open_begin), bool(monotone)
        self.W, self.back, self.hop = min(int(width), self.m), int(back), int(hop)
        self.rows = 0
        self.lo, self.w = 0, 0   # the window of the last row
        self.last = np.nan       # the position written for the last row
        self.q = 0               # the last position that was not NaN
        self.state = None        # D of the last row over all m columns: +inf outside its window
        self.los = []            # lo of every row so far (for the tests)

    def push(self, rows):
        """rows: (k, dims).  Returns (position, cost), k doubles each"""
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, self.b.shape[1])
        if len(rows) == 0:
            return np.zeros(0), np.zeros(0)
        with np.errstate(invalid="ignore", over="ignore"):
            d = local_costs(rows, self.b, self.dim_begin, self.b.shape[1] if self.dim_end is None else self.dim_end)
        return self.push_costs(d)

    def push_costs(self, d):
        """d: (k, m) local costs of the next k rows against ALL columns (only the window's are used)"""
        d = np.asarray(d, dtype=np.float64)
        assert d.ndim == 2 and d.shape[1] == self.m
        inf, m = float("inf"), self.m
        pos, cost = np.empty(len(d)), np.empty(len(d))
        for r in range(len(d)):
            i = self.rows
            if i == 0:
                self.lo, self.w = 0, (m if self.open_begin else self.W)
            elif i % self.hop == 0:
                if not np.isnan(self.last):
                    self.lo = min(max(self.lo, int(self.last) - self.back), m - self.W)
                self.w = self.W
            lo, hi = self.lo, self.lo + self.w
            prev, row = self.state, [inf] * m
            for j in range(lo, hi):
                dij = float(d[r, j])
                if i == 0 and (j == 0 or self.open_begin):
                    row[j] = dij
                    continue
                Dd = prev[j - 1] if prev is not None and j > 0 else inf
                Du = prev[j] if prev is not None else inf
                Dl = row[j - 1] if j > lo else inf
                if Dd <= Du and Dd <= Dl:
                    best = Dd
                elif Du <= Dl:
                    best = Du
                else:
                    best = Dl
                row[j] = dij + best
            best, at = inf, None
            for j in range(lo, hi):
                if self.monotone and j < self.q:
                    continue
                if row[j] < best:
                    best, at = row[j], j
            cost[r] = row[hi - 1] if at is None else best
            pos[r] = np.nan if at is None else float(at)
            if at is not None:
                self.q = at
            self.last = pos[r]
            self.state = row
            self.los.append(lo)
            self.rows += 1
        return pos, cost


def follow(a, b, dim_begin, dim_end, open_begin=False, width=1, back=0, hop=1, monotone=False, cuts=None, los=None):
    """all rows of a through one windowed stream, cut into pushes of the sizes in cuts (None: one push): (position, cost) over all
    rows; los, if a list, receives lo of every row"""
    a = np.asarray(a, dtype=np.float64)
    f = WindowFollower(b, dim_begin, dim_end, open_begin, width, back, hop, monotone)
    cuts = [len(a)] if cuts is None else list(cuts)
    assert sum(cuts) == len(a)
    out, o = [], 0
    for c in cuts:
        out.append(f.push(a[o:o + c]))
        o += c
    if los is not None:
        los.extend(f.los)
    return np.concatenate([p for p, _ in out]), np.concatenate([c for _, c in out])


def followable(s):
    """case s of the followable voices: a track of 300 rows of 8 (a random walk with steps of 0.3 * normal) and a voice of 150 rows
    that samples it linearly from column 0 at a slope drawn per 30 rows from [0.6, 1.7], plus 0.05 * normal noise.  150 rows are the
    most whole blocks of 30 that cannot run off the track at the largest slope (5 * 30 * 1.7 = 255 <= 299 < 6 * 30 * 1.7).  Returns
    (voice, track) and the unwindowed stream's (position, cost); made once per s"""
    if s not in _followable:
        rng = np.random.default_rng(100 + s)
        m, n, dims = 300, 150, 8
        track = np.cumsum(0.3 * rng.standard_normal((m, dims)), axis=0)
        slopes = np.repeat(rng.uniform(0.6, 1.7, n // 30), 30)
        t = np.concatenate([[0.0], np.cumsum(slopes)[:-1]])
        k = t.astype(np.int64)
        f = (t - k)[:, None]
        voice = (1.0 - f) * track[k] + f * track[k + 1] + 0.05 * rng.standard_normal((n, dims))
        _followable[s] = (voice, track, _unwindowed(voice, track, 0, dims))
    return _followable[s]
