"""The rule of an alignment stream's settled positions (include/world_class_align_lag.h, wc_align_stream_set_lag,
wc_align_stream_push_settled_device, wc_align_stream_tail_device) restated in plain Python / numpy on top of
tests/align_stream_rule.py (Follower) and tests/align_window_rule.py (WindowFollower).  A helper of tests/test_align_lag_rule.py and
tests/test_gpu_align_lag.py, not a test module.

A LagFollower wraps one of the two followers, feeds it row by row and keeps the CHOICE of every cell the follower computed (all
of them: the rule needs no ring):
  start           row 0 at j = 0, or any j of row 0 with open_begin
  otherwise       with Dd = D(i - 1, j - 1), Du = D(i - 1, j), Dl = D(i, j - 1) as the follower saw them (+inf outside the matrix
                  and outside the rows' windows): DIAG if Dd <= Du and Dd <= Dl, else UP if Du <= Dl, else LEFT
  path P(i)       from (i, j*_i), j*_i the position the follower wrote for row i, along the choices: DIAG to (r - 1, j - 1), UP to
                  (r - 1, j), LEFT to (r, j - 1), until a start
  settled         for row i with lag L > 0 and t = max(i - L, 0): (jmin + jmax) * 0.5 over the cells of P(i) in row t; NaN when the
                  position of row i is NaN; with lag 0 the position itself
  tail            with n rows received and K = min(L + 1, n): the same half-integer for rows n - K .. n - 1 of P(n - 1), ascending;
                  all NaN when the position of row n - 1 is NaN
A walk that would read a cell the follower never computed (outside a row's window) raises: consequence 5 of the header."""
import numpy as np

from align_rule import DIAG, LEFT, UP, local_costs
from align_stream_rule import Follower
from align_window_rule import WindowFollower

START = 3


class LagFollower:
    """base: a fresh Follower or WindowFollower; lag: L >= 0"""

    def __init__(self, base, lag):
        assert base.rows == 0 and lag >= 0
        self.base, self.lag = base, int(lag)
        self.choice = []  # per row: m entries, None where the follower computed no cell
        self.last = np.nan  # the position written for the newest row

    def push(self, rows):
        """rows: (k, dims).  Returns (position, cost, settled), k doubles each"""
        b = self.base.b
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, b.shape[1])
        if len(rows) == 0:
            return np.zeros(0), np.zeros(0), np.zeros(0)
        with np.errstate(invalid="ignore", over="ignore"):
            d = local_costs(rows, b, self.base.dim_begin, b.shape[1] if self.base.dim_end is None else self.base.dim_end)
        return self.push_costs(d)

    def push_costs(self, d):
        """d: (k, m) local costs of the next k rows"""
        d = np.asarray(d, dtype=np.float64)
        base, inf = self.base, float("inf")
        m = base.m
        pos, cost, settled = np.empty(len(d)), np.empty(len(d)), np.empty(len(d))
        for r in range(len(d)):
            i, prev = base.rows, base.state
            p, c = base.push_costs(d[r:r + 1])
            row = base.state  # D of row i, +inf outside its window
            lo, hi = (base.lo, base.lo + base.w) if isinstance(base, WindowFollower) else (0, m)
            ch = [None] * m
            for j in range(lo, hi):
                if i == 0 and (j == 0 or base.open_begin):
                    ch[j] = START
                    continue
                Dd = prev[j - 1] if prev is not None and j > 0 else inf
                Du = prev[j] if prev is not None else inf
                Dl = row[j - 1] if j > lo else inf
                ch[j] = DIAG if Dd <= Du and Dd <= Dl else UP if Du <= Dl else LEFT
            self.choice.append(ch)
            pos[r], cost[r], self.last = p[0], c[0], p[0]
            if self.lag == 0:
                settled[r] = pos[r]
            elif np.isnan(pos[r]):
                settled[r] = np.nan
            else:
                settled[r] = self.centres(i, int(pos[r]), max(i - self.lag, 0))[0]
        return pos, cost, settled

    def centres(self, i, j, t):
        """the half-integer centres of the path from (i, j) in rows t .. i, ascending"""
        out = []
        while True:
            jmax = j
            while self._at(i, j) == LEFT:
                j -= 1
            out.append((j + jmax) * 0.5)
            if i == t:
                return out[::-1]
            c = self._at(i, j)
            assert c in (DIAG, UP), "the path starts above row t"
            i, j = i - 1, j - (1 if c == DIAG else 0)

    def _at(self, i, j):
        assert j >= 0 and self.choice[i][j] is not None, "the path left the cells the stream computed"
        return self.choice[i][j]

    def tail(self):
        """K = min(lag + 1, rows) doubles"""
        n = self.base.rows
        assert self.lag > 0 and n > 0
        k = min(self.lag + 1, n)
        if np.isnan(self.last):
            return np.full(k, np.nan)
        return np.array(self.centres(n - 1, int(self.last), n - k))


def follower(b, dim_begin, dim_end, open_begin=False, lag=0, win=None):
    """a LagFollower on the track b; win: None or (width, back, hop, monotone)"""
    base = Follower(b, dim_begin, dim_end, open_begin) if win is None else WindowFollower(b, dim_begin, dim_end, open_begin, *win)
    return LagFollower(base, lag)


def follow(a, b, dim_begin, dim_end, open_begin=False, lag=0, win=None, cuts=None, tails=None):
    """all rows of a through one stream, cut into pushes of the sizes in cuts (None: one push): (position, cost, settled) over all
    rows; tails, if a list, receives the tail behind every push"""
    a = np.asarray(a, dtype=np.float64)
    f = follower(b, dim_begin, dim_end, open_begin, lag, win)
    cuts = [len(a)] if cuts is None else list(cuts)
    assert sum(cuts) == len(a)
    out, o = [], 0
    for c in cuts:
        out.append(f.push(a[o:o + c]))
        o += c
        if tails is not None and c:
            tails.append(f.tail())
    return tuple(np.concatenate([x[k] for x in out]) for k in range(3))


def true_positions(s, n=150):
    """where row i of the voice of align_window_rule.followable(s) was sampled from its track: that recipe's time line (the same
    generator, drawn in the same order)"""
    rng = np.random.default_rng(100 + s)
    rng.standard_normal((300, 8))
    slopes = np.repeat(rng.uniform(0.6, 1.7, n // 30), 30)
    return np.concatenate([[0.0], np.cumsum(slopes)[:-1]])
