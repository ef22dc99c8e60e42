"""THE rule of include/world_class_mlpg_stream.h in numpy, twice: by_prefixes is the definition (tests/features_rule.py's mlpg on
every prefix), Stream is the bounded-state recursion the kernels implement -- the carried row, a ring of parked l1, l2, z / d, end
quotient and vuv -- driven by any cut into pushes.  Every operation in float64, rounded on its own, in the header's order: the two
agree bit for bit (a NaN is a NaN, whatever its payload), and the device equals Stream."""
import numpy as np

import features_rule as fr


def emitted(rows, lag):
    """E(rows): the frames a stream that has not ended has emitted after so many rows; -1 for negative arguments"""
    return -1 if rows < 0 or lag < 0 else max(rows - lag, 0)


def out_columns(nd, n_ap):
    """the output column of every static column (vuv stands behind lf0), and S"""
    S = nd + 1 + n_ap
    return [c if c <= nd else c + 1 for c in range(S)], S


def by_prefixes(nd, n_ap, orders, lag, mean, var, var_per_frame):
    """(the rows the pushes emit [max(n - lag, 0), S + 1], the rows of the flush [min(lag, n), S + 1]) of one stream of n rows:
    pushed row i >= lag emits row i - lag of mlpg(rows 0 .. i); the flush is the whole call's last rows"""
    W = fr.width(nd, n_ap, orders)
    mean = np.asarray(mean, dtype=np.float64).reshape(-1, W)
    n = len(mean)
    var = np.asarray(var, dtype=np.float64).reshape(n if var_per_frame else 1, W)
    of = lambda i: fr.mlpg([i + 1], nd, n_ap, orders, mean[:i + 1], var[:i + 1] if var_per_frame else var, var_per_frame)
    pushed = [of(i)[i - lag] for i in range(lag, n)]
    whole = of(n - 1) if n else np.zeros((0, nd + 2 + n_ap))
    return np.array(pushed).reshape(len(pushed), nd + 2 + n_ap), whole[emitted(n, lag):]


class Stream:
    """one stream since its reset.  The state is what the forward kernel carries per static column, before its newest row t is
    finished: the precisions and weighted means of rows t - 1 and t, d and z of rows t - 1 and t - 2, l1(t), l2(t), a2(t - 1) and
    whether a variance so far was bad; the ring holds l1, l2, z / d, the end quotient and vuv of the last `capacity` rows"""

    def __init__(self, nd, n_ap, orders, lag, max_rows_per_push=8, max_lag=None):
        self.nd, self.n_ap, self.orders, self.lag = nd, n_ap, orders, lag
        self.ocols, self.S = out_columns(nd, n_ap)
        cols, self.vuv_col = fr.columns(nd, n_ap, orders)
        self.take = np.array(cols).T   # [orders, S]
        self.max_rows = max_rows_per_push
        self.cap = (lag if max_lag is None else max_lag) + max_rows_per_push + 1
        S = self.S
        self.ring = np.full((self.cap, 4, S), np.nan)   # l1, l2, z / d, z_end / d_end
        self.ring_vuv = np.full(self.cap, np.nan)
        self.rows, self.ended = 0, False
        z = lambda: np.zeros(S)
        self.prev = np.zeros((4, S))   # p1, p2, q1, q2 of row t - 1
        self.cur = np.zeros((6, S))    # p0, p1, p2, q0, q1, q2 of row t
        self.d1, self.d2, self.z1, self.z2, self.l1c, self.l2c, self.a2p = z(), z(), z(), z(), z(), z(), z()
        self.bad = np.zeros(S, dtype=bool)

    def _convert(self, m, v):
        """a row's means and variances [orders, S] -> p0, p1, p2, q0, q1, q2 (the bad variances noted)"""
        with np.errstate(all="ignore"):
            self.bad |= (~(v > 0.0)).any(axis=0)
            pq = np.zeros((6, self.S))
            pq[:self.orders] = 1.0 / v
            pq[3:3 + self.orders] = np.where(pq[:self.orders] == 0.0, 0.0, pq[:self.orders] * m)
        return pq

    def _row(self, m, v, vuv):
        """takes row i = self.rows: finishes row i - 1 now that its successor is known, then parks row i's l1, l2 and end quotient"""
        i, S = self.rows, self.S
        nxt = self._convert(m, v)
        prev, cur = self.prev, self.cur
        with np.errstate(all="ignore"):
            if i >= 1:
                t = i - 1
                a0 = (cur[0] + 0.25 * (prev[0] + nxt[1])) + ((prev[1] + nxt[2]) + 4.0 * cur[2])
                a1 = -2.0 * (cur[2] + nxt[2])
                a2 = nxt[2] - 0.25 * nxt[1]
                r = (cur[3] + 0.5 * (prev[2] - nxt[4])) + ((prev[3] + nxt[5]) - 2.0 * cur[5])
                d, z = a0, r
                if t >= 2:
                    d = d - (self.l2c * self.l2c) * self.d2
                if t >= 1:
                    d = d - (self.l1c * self.l1c) * self.d1
                if t >= 2:
                    z = z - self.l2c * self.z2
                if t >= 1:
                    z = z - self.l1c * self.z1
                self.ring[t % self.cap, 2] = z / d
                if i >= 2:
                    l2n = self.a2p / self.d1
                    l1n = (a1 - (l2n * self.d1) * self.l1c) / d
                else:
                    l2n, l1n = np.zeros(S), a1 / d
                self.d2, self.d1, self.z2, self.z1 = self.d1, d, self.z1, z
                self.l1c, self.l2c, self.a2p = l1n, l2n, a2
                self.prev = np.array([cur[1], cur[2], cur[4], cur[5]])
            self.cur = cur = nxt
            prev = self.prev
            # row i as the last row of its prefix: the same expressions with the successor's zeros
            a0 = (cur[0] + 0.25 * (prev[0] + 0.0)) + ((prev[1] + 0.0) + 4.0 * cur[2])
            r = (cur[3] + 0.5 * (prev[2] - 0.0)) + ((prev[3] + 0.0) - 2.0 * cur[5])
            d, z = a0, r
            if i >= 2:
                d = d - (self.l2c * self.l2c) * self.d2
            if i >= 1:
                d = d - (self.l1c * self.l1c) * self.d1
            if i >= 2:
                z = z - self.l2c * self.z2
            if i >= 1:
                z = z - self.l1c * self.z1
            slot = self.ring[i % self.cap]
            slot[0], slot[1] = self.l1c, self.l2c
            slot[3] = np.where(self.bad, np.nan, z / d)
        self.ring_vuv[i % self.cap] = vuv
        self.rows += 1

    def _walk(self, top, low, every):
        """the back-substitution of the prefix that ends at row `top`, down to frame `low`: that frame, or every frame it passes"""
        out = np.zeros((top - low + 1, self.S + 1))
        c1, c2 = np.zeros(self.S), np.zeros(self.S)
        l1n, l2n, l2nn = np.zeros(self.S), np.zeros(self.S), np.zeros(self.S)
        with np.errstate(all="ignore"):
            for t in range(top, low - 1, -1):
                slot = self.ring[t % self.cap]
                x = slot[3] if t == top else slot[2]
                if t + 1 <= top:
                    x = x - l1n * c1
                if t + 2 <= top:
                    x = x - l2nn * c2
                out[t - low, self.ocols] = x
                out[t - low, self.nd + 1] = self.ring_vuv[t % self.cap]
                c2, c1, l2nn, l2n, l1n = c1, x, l2n, slot[1].copy(), slot[0].copy()
        return out if every else out[:1]

    def push(self, mean, var, var_per_frame=True):
        """rows of means [k, width]; rows of variances [k, width], or one row -> the static rows this push emits"""
        assert not self.ended
        W = fr.width(self.nd, self.n_ap, self.orders)
        mean = np.asarray(mean, dtype=np.float64).reshape(-1, W)
        k = len(mean)
        assert k <= self.max_rows
        var = np.asarray(var, dtype=np.float64).reshape(k if var_per_frame else 1, W) if k else np.zeros((0, W))
        out = []
        for j in range(k):
            self._row(mean[j][self.take], var[j if var_per_frame else 0][self.take], mean[j, self.vuv_col])
            i = self.rows - 1
            if i >= self.lag:
                out.append(self._walk(i, i - self.lag, False)[0])
        return np.array(out).reshape(len(out), self.S + 1)

    def flush(self):
        assert not self.ended
        self.ended = True
        n = self.rows
        if n == 0 or self.lag == 0:
            return np.zeros((0, self.S + 1))
        return self._walk(n - 1, emitted(n, self.lag), True)


def stream(nd, n_ap, orders, lag, mean, var, var_per_frame, cuts, max_rows_per_push=None, max_lag=None):
    """one stream's rows cut into pushes of cuts[0], cuts[1], ... rows (zeros allowed; they sum to the rows): (the list of each
    push's rows, the flush's rows)"""
    W = fr.width(nd, n_ap, orders)
    mean = np.asarray(mean, dtype=np.float64).reshape(-1, W)
    assert sum(cuts) == len(mean)
    var = np.asarray(var, dtype=np.float64).reshape(len(mean) if var_per_frame else 1, W)
    s = Stream(nd, n_ap, orders, lag, max(list(cuts) + [1]) if max_rows_per_push is None else max_rows_per_push, max_lag)
    outs, o = [], 0
    for k in cuts:
        outs.append(s.push(mean[o:o + k], var[o:o + k] if var_per_frame else var, var_per_frame))
        o += k
    return outs, s.flush()
