"""THE rule of include/world_class_feature_stream.h in numpy, twice: by_prefixes is the definition (tests/features_rule.py's pack on
every prefix), Stream is the bounded-state recursion the kernels run -- a ring of the last rows with the log of a voiced F0 parked
on arrival, one carried record, the right neighbour capped at the frame's own prefix -- driven by any cut into pushes.  Every
operation in float64, rounded on its own, in the header's order: the two agree bit for bit, and the device equals Stream.  Stream
keeps a trace of the branches it took, so that a test can assert that a contour reached the branch it was written for."""
import numpy as np

import features_rule as fr


def emitted(rows, lag):
    """E(rows): the rows a stream that has not ended has emitted after so many rows; -1 for negative arguments"""
    return -1 if rows < 0 or lag < 0 else max(rows - lag, 0)


def ring_rows(max_rows_per_push, max_lag):
    """the rows of a stream's ring: a push from T0 to T1 rows at lag L reads rows T0 - L - 1 .. T1 - 1"""
    return max_lag + max_rows_per_push + 1


def _arrays(nd, n_ap, f0, sp, ap, logs):
    f0 = np.asarray(f0, dtype=np.float64).reshape(-1)
    n = len(f0)
    sp = np.asarray(sp, dtype=np.float64).reshape(n, nd)
    ap = np.zeros((n, 0)) if n_ap == 0 else np.asarray(ap, dtype=np.float64).reshape(n, n_ap)
    if logs is None:
        logs = np.zeros(n)
        v = fr.voiced(f0)
        logs[v] = np.log(f0[v])
    return f0, sp, ap, np.asarray(logs, dtype=np.float64).reshape(n)


def by_prefixes(nd, n_ap, orders, lag, fill, f0, sp, ap, logs=None):
    """(the rows the pushes emit [max(n - lag, 0), width], the rows of the flush [min(lag, n), width]) of one stream of n rows:
    pushed row i >= lag emits row i - lag of pack(rows 0 .. i); the flush is the whole call's last rows"""
    f0, sp, ap, logs = _arrays(nd, n_ap, f0, sp, ap, logs)
    n, W = len(f0), fr.width(nd, n_ap, orders)
    of = lambda i: fr.pack([i + 1], nd, n_ap, orders, f0[:i + 1], sp[:i + 1], ap[:i + 1], fill, logs=logs[:i + 1])
    pushed = [of(i)[i - lag] for i in range(lag, n)]
    whole = of(n - 1) if n else np.zeros((0, W))
    return np.array(pushed).reshape(len(pushed), W), whole[emitted(n, lag):]


class Stream:
    """one stream since its reset.  ring[i % cap] is row i: the nd coded envelope values, the parked log (NaN: unvoiced), the n_ap
    coded aperiodicity values.  carry is (index, log) of the last voiced row below the window the next call scans, or None"""

    def __init__(self, nd, n_ap, orders, lag, fill, max_rows_per_push=8, max_lag=None):
        self.nd, self.n_ap, self.orders, self.lag, self.fill = nd, n_ap, orders, lag, float(fill)
        self.S = nd + 1 + n_ap
        self.cols, self.vuv_col = fr.columns(nd, n_ap, orders)
        self.max_rows = max_rows_per_push
        self.cap = ring_rows(max_rows_per_push, lag if max_lag is None else max_lag)
        self.ring = np.full((self.cap, self.S), np.nan)
        self.carry = None
        self.rows, self.emitted, self.ended = 0, 0, False
        self.trace = set()

    def _lf0(self, i, j, lo):
        """the continuous log-F0 of row i in the prefix that ends at row j, from the window lo .. and the carried record: the two
        scans of the kernel, read at one row"""
        lg = lambda r: self.ring[r % self.cap, self.nd]
        left = None                      # the prefix max-scan at i; its initial carry is the carried record
        for r in range(i, lo - 1, -1):
            if not np.isnan(lg(r)):
                left = (r, lg(r))
                break
        if left is None and lo > 0 and self.carry is not None:
            left = self.carry
            self.trace.add("left end is the carried record")
        right = None                     # the suffix min-scan at i over the rows up to the newest, capped at j
        for r in range(i, self.rows):
            if not np.isnan(lg(r)):
                right = (r, lg(r))
                break
        if right is not None and right[0] > j:
            right = None
            self.trace.add("a voiced row beyond the prefix is not seen")
        if left is None and right is None:
            self.trace.add("fill")
            return self.fill
        if left is not None and left[0] == i:
            self.trace.add("voiced")
            return left[1]
        if left is None:
            self.trace.add("leading run")
            return right[1]
        if right is None:
            self.trace.add("hold")
            return left[1]
        self.trace.add("interpolated")
        a = np.float64(i - left[0]) / np.float64(right[0] - left[0])
        return (1.0 - a) * left[1] + a * right[1]

    def _emit(self, e0, n_out):
        """frames e0 .. e0 + n_out - 1, frame t from the prefix that ends at j = min(t + lag, newest row)"""
        W = fr.width(self.nd, self.n_ap, self.orders)
        out = np.zeros((n_out, W))
        last = self.rows - 1
        lo = max(e0 - 1, 0)
        assert n_out == 0 or last - lo + 1 <= self.cap   # the window lies in the ring
        if n_out and last // self.cap != lo // self.cap:
            self.trace.add("the window wraps")
        for f in range(n_out):
            t = e0 + f
            j = min(t + self.lag, last)
            x = np.zeros((3, self.S))    # rows t - 1, t, t + 1; a neighbour outside the prefix counts as 0.0
            for n in (-1, 0, 1):
                if 0 <= t + n <= j:
                    x[n + 1] = self.ring[(t + n) % self.cap]
                    x[n + 1, self.nd] = self._lf0(t + n, j, lo)
            if t == j:
                self.trace.add("the successor counts as 0.0")
            with np.errstate(invalid="ignore", over="ignore"):
                parts = (x[1], 0.5 * (x[2] - x[0]), (x[0] + x[2]) - 2.0 * x[1])
            for c, ks in enumerate(self.cols):
                for k, col in enumerate(ks):
                    out[f, col] = parts[k][c]
            out[f, self.vuv_col] = 0.0 if np.isnan(self.ring[t % self.cap, self.nd]) else 1.0
        return out, lo

    def push(self, f0, sp, ap, logs=None):
        """k <= max_rows_per_push rows -> the rows this push emits"""
        assert not self.ended
        f0, sp, ap, logs = _arrays(self.nd, self.n_ap, f0, sp, ap, logs)
        k = len(f0)
        assert k <= self.max_rows
        if k == 0:
            return np.zeros((0, fr.width(self.nd, self.n_ap, self.orders)))
        v = fr.voiced(f0)
        for r in range(k):   # take: the log of a voiced F0 is parked on arrival
            self.ring[(self.rows + r) % self.cap] = np.concatenate([sp[r], [logs[r] if v[r] else np.nan], ap[r]])
        self.rows += k
        e1 = emitted(self.rows, self.lag)
        out, lo = self._emit(self.emitted, e1 - self.emitted)
        # the carried record advances over the rows below the next call's window
        for r in range(lo, max(e1 - 1, 0)):
            if not np.isnan(self.ring[r % self.cap, self.nd]):
                self.carry = (r, self.ring[r % self.cap, self.nd])
                self.trace.add("the carried record advances")
        self.emitted = e1
        return out

    def flush(self):
        assert not self.ended
        self.ended = True
        out, _ = self._emit(self.emitted, self.rows - self.emitted)
        self.emitted = self.rows
        return out


def stream(nd, n_ap, orders, lag, fill, f0, sp, ap, cuts, logs=None, max_rows_per_push=None, max_lag=None, trace=None):
    """one stream's rows cut into pushes of cuts[0], cuts[1], ... rows (zeros allowed; they sum to the rows): (the list of each
    push's rows, the flush's rows); trace: a set that receives the branches the recursion took"""
    f0, sp, ap, logs = _arrays(nd, n_ap, f0, sp, ap, logs)
    assert sum(cuts) == len(f0)
    s = Stream(nd, n_ap, orders, lag, fill, max(list(cuts) + [1]) if max_rows_per_push is None else max_rows_per_push, max_lag)
    outs, o = [], 0
    for k in cuts:
        outs.append(s.push(f0[o:o + k], sp[o:o + k], ap[o:o + k], logs[o:o + k]))
        o += k
    tail = s.flush()
    if trace is not None:
        trace |= s.trace
    return outs, tail


# ---- contours written to reach every branch of the recursion (tests/test_feature_stream_rule.py, tests/test_gpu_feature_stream.py) ----
def runs(n, lengths, first=2, between=2):
    """voiced everywhere but in unvoiced runs of the given lengths, the first behind row `first`, `between` voiced rows between two"""
    v = np.ones(n, dtype=bool)
    i = first + 1
    for g in lengths:
        v[i:i + g] = False
        i += g + between
    assert i <= n, (i, n)
    return v


def f0_of(v, rng, odd=True):
    """F0 of a voiced mask: 70 .. 500 Hz where voiced; 0 elsewhere, the first unvoiced rows NaN, -1 and +inf instead where odd"""
    v = np.asarray(v, dtype=bool)
    f = np.where(v, rng.uniform(70.0, 500.0, len(v)), 0.0)
    if odd:
        for i, bad in zip(np.flatnonzero(~v)[1:4], (np.nan, -1.0, np.inf)):
            f[i] = bad
    return f


def contours(lag, ring):
    """name -> voiced mask, for a stream of lag `lag` in a ring of `ring` rows"""
    one = lambda n, i: np.arange(n) == i
    L = lag
    return {
        "all unvoiced": np.zeros(L + 5, dtype=bool),
        "a single voiced row": one(2 * L + 9, L + 4),
        "a leading run": np.arange(L + 9) >= L + 3,
        "a trailing run": np.arange(L + 8) < 5,
        "runs of L - 1, L and L + 1": runs(3 * L + 16, [g for g in (L - 1, L, L + 1) if g > 0]),
        "a run longer than the ring": runs(ring + L + 12, [ring + 4]),
        "two runs inside one push": runs(L + 14, [1, 2], first=1, between=1),
        "NaN, 0, negative and +inf": runs(L + 20, [1, 1, 1, 1]),
    }
