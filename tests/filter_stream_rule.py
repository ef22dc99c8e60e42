"""THE rule of include/world_class_filter_stream.h in numpy float64, on tests/filter_rule.py's own centres, spans, weights, log gains
and responses: frame filtering push by push with a bounded state per stream.

    segments done   T(n, F) is the largest T with 0 <= T <= F and c_T <= n
    committed       C(T) = c_{T-1} + 1 if T else 0, which is a_T
    a push          takes n_samples samples and n_rows rows, computes segments T_before .. T_after - 1, gives y[C_before .. C_after)
    the flush       takes the push's samples and rows, then computes segments T .. S - 1 with b_t = min(n - 1, c_{t+1} - 1) and row
                    min(t, F - 1), gives y[C .. n), and the stream has ended until its reset
    acceptance      pending-before plus pushed fits max_pending_samples and max_pending_rows; n stays within 2^31 - 1

The state is bounded: a tail of N partial sums behind C (the sums over the done segments in the whole call's order, t ascending, onto
0.0), the pending samples x[a_T .. n), the pending rows T .. F - 1 and the last row a done segment used.  `mistake` names one of the
one-line mistakes tests/test_filter_stream_rule.py holds the rule against.
"""
import math

import numpy as np

import filter_rule as fr

MISTAKES = ("lt_for_le", "tail_kept_at_reset", "held_before_flush")
MAX_SAMPLES = 2 ** 31 - 1

NEGATIVE = "a negative count"
ENDED = "samples or rows for a stream that has ended (reset it first)"
NO_FIT = "a count that does not fit the windows (pending plus pushed)"
TOO_LONG = "a stream would pass 2^31 - 1 samples"
NO_ROW = "a flush of samples without a row"


class Refused(Exception):
    pass


def segments_done(n, F, frame_period_ms, fs, mistake=None):
    """T(n, F)"""
    if mistake == "held_before_flush" and F > 0:      # (as if the last row could be held already: no bound by F)
        F = n + 2
    T = 0
    while T < F and (fr.centre(T + 1, frame_period_ms, fs) < n if mistake == "lt_for_le" else fr.centre(T + 1, frame_period_ms, fs) <= n):
        T += 1
    return T


def committed(T, frame_period_ms, fs):
    """C(T) = a_T"""
    return fr.centre(T - 1, frame_period_ms, fs) + 1 if T else 0


def min_pending_samples(frame_period_ms, fs):
    """the least max_pending_samples create takes: 2 ceil(h)"""
    return 2 * math.ceil(fr.hop(frame_period_ms, fs))


def latency_bound(frame_period_ms, fs):
    return 2 * math.ceil(fr.hop(frame_period_ms, fs)) - 2


class Counts:
    """the host half on counts alone: what a push does to (n, F, T, C, ended) of one stream"""

    def __init__(self, fs, frame_period_ms, max_pending_samples, max_pending_rows, mistake=None):
        self.fs, self.fp, self.max_s, self.max_r, self.mistake = fs, frame_period_ms, max_pending_samples, max_pending_rows, mistake
        self.n = self.F = self.T = self.C = 0
        self.ended = False

    pending_samples = property(lambda self: self.n - self.C)
    pending_rows = property(lambda self: 0 if self.ended else self.F - self.T)

    def refusal(self, ns, nr, flush):
        """why a push is refused, or None: the checks in the library's order"""
        if ns < 0 or nr < 0:
            return NEGATIVE
        if self.ended and (ns > 0 or nr > 0):
            return ENDED
        if (self.n - self.C) + ns > self.max_s or (self.F - self.T) + nr > self.max_r:
            return NO_FIT
        if self.n + ns > MAX_SAMPLES:
            return TOO_LONG
        if flush and not self.ended and self.n + ns > 0 and self.F + nr == 0:
            return NO_ROW
        return None

    def step(self, ns, nr, flush):
        """-> (T_before, T_after, C_before, C_after); the state moves"""
        why = self.refusal(ns, nr, flush)
        if why:
            raise Refused(why)
        T0, C0 = self.T, self.C
        flush = bool(flush) and not self.ended
        if ns > 0 or nr > 0 or flush:
            self.n += ns
            self.F += nr
            if flush:
                self.T, self.C, self.ended = fr.segments(self.n, self.fp, self.fs), self.n, True
            else:
                self.T = segments_done(self.n, self.F, self.fp, self.fs, self.mistake)
                self.C = committed(self.T, self.fp, self.fs)
        return T0, self.T, C0, self.C


class Stream(Counts):
    """one stream: push(x, rows, flush) -> the outputs the push commits"""

    def __init__(self, fs, fft_size, frame_period_ms, kind, max_pending_samples, max_pending_rows, mistake=None):
        Counts.__init__(self, fs, frame_period_ms, max_pending_samples, max_pending_rows, mistake)
        self.N, self.kind = fft_size, kind
        self.tail = np.zeros(fft_size)
        self.x = np.zeros(0)                                 # x[C .. n)
        self.rows = np.zeros((0, fft_size // 2 + 1))         # rows T .. F - 1
        self.last_row = None                                 # row T - 1

    def reset(self):
        self.n = self.F = self.T = self.C = 0
        self.ended = False
        self.x, self.rows, self.last_row = np.zeros(0), np.zeros((0, self.N // 2 + 1)), None
        if self.mistake != "tail_kept_at_reset":
            self.tail = np.zeros(self.N)

    def push(self, x=(), rows=None, flush=False):
        x = np.asarray(x, dtype=np.float64).ravel()
        rows = np.zeros((0, self.N // 2 + 1)) if rows is None else np.asarray(rows, dtype=np.float64).reshape(-1, self.N // 2 + 1)
        flushing = bool(flush) and not self.ended
        T0, T1, C0, C1 = self.step(len(x), len(rows), flush)
        # the new windows, assembled before a segment is consumed
        xw, rw = np.concatenate([self.x, x]), np.concatenate([self.rows, rows])
        assert len(xw) <= self.max_s and len(rw) <= self.max_r
        s, ls, starts = np.zeros((T1 - T0, self.N)), np.zeros((T1 - T0, self.N // 2 + 1)), []
        for t in range(T0, T1):
            a, b, L = fr.span(t, self.n, self.fp, self.fs)
            if self.mistake is None:
                assert flushing or b == fr.centre(t + 1, self.fp, self.fs) - 1  # a done segment has every sample below c_{t+1}
            got = xw[a - C0:b + 1 - C0]
            s[t - T0, :len(got)] = got * fr.weights(t, self.n, self.fp, self.fs)[:len(got)]
            row = rw[t - T0] if t - T0 < len(rw) else (rw[-1] if len(rw) else self.last_row)   # (the held one: at a flush only)
            ls[t - T0] = fr.log_gains(row, self.kind)
            starts.append(a)
        out = C1 - C0
        span = out if flushing else out + self.N
        acc = np.zeros(span)
        m = min(self.N, span)
        acc[:m] = self.tail[:m]
        if T1 > T0:
            r, _, _ = fr.responses(s, ls, self.N)
            for i, a in enumerate(starts):
                hi = min(a - C0 + self.N, span)
                acc[a - C0:hi] += r[i, :hi - (a - C0)]
        y = acc[:out].copy()
        if len(x) or len(rows) or flushing:
            self.tail = np.zeros(self.N) if flushing else acc[out:out + self.N].copy()
            self.x = xw[C1 - C0:]
            used = min(T1 - T0, len(rw))
            if used:
                self.last_row = rw[used - 1]
            self.rows = rw[used:]
        return y


def one_call(fs, fft_size, frame_period_ms, kind, x, rows, pushes, max_pending_samples=None, max_pending_rows=None, mistake=None):
    """a stream driven by pushes [(n_samples, n_rows, flush)] over x and rows -> the concatenated outputs"""
    st = Stream(fs, fft_size, frame_period_ms, kind, max_pending_samples or max(len(x), min_pending_samples(frame_period_ms, fs)),
                max_pending_rows or max(len(rows), 1), mistake)
    i = j = 0
    out = []
    for ns, nr, flush in pushes:
        out.append(st.push(x[i:i + ns], rows[j:j + nr], flush))
        i, j = i + ns, j + nr
    assert i == len(x) and j == len(rows)
    return np.concatenate(out) if out else np.zeros(0)


# ---- the cuts the tests share: lists of (n_samples, n_rows, flush) that end in a flush -------------------------------------------------
CUTS = ("one_sample", "hop_and_row", "rows_first", "samples_first", "random", "all_at_once")


def cut(how, n, F, frame_period_ms, fs, seed=0):
    h = max(int(fr.hop(frame_period_ms, fs)), 1)
    if how == "all_at_once":
        return [(n, F, 1)]
    if how == "one_sample":                          # row t comes with the sample at c_t, what is left of the rows with the flush
        pushes, j = [], 0
        for k in range(n):
            nr = 1 if j < F and fr.centre(j, frame_period_ms, fs) <= k else 0
            pushes.append((1, nr, 0))
            j += nr
        return pushes + [(0, F - j, 1)]
    if how == "hop_and_row":
        pushes, i, j = [], 0, 0
        while i < n or j < F:
            ns, nr = min(h, n - i), min(1, F - j)
            pushes.append((ns, nr, 0))
            i, j = i + ns, j + nr
        return pushes + [(0, 0, 1)]
    if how == "rows_first":
        return [(0, F, 0)] + [(min(7, n - i), 0, 0) for i in range(0, n, 7)] + [(0, 0, 1)]
    if how == "samples_first":
        return [(min(7, n - i), 0, 0) for i in range(0, n, 7)] + [(0, 1, 0)] * F + [(0, 0, 1)]
    assert how == "random"
    rng = np.random.default_rng(4000 + seed)
    pushes, i, j = [], 0, 0
    while i < n or j < F:
        ns = int(min(n - i, rng.integers(0, 3 * h + 1))) if rng.random() < 0.8 else 0
        nr = int(min(F - j, rng.integers(0, 4))) if rng.random() < 0.6 else 0
        pushes.append((ns, nr, 0))
        i, j = i + ns, j + nr
    return pushes + [(0, 0, 1)]
