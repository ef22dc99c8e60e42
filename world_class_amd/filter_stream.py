"""Python mirror of include/world_class_filter_stream.h: filter streams -- frame filtering push by push.  A FilterStream takes the samples
and the gain rows of live voices as they arrive and commits, push by push, the outputs FrameFilter gives on the whole signal, bit for
bit; the flush (a flag per stream in a push) commits the rest.  tests/filter_stream_rule.py states the rule."""
import ctypes as C

import numpy as np

from . import DeviceArray, WorldClassError, _check, _ints, _opt, last_error  # noqa: F401
from ._binding import _binder, _count, _Handle, pack_rows, split_rows, uploaded
from .filter import KINDS

_vp = C.c_void_p
_ip = C.POINTER(C.c_int)
_ll = C.c_longlong

FILTER_STREAM_SIGNATURES = {
    "wc_filter_stream_segments_done": (_ll, [C.c_int, C.c_double, _ll, _ll]),
    "wc_filter_stream_committed": (_ll, [C.c_int, C.c_double, _ll]),
    "wc_filter_stream_create": (_vp, [C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int]),
    "wc_filter_stream_destroy": (None, [_vp]),
    "wc_filter_stream_reset": (C.c_int, [_vp, C.c_int]),
    "wc_filter_stream_push_device": (C.c_int, [_vp, _ip, _vp, _ip, _vp, _ip, _vp, _ip]),
    "wc_filter_stream_push_coded_device": (C.c_int, [_vp, _ip, _vp, _ip, _vp, _vp, C.c_int, C.c_int, _ip, _vp, _ip]),
    "wc_filter_stream_samples_received": (_ll, [_vp, C.c_int]),
    "wc_filter_stream_rows_received": (_ll, [_vp, C.c_int]),
    "wc_filter_stream_segments_done_of": (_ll, [_vp, C.c_int]),
    "wc_filter_stream_samples_committed": (_ll, [_vp, C.c_int]),
    "wc_filter_stream_pending_samples": (C.c_int, [_vp, C.c_int]),
    "wc_filter_stream_pending_rows": (C.c_int, [_vp, C.c_int]),
}

_L = _binder(FILTER_STREAM_SIGNATURES)


def segments_done(fs, frame_period_ms, n, rows):
    """T(n, F): the segments a stream has done after n samples and so many rows"""
    t = int(_L().wc_filter_stream_segments_done(int(fs), float(frame_period_ms), int(n), int(rows)))
    if t < 0:
        raise ValueError("a setting create refuses, or a negative count")
    return t


def committed(fs, frame_period_ms, segments):
    """C(T): the outputs a stream has committed after so many segments"""
    c = int(_L().wc_filter_stream_committed(int(fs), float(frame_period_ms), int(segments)))
    if c < 0:
        raise ValueError("a setting create refuses, or a negative count")
    return c


class FilterStream(_Handle):
    """n_streams concurrent filter streams of one (fs, fft_size, frame period, kind): a stream holds at most max_pending_samples
    samples (at least 2 ceil(hop)) and max_pending_rows rows that wait for each other.  The handle lives on the device current at
    construction and serves one call at a time"""
    _lib = staticmethod(_L)
    _sym = "wc_filter_stream"

    def __init__(self, fs, fft_size, frame_period_ms=5.0, kind="power", n_streams=1, max_pending_samples=None, max_pending_rows=8):
        self.fs, self.fft_size, self.frame_period_ms, self.kind = int(fs), int(fft_size), float(frame_period_ms), kind
        self.n_streams, self.width = int(n_streams), int(fft_size) // 2 + 1
        if max_pending_samples is None:      # room for max_pending_rows hops beside the two a stream may be behind
            max_pending_samples = int(np.ceil(self.frame_period_ms * self.fs / 1000.0)) * (2 + int(max_pending_rows))
        self.max_pending_samples, self.max_pending_rows = int(max_pending_samples), int(max_pending_rows)
        self._create(self.fs, self.fft_size, self.frame_period_ms, KINDS[kind], self.n_streams, self.max_pending_samples, self.max_pending_rows)

    def reset(self, stream):
        """the stream forgets everything and is a fresh one"""
        _check(self._fn("_reset")(self._h, int(stream)))

    def _counts(self, n_samples, n_rows, flush):
        if len(n_samples) != self.n_streams or len(n_rows) != self.n_streams or (flush is not None and len(flush) != self.n_streams):
            raise ValueError("one entry per stream")
        return _ints(n_samples), _ints(n_rows), None if flush is None else _ints([1 if f else 0 for f in flush]), (C.c_int * self.n_streams)()

    def push(self, n_samples, d_x, n_rows, d_rows, d_y, flush=None):
        """n_samples[u] samples packed in d_x and n_rows[u] rows of fft_size/2+1 gains packed in d_rows per stream; the committed
        outputs packed in d_y (room for n_streams x max_pending_samples) by the counts that come back; enqueue-only"""
        ns, nr, fl, got = self._counts(n_samples, n_rows, flush)
        _check(self._fn("_push_device")(self._h, ns, _opt(d_x), nr, _opt(d_rows), fl, _opt(d_y), got))
        return list(got)

    def push_coded(self, n_samples, d_x, n_rows, d_coded_to, d_coded_from, number_of_dimensions, d_y, skip_energy=False, flush=None):
        """as push, the gain of a row being the decoded difference of its two coded rows (d_coded_from None: of d_coded_to alone)"""
        ns, nr, fl, got = self._counts(n_samples, n_rows, flush)
        _check(self._fn("_push_coded_device")(self._h, ns, _opt(d_x), nr, _opt(d_coded_to), _opt(d_coded_from), int(number_of_dimensions),
                                              int(bool(skip_energy)), fl, _opt(d_y), got))
        return list(got)

    def samples_received(self, stream):
        return _count(self._fn("_samples_received")(self._h, int(stream)))

    def rows_received(self, stream):
        return _count(self._fn("_rows_received")(self._h, int(stream)))

    def segments_done(self, stream):
        return _count(self._fn("_segments_done_of")(self._h, int(stream)))

    def samples_committed(self, stream):
        return _count(self._fn("_samples_committed")(self._h, int(stream)))

    def pending_samples(self, stream):
        return _count(self._fn("_pending_samples")(self._h, int(stream)))

    def pending_rows(self, stream):
        return _count(self._fn("_pending_rows")(self._h, int(stream)))

    def _host(self, xs, width, mats, flush, call):
        ns, x = pack_rows(xs, 1)
        packed = [pack_rows(m, width) for m in mats if m is not None]
        nr = packed[0][0]
        if any(p[0] != nr for p in packed):
            raise ValueError("as many rows to convert from as to convert to")
        flat = iter(p[1] for p in packed)
        with uploaded(x, *[None if m is None else next(flat) for m in mats]) as held:
            d_y = DeviceArray(self.n_streams * self.max_pending_samples)
            try:
                got = call(ns, held, nr, d_y)
                y = d_y.to_host()      # (the copy waits for the stream)
            finally:
                d_y.free()
        return split_rows(y, got)

    def push_host(self, xs, rows, flush=None):
        """xs[u]: the stream's new samples (None or empty: none), rows[u]: its new rows [k, fft_size/2+1] (None: none) -> the
        outputs each stream commits, one array per stream"""
        return self._host(xs, self.width, [rows], flush, lambda ns, d, nr, d_y: self.push(ns, d[0], nr, d[1], d_y, flush))

    def push_coded_host(self, xs, coded_to, coded_from=None, skip_energy=False, flush=None):
        """as push_host with coded rows [k, number_of_dimensions]; the width is that of the first stream that has rows"""
        nd = next((int(np.shape(m)[1]) for m in coded_to if m is not None and np.ndim(m) == 2), 1)
        return self._host(xs, nd, [coded_to, coded_from], flush,
                          lambda ns, d, nr, d_y: self.push_coded(ns, d[0], nr, d[1], d[2], nd, d_y, skip_energy, flush))
