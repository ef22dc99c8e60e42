"""Python mirror of include/world_class_feature_stream.h: feature streams.  A FeatureStream takes rows of F0, coded envelope and
coded aperiodicity push by push, the arrays an analysis stream's coded push writes, and emits, `lag` rows behind the newest, the
packed rows a model reads; each emitted row is features.pack's on the prefix that ends `lag` rows later, bit for bit, and the flush
is the whole call's last rows."""
import ctypes as C

from . import DeviceArray, _check, _ints, _opt  # noqa: F401  (_ints: for raw calls through _L(), as the tests make them)
from .features import FORMATS
from ._binding import _binder, _lag_emitted, _LagStream

_ip = C.POINTER(C.c_int)
_vp = C.c_void_p

FEATURE_STREAM_SIGNATURES = {
    "wc_feature_stream_emitted": (C.c_longlong, [C.c_longlong, C.c_int]),
    "wc_feature_stream_create": (_vp, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "wc_feature_stream_destroy": (None, [_vp]),
    "wc_feature_stream_reset": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double]),
    "wc_feature_stream_push_device": (C.c_int, [_vp, _ip, _vp, _vp, _vp, C.c_int, _vp, _ip]),
    "wc_feature_stream_flush_device": (C.c_int, [_vp, _ip, C.c_int, _vp, _ip]),
    "wc_feature_stream_max_frames_per_push": (C.c_int, [_vp]),
    "wc_feature_stream_max_frames_per_flush": (C.c_int, [_vp]),
    "wc_feature_stream_rows_received": (C.c_longlong, [_vp, C.c_int]),
    "wc_feature_stream_frames_emitted": (C.c_longlong, [_vp, C.c_int]),
    "wc_feature_stream_get_lag": (C.c_int, [_vp, C.c_int]),
}

_L = _binder(FEATURE_STREAM_SIGNATURES)


emitted = _lag_emitted(_L, "wc_feature_stream_emitted",
                       "E(rows) = max(rows - lag, 0): the rows a stream that has not ended has emitted after so many rows")


class FeatureStream(_LagStream):
    """n_streams concurrent streams of rows of one F0, nd coded envelope and n_ap coded aperiodicity values, at most
    max_rows_per_push rows per stream and push, each stream with a lag of at most max_lag rows and an lf0_fill given at its reset.
    Emitted rows have orders * (nd + 1 + n_ap) + 1 columns (orders 1, 2 or 3)"""
    _lib = staticmethod(_L)
    _sym = "wc_feature"

    def __init__(self, n_streams, nd, n_ap, orders, max_rows_per_push, max_lag):
        self.n_streams, self.nd, self.n_ap, self.orders = int(n_streams), int(nd), int(n_ap), int(orders)
        self._create(self.n_streams, self.nd, self.n_ap, self.orders, int(max_rows_per_push), int(max_lag))

    def reset(self, stream, lag, lf0_fill=0.0):
        """the stream forgets everything and takes rows again, emitting `lag` rows behind the newest"""
        _check(self._fn("_stream_reset")(self._h, int(stream), int(lag), float(lf0_fill)))

    def push_device(self, n_rows, d_f0, d_coded_sp, d_coded_ap, d_rows, out_format="f64"):
        """n_rows[u] rows per stream packed in d_f0, d_coded_sp and d_coded_ap (None where n_ap is 0), the emitted rows packed by
        the counts that come back; enqueue-only.  n_rows may be the ctypes array an analysis push filled.  Returns frames_out"""
        counts, got = self._counts(n_rows)
        _check(self._fn("_stream_push_device")(self._h, counts, _opt(d_f0), _opt(d_coded_sp), _opt(d_coded_ap), FORMATS[out_format][0],
                                               _opt(d_rows), got))
        return list(got)

    def flush_device(self, want, d_rows, out_format="f64"):
        """the last min(lag, rows) rows of every wanted stream, which then has ended; enqueue-only.  Returns frames_out"""
        counts, got = self._counts([1 if w else 0 for w in want])
        _check(self._fn("_stream_flush_device")(self._h, counts, FORMATS[out_format][0], _opt(d_rows), got))
        return list(got)
