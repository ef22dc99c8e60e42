"""Python mirror of include/world_class_mlpg_stream.h: MLPG streams.  An MlpgStream takes rows of predicted means and variances push
by push and emits, `lag` rows behind the newest, the static rows features.unpack(orders=1) and then a synthesis stream take; each
emitted row is features.mlpg's on the prefix that ends `lag` rows later, bit for bit, and the flush is the whole call's last rows."""
import ctypes as C

from . import DeviceArray, _check, _ints, _opt  # noqa: F401  (_ints: for raw calls through _L(), as the tests make them)
from .features import FORMATS
from ._binding import _binder, _lag_emitted, _LagStream

_ip = C.POINTER(C.c_int)
_vp = C.c_void_p

MLPG_STREAM_SIGNATURES = {
    "wc_mlpg_stream_emitted": (C.c_longlong, [C.c_longlong, C.c_int]),
    "wc_mlpg_stream_create": (_vp, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "wc_mlpg_stream_destroy": (None, [_vp]),
    "wc_mlpg_stream_reset": (C.c_int, [_vp, C.c_int, C.c_int]),
    "wc_mlpg_stream_push_device": (C.c_int, [_vp, _ip, C.c_int, _vp, _vp, C.c_int, _vp, _ip]),
    "wc_mlpg_stream_flush_device": (C.c_int, [_vp, _ip, _vp, _ip]),
    "wc_mlpg_stream_max_frames_per_push": (C.c_int, [_vp]),
    "wc_mlpg_stream_max_frames_per_flush": (C.c_int, [_vp]),
    "wc_mlpg_stream_rows_received": (C.c_longlong, [_vp, C.c_int]),
    "wc_mlpg_stream_frames_emitted": (C.c_longlong, [_vp, C.c_int]),
    "wc_mlpg_stream_get_lag": (C.c_int, [_vp, C.c_int]),
}

_L = _binder(MLPG_STREAM_SIGNATURES)


emitted = _lag_emitted(_L, "wc_mlpg_stream_emitted",
                       "E(rows) = max(rows - lag, 0): the frames a stream that has not ended has emitted after so many rows")


class MlpgStream(_LagStream):
    """n_streams concurrent streams of rows of width orders * (nd + 1 + n_ap) + 1 (orders 2 or 3), at most max_rows_per_push rows per
    stream and push, each stream with a lag of at most max_lag rows given at its reset.  Emitted rows have nd + 2 + n_ap doubles"""
    _lib = staticmethod(_L)
    _sym = "wc_mlpg"

    def __init__(self, n_streams, nd, n_ap, orders, max_rows_per_push, max_lag):
        self.n_streams, self.nd, self.n_ap, self.orders = int(n_streams), int(nd), int(n_ap), int(orders)
        self._create(self.n_streams, self.nd, self.n_ap, self.orders, int(max_rows_per_push), int(max_lag))

    def reset(self, stream, lag):
        """the stream forgets everything and takes rows again, emitting `lag` rows behind the newest"""
        _check(self._fn("_stream_reset")(self._h, int(stream), int(lag)))

    def push_device(self, n_rows, d_mean, d_var, d_static, var_per_frame=False, in_format="f64"):
        """n_rows[u] rows per stream packed in d_mean (and in d_var, or one row of variances for the push), the emitted static rows
        packed by the counts that come back; enqueue-only.  Returns frames_out"""
        counts, got = self._counts(n_rows)
        _check(self._fn("_stream_push_device")(self._h, counts, FORMATS[in_format][0], _opt(d_mean), _opt(d_var), 1 if var_per_frame else 0,
                                               _opt(d_static), got))
        return list(got)

    def flush_device(self, want, d_static):
        """the last min(lag, rows) rows of every wanted stream, which then has ended; enqueue-only.  Returns frames_out"""
        counts, got = self._counts([1 if w else 0 for w in want])
        _check(self._fn("_stream_flush_device")(self._h, counts, _opt(d_static), got))
        return list(got)
