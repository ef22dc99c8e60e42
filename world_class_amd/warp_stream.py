"""Python mirror of include/world_class_warp_stream.h: a resident track played on a live voice's timing.  warp_along_map_device is
warp.map_positions_device followed by warp.warp_device without the positions in between; a WarpStream consumes the settled positions
of an alignment stream where they lie, push by push, and its concatenated outputs are that call's bit for bit."""
import ctypes as C

import numpy as np

from . import DeviceArray, _check, _ints, _opt  # noqa: F401  (_ints: for raw calls through _L(), as the tests make them)
from ._binding import IN_FORMATS, OUT_FORMATS, _binder, _count, _Handle
from .vresample import _plan, _step

_ip = C.POINTER(C.c_int)
_vp = C.c_void_p

WARP_STREAM_SIGNATURES = {
    "wc_warp_stream_committed": (C.c_longlong, [C.c_longlong, C.c_double]),
    "wc_warp_along_map_device": (C.c_int, [_vp, C.c_int, _vp, C.c_int, _ip, _vp, _ip, C.c_double, C.c_double, _ip, _vp, C.c_int]),
    "wc_warp_stream_create": (_vp, _plan + [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double]),
    "wc_warp_stream_destroy": (None, [_vp]),
    "wc_warp_stream_set_track_device": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "wc_warp_stream_reset": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double]),
    "wc_warp_stream_max_out_per_push": (C.c_int, [_vp]),
    "wc_warp_stream_max_out_per_flush": (C.c_int, [_vp]),
    "wc_warp_stream_push_device": (C.c_int, [_vp, _ip, _vp, _vp, C.c_int, _ip]),
    "wc_warp_stream_flush_device": (C.c_int, [_vp, _ip, _vp, _vp, C.c_int, _ip]),
    "wc_warp_stream_rows_received": (C.c_longlong, [_vp, C.c_int]),
    "wc_warp_stream_entries_consumed": (C.c_longlong, [_vp, C.c_int]),
    "wc_warp_stream_samples_committed": (C.c_longlong, [_vp, C.c_int]),
    "wc_warp_stream_get_delay": (C.c_int, [_vp, C.c_int]),
    "wc_warp_stream_track_length": (C.c_int, [_vp, C.c_int]),
}

_L = _binder(WARP_STREAM_SIGNATURES)


def committed(entries, out_per_entry):
    """c(entries): the outputs a stream has committed after so many consumed map entries"""
    return _count(_L().wc_warp_stream_committed(int(entries), float(out_per_entry)))


def warp_along_map_device(resampler, d_x, x_lengths, d_map, map_lengths, out_per_entry, in_per_unit, out_lengths, d_y, in_format="f64",
                          out_format="f64"):
    """packed device arrays: utterance u's map (float64) at the sum of the map_lengths before it, its outputs at the sum of the
    out_lengths before it, each at the position the map rule gives it; enqueue-only"""
    if len(map_lengths) != len(x_lengths) or len(out_lengths) != len(x_lengths):
        raise ValueError("one map length and one output length per utterance")
    _check(_L().wc_warp_along_map_device(resampler._h, len(x_lengths), _opt(d_x), IN_FORMATS[in_format][0], _ints(x_lengths), _opt(d_map),
                                         _ints(map_lengths), float(out_per_entry), float(in_per_unit), _ints(out_lengths), _opt(d_y),
                                         OUT_FORMATS[out_format][0]))


class WarpStream(_Handle):
    """n_streams concurrent outputs, each a resident track read along a map that arrives entry by entry (one double per pushed row,
    the first `delay` rows of a stream unread).  For any cut into pushes a stream's concatenated outputs, flush included, are
    warp_along_map_device's for the track and the map of all consumed entries"""
    _lib = staticmethod(_L)
    _sym = "wc_warp"
    _kind = "_stream"

    def __init__(self, step_min, step_max, n_streams, n_tracks, max_track_samples, max_entries_per_push, max_delay, max_out_per_entry,
                 track_format="f64", zeros=0, rolloff=0.0, beta=0.0, phase_bits=0, degree=0):
        self.step_min, self.step_max = int(step_min), int(step_max)
        self.n_streams, self.n_tracks, self.track_format = int(n_streams), int(n_tracks), track_format
        self._create(_step(step_min), _step(step_max), int(zeros), float(rolloff), float(beta), int(phase_bits), int(degree), self.n_streams,
                     self.n_tracks, int(max_track_samples), IN_FORMATS[track_format][0], int(max_entries_per_push), int(max_delay),
                     float(max_out_per_entry))

    @property
    def max_out_per_push(self):
        return int(self._fn("_stream_max_out_per_push")(self._h))

    @property
    def max_out_per_flush(self):
        return int(self._fn("_stream_max_out_per_flush")(self._h))

    def set_track_device(self, track, n_samples, d_x):
        """n_samples samples of the handle's track_format from device memory into a slot; stream-ordered"""
        _check(self._fn("_stream_set_track_device")(self._h, int(track), int(n_samples), _opt(d_x)))

    def set_track(self, track, x):
        """a 1-D host array into a slot, as the handle's track_format"""
        x = np.ascontiguousarray(x, dtype=IN_FORMATS[self.track_format][1]).ravel()
        d_x = DeviceArray.from_host(x, dtype=IN_FORMATS[self.track_format][1])
        try:
            self.set_track_device(track, len(x), d_x)
            _check(self._lib().wc_synchronize())  # (the copy has read d_x)
        finally:
            d_x.free()

    def reset(self, stream, track, delay, out_per_entry, in_per_unit):
        _check(self._fn("_stream_reset")(self._h, int(stream), int(track), int(delay), float(out_per_entry), float(in_per_unit)))

    def _run(self, name, counts, d_in, d_y, out_format):
        if len(counts) != self.n_streams:
            raise ValueError("one entry per stream")
        got = (C.c_int * self.n_streams)()
        _check(self._fn(name)(self._h, _ints(counts), _opt(d_in), _opt(d_y), OUT_FORMATS[out_format][0], got))
        return list(got)

    def push_device(self, n_rows, d_map, d_y, out_format="f64"):
        """n_rows[u] doubles per stream packed in d_map, outputs packed by the counts that come back; enqueue-only.  Returns
        samples_out"""
        return self._run("_stream_push_device", n_rows, d_map, d_y, out_format)

    def flush_device(self, want, d_tail, d_y, out_format="f64"):
        """d_tail in the layout of an alignment stream's tail for the same want; enqueue-only.  Returns samples_out"""
        return self._run("_stream_flush_device", [1 if w else 0 for w in want], d_tail, d_y, out_format)

    def rows_received(self, stream):
        return int(self._fn("_stream_rows_received")(self._h, int(stream)))

    def entries_consumed(self, stream):
        return int(self._fn("_stream_entries_consumed")(self._h, int(stream)))

    def samples_committed(self, stream):
        return int(self._fn("_stream_samples_committed")(self._h, int(stream)))

    def get_delay(self, stream):
        return int(self._fn("_stream_get_delay")(self._h, int(stream)))

    def track_length(self, track):
        return int(self._fn("_stream_track_length")(self._h, int(track)))
