"""Python mirror of include/world_class_filter.h: frame filtering on the device -- a waveform shaped by one gain row per frame,
without the vocoder.  Rows are power gains ("power", the kind of a spectrogram row), natural-log amplitude gains ("log"), or the
difference of two coded spectral envelopes (run_coded: spectral-differential conversion).  tests/filter_rule.py states the rule."""
import ctypes as C

import numpy as np

from . import DeviceArray, WorldClassError, _check, _ints, _opt, last_error  # noqa: F401
from ._binding import _binder, _count, _Handle

_vp = C.c_void_p
_ip = C.POINTER(C.c_int)

FILTER_SIGNATURES = {
    "wc_frame_filter_create": (_vp, [C.c_int, C.c_int, C.c_double]),
    "wc_frame_filter_destroy": (None, [_vp]),
    "wc_frame_filter_segments": (C.c_int, [_vp, C.c_int]),
    "wc_frame_filter_run_device": (C.c_int, [_vp, C.c_int, _vp, _ip, C.c_int, _vp, _ip, _vp]),
    "wc_frame_filter_run_coded_device": (C.c_int, [_vp, C.c_int, _vp, _ip, _vp, _vp, C.c_int, C.c_int, _ip, _vp]),
}

KINDS = {"power": 0, "log": 1}  # WC_FILTER_POWER, WC_FILTER_LOG

_L = _binder(FILTER_SIGNATURES)


def _signals(xs):
    """one 1-D array or a list of them -> (whether it was a list, the list as float64 vectors)"""
    many = isinstance(xs, (list, tuple))
    return many, [np.ascontiguousarray(x, dtype=np.float64).ravel() for x in (xs if many else [xs])]


def _rows_of(rows, n, width):
    """one [frames, width] array or a list of n of them -> the list as float64 matrices"""
    rows = rows if isinstance(rows, (list, tuple)) else [rows]
    if len(rows) != n:
        raise ValueError("one array of rows per signal")
    out = [np.ascontiguousarray(r, dtype=np.float64) for r in rows]
    for r in out:
        if r.ndim != 2 or r.shape[1] != width:
            raise ValueError(f"rows of {width} values")
    return out


class FrameFilter(_Handle):
    """A frame filter of one (fs, fft_size, frame period): the handle lives on the device current at construction and serves one call
    at a time; its scratch (the response rows of a batch) grows on demand and goes with it."""
    _lib = staticmethod(_L)
    _sym = "wc_frame_filter"

    def __init__(self, fs, fft_size, frame_period_ms=5.0):
        self.fs, self.fft_size, self.frame_period_ms = int(fs), int(fft_size), float(frame_period_ms)
        self._create(self.fs, self.fft_size, self.frame_period_ms)

    def segments(self, x_length):
        """S of the rule for a signal of x_length samples"""
        return _count(_L().wc_frame_filter_segments(self._h, int(x_length)))

    def run(self, d_x, x_lengths, d_rows, f_lengths, d_y, kind="power"):
        """packed device arrays: utterance u's samples (and outputs) at the sum of the x_lengths before it, its rows of
        fft_size/2+1 values at the sum of the f_lengths before it; d_y may be d_x; enqueue-only"""
        if len(f_lengths) != len(x_lengths):
            raise ValueError("one row count per utterance")
        _check(_L().wc_frame_filter_run_device(self._h, len(x_lengths), _opt(d_x), _ints(x_lengths), KINDS[kind], _opt(d_rows),
                                               _ints(f_lengths), _opt(d_y)))

    def run_coded(self, d_x, x_lengths, d_coded_to, d_coded_from, number_of_dimensions, f_lengths, d_y, skip_energy=False):
        """the gain of frame t is the decoded difference of its two coded rows (d_coded_from None: of d_coded_to alone; skip_energy:
        without coefficient 0); enqueue-only"""
        if len(f_lengths) != len(x_lengths):
            raise ValueError("one row count per utterance")
        _check(_L().wc_frame_filter_run_coded_device(self._h, len(x_lengths), _opt(d_x), _ints(x_lengths), _opt(d_coded_to),
                                                     _opt(d_coded_from), int(number_of_dimensions), int(bool(skip_energy)),
                                                     _ints(f_lengths), _opt(d_y)))

    def _host(self, xs, mats, call):
        many, xs = _signals(xs)
        lengths = [len(x) for x in xs]
        held = [DeviceArray.from_host(np.concatenate(xs) if xs else np.zeros(0))]
        try:
            held += [None if m is None else DeviceArray.from_host(np.concatenate(m)) for m in mats]
            call(held, lengths)
            y = held[0].to_host()   # (the copy waits for the stream)
        finally:
            for d in held:
                if d is not None:
                    d.free()
        ys = [y[e - n:e].copy() for n, e in zip(lengths, np.cumsum(lengths))]
        return ys if many else ys[0]

    def filter(self, x, rows, kind="power"):
        """x: one 1-D host array or a list of them; rows: for each, [frames, fft_size/2+1] gains -> the filtered signal(s)"""
        n = len(x) if isinstance(x, (list, tuple)) else 1
        rows = _rows_of(rows, n, self.fft_size // 2 + 1)
        return self._host(x, [rows], lambda d, lengths: self.run(d[0], lengths, d[1], [len(r) for r in rows], d[0], kind))

    def filter_coded(self, x, coded_to, coded_from=None, skip_energy=False):
        """x as for filter; coded_to (and coded_from): for each signal [frames, number_of_dimensions] coded envelopes"""
        n = len(x) if isinstance(x, (list, tuple)) else 1
        nd = int(np.shape(coded_to[0] if isinstance(coded_to, (list, tuple)) else coded_to)[1])
        to = _rows_of(coded_to, n, nd)
        frm = None if coded_from is None else _rows_of(coded_from, n, nd)
        if frm is not None and [len(r) for r in frm] != [len(r) for r in to]:
            raise ValueError("as many rows to convert from as to convert to")
        return self._host(x, [to, frm], lambda d, lengths: self.run_coded(d[0], lengths, d[1], d[2], nd, [len(r) for r in to], d[0],
                                                                         skip_energy))
