"""Python mirror of include/world_class_resample.h: sample-rate conversion on the device, whole batches and streams."""
import ctypes as C

import numpy as np

from . import DeviceArray, _check, _ints, _opt
# (the definitions live in _binding; the names stay importable from here, where other modules, tests and tools take them)
from ._binding import IN_FORMATS, OUT_FORMATS, _binder, _count, _Handle, _lag_emitted, _LagStream, pack_rows, split_rows, uploaded  # noqa: F401

_ip = C.POINTER(C.c_int)
_vp = C.c_void_p
_plan = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double]  # fs_in, fs_out, zeros, rolloff, beta

RESAMPLE_SIGNATURES = {
    "wc_resample_plan": (C.c_int, _plan + [_ip, _ip, _ip]),
    "wc_resample_filter": (C.c_int, _plan + [C.POINTER(C.c_double), C.c_longlong]),
    "wc_resample_out_length": (C.c_longlong, [C.c_int, C.c_int, C.c_longlong]),
    "wc_resample_committed": (C.c_longlong, [C.c_int, C.c_int, C.c_int, C.c_double, C.c_longlong, C.c_int]),
    "wc_resample_tiling": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_double, _ip, _ip, _ip]),
    "wc_resampler_create": (_vp, _plan),
    "wc_resampler_destroy": (None, [_vp]),
    "wc_resample_device": (C.c_int, [_vp, C.c_int, _vp, C.c_int, _ip, _vp, C.c_int]),
    "wc_resample_stream_create": (_vp, _plan + [C.c_int, C.c_int]),
    "wc_resample_stream_destroy": (None, [_vp]),
    "wc_resample_stream_max_out_per_push": (C.c_int, [_vp]),
    "wc_resample_stream_reset": (C.c_int, [_vp, C.c_int]),
    "wc_resample_stream_push_device": (C.c_int, [_vp, _vp, C.c_int, _ip, _ip, _vp, C.c_int, _ip]),
    "wc_resample_stream_samples_received": (C.c_longlong, [_vp, C.c_int]),
    "wc_resample_stream_samples_committed": (C.c_longlong, [_vp, C.c_int]),
}

WAVE = 64  # outputs of one phase that a wavefront of the phase mapping takes

_L = _binder(RESAMPLE_SIGNATURES)


def plan(fs_in, fs_out, zeros=0, rolloff=0.0, beta=0.0):
    """(L, M, K) of the rule: up, down and the half width of a table row in input samples"""
    v = [C.c_int() for _ in range(3)]
    _check(_L().wc_resample_plan(int(fs_in), int(fs_out), int(zeros), float(rolloff), float(beta), *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def filter_taps(fs_in, fs_out, zeros=0, rolloff=0.0, beta=0.0):
    """the table G as an [L, 2K+1] array"""
    up, _, k = plan(fs_in, fs_out, zeros, rolloff, beta)
    g = np.empty((up, 2 * k + 1))
    _check(_L().wc_resample_filter(int(fs_in), int(fs_out), int(zeros), float(rolloff), float(beta),
                                   g.ctypes.data_as(C.POINTER(C.c_double)), g.size))
    return g


def out_length(fs_in, fs_out, n):
    return _count(_L().wc_resample_out_length(int(fs_in), int(fs_out), int(n)))


def committed(fs_in, fs_out, samples_in, flushed=False, zeros=0, rolloff=0.0):
    """outputs a stream has committed after samples_in samples (flushed: after its flush)"""
    return _count(_L().wc_resample_committed(int(fs_in), int(fs_out), int(zeros), float(rolloff), int(samples_in), 1 if flushed else 0))


def tiling(fs_in, fs_out, zeros=0, rolloff=0.0):
    """(tile_outputs, phase_min, plain_block): a signal or push of at least phase_min outputs is cut into tiles of tile_outputs outputs
    whose wavefronts take WAVE outputs of one phase each (tile_outputs 0: never); a shorter one goes in blocks of plain_block"""
    v = [C.c_int() for _ in range(3)]
    _check(_L().wc_resample_tiling(int(fs_in), int(fs_out), int(zeros), float(rolloff), *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def _in_format(arrays):
    """the in_format name of host arrays: int16 and float32 go up as they are, everything else as float64"""
    kinds = {np.asarray(a).dtype for a in arrays if a is not None}
    if kinds == {np.dtype(np.int16)}:
        return "i16"
    if kinds == {np.dtype(np.float32)}:
        return "f32"
    return "f64"


class _Batch(_Handle):
    """the batch handle of either converter: the packing of host arrays around its run_device"""
    _lib = staticmethod(_L)
    _sym = "wc_resample"
    _kind = "r"

    def _device(self, d_x, x_lengths, extra, d_y, in_format, out_format):
        _check(self._fn("_device")(self._h, len(x_lengths), _opt(d_x), IN_FORMATS[in_format][0], _ints(x_lengths), *extra, _opt(d_y),
                                   OUT_FORMATS[out_format][0]))

    @staticmethod
    def _pack(xs):
        """(the in_format name, the signals as contiguous arrays of its type)"""
        fmt = _in_format(xs)
        xs = [np.ascontiguousarray(x, dtype=IN_FORMATS[fmt][1]).ravel() for x in xs]
        if not xs or any(len(x) == 0 for x in xs):
            raise ValueError("at least one signal, none of them empty")
        return fmt, xs

    @staticmethod
    def _run(fmt, xs, outs, out_format, run_device):
        """the packed signals up, run_device(d_x, d_y), the outputs of lengths outs down"""
        d_y = DeviceArray(sum(outs), dtype=OUT_FORMATS[out_format][1])
        try:
            with uploaded(np.concatenate(xs), dtype=IN_FORMATS[fmt][1]) as (d_x,):
                run_device(d_x, d_y)
                y = d_y.to_host()  # (the copy waits for the stream)
        finally:
            d_y.free()
        return split_rows(y, outs)


class Resampler(_Batch):
    """whole signals from fs_in to fs_out: the rule of the header on the device"""

    def __init__(self, fs_in, fs_out, zeros=0, rolloff=0.0, beta=0.0):
        self.fs_in, self.fs_out = int(fs_in), int(fs_out)
        self._create(self.fs_in, self.fs_out, int(zeros), float(rolloff), float(beta))

    def out_length(self, n):
        return out_length(self.fs_in, self.fs_out, n)

    def run_device(self, d_x, x_lengths, d_y, in_format="f64", out_format="f64"):
        """packed device arrays in and out (utterance u's output at the sum of the out_length before it); enqueue-only"""
        self._device(d_x, x_lengths, (), d_y, in_format, out_format)

    def run(self, xs, out_format="f64"):
        """a list of 1-D host arrays (all int16, all float32, or anything else as float64) -> the list of their conversions"""
        fmt, xs = self._pack(xs)
        lengths = [len(x) for x in xs]
        return self._run(fmt, xs, [self.out_length(n) for n in lengths], out_format,
                         lambda d_x, d_y: self.run_device(d_x, lengths, d_y, fmt, out_format))


class _Stream(_Handle):
    """the stream handle of either converter: everything but its create and what only one of them has"""
    _lib = staticmethod(_L)
    _sym = "wc_resample"
    _kind = "_stream"

    def _create(self, n_streams, max_samples, *plan):
        self.n_streams, self.max_samples = int(n_streams), int(max_samples)
        self._out = {}  # the output arrays of push, by format: allocated on first use
        super()._create(*plan, self.n_streams, self.max_samples)

    @property
    def max_out_per_push(self):
        return int(self._fn("_stream_max_out_per_push")(self._h))

    def reset(self, stream):
        _check(self._fn("_stream_reset")(self._h, int(stream)))

    def samples_received(self, stream):
        return int(self._fn("_stream_samples_received")(self._h, int(stream)))

    def samples_committed(self, stream):
        return int(self._fn("_stream_samples_committed")(self._h, int(stream)))

    def push_device(self, n_new, d_chunk, flush, d_y, in_format="f64", out_format="f64"):
        """device pointers in and out (packed by n_new and by the counts that come back); enqueue-only.  Returns samples_out"""
        if len(n_new) != self.n_streams or (flush is not None and len(flush) != self.n_streams):
            raise ValueError("one entry per stream")
        got = (C.c_int * self.n_streams)()
        _check(self._fn("_stream_push_device")(self._h, _opt(d_chunk), IN_FORMATS[in_format][0], _ints(n_new),
                                               None if flush is None else _ints([1 if f else 0 for f in flush]), _opt(d_y),
                                               OUT_FORMATS[out_format][0], got))
        return list(got)

    def push(self, chunks, flush=None, out_format="f64"):
        """chunks[u]: the new samples of stream u (None: none; all int16, all float32, or anything else as float64); flush[u]: the
        stream ends here.  Returns the committed outputs per stream"""
        if len(chunks) != self.n_streams:
            raise ValueError("one entry per stream")
        fmt = _in_format(chunks)
        idt, odt = IN_FORMATS[fmt][1], OUT_FORMATS[out_format][1]
        counts, flat = pack_rows([None if c is None else np.ravel(c) for c in chunks], 1, dtype=idt, placeholder=False)  # (nothing pushed: NULL)
        if out_format not in self._out:
            self._out[out_format] = DeviceArray(self.n_streams * self.max_out_per_push, dtype=odt)
        d_y = self._out[out_format]
        with uploaded(flat, dtype=idt) as (d,):
            got = self.push_device(counts, d, flush, d_y, fmt, out_format)
            y = d_y.to_host() if sum(got) else np.zeros(0, dtype=odt)
        return split_rows(y, got)

    def close(self):
        super().close()
        for d in self._out.values():
            d.free()
        self._out = {}


class ResampleStream(_Stream):
    """n_streams concurrent signals from fs_in to fs_out, pushed piece by piece: the concatenated outputs of a stream are bit for
    bit Resampler.run of its whole signal.  Output n is committed once its last tap has arrived (K samples of latency); the flush
    adds the zero tail."""

    def __init__(self, fs_in, fs_out, n_streams, max_samples, zeros=0, rolloff=0.0, beta=0.0):
        self.fs_in, self.fs_out = int(fs_in), int(fs_out)
        self._create(n_streams, max_samples, self.fs_in, self.fs_out, int(zeros), float(rolloff), float(beta))


