"""Python mirror of include/world_class_vresample.h: variable-ratio sample-rate conversion on the device, whole batches with a step
per utterance and streams whose steps move between pushes.  A step is a Python int: input samples per output in units of 2^-32."""
import ctypes as C

import numpy as np

from . import _check, _ints  # noqa: F401  (_ints: for raw calls through _L(), as the tests make them)
from ._binding import IN_FORMATS, OUT_FORMATS, _binder, _count  # noqa: F401  (the formats are the rational converter's too)
from .resample import WAVE, _Batch, _Stream  # noqa: F401

_ip = C.POINTER(C.c_int)
_vp = C.c_void_p
_u64 = C.c_ulonglong
_plan = [_u64, _u64, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int]  # step_min, step_max, zeros, rolloff, beta, phase_bits, degree

VRESAMPLE_SIGNATURES = {
    "wc_vresample_plan": (C.c_int, _plan + [_ip, _ip, _ip, C.POINTER(C.c_double)]),
    "wc_vresample_filter": (C.c_int, _plan + [C.POINTER(C.c_double), C.c_longlong]),
    "wc_vresample_out_length": (C.c_longlong, [_u64, C.c_longlong]),
    "wc_vresample_committed": (C.c_longlong, [C.c_longlong, C.c_uint, _u64, C.c_int, C.c_longlong, C.c_int]),
    "wc_vresample_tiling": (C.c_int, [_u64, _u64, C.c_int, C.c_double, C.c_int, C.c_int, _ip, _ip, _ip]),
    "wc_vresampler_create": (_vp, _plan),
    "wc_vresampler_destroy": (None, [_vp]),
    "wc_vresample_device": (C.c_int, [_vp, C.c_int, _vp, C.c_int, _ip, C.POINTER(_u64), _vp, C.c_int]),
    "wc_vresample_stream_create": (_vp, _plan + [C.c_int, C.c_int]),
    "wc_vresample_stream_destroy": (None, [_vp]),
    "wc_vresample_stream_max_out_per_push": (C.c_int, [_vp]),
    "wc_vresample_stream_reset": (C.c_int, [_vp, C.c_int]),
    "wc_vresample_stream_set_step": (C.c_int, [_vp, C.c_int, _u64]),
    "wc_vresample_stream_push_device": (C.c_int, [_vp, _vp, C.c_int, _ip, _ip, _vp, C.c_int, _ip]),
    "wc_vresample_stream_samples_received": (C.c_longlong, [_vp, C.c_int]),
    "wc_vresample_stream_samples_committed": (C.c_longlong, [_vp, C.c_int]),
}

ONE = 1 << 32  # the step of ratio 1
STEP_LO, STEP_HI = 1 << 28, 1 << 36

_L = _binder(VRESAMPLE_SIGNATURES)


def _step(step):
    """a step as the C call takes it: anything outside 64 unsigned bits becomes 0, which every call refuses"""
    step = int(step)
    return step if 0 <= step < 1 << 64 else 0


def step_of(ratio):
    """the step of the ratio fs_out / fs_in: round(2^32 / ratio) as a Python int"""
    return int(round(4294967296.0 / float(ratio)))


def plan(step_min, step_max, zeros=0, rolloff=0.0, beta=0.0, phase_bits=0, degree=0):
    """(K, P, D, s) of the rule: the half width of a tap row in input samples, the segments, the degree and the cut-off"""
    v = [C.c_int() for _ in range(3)]
    s = C.c_double()
    _check(_L().wc_vresample_plan(_step(step_min), _step(step_max), int(zeros), float(rolloff), float(beta), int(phase_bits), int(degree),
                                  *[C.byref(x) for x in v], C.byref(s)))
    return tuple(x.value for x in v) + (s.value,)


def filter_table(step_min, step_max, zeros=0, rolloff=0.0, beta=0.0, phase_bits=0, degree=0):
    """the table C as a [P, 2K+1, D+1] array"""
    k, p, d, _ = plan(step_min, step_max, zeros, rolloff, beta, phase_bits, degree)
    c = np.empty((p, 2 * k + 1, d + 1))
    _check(_L().wc_vresample_filter(_step(step_min), _step(step_max), int(zeros), float(rolloff), float(beta), int(phase_bits), int(degree),
                                    c.ctypes.data_as(C.POINTER(C.c_double)), c.size))
    return c


def out_length(step, n):
    return _count(_L().wc_vresample_out_length(_step(step), int(n)))


def committed(q, f, step, half_width, samples_in, flushed=False):
    """outputs a stream commits out of the position (q, f) with this step once it has samples_in samples (flushed: after its flush)"""
    return _count(_L().wc_vresample_committed(int(q), int(f), _step(step), int(half_width), int(samples_in), 1 if flushed else 0))


def tiling(step_min, step_max, zeros=0, rolloff=0.0, phase_bits=0, degree=0):
    """(tile_outputs, segment_min, plain_block): a signal or push of at least segment_min outputs is cut into tiles of tile_outputs
    outputs, sorted by segment so that a wavefront takes WAVE outputs of one segment (tile_outputs 0: never); a shorter one goes in
    blocks of plain_block"""
    v = [C.c_int() for _ in range(3)]
    _check(_L().wc_vresample_tiling(_step(step_min), _step(step_max), int(zeros), float(rolloff), int(phase_bits), int(degree),
                                    *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


class VResampler(_Batch):
    """whole signals at a step each, anywhere in [step_min, step_max]: the rule of the header on the device"""
    _lib = staticmethod(_L)
    _sym = "wc_vresample"

    def __init__(self, step_min, step_max, zeros=0, rolloff=0.0, beta=0.0, phase_bits=0, degree=0):
        self.step_min, self.step_max = int(step_min), int(step_max)
        self._create(_step(step_min), _step(step_max), int(zeros), float(rolloff), float(beta), int(phase_bits), int(degree))

    def run_device(self, d_x, x_lengths, steps, d_y, in_format="f64", out_format="f64"):
        """packed device arrays in and out (utterance u's output at the sum of the out_length before it); enqueue-only"""
        if len(steps) != len(x_lengths):
            raise ValueError("one step per utterance")
        self._device(d_x, x_lengths, ((_u64 * len(steps))(*[_step(s) for s in steps]),), d_y, in_format, out_format)

    def run(self, xs, steps, out_format="f64"):
        """a list of 1-D host arrays (all int16, all float32, or anything else as float64) and their steps (one int: the same for
        all) -> the list of their conversions"""
        fmt, xs = self._pack(xs)
        steps = [int(steps)] * len(xs) if np.isscalar(steps) else [int(s) for s in steps]
        if len(steps) != len(xs):
            raise ValueError("one step per utterance")
        lengths = [len(x) for x in xs]
        return self._run(fmt, xs, [out_length(s, n) for s, n in zip(steps, lengths)], out_format,
                         lambda d_x, d_y: self.run_device(d_x, lengths, steps, d_y, fmt, out_format))


class VResampleStream(_Stream):
    """n_streams concurrent signals, pushed piece by piece, each at a step of its own that set_step moves between pushes (step_max
    after create).  With a constant step the concatenated outputs of a stream are bit for bit VResampler.run of its whole signal.  An
    output is committed once its last tap has arrived (K samples of latency); the flush adds the zero tail."""
    _lib = staticmethod(_L)
    _sym = "wc_vresample"

    def __init__(self, step_min, step_max, n_streams, max_samples, zeros=0, rolloff=0.0, beta=0.0, phase_bits=0, degree=0):
        self.step_min, self.step_max = int(step_min), int(step_max)
        self._create(n_streams, max_samples, _step(step_min), _step(step_max), int(zeros), float(rolloff), float(beta), int(phase_bits),
                     int(degree))

    def set_step(self, stream, step):
        """from the stream's next uncommitted output on, which keeps its position"""
        _check(self._fn("_stream_set_step")(self._h, int(stream), _step(step)))


