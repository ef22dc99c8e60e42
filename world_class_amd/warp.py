"""Python mirror of include/world_class_warp.h: signals resampled along positions read on the device, on a vresample.VResampler and
its table, and the map rule that turns a frame-level time map into such positions.  A position is a Python int (or an int64):
pos = q 2^32 + f."""
import ctypes as C

import numpy as np

from . import DeviceArray, _check, _ints, _opt  # noqa: F401  (_ints: for raw calls through _L(), as the tests make them)
from ._binding import IN_FORMATS, OUT_FORMATS, _binder, _count
from .resample import _Batch
from .vresample import _step, _u64

_ip = C.POINTER(C.c_int)
_vp = C.c_void_p
_dp = C.POINTER(C.c_double)
_llp = C.POINTER(C.c_longlong)

WARP_SIGNATURES = {
    "wc_warp_tiling": (C.c_int, [_u64, _u64, C.c_int, C.c_double, C.c_int, C.c_int, _ip, _ip, _ip, _ip]),
    "wc_warp_map_out_length": (C.c_longlong, [C.c_int, C.c_double]),
    "wc_warp_map_positions": (C.c_int, [_dp, C.c_int, C.c_double, C.c_double, C.c_longlong, _llp]),
    "wc_warp_device": (C.c_int, [_vp, C.c_int, _vp, C.c_int, _ip, _vp, _ip, _vp, C.c_int]),
    "wc_warp_map_positions_device": (C.c_int, [_vp, C.c_int, _vp, _ip, C.c_double, C.c_double, _ip, _vp]),
}

NO_POSITION = -(1 << 63)  # WC_WARP_NO_POSITION: before every signal

_L = _binder(WARP_SIGNATURES)


def tiling(step_min, step_max, zeros=0, rolloff=0.0, phase_bits=0, degree=0):
    """(tile_outputs, span_max, segment_min, plain_block): vresample.tiling's cut, and the input samples a near tile may span -- a
    tile whose live outputs reach over more reads its inputs from global memory"""
    v = [C.c_int() for _ in range(4)]
    _check(_L().wc_warp_tiling(_step(step_min), _step(step_max), int(zeros), float(rolloff), int(phase_bits), int(degree),
                               *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def map_out_length(map_length, out_per_entry):
    """the outputs up to a map's last entry: floor((map_length - 1) out_per_entry) + 1"""
    return _count(_L().wc_warp_map_out_length(int(map_length), float(out_per_entry)))


def map_positions(time_map, out_per_entry, in_per_unit, n_out=None):
    """the map rule on the host: n_out positions (default: map_out_length) as an int64 array"""
    m = np.ascontiguousarray(time_map, dtype=np.float64).ravel()
    n = map_out_length(len(m), out_per_entry) if n_out is None else int(n_out)
    pos = np.empty(max(n, 0), dtype=np.int64)
    _check(_L().wc_warp_map_positions(m.ctypes.data_as(_dp), len(m), float(out_per_entry), float(in_per_unit), n, pos.ctypes.data_as(_llp)))
    return pos


def map_positions_device(resampler, d_map, map_lengths, out_per_entry, in_per_unit, out_lengths, d_pos):
    """the map rule on the device: maps packed by map_lengths (float64), positions packed by out_lengths (int64); enqueue-only"""
    if len(out_lengths) != len(map_lengths):
        raise ValueError("one output length per map")
    _check(_L().wc_warp_map_positions_device(resampler._h, len(map_lengths), _opt(d_map), _ints(map_lengths), float(out_per_entry),
                                             float(in_per_unit), _ints(out_lengths), _opt(d_pos)))


def warp_device(resampler, d_x, x_lengths, d_pos, out_lengths, d_y, in_format="f64", out_format="f64"):
    """packed device arrays: utterance u's positions (int64) and outputs at the sum of the out_lengths before it; enqueue-only"""
    if len(out_lengths) != len(x_lengths):
        raise ValueError("one output length per utterance")
    _check(_L().wc_warp_device(resampler._h, len(x_lengths), _opt(d_x), IN_FORMATS[in_format][0], _ints(x_lengths), _opt(d_pos),
                               _ints(out_lengths), _opt(d_y), OUT_FORMATS[out_format][0]))


def warp(resampler, xs, positions, out_format="f64"):
    """a list of 1-D host arrays (all int16, all float32, or anything else as float64) and, for each, its outputs' positions -> the
    list of their warps"""
    fmt, xs = _Batch._pack(xs)
    ps = [np.ascontiguousarray(p, dtype=np.int64).ravel() for p in positions]
    if len(ps) != len(xs):
        raise ValueError("one array of positions per utterance")
    lengths, outs = [len(x) for x in xs], [len(p) for p in ps]
    d_pos = DeviceArray.from_host(np.concatenate(ps), dtype=np.int64)
    try:
        return _Batch._run(fmt, xs, outs, out_format, lambda d_x, d_y: warp_device(resampler, d_x, lengths, d_pos, outs, d_y, fmt, out_format))
    finally:
        d_pos.free()
