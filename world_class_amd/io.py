"""Python mirror of include/world_class_io.h: the reference's WAV / parameter-file functions (same names as reference
tools/audioio.hpp and tools/parameterio.hpp), device-side PCM conversion and parameter modification."""
import ctypes as C

import numpy as np

from . import WorldClassError, _c, _check, _opt, _ptr, _rows, lib
from ._binding import _binder

_dp = C.POINTER(C.c_double)
_i16p = C.POINTER(C.c_int16)
_rows_t = C.POINTER(_dp)

IO_SIGNATURES = {
    "wavwrite": (None, [_dp, C.c_int, C.c_int, C.c_int, C.c_char_p]),
    "GetAudioLength": (C.c_int, [C.c_char_p]),
    "wavread": (None, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), _dp]),
    "WriteF0": (None, [C.c_char_p, C.c_int, C.c_double, _dp, _dp, C.c_int]),
    "ReadF0": (C.c_int, [C.c_char_p, _dp, _dp]),
    "GetHeaderInformation": (C.c_double, [C.c_char_p, C.c_char_p]),
    "WriteSpectralEnvelope": (None, [C.c_char_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, _rows_t]),
    "ReadSpectralEnvelope": (C.c_int, [C.c_char_p, _rows_t]),
    "WriteAperiodicity": (None, [C.c_char_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, _rows_t]),
    "ReadAperiodicity": (C.c_int, [C.c_char_p, _rows_t]),
    "wc_wavread_pcm16": (C.c_int, [C.c_char_p, C.POINTER(C.c_int), _i16p, C.c_int]),
    "wc_pcm16_to_double_device": (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p]),
    "wc_float_to_double_device": (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p]),
    "wc_double_to_pcm16_device": (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p]),
    "wc_modify_parameters_device": (C.c_int, [C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_double, C.c_double]),
    "wc_modify_parameters_frames_device": (C.c_int, [C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "wc_retime_parameters_device": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int),
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "wc_morph_parameters_device": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int),
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)] + [C.c_void_p] * 9),
    "wc_align_features_device": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_int, C.c_int, C.c_int,
                                           C.c_int] + [C.c_void_p] * 5),
    "wc_align_features_ex_device": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_int, C.c_int, C.c_int,
                                              C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 8),
}

ALIGN_OPEN_BEGIN, ALIGN_OPEN_END = 1, 2  # WC_ALIGN_OPEN_BEGIN, WC_ALIGN_OPEN_END

_io = _binder(IO_SIGNATURES)


def _path(p):
    return str(p).encode()


def wavwrite(x, fs, filename, nbit=16):
    x = _c(x)
    _io().wavwrite(x.ctypes.data_as(_dp), len(x), int(fs), int(nbit), _path(filename))


def audio_length(filename):
    return _io().GetAudioLength(_path(filename))


def wavread(filename):
    """(x, fs, nbit) like the reference's wavread; raises if the reference would have rejected the file."""
    n = audio_length(filename)
    if n <= 0:
        raise WorldClassError(f"cannot read {filename} (GetAudioLength = {n})")
    x = np.empty(n)
    fs, nbit = C.c_int(0), C.c_int(0)
    _io().wavread(_path(filename), C.byref(fs), C.byref(nbit), x.ctypes.data_as(_dp))
    return x, fs.value, nbit.value


def wavread_pcm16(filename):
    """(int16 samples as stored, fs) -- upload these and expand on the device with pcm16_to_double_device."""
    n = audio_length(filename)
    if n <= 0:
        raise WorldClassError(f"cannot read {filename} (GetAudioLength = {n})")
    pcm = np.empty(n, dtype=np.int16)
    fs = C.c_int(0)
    got = _io().wc_wavread_pcm16(_path(filename), C.byref(fs), pcm.ctypes.data_as(_i16p), n)
    if got < 0:
        raise WorldClassError(f"{filename} is not 16-bit PCM")
    return pcm[:got], fs.value


def header_information(filename, parameter):
    return _io().GetHeaderInformation(_path(filename), parameter.encode())


def write_f0(filename, temporal_positions, f0, frame_period, text=False):
    t, f = _c(temporal_positions), _c(f0)
    _io().WriteF0(_path(filename), len(f), float(frame_period), t.ctypes.data_as(_dp), f.ctypes.data_as(_dp), 1 if text else 0)


def read_f0(filename):
    n = int(header_information(filename, "NOF "))
    t, f = np.empty(n), np.empty(n)
    if _io().ReadF0(_path(filename), t.ctypes.data_as(_dp), f.ctypes.data_as(_dp)) != 1:
        raise WorldClassError(f"cannot read {filename}")
    return t, f


def _write_matrix(fn, filename, mat, fs, frame_period, fft_size, number_of_dimensions):
    mat = np.ascontiguousarray(mat, dtype=np.float64)
    fn(_path(filename), int(fs), mat.shape[0], float(frame_period), int(fft_size), int(number_of_dimensions), _rows(mat))


def _read_matrix(fn, filename):
    n = int(header_information(filename, "NOF "))
    fft_size = int(header_information(filename, "FFT "))
    nd = int(header_information(filename, "NOD ")) or fft_size // 2 + 1
    mat = np.empty((n, nd))
    if fn(_path(filename), _rows(mat)) != 1:
        raise WorldClassError(f"cannot read {filename}")
    return mat


def write_spectral_envelope(filename, sp, fs, frame_period, fft_size, number_of_dimensions=0):
    _write_matrix(_io().WriteSpectralEnvelope, filename, sp, fs, frame_period, fft_size, number_of_dimensions)


def read_spectral_envelope(filename):
    return _read_matrix(_io().ReadSpectralEnvelope, filename)


def write_aperiodicity(filename, ap, fs, frame_period, fft_size, number_of_dimensions=0):
    _write_matrix(_io().WriteAperiodicity, filename, ap, fs, frame_period, fft_size, number_of_dimensions)


def read_aperiodicity(filename):
    return _read_matrix(_io().ReadAperiodicity, filename)


def pcm16_to_double_device(d_pcm, n, d_x):
    _check(_io().wc_pcm16_to_double_device(_ptr(d_pcm), int(n), _ptr(d_x)))


def float_to_double_device(d_f, n, d_x):
    _check(_io().wc_float_to_double_device(_ptr(d_f), int(n), _ptr(d_x)))


def double_to_pcm16_device(d_y, n, d_pcm):
    _check(_io().wc_double_to_pcm16_device(_ptr(d_y), int(n), _ptr(d_pcm)))


def modify_parameters_device(fs, fft_size, n_frames, d_f0, d_sp, f0_scale=1.0, spectral_ratio=0.0):
    """reference test/test.cpp:201-243 on device-resident parameters (0 = leave the spectra alone)"""
    _check(_io().wc_modify_parameters_device(int(fs), int(fft_size), int(n_frames), _ptr(d_f0), _ptr(d_sp), float(f0_scale),
                                             float(spectral_ratio)))


def modify_parameters_frames_device(fs, fft_size, n_frames, d_f0, d_sp, d_f0_scale=None, d_spectral_ratio=None):
    """modify_parameters_device with an F0 scale and a spectral ratio per frame (device arrays of n_frames doubles; None = leave
    it, as for d_f0 / d_sp).  Per frame a ratio of 0 leaves the row, an invalid one (negative, NaN, infinite, below
    2 / fft_size) makes it NaN."""
    _check(_io().wc_modify_parameters_frames_device(int(fs), int(fft_size), int(n_frames), _opt(d_f0), _opt(d_sp), _opt(d_f0_scale),
                                                    _opt(d_spectral_ratio)))


def retime_parameters_device(fs, fft_size, in_lengths, d_f0_in, d_sp_in, d_ap_in, out_lengths, d_position, d_f0_scale=None,
                             d_spectral_ratio=None, d_f0_out=None, d_sp_out=None, d_ap_out=None):
    """wc_retime_parameters_device: the frames of a packed batch resampled along a position per output frame (in source frames,
    from the utterance's first frame; the end frames are held, a position that is not finite makes its own frame NaN), then F0
    scaled and sp stretched per OUTPUT frame as by modify_parameters_frames_device.  in_lengths / out_lengths: frames per
    utterance (host lists); each of the pairs (d_f0_in, d_f0_out), (d_sp_in, d_sp_out), (d_ap_in, d_ap_out) may be None together."""
    from . import _ints
    if len(in_lengths) != len(out_lengths):
        raise ValueError("retime_parameters_device: in_lengths and out_lengths must have one entry per utterance each")
    _check(_io().wc_retime_parameters_device(int(fs), int(fft_size), len(in_lengths), _ints(in_lengths), _opt(d_f0_in), _opt(d_sp_in),
                                             _opt(d_ap_in), _ints(out_lengths), _opt(d_position), _opt(d_f0_scale), _opt(d_spectral_ratio),
                                             _opt(d_f0_out), _opt(d_sp_out), _opt(d_ap_out)))


def retime_parameters(f0, sp, ap, position, fs, fft_size, f0_scale=None, spectral_ratio=None):
    """one utterance, numpy in, numpy out: (f0, sp, ap) at the positions (see retime_parameters_device), through the device call"""
    from . import DeviceArray
    f0, sp, ap, position = _c(f0), _c(sp), _c(ap), _c(position)
    n, m, bins = len(f0), len(position), int(fft_size) // 2 + 1
    if sp.shape != (n, bins) or ap.shape != (n, bins) or position.ndim != 1:
        raise ValueError(f"retime_parameters: sp and ap must be ({n}, {bins}), position a vector")
    per_frame = [None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (m,))) for a in (f0_scale, spectral_ratio)]
    held = [DeviceArray.from_host(a) for a in (f0, sp, ap, position)] + [None if a is None else DeviceArray.from_host(a) for a in per_frame]
    outs = [DeviceArray(m), DeviceArray(m * bins), DeviceArray(m * bins)]
    try:
        retime_parameters_device(fs, fft_size, [n], held[0], held[1], held[2], [m], held[3], held[4], held[5], *outs)
        _check(lib().wc_synchronize())
        return outs[0].to_host()[:m], outs[1].to_host()[:m * bins].reshape(m, bins), outs[2].to_host()[:m * bins].reshape(m, bins)
    finally:
        for a in held + outs:
            if a is not None:
                a.free()


def morph_parameters_device(fs, fft_size, a_lengths, d_f0_a, d_sp_a, d_ap_a, b_lengths, d_f0_b, d_sp_b, d_ap_b, out_lengths, d_position_a,
                            d_position_b, d_weight, d_f0_weight=None, d_ratio_a=None, d_ratio_b=None, d_f0_out=None, d_sp_out=None, d_ap_out=None):
    """wc_morph_parameters_device: every output frame of a packed batch of pairs is the blend of A's frame at d_position_a and B's
    frame at d_position_b (both as retime_parameters_device forms them) with d_weight -- log-F0 (d_f0_weight, None = d_weight),
    log-envelope (each source's axis stretched by d_ratio_a / d_ratio_b first, None or 0 = as it is) and aperiodicity (linear);
    weight 0 is A, 1 is B.  a_lengths / b_lengths / out_lengths: frames per pair (host lists); each of the triples (d_f0_a, d_f0_b,
    d_f0_out), (d_sp_a, d_sp_b, d_sp_out), (d_ap_a, d_ap_b, d_ap_out) may be None together."""
    from . import _ints
    if not (len(a_lengths) == len(b_lengths) == len(out_lengths)):
        raise ValueError("morph_parameters_device: a_lengths, b_lengths and out_lengths must have one entry per pair each")
    _check(_io().wc_morph_parameters_device(int(fs), int(fft_size), len(a_lengths), _ints(a_lengths), _opt(d_f0_a), _opt(d_sp_a), _opt(d_ap_a),
                                            _ints(b_lengths), _opt(d_f0_b), _opt(d_sp_b), _opt(d_ap_b), _ints(out_lengths), _opt(d_position_a),
                                            _opt(d_position_b), _opt(d_weight), _opt(d_f0_weight), _opt(d_ratio_a), _opt(d_ratio_b),
                                            _opt(d_f0_out), _opt(d_sp_out), _opt(d_ap_out)))


def morph_parameters(a, b, position_a, position_b, weight, fs, fft_size, f0_weight=None, ratio_a=None, ratio_b=None):
    """one pair, numpy in, numpy out: a and b are (f0, sp, ap); (f0, sp, ap) of the blend at the positions (see
    morph_parameters_device), through the device call.  weight, f0_weight and the ratios: one value per output frame, or a scalar"""
    from . import DeviceArray
    bins = int(fft_size) // 2 + 1
    srcs = []
    for name, (f0, sp, ap) in (("a", a), ("b", b)):
        f0, sp, ap = _c(f0), _c(sp), _c(ap)
        if f0.ndim != 1 or sp.shape != (len(f0), bins) or ap.shape != (len(f0), bins):
            raise ValueError(f"morph_parameters: {name} must be (f0, sp, ap) with sp and ap ({len(f0)}, {bins})")
        srcs.append((f0, sp, ap))
    position_a, position_b = _c(position_a), _c(position_b)
    if position_a.ndim != 1 or position_a.shape != position_b.shape:
        raise ValueError("morph_parameters: position_a and position_b must be vectors of one length")
    m = len(position_a)
    per_frame = [None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (m,)))
                 for v in (weight, f0_weight, ratio_a, ratio_b)]
    if per_frame[0] is None:
        raise ValueError("morph_parameters: weight is required")
    held, outs = [], []
    try:
        for v in srcs[0] + srcs[1] + (position_a, position_b) + tuple(per_frame):
            held.append(None if v is None else DeviceArray.from_host(v))
        for n in (m, m * bins, m * bins):
            outs.append(DeviceArray(n))
        morph_parameters_device(fs, fft_size, [len(srcs[0][0])], held[0], held[1], held[2], [len(srcs[1][0])], held[3], held[4], held[5], [m],
                                held[6], held[7], held[8], held[9], held[10], held[11], *outs)
        _check(lib().wc_synchronize())
        return outs[0].to_host()[:m], outs[1].to_host()[:m * bins].reshape(m, bins), outs[2].to_host()[:m * bins].reshape(m, bins)
    finally:
        for v in held + outs:
            if v is not None:
                v.free()


def align_features_device(a_lengths, d_feat_a, b_lengths, d_feat_b, dims, dim_begin, dim_end, band, d_cost, d_path_length, d_path=None,
                          d_b_on_a=None, d_a_on_b=None):
    """wc_align_features_device: dynamic time warping of a packed batch of pairs of feature rows (dims doubles each, coefficients
    dim_begin <= c < dim_end compared, band 0 = every cell, else a Sakoe-Chiba band).  a_lengths / b_lengths: rows per pair (host
    lists).  d_cost: one double per pair, d_path_length: one int32 per pair (0 where the total cost is not finite), d_path: (i, j)
    int32 pairs, a_length + b_length - 1 entries per pair; d_b_on_a / d_a_on_b: B's position per frame of A and the reverse -- the
    d_position of retime_parameters_device / morph_parameters_device.  The last three may be None."""
    from . import _ints
    if len(a_lengths) != len(b_lengths):
        raise ValueError("align_features_device: a_lengths and b_lengths must have one entry per pair each")
    _check(_io().wc_align_features_device(len(a_lengths), _ints(a_lengths), _opt(d_feat_a), _ints(b_lengths), _opt(d_feat_b), int(dims),
                                          int(dim_begin), int(dim_end), int(band), _opt(d_cost), _opt(d_path_length), _opt(d_path),
                                          _opt(d_b_on_a), _opt(d_a_on_b)))


def align_features(feat_a, feat_b, dim_begin=1, dim_end=None, band=0):
    """one pair, numpy in, numpy out: feat_a (n, dims) and feat_b (m, dims) aligned through the device call (see
    align_features_device).  A dict of cost, path (K x 2 int array of (i, j); K = 0 where the cost is not finite), b_on_a (n) and
    a_on_b (m)."""
    from . import DeviceArray
    feat_a, feat_b = _c(feat_a), _c(feat_b)
    if feat_a.ndim != 2 or feat_b.ndim != 2 or feat_a.shape[1] != feat_b.shape[1]:
        raise ValueError("align_features: feat_a and feat_b must be (frames, dims) with the same dims")
    (n, dims), m = feat_a.shape, feat_b.shape[0]
    if dim_end is None:
        dim_end = dims
    held = [DeviceArray.from_host(feat_a), DeviceArray.from_host(feat_b)]
    outs = [DeviceArray(1), DeviceArray(1, np.int32), DeviceArray(2 * max(n + m - 1, 1), np.int32), DeviceArray(n), DeviceArray(m)]
    try:
        align_features_device([n], held[0], [m], held[1], dims, dim_begin, dim_end, band, *outs)
        _check(lib().wc_synchronize())
        k = int(outs[1].to_host()[0])
        return {"cost": float(outs[0].to_host()[0]), "path": outs[2].to_host()[:2 * k].reshape(k, 2).copy(), "b_on_a": outs[3].to_host()[:n],
                "a_on_b": outs[4].to_host()[:m]}
    finally:
        for a in held + outs:
            a.free()


def align_features_ex_device(a_lengths, d_feat_a, b_lengths, d_feat_b, dims, dim_begin, dim_end, band, step_pattern, flags, d_cost, d_path_length,
                             d_path=None, d_b_on_a=None, d_a_on_b=None, d_span=None, d_timeline_a=None, d_timeline_b=None):
    """wc_align_features_ex_device: align_features_device under the wider rule.  step_pattern 0: the steps of align_features_device; 1:
    the slope stays between 1/2 and 2.  flags: ALIGN_OPEN_BEGIN | ALIGN_OPEN_END, the path may start at any (0, j) / end at any
    (n - 1, j) (band must be 0 then).  d_a_on_b holds 0 before and n - 1 behind the path's columns.  d_span: two int32 per pair, the
    columns of the path's first and last cell ((-1, -1) where the total cost is not finite); d_timeline_a / d_timeline_b: doubles
    packed like d_path, i_k and j_k of the path's K cells -- d_position_a / d_position_b of morph_parameters_device with out_length
    = K, which the caller reads back from d_path_length.  The last six may be None."""
    from . import _ints
    if len(a_lengths) != len(b_lengths):
        raise ValueError("align_features_ex_device: a_lengths and b_lengths must have one entry per pair each")
    _check(_io().wc_align_features_ex_device(len(a_lengths), _ints(a_lengths), _opt(d_feat_a), _ints(b_lengths), _opt(d_feat_b), int(dims),
                                             int(dim_begin), int(dim_end), int(band), int(step_pattern), int(flags), _opt(d_cost),
                                             _opt(d_path_length), _opt(d_path), _opt(d_b_on_a), _opt(d_a_on_b), _opt(d_span),
                                             _opt(d_timeline_a), _opt(d_timeline_b)))


def align_features_ex(feat_a, feat_b, dim_begin=1, dim_end=None, band=0, step_pattern=0, open_begin=False, open_end=False):
    """one pair, numpy in, numpy out, through align_features_ex_device: the dict of align_features plus span (two ints, (-1, -1)
    where the cost is not finite), timeline_a and timeline_b (K doubles each)."""
    from . import DeviceArray
    feat_a, feat_b = _c(feat_a), _c(feat_b)
    if feat_a.ndim != 2 or feat_b.ndim != 2 or feat_a.shape[1] != feat_b.shape[1]:
        raise ValueError("align_features_ex: feat_a and feat_b must be (frames, dims) with the same dims")
    (n, dims), m = feat_a.shape, feat_b.shape[0]
    if dim_end is None:
        dim_end = dims
    flags = (ALIGN_OPEN_BEGIN if open_begin else 0) | (ALIGN_OPEN_END if open_end else 0)
    entries = max(n + m - 1, 1)
    held = [DeviceArray.from_host(feat_a), DeviceArray.from_host(feat_b)]
    outs = [DeviceArray(1), DeviceArray(1, np.int32), DeviceArray(2 * entries, np.int32), DeviceArray(n), DeviceArray(m), DeviceArray(2, np.int32),
            DeviceArray(entries), DeviceArray(entries)]
    try:
        align_features_ex_device([n], held[0], [m], held[1], dims, dim_begin, dim_end, band, step_pattern, flags, *outs)
        _check(lib().wc_synchronize())
        k = int(outs[1].to_host()[0])
        return {"cost": float(outs[0].to_host()[0]), "path": outs[2].to_host()[:2 * k].reshape(k, 2).copy(), "b_on_a": outs[3].to_host()[:n],
                "a_on_b": outs[4].to_host()[:m], "span": outs[5].to_host()[:2].copy(), "timeline_a": outs[6].to_host()[:k].copy(),
                "timeline_b": outs[7].to_host()[:k].copy()}
    finally:
        for a in held + outs:
            a.free()


def time_map(n_frames, speed):
    """positions for retime_parameters*: `speed` source frames per output frame.  A positive scalar: arange(floor((n_frames - 1) /
    speed) + 1) * speed (the whole utterance at that speed); an array of one speed per output frame: pos[0] = 0, pos[k] =
    pos[k - 1] + speed[k - 1].  Host only."""
    if np.ndim(speed) == 0:
        speed = float(speed)
        if not (speed > 0.0 and np.isfinite(speed)) or n_frames < 1:
            raise ValueError("time_map: speed must be a positive finite number and n_frames at least 1")
        return np.arange(int(np.floor((n_frames - 1) / speed)) + 1, dtype=np.float64) * speed
    speed = np.asarray(speed, dtype=np.float64).ravel()
    pos = np.zeros(len(speed))
    np.cumsum(speed[:-1], out=pos[1:])
    return pos
