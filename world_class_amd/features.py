"""Python mirror of include/world_class_features.h: model features on the device -- continuous log-F0, the voiced/unvoiced flag and
deltas packed into one row per frame, maximum-likelihood parameter generation (MLPG) over predicted statics and deltas, and the way
back to the arrays coded Synthesis takes.  Row formats are "f64" and "f32"."""
import ctypes as C

import numpy as np

from . import DeviceArray, _check, _ints, _opt  # noqa: F401  (_ints: for raw calls through _L(), as the tests make them)
from ._binding import _binder

_ip = C.POINTER(C.c_int)
_vp = C.c_void_p

FEATURES_SIGNATURES = {
    "wc_model_feature_width": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "wc_pack_model_features_device": (C.c_int, [C.c_int, _ip, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_double, C.c_int, _vp]),
    "wc_mlpg_device": (C.c_int, [C.c_int, _ip, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp]),
    "wc_unpack_model_features_device": (C.c_int, [C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_double, _vp, _vp, _vp]),
}

FORMATS = {"f64": (0, np.float64), "f32": (1, np.float32)}  # WC_FEAT_F64, WC_FEAT_F32

_L = _binder(FEATURES_SIGNATURES)


def width(nd, n_ap, orders):
    """columns of a row: orders * (nd + 1 + n_ap) + 1"""
    w = int(_L().wc_model_feature_width(int(nd), int(n_ap), int(orders)))
    if w < 0:
        raise ValueError("nd >= 1, n_ap >= 0 and orders in {1, 2, 3}")
    return w


def pack(lengths, nd, n_ap, orders, d_f0, d_coded_sp, d_coded_ap, d_rows, lf0_fill=0.0, out_format="f64"):
    """packed device arrays (float64) -> rows of out_format: statics, deltas, continuous lf0 and vuv; enqueue-only"""
    _check(_L().wc_pack_model_features_device(len(lengths), _ints(lengths), int(nd), int(n_ap), int(orders), _opt(d_f0), _opt(d_coded_sp),
                                              _opt(d_coded_ap), float(lf0_fill), FORMATS[out_format][0], _opt(d_rows)))


def mlpg(lengths, nd, n_ap, orders, d_mean, d_var, d_static, var_per_frame=False, in_format="f64"):
    """rows of means and variances (one row of variances per frame, or one for the batch) -> static rows (float64, the orders == 1
    layout); enqueue-only"""
    _check(_L().wc_mlpg_device(len(lengths), _ints(lengths), int(nd), int(n_ap), int(orders), FORMATS[in_format][0], _opt(d_mean), _opt(d_var),
                               1 if var_per_frame else 0, _opt(d_static)))


def unpack(n_frames, nd, n_ap, orders, d_rows, d_f0, d_coded_sp, d_coded_ap, vuv_threshold=0.5, in_format="f64"):
    """rows -> f0 (exp(lf0) where vuv > vuv_threshold, else 0), coded sp, coded ap (float64; each may be None); enqueue-only"""
    _check(_L().wc_unpack_model_features_device(int(n_frames), int(nd), int(n_ap), int(orders), FORMATS[in_format][0], _opt(d_rows),
                                                float(vuv_threshold), _opt(d_f0), _opt(d_coded_sp), _opt(d_coded_ap)))


def _up(arrays, dtype=np.float64):
    a = np.concatenate([np.ascontiguousarray(x, dtype=dtype).ravel() for x in arrays]) if len(arrays) else np.zeros(0, dtype=dtype)
    return DeviceArray.from_host(a, dtype=dtype)


def _split(flat, lengths, cols):
    cuts = np.cumsum([n * cols for n in lengths])[:-1]
    return [part.reshape(n, cols).copy() for part, n in zip(np.split(flat, cuts), lengths)]


def pack_host(f0s, coded_sps, coded_aps, orders=3, lf0_fill=0.0, out_format="f64"):
    """lists of host arrays per utterance (f0 [n], coded sp [n, nd], coded ap [n, n_ap] or None for no bands) -> the list of their
    rows [n, width]"""
    lengths = [len(f) for f in f0s]
    sps = [np.asarray(s, dtype=np.float64).reshape(n, -1) for s, n in zip(coded_sps, lengths)]
    if len(sps) != len(lengths) or (coded_aps is not None and len(coded_aps) != len(lengths)) or not lengths:
        raise ValueError("one contour, one coded sp and one coded ap per utterance, one utterance at least")
    nd = sps[0].shape[1]
    aps = None if coded_aps is None else [np.asarray(a, dtype=np.float64).reshape(n, -1) for a, n in zip(coded_aps, lengths)]
    n_ap = 0 if aps is None else aps[0].shape[1]
    if any(s.shape[1] != nd for s in sps) or (aps is not None and any(a.shape[1] != n_ap for a in aps)):
        raise ValueError("every utterance has the same columns")
    w = width(nd, n_ap, orders)
    held = [_up(f0s), _up(sps), None if n_ap == 0 else _up(aps), DeviceArray(sum(lengths) * w, dtype=FORMATS[out_format][1])]
    try:
        pack(lengths, nd, n_ap, orders, held[0], held[1], held[2], held[3], lf0_fill, out_format)
        return _split(held[3].to_host(), lengths, w)  # (the copy waits for the stream)
    finally:
        for d in held:
            if d is not None:
                d.free()


def mlpg_host(means, variances, nd, n_ap, orders=3):
    """means: a list of rows [n, width] per utterance (all float32, or anything else as float64); variances: such a list as well, or one
    row [width] for all -> the list of static rows [n, nd + 2 + n_ap]"""
    fmt = "f32" if {np.asarray(m).dtype for m in means} == {np.dtype(np.float32)} else "f64"
    dt = FORMATS[fmt][1]
    w = width(nd, n_ap, orders)
    lengths = [np.asarray(m).size // w for m in means]
    per_frame = isinstance(variances, (list, tuple))
    held = [_up(means, dt), _up(variances if per_frame else [variances], dt), DeviceArray(sum(lengths) * (nd + 2 + n_ap))]
    try:
        mlpg(lengths, nd, n_ap, orders, held[0], held[1], held[2], per_frame, fmt)
        return _split(held[2].to_host(), lengths, nd + 2 + n_ap)
    finally:
        for d in held:
            d.free()


def unpack_host(rows, nd, n_ap, orders=1, vuv_threshold=0.5):
    """rows [n, width] (float32, or anything else as float64) -> f0 [n], coded sp [n, nd], coded ap [n, n_ap]"""
    fmt = "f32" if np.asarray(rows).dtype == np.float32 else "f64"
    w = width(nd, n_ap, orders)
    n = np.asarray(rows).size // w
    held = [_up([rows], FORMATS[fmt][1]), DeviceArray(n), DeviceArray(n * nd), DeviceArray(n * n_ap) if n_ap else None]
    try:
        unpack(n, nd, n_ap, orders, held[0], held[1], held[2], held[3], vuv_threshold, fmt)
        return held[1].to_host(), held[2].to_host((n, nd)), held[3].to_host((n, n_ap)) if n_ap else np.zeros((n, 0))
    finally:
        for d in held:
            if d is not None:
                d.free()
