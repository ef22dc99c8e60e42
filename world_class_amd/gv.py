"""Python mirror of include/world_class_gv.h: parameter generation with a global-variance (GV) term behind MLPG on the device -- the
variance-scaling post-filter, the Newton-like ascent steps on the likelihood of the model and of the utterance-level variance, and the
masked mean and variance of every static column.  The static rows are those of features.mlpg (float64, nd + 2 + n_ap columns); the GV
arrays hold one double per static column in the order mgc, lf0, bands; a mask holds one byte per frame (None: every frame counts)."""
import ctypes as C

import numpy as np

from . import DeviceArray, _check, _ints, _opt  # noqa: F401  (_ints: for raw calls through _L(), as the tests make them)
from .features import FORMATS, _split, _up, width
from ._binding import _binder

_ip = C.POINTER(C.c_int)
_vp = C.c_void_p

GV_SIGNATURES = {
    "wc_gv_stats_device": (C.c_int, [C.c_int, _ip, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "wc_mlpg_gv_device": (C.c_int, [C.c_int, _ip, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_double, C.c_double,
                                    C.c_double, C.c_int, _vp]),
}

_L = _binder(GV_SIGNATURES)


def stats(lengths, nd, n_ap, d_static, d_mean_out, d_var_out, d_mask=None):
    """static rows -> the mean and the variance of every (utterance, static column) over the masked frames, [n_utt, S] each;
    enqueue-only"""
    _check(_L().wc_gv_stats_device(len(lengths), _ints(lengths), int(nd), int(n_ap), _opt(d_static), _opt(d_mask), _opt(d_mean_out),
                                   _opt(d_var_out)))


def mlpg_gv(lengths, nd, n_ap, orders, d_mean, d_var, d_gv_mean, d_gv_var, d_static, d_mask=None, var_per_frame=False, in_format="f64",
            w_ml=1.0, w_gv=1.0, step_init=0.1, max_iter=5):
    """features.mlpg's output d_static on the same d_mean / d_var, refined in place: the variance-scaling start and max_iter ascent
    steps on w_ml * omega * log-likelihood + w_gv * GV likelihood; enqueue-only"""
    _check(_L().wc_mlpg_gv_device(len(lengths), _ints(lengths), int(nd), int(n_ap), int(orders), FORMATS[in_format][0], _opt(d_mean), _opt(d_var),
                                  1 if var_per_frame else 0, _opt(d_gv_mean), _opt(d_gv_var), _opt(d_mask), float(w_ml), float(w_gv),
                                  float(step_init), int(max_iter), _opt(d_static)))


def scale(lengths, nd, n_ap, d_gv_mean, d_gv_var, d_static, d_mask=None):
    """the closed-form variance-scaling post-filter alone (max_iter == 0: no means or variances are read): every static column of every
    utterance takes the variance gv_mean over its masked frames, in place; enqueue-only"""
    mlpg_gv(lengths, nd, n_ap, 2, None, None, d_gv_mean, d_gv_var, d_static, d_mask, max_iter=0)


def _mask_up(masks):
    return None if masks is None else _up([np.asarray(m) != 0 for m in masks], np.uint8)


def _free(held):
    for d in held:
        if d is not None:
            d.free()


def stats_host(statics, nd, n_ap, masks=None):
    """statics: a list of static rows [n, nd + 2 + n_ap] per utterance; masks: such a list of [n], or None -> mean, variance [n_utt, S]"""
    lengths, S = [np.asarray(s).size // (nd + 2 + n_ap) for s in statics], nd + 1 + n_ap
    held = [_up(statics), _mask_up(masks), DeviceArray(len(lengths) * S), DeviceArray(len(lengths) * S)]
    try:
        stats(lengths, nd, n_ap, held[0], held[2], held[3], held[1])
        return held[2].to_host((len(lengths), S)), held[3].to_host((len(lengths), S))   # (the copy waits for the stream)
    finally:
        _free(held)


def mlpg_gv_host(means, variances, statics, gv_mean, gv_var, nd, n_ap, orders=3, masks=None, w_ml=1.0, w_gv=1.0, step_init=0.1, max_iter=5):
    """means, variances: as features.mlpg_host takes them; statics: its result on them -> the list of refined static rows"""
    fmt = "f32" if {np.asarray(m).dtype for m in means} == {np.dtype(np.float32)} else "f64"
    dt = FORMATS[fmt][1]
    w = width(nd, n_ap, orders)
    lengths = [np.asarray(m).size // w for m in means]
    per_frame = isinstance(variances, (list, tuple))
    held = [_up(means, dt), _up(variances if per_frame else [variances], dt), _up([gv_mean]), _up([gv_var]), _up(statics), _mask_up(masks)]
    try:
        mlpg_gv(lengths, nd, n_ap, orders, held[0], held[1], held[2], held[3], held[4], held[5], per_frame, fmt, w_ml, w_gv, step_init, max_iter)
        return _split(held[4].to_host(), lengths, nd + 2 + n_ap)
    finally:
        _free(held)


def scale_host(statics, gv_mean, gv_var, nd, n_ap, masks=None):
    """statics: a list of static rows [n, nd + 2 + n_ap] per utterance -> the list of variance-scaled static rows"""
    lengths = [np.asarray(s).size // (nd + 2 + n_ap) for s in statics]
    held = [_up([gv_mean]), _up([gv_var]), _up(statics), _mask_up(masks)]
    try:
        scale(lengths, nd, n_ap, held[0], held[1], held[2], held[3])
        return _split(held[2].to_host(), lengths, nd + 2 + n_ap)
    finally:
        _free(held)
