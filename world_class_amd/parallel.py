"""Python mirror of include/world_class_parallel.h: what lies between the alignment and the training of a joint-density mixture -- the
gather of two speakers' rows along an alignment path into joint rows [x; y] with a mask byte per row, the speech mask that keeps
silence out of the training, and the distortion along the path.  Row formats are "f64" and "f32"; a mask is one byte per frame (a
frame counts where its byte is not 0); a path is what io.align_features[_ex]_device writes."""
import ctypes as C
import math

import numpy as np

from . import DeviceArray, WorldClassError, _check, _ints, _opt, last_error  # noqa: F401
from .features import FORMATS, _up
from ._binding import _binder

_vp = C.c_void_p
_ip = C.POINTER(C.c_int)

PARALLEL_SIGNATURES = {
    "wc_joint_rows_device": (C.c_int, [C.c_int, _ip, _ip, C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.c_int,
                                       _vp, _vp, _vp, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp]),
    "wc_speech_mask_device": (C.c_int, [C.c_int, _ip, C.c_int, _vp, C.c_int, C.c_int, C.c_double, C.c_double, _vp]),
    "wc_path_distortion_device": (C.c_int, [C.c_int, _ip, _ip, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.c_int,
                                            _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}

_L = _binder(PARALLEL_SIGNATURES)

DB_IN_C0 = math.log(10.0) / 10.0  # one decibel of frame power in units of c0, the column the speech mask reads (see the header)


def _pairs(a_lengths, b_lengths):
    if len(a_lengths) != len(b_lengths):
        raise ValueError("a_lengths and b_lengths have one entry per pair each")
    return len(a_lengths), _ints(a_lengths), _ints(b_lengths)


def slots(a_lengths, b_lengths):
    """the rows of the joint matrix and the entries of the path: sum of a + b - 1 over the pairs"""
    return int(sum(int(a) + int(b) - 1 for a, b in zip(a_lengths, b_lengths)))


def joint_rows(a_lengths, b_lengths, d_rows_a, ld_a, dx, d_rows_b, ld_b, dy, d_path_length, d_path, d_joint, ld_out, d_joint_mask=None,
               col_a=0, col_b=0, col_out=0, d_mask_a=None, d_mask_b=None, a_format="f64", b_format="f64", out_format="f64"):
    """one joint row [x; y] and one mask byte per slot of the path: columns [col_a, col_a + dx) of A's frame i and [col_b, col_b + dy)
    of B's frame j into columns [col_out, col_out + dx + dy) of row P_u + s; a slot that is not on the path gets +0.0 and the byte 0;
    enqueue-only"""
    n, al, bl = _pairs(a_lengths, b_lengths)
    _check(_L().wc_joint_rows_device(n, al, bl, FORMATS[a_format][0], _opt(d_rows_a), int(ld_a), int(col_a), int(dx), FORMATS[b_format][0],
                                     _opt(d_rows_b), int(ld_b), int(col_b), int(dy), _opt(d_path_length), _opt(d_path), _opt(d_mask_a),
                                     _opt(d_mask_b), FORMATS[out_format][0], _opt(d_joint), int(ld_out), int(col_out), _opt(d_joint_mask)))


def speech_mask(lengths, d_rows, ld, d_mask, col=0, margin=math.inf, floor=-math.inf, format="f64"):
    """one byte per frame: 1 where the value of column col is finite, within margin of its utterance's greatest finite value and not
    below floor.  margin is in the column's units: margin_db * DB_IN_C0 for c0; enqueue-only"""
    _check(_L().wc_speech_mask_device(len(lengths), _ints(lengths), FORMATS[format][0], _opt(d_rows), int(ld), int(col), float(margin),
                                      float(floor), _opt(d_mask)))


def path_distortion(a_lengths, b_lengths, d_rows_a, ld_a, d_rows_b, ld_b, dims, d_path_length, d_path, d_sum=None, d_count=None, d_cell=None,
                    col_a=0, col_b=0, d_mask_a=None, d_mask_b=None, a_format="f64", b_format="f64"):
    """per pair the sum (float64) of the Euclidean distances over dims columns along the live slots of the path, in ascending order,
    and their count (int64); per slot the distance (float64, packed like the path); each output may be None, not all three;
    enqueue-only"""
    n, al, bl = _pairs(a_lengths, b_lengths)
    _check(_L().wc_path_distortion_device(n, al, bl, FORMATS[a_format][0], _opt(d_rows_a), int(ld_a), int(col_a), FORMATS[b_format][0],
                                          _opt(d_rows_b), int(ld_b), int(col_b), int(dims), _opt(d_path_length), _opt(d_path),
                                          _opt(d_mask_a), _opt(d_mask_b), _opt(d_sum), _opt(d_count), _opt(d_cell)))


def mcd_db(total, count):
    """mel-cepstral distortion in dB: (10 / ln 10) * sqrt(2) * total / count, total the sum of distances over count cells"""
    return (10.0 / math.log(10.0)) * math.sqrt(2.0) * float(total) / float(count)


def _fmt(a):
    return "f32" if np.asarray(a).dtype == np.float32 else "f64"


def joint_rows_host(a_lengths, b_lengths, rows_a, rows_b, path_length, path, mask_a=None, mask_b=None, col_a=0, dx=None, col_b=0, dy=None,
                    out_format="f64"):
    """numpy in, numpy out: rows_a [frames_a, ld_a], rows_b [frames_b, ld_b] (float32, or anything else as float64), path_length
    [pairs] and path [slots, 2] as the alignment wrote them -> (joint [slots, dx + dy] of out_format, mask [slots] uint8)"""
    fa, fb = _fmt(rows_a), _fmt(rows_b)
    rows_a, rows_b = np.ascontiguousarray(rows_a, dtype=FORMATS[fa][1]), np.ascontiguousarray(rows_b, dtype=FORMATS[fb][1])
    ld_a, ld_b = rows_a.shape[1], rows_b.shape[1]
    dx, dy = ld_a - col_a if dx is None else dx, ld_b - col_b if dy is None else dy
    n = slots(a_lengths, b_lengths)
    odt = FORMATS[out_format][1]
    held = [_up([rows_a], FORMATS[fa][1]), _up([rows_b], FORMATS[fb][1]), _up([path_length], np.int32), _up([path], np.int32),
            None if mask_a is None else _up([mask_a], np.uint8), None if mask_b is None else _up([mask_b], np.uint8),
            DeviceArray(n * (dx + dy), odt), DeviceArray(n, np.uint8)]
    try:
        joint_rows(a_lengths, b_lengths, held[0], ld_a, dx, held[1], ld_b, dy, held[2], held[3], held[6], dx + dy, held[7], col_a, col_b, 0,
                   held[4], held[5], fa, fb, out_format)
        return held[6].to_host((n, dx + dy)), held[7].to_host()  # (the copy waits for the stream)
    finally:
        for d in held:
            if d is not None:
                d.free()


def fit_parallel(a_lengths, b_lengths, nd, n_ap, orders, d_f0_a, d_sp_a, d_ap_a, d_f0_b, d_sp_b, d_ap_b, n_mix, rounds=1, iters=5,
                 margin_db=40.0, floor=-math.inf, band=0, model=None, seed=0, min_occupancy=1.0, var_floor=None, keep=None):
    """The loop of joint-density training on a parallel corpus, on the library's calls alone.  Both speakers' coded features stand on
    the device as features.pack takes them (f0 [frames], coded sp [frames, nd], coded ap [frames, n_ap] or None, float64, packed pair
    after pair).  Packs both speakers' model rows, masks silence on c0 (margin_db below the utterance's loudest frame, floor in c0's
    units), then `rounds` times: align (A as it is in round 0; afterwards A converted through the current model and MLPG) on the
    static mel-cepstrum without c0, join A's and B's spectral columns [0, orders * nd) along the path, and run `iters` iterations of
    EM.  -> (the GmmTrainer, one (logliks, mcd) per round): logliks[k] is the total log-likelihood under the model iteration k started
    from, mcd the mel-cepstral distortion in dB along that round's path over the frames both masks keep (nan with none).

    What comes back from the device in a round is the M-step's statistics, the model and two scalars per pair.  model: (weight, mean,
    cov) to start from; None reads the first round's joint rows back once and draws gmm_train.initial_model from the live ones with
    `seed`.  keep: a dict that receives the device arrays of the last round (rows_a, rows_b, mask_a, mask_b, path_length, path,
    joint, joint_mask) instead of their being freed -- theirs to free."""
    from . import features as ft, io as wio
    from .gmm_train import GmmTrainer, initial_model
    n_pairs = len(a_lengths)
    if n_pairs != len(b_lengths) or n_pairs == 0:
        raise ValueError("a_lengths and b_lengths have one entry per pair each, one pair at the least")
    if rounds < 1 or (rounds > 1 and orders < 2):
        raise ValueError("rounds >= 1; a second round converts through MLPG, which takes orders 2 or 3")
    Fa, Fb, n_slots = int(sum(a_lengths)), int(sum(b_lengths)), slots(a_lengths, b_lengths)
    W, S1 = ft.width(nd, n_ap, orders), ft.width(nd, n_ap, 1)
    dx = dy = orders * nd
    D = dx + dy
    lo = 1 if nd > 1 else 0  # the alignment and the distortion leave c0 out where there is anything else
    held = {}

    def dev(name, n, dtype=np.float64):
        held[name] = DeviceArray(n, dtype)
        return held[name]

    try:
        rows_a, rows_b = dev("rows_a", Fa * W), dev("rows_b", Fb * W)
        ft.pack(a_lengths, nd, n_ap, orders, d_f0_a, d_sp_a, d_ap_a, rows_a)
        ft.pack(b_lengths, nd, n_ap, orders, d_f0_b, d_sp_b, d_ap_b, rows_b)
        stat_a, stat_b = dev("stat_a", Fa * S1), dev("stat_b", Fb * S1)  # the orders == 1 layout: what the alignment compares
        ft.pack(a_lengths, nd, n_ap, 1, d_f0_a, d_sp_a, d_ap_a, stat_a)
        ft.pack(b_lengths, nd, n_ap, 1, d_f0_b, d_sp_b, d_ap_b, stat_b)
        mask_a, mask_b = dev("mask_a", Fa, np.uint8), dev("mask_b", Fb, np.uint8)
        speech_mask(a_lengths, rows_a, W, mask_a, 0, margin_db * DB_IN_C0, floor)
        speech_mask(b_lengths, rows_b, W, mask_b, 0, margin_db * DB_IN_C0, floor)
        cost, path_length, path = dev("cost", n_pairs), dev("path_length", n_pairs, np.int32), dev("path", 2 * n_slots, np.int32)
        joint, joint_mask = dev("joint", n_slots * D), dev("joint_mask", n_slots, np.uint8)
        d_sum, d_count = dev("sum", n_pairs), dev("count", n_pairs, np.int64)
        if rounds > 1:
            mean, conv = dev("mean", Fa * W), dev("conv", Fa * S1)
            held["var"] = DeviceArray.from_host(np.ones(Fa * W))  # the columns the conversion does not write keep a variance of 1
        trainer = GmmTrainer(n_mix, dx, dy)
        out = []
        for r in range(int(rounds)):
            src = stat_a
            if r > 0:  # A through the model in force: the other columns' means are A's own
                g = trainer.to_gmm()
                try:
                    ft.pack(a_lengths, nd, n_ap, orders, d_f0_a, d_sp_a, d_ap_a, mean)
                    g.convert(Fa, rows_a, W, mean, held["var"], W)
                    ft.mlpg(a_lengths, nd, n_ap, orders, mean, held["var"], conv, True)
                    _check(_L().wc_synchronize())  # the handle goes before the next call: its arrays are read until here
                finally:
                    g.close()
                src = conv
            wio.align_features_device(a_lengths, src, b_lengths, stat_b, S1, lo, nd, band, cost, path_length, path)
            joint_rows(a_lengths, b_lengths, rows_a, W, dx, rows_b, W, dy, path_length, path, joint, D, joint_mask, d_mask_a=mask_a, d_mask_b=mask_b)
            path_distortion(a_lengths, b_lengths, src, S1, stat_b, S1, nd - lo, path_length, path, d_sum, d_count, None, lo, lo, mask_a, mask_b)
            if r == 0:
                if model is None:
                    live = joint_mask.to_host() != 0
                    model = initial_model(joint.to_host((n_slots, D))[live], n_mix, seed)
                trainer.set_model(*model)
            infos = trainer.fit(joint, n_slots, D, iters, 0, joint_mask, "f64", min_occupancy, var_floor)
            total, count = float(d_sum.to_host().sum()), int(d_count.to_host().sum())
            out.append(([i["loglik"] for i in infos], mcd_db(total, count) if count else math.nan))
        if keep is not None:
            for name in ("rows_a", "rows_b", "mask_a", "mask_b", "path_length", "path", "joint", "joint_mask"):
                keep[name] = held.pop(name)
        return trainer, out
    finally:
        for d in held.values():
            d.free()
