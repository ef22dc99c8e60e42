"""Python mirror of include/world_class_gmm_train.h: expectation-maximisation for the joint-density mixture that gmm.Gmm converts
with -- posteriors of every frame of joint rows [x; y] under the model in force, the sufficient statistics of every mixture summed on
the device, the re-estimation on the host.  Row formats are "f64" and "f32"; a mask is one byte per frame (a frame counts where its
byte is not 0)."""
import ctypes as C

import numpy as np

from . import DeviceArray, WorldClassError, _check, _handle, _opt, last_error  # noqa: F401
from .features import FORMATS, _up
from ._binding import _binder, _Handle

_vp = C.c_void_p
_dp = C.POINTER(C.c_double)


class TrainInfo(C.Structure):
    """wc_gmm_train_info"""
    _fields_ = [("loglik", C.c_double), ("n_live", C.c_longlong), ("n_dropped", C.c_longlong), ("n_starved", C.c_int), ("n_kept", C.c_int)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_ip = C.POINTER(TrainInfo)

GMM_TRAIN_SIGNATURES = {
    "wc_gmm_trainer_create": (_vp, [C.c_int, C.c_int, C.c_int]),
    "wc_gmm_trainer_destroy": (None, [_vp]),
    "wc_gmm_trainer_set_model": (C.c_int, [_vp, _dp, _dp, _dp]),
    "wc_gmm_trainer_model_host": (C.c_int, [_vp, _dp, _dp, _dp]),
    "wc_gmm_trainer_posterior_device": (C.c_int, [_vp, C.c_longlong, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    "wc_gmm_trainer_accumulate_device": (C.c_int, [_vp, C.c_longlong, C.c_int, _vp, C.c_int, C.c_int, _vp]),
    "wc_gmm_trainer_stats_host": (C.c_int, [_vp, _dp, _dp, _dp, _ip]),
    "wc_gmm_trainer_update": (C.c_int, [_vp, C.c_double, _dp, _ip]),
    "wc_gmm_trainer_reset_stats": (C.c_int, [_vp]),
    "wc_gmm_trainer_set_segments_per_launch": (C.c_int, [_vp, C.c_int]),
}

_L = _binder(GMM_TRAIN_SIGNATURES)


def _host(a):
    return None if a is None else a.ctypes.data_as(_dp)


def initial_model(rows, n_mix, seed=0):
    """rows [n, D] on the host -> (weight [n_mix], mean [n_mix, D], cov [n_mix, D, D]): n_mix distinct frames drawn with
    numpy.random.default_rng(seed) as means, the global diagonal covariance for every mixture, equal weights"""
    rows = np.asarray(rows, dtype=np.float64)
    n, D = rows.shape
    if not 1 <= n_mix <= n:
        raise ValueError("n_mix lies in 1 .. the number of frames")
    picks = np.sort(np.random.default_rng(seed).choice(n, size=n_mix, replace=False))
    cov = np.tile(np.diag(rows.var(axis=0)), (n_mix, 1, 1))
    return np.full(n_mix, 1.0 / n_mix), rows[picks].copy(), cov


class GmmTrainer(_Handle):
    """A trainer handle: a model, and the statistics accumulated under it since the last update or reset.  It lives on the device
    current at construction and belongs to one host thread at a time."""
    _lib = staticmethod(_L)
    _sym = "wc_gmm_trainer"

    def __init__(self, n_mix, dx, dy):
        self.n_mix, self.dx, self.dy = int(n_mix), int(dx), int(dy)
        self.D = self.dx + self.dy
        self._create(self.n_mix, self.dx, self.dy)

    def set_model(self, weight, mean, cov):
        """the arrays gmm.Gmm takes: weight [n_mix], mean [n_mix, D], cov [n_mix, D, D] (the lower triangle is read)"""
        w = np.ascontiguousarray(weight, dtype=np.float64).ravel()
        m = np.ascontiguousarray(mean, dtype=np.float64).ravel()
        cv = np.ascontiguousarray(cov, dtype=np.float64).ravel()
        if w.size != self.n_mix or m.size != self.n_mix * self.D or cv.size != self.n_mix * self.D * self.D:
            raise ValueError("weight, mean and cov hold n_mix, n_mix * D and n_mix * D * D values")
        _check(_L().wc_gmm_trainer_set_model(self._h, _host(w), _host(m), _host(cv)))

    def model(self):
        """-> weight [n_mix], mean [n_mix, D], cov [n_mix, D, D] (both triangles), as gmm.Gmm takes them"""
        w, m, cv = np.empty(self.n_mix), np.empty((self.n_mix, self.D)), np.empty((self.n_mix, self.D, self.D))
        _check(_L().wc_gmm_trainer_model_host(self._h, _host(w), _host(m), _host(cv)))
        return w, m, cv

    def posterior(self, n_frames, d_rows, ld, d_post, d_frame_ll, col=0, d_mask=None, format="f64"):
        """the E-step alone: the posteriors [n_frames, n_mix] and the frames' log-likelihoods [n_frames] (float64; one of the two may be
        None); enqueue-only"""
        _check(_L().wc_gmm_trainer_posterior_device(self._h, int(n_frames), FORMATS[format][0], _opt(d_rows), int(ld), int(col), _opt(d_mask),
                                                    _opt(d_post), _opt(d_frame_ll)))

    def accumulate(self, n_frames, d_rows, ld, col=0, d_mask=None, format="f64"):
        """the E-step and the statistics of n_frames rows, added to the handle's totals; enqueue-only"""
        _check(_L().wc_gmm_trainer_accumulate_device(self._h, int(n_frames), FORMATS[format][0], _opt(d_rows), int(ld), int(col), _opt(d_mask)))

    def stats(self):
        """waits -> N [n_mix], S1 [n_mix, D], S2 [n_mix, D(D+1)/2] (lower triangles packed row by row), info (a dict)"""
        N, S1, S2 = np.empty(self.n_mix), np.empty((self.n_mix, self.D)), np.empty((self.n_mix, self.D * (self.D + 1) // 2))
        info = TrainInfo()
        _check(_L().wc_gmm_trainer_stats_host(self._h, _host(N), _host(S1), _host(S2), C.byref(info)))
        return N, S1, S2, info.as_dict()

    def update(self, min_occupancy=1.0, var_floor=None):
        """waits; the M-step on the host from the totals, which it clears -> info (a dict: loglik under the model the statistics were taken
        with, n_live, n_dropped, n_starved, n_kept)"""
        floor = None
        if var_floor is not None:
            floor = np.ascontiguousarray(var_floor, dtype=np.float64).ravel()
            if floor.size != self.D:
                raise ValueError("var_floor holds D values")
        info = TrainInfo()
        _check(_L().wc_gmm_trainer_update(self._h, float(min_occupancy), _host(floor), C.byref(info)))
        return info.as_dict()

    def reset_stats(self):
        _check(_L().wc_gmm_trainer_reset_stats(self._h))

    def set_segments_per_launch(self, g):
        """g segments of 1024 frames per launch; 0: chosen from the scratch budget.  Never changes a result"""
        _check(_L().wc_gmm_trainer_set_segments_per_launch(self._h, int(g)))

    def fit(self, d_rows, n, ld, iters, col=0, d_mask=None, format="f64", min_occupancy=1.0, var_floor=None):
        """iters iterations of EM over n rows on the device -> the list of every iteration's info; info["loglik"] of iteration k is the
        total log-likelihood under the model that iteration started from"""
        out = []
        self.reset_stats()
        for _ in range(int(iters)):
            self.accumulate(n, d_rows, ld, col, d_mask, format)
            out.append(self.update(min_occupancy, var_floor))
        return out

    def fit_host(self, rows, iters, min_occupancy=1.0, var_floor=None):
        """rows [n, D] (float32, or anything else as float64) on the host -> fit's list"""
        rows = np.asarray(rows)
        fmt = "f32" if rows.dtype == np.float32 else "f64"
        rows = np.ascontiguousarray(rows, dtype=FORMATS[fmt][1])
        n, ld = rows.shape
        d = _up([rows], FORMATS[fmt][1])
        try:
            return self.fit(d, n, ld, iters, 0, None, fmt, min_occupancy, var_floor)
        finally:
            d.free()

    def to_gmm(self):
        """-> gmm.Gmm prepared from the model in force"""
        from .gmm import Gmm
        w, m, cv = self.model()
        return Gmm(w, m, cv, self.dx)
