"""Python mirror of include/world_class_gmm.h: joint-density GMM conversion in front of MLPG on the device -- the log-likelihood of
every mixture per frame, the most likely mixture, and its conditional mean and variance written into the columns of MLPG's mean and
variance rows.  Row formats are "f64" and "f32"; the model comes from elsewhere as host arrays (weights, joint means [x; y], joint
covariances, of which the lower triangle is read)."""
import ctypes as C

import numpy as np

from . import DeviceArray, WorldClassError, _check, _handle, _opt, last_error  # noqa: F401
from .features import FORMATS, _up
from ._binding import _binder, _Handle

_vp = C.c_void_p
_dp = C.POINTER(C.c_double)

GMM_SIGNATURES = {
    "wc_gmm_create": (_vp, [C.c_int, C.c_int, C.c_int, _dp, _dp, _dp]),
    "wc_gmm_destroy": (None, [_vp]),
    "wc_gmm_prepared_host": (C.c_int, [_vp, _dp, _dp, _dp, _dp]),
    "wc_gmm_convert_device": (C.c_int, [_vp, C.c_longlong, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, _vp]),
}

_L = _binder(GMM_SIGNATURES)


def _host(a):
    return None if a is None else a.ctypes.data_as(_dp)


def joint_from_blocks(mux, muy, sxx, syx, syy):
    """mux [n_mix, dx], muy [n_mix, dy], sxx [n_mix, dx, dx], syx [n_mix, dy, dx], syy [n_mix, dy, dy] (or [n_mix, dy] for a diagonal)
    -> the joint mean [n_mix, dx + dy] and covariance [n_mix, dx + dy, dx + dy] that Gmm takes (symmetric: Sxy = Syx^T)"""
    mux, muy = np.atleast_2d(np.asarray(mux, dtype=np.float64)), np.atleast_2d(np.asarray(muy, dtype=np.float64))
    n_mix, dx, dy = mux.shape[0], mux.shape[1], muy.shape[1]
    sxx = np.asarray(sxx, dtype=np.float64).reshape(n_mix, dx, dx)
    syx = np.asarray(syx, dtype=np.float64).reshape(n_mix, dy, dx)
    syy = np.asarray(syy, dtype=np.float64)
    if syy.size == n_mix * dy:
        syy = np.stack([np.diag(v) for v in syy.reshape(n_mix, dy)])
    syy = syy.reshape(n_mix, dy, dy)
    mean = np.concatenate([mux, muy], axis=1)
    cov = np.zeros((n_mix, dx + dy, dx + dy))
    cov[:, :dx, :dx], cov[:, dx:, :dx], cov[:, :dx, dx:], cov[:, dx:, dx:] = sxx, syx, syx.transpose(0, 2, 1), syy
    return mean, cov


class Gmm(_Handle):
    """A joint-density mixture prepared for conversion: the handle lives on the device current at construction and is read-only, so
    several host threads may convert with it on their own streams."""
    _lib = staticmethod(_L)
    _sym = "wc_gmm"

    def __init__(self, weight, mean, cov, dx):
        w = np.ascontiguousarray(weight, dtype=np.float64).ravel()
        self.n_mix, self.dx = int(w.size), int(dx)
        m = np.ascontiguousarray(mean, dtype=np.float64).reshape(self.n_mix, -1)
        self.dy = int(m.shape[1]) - self.dx
        D = self.dx + self.dy
        cv = np.ascontiguousarray(cov, dtype=np.float64)
        if cv.size != self.n_mix * D * D:
            raise ValueError("cov holds n_mix * (dx + dy) * (dx + dy) values")
        self._create(self.n_mix, self.dx, self.dy, _host(w), _host(m), _host(cv))

    def convert(self, n_frames, d_rows_in, ld_in, d_mean, d_var, ld_out, col_in=0, col_out=0, d_best=None, d_loglik=None, in_format="f64",
                out_format="f64"):
        """columns [col_in, col_in + dx) of n_frames input rows -> columns [col_out, col_out + dy) of the mean and variance rows, the
        best mixture of every frame (int32) and the table of log-likelihoods [n_frames, n_mix] (float64); each output may be None;
        enqueue-only"""
        _check(_L().wc_gmm_convert_device(self._h, int(n_frames), FORMATS[in_format][0], _opt(d_rows_in), int(ld_in), int(col_in),
                                          FORMATS[out_format][0], _opt(d_mean), _opt(d_var), int(ld_out), int(col_out), _opt(d_best),
                                          _opt(d_loglik)))

    def convert_host(self, rows, col_in=0, out_format="f64"):
        """rows [n, ld_in] (float32, or anything else as float64) -> (mean [n, dy], var [n, dy] of out_format, best [n] int32,
        loglik [n, n_mix])"""
        rows = np.asarray(rows)
        fmt = "f32" if rows.dtype == np.float32 else "f64"
        rows = np.ascontiguousarray(rows, dtype=FORMATS[fmt][1])
        rows = rows.reshape(-1, self.dx) if rows.ndim < 2 else rows
        n, ld = rows.shape
        odt = FORMATS[out_format][1]
        held = [_up([rows], FORMATS[fmt][1]), DeviceArray(n * self.dy, odt), DeviceArray(n * self.dy, odt), DeviceArray(n, np.int32),
                DeviceArray(n * self.n_mix)]
        try:
            self.convert(n, held[0], ld, held[1], held[2], self.dy, col_in, 0, held[3], held[4], fmt, out_format)
            return (held[1].to_host((n, self.dy)), held[2].to_host((n, self.dy)), held[3].to_host(),   # (the copy waits for the stream)
                    held[4].to_host((n, self.n_mix)))
        finally:
            for d in held:
                d.free()

    def prepared(self):
        """-> c [n_mix], W [n_mix, dx, dx] (the upper part 0.0), B [n_mix, dy, dx], cvar [n_mix, dy] as create prepared them"""
        c, W = np.empty(self.n_mix), np.empty((self.n_mix, self.dx, self.dx))
        B, cvar = np.empty((self.n_mix, self.dy, self.dx)), np.empty((self.n_mix, self.dy))
        _check(_L().wc_gmm_prepared_host(self._h, _host(c), _host(W), _host(B), _host(cvar)))
        return c, W, B, cvar
