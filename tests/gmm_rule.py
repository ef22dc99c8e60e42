"""THE rule of include/world_class_gmm.h in numpy and Python floats, in exactly the header's order.

Every element goes through the header's own sequence of operations; numpy only carries many elements through it side by side (all
mixtures, all frames, the rows or columns that do not depend on each other).  An elementwise numpy *, +, -, / or sqrt on float64 is the
correctly rounded IEEE operation, one at a time, so the bits are those of the scalar loop.  The logarithm is math.log: Python's math.log
and the library's log are the same libm function in one process; numpy's own SIMD log promises no such thing."""
import math

import numpy as np

LOG_2PI = 1.8378770664093453


def _finite(a):
    return np.isfinite(a)


def prepare(weight, mean, cov, dx, dy):
    """weight [n_mix], mean [n_mix, dx + dy], cov [n_mix, D, D] (only the lower triangle is read) -> dict(c [n_mix], W [n_mix, dx, dx]
    with the upper part 0.0, B [n_mix, dy, dx], cvar [n_mix, dy], mux [n_mix, dx], muy [n_mix, dy]).  A refusal raises ValueError
    whose text names the mixture and the row as the library's does"""
    if weight is None or mean is None or cov is None:
        raise ValueError("null array")
    weight = np.asarray(weight, dtype=np.float64).ravel()
    n_mix, D = weight.size, dx + dy
    if not 1 <= n_mix <= 1024:
        raise ValueError("n_mix outside 1 .. 1024")
    if not (1 <= dx <= 192 and 1 <= dy <= 192):
        raise ValueError("dx and dy lie in 1 .. 192")
    mean = np.asarray(mean, dtype=np.float64).reshape(n_mix, D)
    cov = np.asarray(cov, dtype=np.float64).reshape(n_mix, D, D)
    low = np.tril(np.ones((D, D), dtype=bool))
    for m in range(n_mix):
        if not (weight[m] > 0.0 and math.isfinite(weight[m])):
            raise ValueError("mixture %d: a weight that is not finite or not > 0" % m)
        for i in range(D):
            if not math.isfinite(mean[m, i]):
                raise ValueError("mixture %d, row %d: a mean that is not finite" % (m, i))
            if not _finite(cov[m, i][low[i]]).all():
                raise ValueError("mixture %d, row %d: a covariance entry that is not finite" % (m, i))
    Sxx, Syx = cov[:, :dx, :dx], cov[:, dx:, :dx]
    Syy = np.stack([cov[:, dx + j, dx + j] for j in range(dy)], axis=1)
    with np.errstate(all="ignore"):
        # Cholesky: element (i, j) takes k = 0 .. j-1 ascending; column by column, all rows i >= j and all mixtures side by side
        L = np.zeros((n_mix, dx, dx))
        diag_s = np.zeros((n_mix, dx))
        for j in range(dx):
            s = Sxx[:, j:, j].copy()
            for k in range(j):
                s = s - L[:, j:, k] * L[:, j, k][:, None]
            diag_s[:, j] = s[:, 0]
            L[:, j, j] = np.sqrt(s[:, 0])
            L[:, j + 1:, j] = s[:, 1:] / L[:, j, j][:, None]
        # W = L^-1: element (i, j) takes k = j+1 .. i-1 ascending; row by row, all columns j < i side by side
        W = np.zeros((n_mix, dx, dx))
        for i in range(dx):
            W[:, i, i] = 1.0 / L[:, i, i]
        for i in range(1, dx):
            s = L[:, i, :i] * np.stack([W[:, j, j] for j in range(i)], axis=1)
            for k in range(1, i):
                s[:, :k] = s[:, :k] + L[:, i, k][:, None] * W[:, k, :k]
            W[:, i, :i] = -s / L[:, i, i][:, None]
        # B = Syx W^T: element (j, k) takes i = 0 .. k ascending and starts at its first product
        B = np.zeros((n_mix, dy, dx))
        for k in range(dx):
            s = Syx[:, :, 0] * W[:, k, 0][:, None]
            for i in range(1, k + 1):
                s = s + Syx[:, :, i] * W[:, k, i][:, None]
            B[:, :, k] = s
        cvar = Syy.copy()
        for k in range(dx):
            cvar = cvar - B[:, :, k] * B[:, :, k]
    c = np.zeros(n_mix)
    for m in range(n_mix):   # the refusals in the library's order: mixture by mixture, the Cholesky rows, then the conditional variances
        for i in range(dx):
            if not (diag_s[m, i] > 0.0 and math.isfinite(diag_s[m, i])):
                raise ValueError("mixture %d, row %d: the source covariance is not positive definite" % (m, i))
        for j in range(dy):
            if not (cvar[m, j] > 0.0 and math.isfinite(cvar[m, j])):
                raise ValueError("mixture %d, row %d: a conditional variance that is not > 0 or not finite" % (m, dx + j))
        ld = math.log(float(L[m, 0, 0]))
        for i in range(1, dx):
            ld = ld + math.log(float(L[m, i, i]))
        c[m] = (math.log(float(weight[m])) - ld) - (0.5 * float(dx)) * LOG_2PI
    return dict(c=c, W=W, B=B, cvar=cvar, mux=mean[:, :dx].copy(), muy=mean[:, dx:].copy())


def loglik(prepared, x):
    """x [n, dx] -> ll [n, n_mix], z [n, n_mix, dx], q [n, n_mix]"""
    W, mux, c = prepared["W"], prepared["mux"], prepared["c"]
    x = np.asarray(x, dtype=np.float64)   # (a float input is widened exactly)
    n_mix, dx = mux.shape
    x = x.reshape(-1, dx)
    with np.errstate(all="ignore"):
        d = x[:, None, :] - mux[None, :, :]
        z = np.zeros((x.shape[0], n_mix, dx))
        q = None
        for i in range(dx):
            s = W[None, :, i, 0] * d[:, :, 0]
            for k in range(1, i + 1):
                s = s + W[None, :, i, k] * d[:, :, k]
            z[:, :, i] = s
            q = s * s if q is None else q + s * s
        return c[None, :] - 0.5 * q, z, q


def convert(prepared, x, out_dtype=np.float64):
    """x [n, dx] -> mean [n, dy], var [n, dy] (of out_dtype: the cast of the double), best [n] int32, ll [n, n_mix]"""
    B, cvar, muy = prepared["B"], prepared["cvar"], prepared["muy"]
    dy, dx = B.shape[1], B.shape[2]
    ll, z, _ = loglik(prepared, x)
    n = ll.shape[0]
    valid = ~np.isnan(ll)
    with np.errstate(all="ignore"):
        top = np.max(np.where(valid, ll, -np.inf), axis=1) if n else np.zeros(0)
        first = valid & (ll == top[:, None])          # the least m whose ll is not NaN and >= every other that is not NaN
        best = np.where(valid.any(axis=1), np.argmax(first, axis=1), -1).astype(np.int32)
        b = np.maximum(best, 0)
        zb, Bb = z[np.arange(n), b], B[b]             # [n, dx], [n, dy, dx]
        s = Bb[:, :, 0] * zb[:, 0][:, None]
        for k in range(1, dx):
            s = s + Bb[:, :, k] * zb[:, k][:, None]
        mean, var = muy[b] + s, cvar[b].copy()
    none = best < 0
    mean[none], var[none] = 0.0, np.inf
    return mean.astype(out_dtype), var.astype(out_dtype), best, ll
