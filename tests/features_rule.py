"""THE rule of include/world_class_features.h in numpy: the row layout, the continuous log-F0, the deltas, MLPG and unpack, every
operation in float64 and rounded on its own in the order the header states -- the device equals this bit for bit."""
import numpy as np

DBL_MAX = np.finfo(np.float64).max


def width(nd, n_ap, orders):
    return orders * (nd + 1 + n_ap) + 1


def columns(nd, n_ap, orders):
    """for each static column (mgc coefficients, lf0, bands): [its column at order k for k < orders]; and the vuv column"""
    cols = [[k * nd + c for k in range(orders)] for c in range(nd)]
    cols.append([orders * nd + k for k in range(orders)])
    cols += [[orders * (nd + 1) + 1 + k * n_ap + b for k in range(orders)] for b in range(n_ap)]
    return cols, orders * (nd + 1)


def voiced(f0):
    f0 = np.asarray(f0, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (f0 > 0.0) & (f0 <= DBL_MAX)


def continuous_lf0(f0, lf0_fill, logs=None):
    """one utterance.  logs: log(f0) on the voiced frames as another library gave it (the device's own), numpy's otherwise"""
    f0 = np.asarray(f0, dtype=np.float64)
    n, v = len(f0), voiced(f0)
    l = np.zeros(n)
    l[v] = np.log(f0[v]) if logs is None else np.asarray(logs, dtype=np.float64)[v]
    out = np.full(n, float(lf0_fill))
    idx = np.flatnonzero(v)
    if len(idx) == 0:
        return out
    for i in range(n):
        k = np.searchsorted(idx, i, side="right") - 1       # idx[k] = L(i), the greatest voiced index <= i
        L = idx[k] if k >= 0 else -1
        R = L if L == i else (idx[k + 1] if k + 1 < len(idx) else n)
        if L == i:
            out[i] = l[i]
        elif L < 0:
            out[i] = l[R]
        elif R >= n:
            out[i] = l[L]
        else:
            a = np.float64(i - L) / np.float64(R - L)
            out[i] = (1.0 - a) * l[L] + a * l[R]
    return out


def deltas(x):
    """(D x, DD x) of the columns of x [n] or [n, cols]; a neighbour outside the utterance counts as 0.0"""
    x = np.asarray(x, dtype=np.float64)
    xm, xp = np.zeros_like(x), np.zeros_like(x)
    xm[1:], xp[:-1] = x[:-1], x[1:]
    with np.errstate(invalid="ignore", over="ignore"):
        return 0.5 * (xp - xm), (xm + xp) - 2.0 * x


def pack(lengths, nd, n_ap, orders, f0, coded_sp, coded_ap, lf0_fill, logs=None):
    """the rows of a packed batch as float64 [frames, width]"""
    total = int(sum(lengths))
    f0 = np.asarray(f0, dtype=np.float64).reshape(total)
    sp = np.asarray(coded_sp, dtype=np.float64).reshape(total, nd)
    ap = np.zeros((total, 0)) if n_ap == 0 else np.asarray(coded_ap, dtype=np.float64).reshape(total, n_ap)
    logs = None if logs is None else np.asarray(logs, dtype=np.float64).reshape(total)
    cols, vuv_col = columns(nd, n_ap, orders)
    rows = np.zeros((total, width(nd, n_ap, orders)))
    o = 0
    for n in lengths:
        if n == 0:
            continue
        s = slice(o, o + n)
        lf0 = continuous_lf0(f0[s], lf0_fill, None if logs is None else logs[s])
        x = np.concatenate([sp[s], lf0[:, None], ap[s]], axis=1)
        parts = (x,) + deltas(x)
        for c, ks in enumerate(cols):
            for k, col in enumerate(ks):
                rows[s, col] = parts[k][:, c]
        rows[s, vuv_col] = np.where(voiced(f0[s]), 1.0, 0.0)
        o += n
    return rows


def mlpg_system(mean, var):
    """one utterance, every static column at once: mean, var [n, orders, cols] (orders 2 or 3) -> a0, a1, a2, r [n, cols]"""
    n, orders, cols = mean.shape
    with np.errstate(all="ignore"):
        p = np.zeros((n + 2, 3, cols))   # rows 0 and n + 1: outside the utterance
        q = np.zeros((n + 2, 3, cols))
        p[1:n + 1, :orders] = 1.0 / var
        q[1:n + 1, :orders] = np.where(p[1:n + 1, :orders] == 0.0, 0.0, p[1:n + 1, :orders] * mean)
        pm, pc, pp = p[0:n], p[1:n + 1], p[2:n + 2]
        qm, qc, qp = q[0:n], q[1:n + 1], q[2:n + 2]
        a0 = (pc[:, 0] + 0.25 * (pm[:, 1] + pp[:, 1])) + ((pm[:, 2] + pp[:, 2]) + 4.0 * pc[:, 2])
        a1 = -2.0 * (pc[:, 2] + pp[:, 2])
        a2 = pp[:, 2] - 0.25 * pp[:, 1]
        r = (qc[:, 0] + 0.5 * (qm[:, 1] - qp[:, 1])) + ((qm[:, 2] + qp[:, 2]) - 2.0 * qc[:, 2])
    a1[n - 1:] = 0.0
    a2[max(n - 2, 0):] = 0.0
    return a0, a1, a2, r


def mlpg_solve(a0, a1, a2, r):
    """L D L^T in ascending t, back-substitution in descending t: the header's order"""
    n, cols = a0.shape
    l1, l2, d, z = (np.zeros((n, cols)) for _ in range(4))
    with np.errstate(all="ignore"):
        for t in range(n):
            dt, zt = a0[t], r[t]
            if t >= 2:
                l2[t] = a2[t - 2] / d[t - 2]
            if t >= 1:
                num = a1[t - 1]
                if t >= 2:
                    num = a1[t - 1] - (l2[t] * d[t - 2]) * l1[t - 1]
                l1[t] = num / d[t - 1]
            if t >= 2:
                dt = dt - (l2[t] * l2[t]) * d[t - 2]
                zt = zt - l2[t] * z[t - 2]
            if t >= 1:
                dt = dt - (l1[t] * l1[t]) * d[t - 1]
                zt = zt - l1[t] * z[t - 1]
            d[t], z[t] = dt, zt
        c = np.zeros((n, cols))
        for t in range(n - 1, -1, -1):
            x = z[t] / d[t]
            if t + 1 < n:
                x = x - l1[t + 1] * c[t + 1]
            if t + 2 < n:
                x = x - l2[t + 2] * c[t + 2]
            c[t] = x
    return c


def mlpg(lengths, nd, n_ap, orders, mean, var, var_per_frame):
    """rows of means [frames, width] and of variances ([frames, width], or one row) -> static rows [frames, nd + 2 + n_ap]"""
    total, W = int(sum(lengths)), width(nd, n_ap, orders)
    mean = np.asarray(mean, dtype=np.float64).reshape(total, W)
    var = np.asarray(var, dtype=np.float64).reshape(total if var_per_frame else 1, W)
    cols, vuv_col = columns(nd, n_ap, orders)
    take = np.array(cols).T   # [orders, static columns]
    out = np.zeros((total, nd + 2 + n_ap))
    out_cols = [c if c <= nd else c + 1 for c in range(nd + 1 + n_ap)]
    o = 0
    for n in lengths:
        if n == 0:
            continue
        m = mean[o:o + n][:, take]
        v = var[o:o + n][:, take] if var_per_frame else np.broadcast_to(var[0][take], m.shape)
        c = mlpg_solve(*mlpg_system(m, v))
        with np.errstate(invalid="ignore"):
            bad = ~(v > 0.0)
        c[:, bad.any(axis=(0, 1))] = np.nan
        out[o:o + n][:, out_cols] = c
        out[o:o + n, nd + 1] = mean[o:o + n, vuv_col]
        o += n
    return out


def unpack(nd, n_ap, orders, rows, vuv_threshold, exps=None):
    """rows [frames, width] -> f0, coded sp [frames, nd], coded ap [frames, n_ap]"""
    rows = np.asarray(rows, dtype=np.float64)
    cols, vuv_col = columns(nd, n_ap, orders)
    with np.errstate(invalid="ignore", over="ignore"):
        on = rows[:, vuv_col] > vuv_threshold
        f0 = np.where(on, np.exp(rows[:, orders * nd]) if exps is None else exps, 0.0)
    return f0, rows[:, :nd].copy(), rows[:, [ks[0] for ks in cols[nd + 1:]]].reshape(len(rows), n_ap).copy()


def dense_system(mean, var):
    """W^T P W and W^T P mu of one static column: mean, var [n, orders] -- the windows as matrices, for the tests"""
    n, orders = mean.shape
    eye = np.eye(n)
    wins = [eye, 0.5 * (np.eye(n, k=1) - np.eye(n, k=-1)), np.eye(n, k=1) + np.eye(n, k=-1) - 2.0 * eye][:orders]
    Wm = np.concatenate(wins, axis=0)
    P = np.concatenate([1.0 / var[:, k] for k in range(orders)])
    mu = np.concatenate([mean[:, k] for k in range(orders)])
    return Wm.T @ (P[:, None] * Wm), Wm.T @ (P * mu)
