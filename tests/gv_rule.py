"""THE rule of include/world_class_gv.h in numpy, on top of features_rule.mlpg_system: the fixed-order sum, stat, the banded product,
the variance-scaling start and the Newton-like ascent steps with a global-variance term, every operation in float64 and rounded on its
own in the order the header states -- the device equals this bit for bit.  One utterance at a time, every static column at once."""
import numpy as np

import features_rule as fr

_LANES = np.arange(64)


def gv_sum(x):
    """THE sum over axis 0 of x [n] or [n, cols]: lane l adds x(l), x(l + 64), ... in ascending t to a partial that starts at +0.0
    (a partial never is -0.0, so a term that is left out is a term of +0.0), then p[l] + p[l ^ off] for off = 32 ... 1"""
    x = np.asarray(x, dtype=np.float64)
    p = np.zeros((64,) + x.shape[1:])
    with np.errstate(all="ignore"):
        for k in range(0, x.shape[0], 64):
            blk = x[k:k + 64]
            p[:len(blk)] = p[:len(blk)] + blk
        for off in (32, 16, 8, 4, 2, 1):
            p = p + p[_LANES ^ off]
    return p[0]


def stat(c, m):
    """c [n, cols], m [n] bool -> mean [cols], d [n, cols], v [cols], N"""
    c = np.asarray(c, dtype=np.float64)
    on = np.asarray(m, dtype=bool)[:, None]
    N = np.float64(np.count_nonzero(m))
    with np.errstate(all="ignore"):
        mean = gv_sum(np.where(on, c, 0.0)) / N
        d = np.where(on, c - mean, 0.0)
        v = gv_sum(d * d) / N
    return mean, d, v, N


def banded(a0, a1, a2, c):
    """(A c)(t), a term with an index outside [0, n) a +0.0"""
    z = lambda: np.zeros_like(c)
    m2, m1, p1, p2 = z(), z(), z(), z()
    with np.errstate(all="ignore"):
        m2[2:] = a2[:-2] * c[:-2]
        m1[1:] = a1[:-1] * c[:-1]
        p1[:-1] = a1[:-1] * c[1:]
        p2[:-2] = a2[:-2] * c[2:]
        return ((m2 + m1) + a0 * c) + (p1 + p2)


def objective(a0, a1, a2, r, c, m, orders, gv_mean, gv_var, w_ml, w_gv):
    """J of the header for c [n, cols]"""
    _, _, v, _ = stat(c, m)
    with np.errstate(all="ignore"):
        omega = np.float64(w_ml) / np.float64(orders * len(c))
        e = v - gv_mean
        return omega * gv_sum(c * (r - 0.5 * banded(a0, a1, a2, c))) - (0.5 * w_gv) * ((e * e) * (1.0 / gv_var))


def refine(system, c, m, orders, gv_mean, gv_var, w_ml=1.0, w_gv=1.0, step_init=0.1, max_iter=5, ratios=None, trace=None):
    """one utterance: system = (a0, a1, a2, r) [n, cols] (None with max_iter == 0), c [n, cols] the MLPG statics, m [n] bool ->
    the refined c.  ratios: the start's sqrt as another library gave it [cols].  trace: a list that receives one dict per step
    (J, step as it was used, v) and a last one with the v of the result"""
    c = np.array(c, dtype=np.float64)
    n, S = c.shape
    m = np.ones(n, dtype=bool) if m is None else np.asarray(m, dtype=bool)
    gv_mean, gv_var = np.asarray(gv_mean, dtype=np.float64), np.asarray(gv_var, dtype=np.float64)
    w_ml, w_gv = np.float64(w_ml), np.float64(w_gv)
    out = c.copy()
    with np.errstate(all="ignore"):
        off = np.isposinf(gv_var)
        bad = ~off & (~(gv_var > 0.0) | ~(gv_mean > 0.0) | np.isposinf(gv_mean))
        out[np.ix_(m, bad)] = np.nan
        N = np.float64(np.count_nonzero(m))
        if n == 0 or N < 2.0:
            return out
        mean, d, v, _ = stat(c, m)
        live = ~off & ~bad & (v > 0.0)
        ratio = np.sqrt(gv_mean / v) if ratios is None else np.asarray(ratios, dtype=np.float64)
        on = m[:, None]
        cur = np.where(on, ratio * d + mean, c)
        if max_iter > 0:
            a0, a1, a2, r = system
            pv = 1.0 / gv_var
            omega = w_ml / np.float64(orders * n)
            step = np.full(S, np.float64(step_init))
            J_prev = None
            for it in range(1, max_iter + 1):
                mean, d, v, _ = stat(cur, m)
                Ac = banded(a0, a1, a2, cur)
                e = v - gv_mean
                J = omega * gv_sum(cur * (r - 0.5 * Ac)) - (0.5 * w_gv) * ((e * e) * pv)
                if it > 1:
                    step = np.where(J < J_prev, step * 0.5, np.where(J > J_prev, step * 1.2, step))
                h = omega * a0 + (w_gv * (2.0 / (N * N))) * (((N - 1.0) * pv) * e + (2.0 * pv) * (d * d))
                g = (omega * (r - Ac) - ((w_gv * (2.0 / N)) * (pv * e)) * d) / h
                if trace is not None:
                    trace.append({"J": J.copy(), "step": step.copy(), "v": v.copy(), "h": h.copy(), "g": g.copy()})
                cur = np.where(on, cur + step * g, cur)
                J_prev = J
        if trace is not None:
            trace.append({"v": stat(cur, m)[2]})
        out[:, live] = cur[:, live]
    return out


def _static_columns(nd, n_ap):
    return [c if c <= nd else c + 1 for c in range(nd + 1 + n_ap)]


def _masks(lengths, mask):
    total = int(sum(lengths))
    return np.ones(total, dtype=bool) if mask is None else np.asarray(mask).reshape(total) != 0


def stats(lengths, nd, n_ap, static, mask=None):
    """static rows [frames, nd + 2 + n_ap] -> mean, v [n_utt, S] over the masked frames"""
    total, cols = int(sum(lengths)), _static_columns(nd, n_ap)
    static = np.asarray(static, dtype=np.float64).reshape(total, nd + 2 + n_ap)
    m = _masks(lengths, mask)
    mean, var = np.zeros((len(lengths), len(cols))), np.zeros((len(lengths), len(cols)))
    o = 0
    for u, n in enumerate(lengths):
        mean[u], _, var[u], _ = stat(static[o:o + n][:, cols], m[o:o + n])
        o += n
    return mean, var


def mlpg_gv(lengths, nd, n_ap, orders, mean, var, var_per_frame, gv_mean, gv_var, mask, static, w_ml=1.0, w_gv=1.0, step_init=0.1,
            max_iter=5, traces=None):
    """the static rows of fr.mlpg on the same means and variances -> the refined static rows"""
    total, cols = int(sum(lengths)), _static_columns(nd, n_ap)
    out = np.array(static, dtype=np.float64).reshape(total, nd + 2 + n_ap)
    m = _masks(lengths, mask)
    if max_iter > 0:
        W = fr.width(nd, n_ap, orders)
        mean = np.asarray(mean, dtype=np.float64).reshape(total, W)
        var = np.asarray(var, dtype=np.float64).reshape(total if var_per_frame else 1, W)
        take = np.array(fr.columns(nd, n_ap, orders)[0]).T   # [orders, static columns]
    o = 0
    for n in lengths:
        if n > 0:
            system = None
            if max_iter > 0:
                mu = mean[o:o + n][:, take]
                with np.errstate(all="ignore"):
                    system = fr.mlpg_system(mu, var[o:o + n][:, take] if var_per_frame else np.broadcast_to(var[0][take], mu.shape))
            trace = None if traces is None else []
            out[o:o + n, cols] = refine(system, out[o:o + n][:, cols], m[o:o + n], orders, gv_mean, gv_var, w_ml, w_gv, step_init, max_iter,
                                        trace=trace)
            if traces is not None:
                traces.append(trace)
        o += n
    return out
