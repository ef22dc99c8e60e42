"""THE rule of include/world_class_gmm_train.h in numpy and Python floats, in exactly the header's order.

As in gmm_rule.py, numpy only carries many elements through the header's sequence of operations side by side; an elementwise float64
*, +, -, / or sqrt is the correctly rounded IEEE operation.  The sums over frames are Python loops over the live frames, ascending,
that start at their first term.  exp and log are math.exp and math.log (libm): the one place where the device may differ."""
import math

import numpy as np

import gmm_rule as gm

SEGMENT = 1024


def tri(D):
    """the (i, j) of the packed lower triangle, row by row"""
    return np.tril_indices(D)


def factor(cov):
    """cov [n_mix, D, D] (lower triangles read) -> L, W (upper parts 0.0) and bad [n_mix]: the first row whose Cholesky diagonal is not
    > 0 or not finite, -1 where there is none.  create's rule of world_class_gmm.h with dx := D"""
    cov = np.asarray(cov, dtype=np.float64)
    n_mix, D = cov.shape[0], cov.shape[1]
    with np.errstate(all="ignore"):
        L = np.zeros((n_mix, D, D))
        diag_s = np.zeros((n_mix, D))
        for j in range(D):
            s = cov[:, j:, j].copy()
            for k in range(j):
                s = s - L[:, j:, k] * L[:, j, k][:, None]
            diag_s[:, j] = s[:, 0]
            L[:, j, j] = np.sqrt(s[:, 0])
            L[:, j + 1:, j] = s[:, 1:] / L[:, j, j][:, None]
        W = np.zeros((n_mix, D, D))
        for i in range(D):
            W[:, i, i] = 1.0 / L[:, i, i]
        for i in range(1, D):
            s = L[:, i, :i] * np.stack([W[:, j, j] for j in range(i)], axis=1)
            for k in range(1, i):
                s[:, :k] = s[:, :k] + L[:, i, k][:, None] * W[:, k, :k]
            W[:, i, :i] = -s / L[:, i, i][:, None]
    wrong = ~((diag_s > 0.0) & np.isfinite(diag_s))
    bad = np.where(wrong.any(axis=1), np.argmax(wrong, axis=1), -1)
    return L, W, bad


def constant(weight, L):
    D = L.shape[0]
    ld = math.log(float(L[0, 0]))
    for i in range(1, D):
        ld = ld + math.log(float(L[i, i]))
    return (math.log(float(weight)) - ld) - (0.5 * float(D)) * gm.LOG_2PI


def prepare(weight, mean, cov):
    """the joint preparation -> dict(W, c, mux) that gmm_rule.loglik takes with the joint rows as x.  A refusal raises ValueError"""
    weight = np.asarray(weight, dtype=np.float64).ravel()
    n_mix = weight.size
    mean = np.asarray(mean, dtype=np.float64).reshape(n_mix, -1)
    D = mean.shape[1]
    cov = np.asarray(cov, dtype=np.float64).reshape(n_mix, D, D)
    low = np.tril(np.ones((D, D), dtype=bool))
    for m in range(n_mix):
        if not (weight[m] > 0.0 and math.isfinite(weight[m])):
            raise ValueError("mixture %d: a weight that is not finite or not > 0" % m)
        for i in range(D):
            if not math.isfinite(mean[m, i]):
                raise ValueError("mixture %d, row %d: a mean that is not finite" % (m, i))
            if not np.isfinite(cov[m, i][low[i]]).all():
                raise ValueError("mixture %d, row %d: a covariance entry that is not finite" % (m, i))
    L, W, bad = factor(cov)
    for m in range(n_mix):
        if bad[m] >= 0:
            raise ValueError("mixture %d, row %d: the joint covariance is not positive definite" % (m, bad[m]))
    c = np.array([constant(weight[m], L[m]) for m in range(n_mix)])
    return dict(W=W, c=c, mux=mean.copy())


def posteriors(prepared, rows, mask=None, exp=math.exp, log=math.log):
    """rows [n, D] -> gamma [n, n_mix], frame_ll [n], state [n] (0 masked, 1 live, 2 dropped), and (top [n], log s [n]) of the live frames
    (0.0 elsewhere) for the tests' bounds"""
    ll, _, _ = gm.loglik(prepared, rows)
    n, n_mix = ll.shape
    gamma, frame_ll, state = np.zeros((n, n_mix)), np.zeros(n), np.zeros(n, dtype=np.uint8)
    tops, logs = np.zeros(n), np.zeros(n)
    for t in range(n):
        if mask is not None and mask[t] == 0:
            continue
        top = None
        for m in range(n_mix):
            v = float(ll[t, m])
            if v == v and (top is None or v > top):
                top = v
        if top is None or not math.isfinite(top):
            state[t] = 2
            continue
        state[t] = 1
        e = [0.0 if ll[t, m] != ll[t, m] else (0.0 if ll[t, m] == -math.inf else exp(float(ll[t, m]) - top)) for m in range(n_mix)]
        s = e[0]
        for m in range(1, n_mix):
            s = s + e[m]
        for m in range(n_mix):
            gamma[t, m] = e[m] / s
        tops[t], logs[t] = top, log(s)
        frame_ll[t] = top + logs[t]
    return gamma, frame_ll, state, (tops, logs)


def statistics(rows, mean, gamma, frame_ll, live, cuts=None, start=None):
    """the totals of THE rule: rows [n, D] (read only where live), mean [n_mix, D] of the model in force, gamma [n, n_mix], frame_ll [n],
    live [n] bool -> dict(N [n_mix], S1 [n_mix, D], S2 [n_mix, D(D+1)/2], LL, n_live).  cuts: the lengths of the calls the frames came
    in (every call starts new segments); start: totals to go on from"""
    rows = np.asarray(rows, dtype=np.float64)
    n, D = rows.shape
    n_mix = mean.shape[0]
    ii, jj = tri(D)
    tot = start or dict(N=np.zeros(n_mix), S1=np.zeros((n_mix, D)), S2=np.zeros((n_mix, ii.size)), LL=0.0, n_live=0)
    tot = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in tot.items()}
    cuts = [n] if cuts is None else list(cuts)
    assert sum(cuts) == n
    o = 0
    with np.errstate(all="ignore"):
        for length in cuts:
            for a in range(o, o + length, SEGMENT):
                b = min(a + SEGMENT, o + length)
                N = S1 = S2 = LL = None
                for t in range(a, b):
                    if not live[t]:
                        continue
                    d = rows[t][None, :] - mean                       # [n_mix, D]
                    g = gamma[t][:, None] * d
                    t2 = g[:, ii] * d[:, jj]                          # [n_mix, packed]
                    if N is None:
                        N, S1, S2, LL = gamma[t].copy(), g, t2, float(frame_ll[t])
                    else:
                        N, S1, S2, LL = N + gamma[t], S1 + g, S2 + t2, LL + float(frame_ll[t])
                if N is None:
                    N, S1, S2, LL = np.zeros(n_mix), np.zeros((n_mix, D)), np.zeros((n_mix, ii.size)), 0.0
                tot["N"], tot["S1"], tot["S2"], tot["LL"] = tot["N"] + N, tot["S1"] + S1, tot["S2"] + S2, tot["LL"] + LL
            o += length
    tot["n_live"] += int(np.count_nonzero(live))
    return tot


def update(weight, mean, cov, tot, min_occupancy=1.0, floor=None):
    """the M-step -> (weight, mean, cov) of the new model (both triangles), n_starved, n_kept"""
    weight, mean, cov = np.array(weight, dtype=np.float64), np.array(mean, dtype=np.float64), np.array(cov, dtype=np.float64)
    n_mix, D = mean.shape
    ii, jj = tri(D)
    n_live = float(tot["n_live"])
    n_starved = n_kept = 0
    with np.errstate(all="ignore"):
        for m in range(n_mix):
            Nm = float(tot["N"][m])
            if not Nm >= min_occupancy:
                n_starved += 1
                continue
            w = Nm / n_live
            delta = tot["S1"][m] / Nm
            new_mean = mean[m] + delta
            packed = tot["S2"][m] / Nm - delta[ii] * delta[jj]
            new_cov = np.zeros((D, D))
            new_cov[ii, jj] = packed
            if floor is not None:
                f = np.asarray(floor, dtype=np.float64)
                dg = np.diag(new_cov).copy()
                dg[dg < f] = f[dg < f]
                new_cov[np.arange(D), np.arange(D)] = dg
            new_cov[jj, ii] = new_cov[ii, jj]
            fine = w > 0.0 and math.isfinite(w) and np.isfinite(new_mean).all() and np.isfinite(new_cov).all()
            if not fine or factor(new_cov[None])[2][0] >= 0:
                n_kept += 1
                continue
            weight[m], mean[m], cov[m] = w, new_mean, new_cov
    return weight, mean, cov, n_starved, n_kept


def iterate(weight, mean, cov, rows, iters, mask=None, min_occupancy=1.0, floor=None):
    """iters iterations of EM by the rule with libm -> the model after them and the list of every iteration's loglik"""
    out = []
    for _ in range(iters):
        gamma, fll, state, _ = posteriors(prepare(weight, mean, cov), rows, mask)
        tot = statistics(rows, np.asarray(mean, dtype=np.float64), gamma, fll, state == 1)
        out.append(tot["LL"])
        weight, mean, cov, _, _ = update(weight, mean, cov, tot, min_occupancy, floor)
    return (weight, mean, cov), out


def planted(n=3000, D=4, n_mix=3, seed=12):
    """the planted-mixture fixture: n frames from n_mix well-spread Gaussians, and a deliberately poor start (the first frames as
    means, the global diagonal covariance, equal weights)"""
    rng = np.random.default_rng(seed)
    centres = 3.0 * rng.normal(size=(n_mix, D))
    which = rng.integers(0, n_mix, size=n)
    rows = centres[which] + rng.normal(size=(n, D)) * (0.5 + 0.5 * rng.random(size=(n_mix, D)))[which]
    start = (np.full(n_mix, 1.0 / n_mix), rows[:n_mix].copy(), np.tile(np.diag(rows.var(axis=0)), (n_mix, 1, 1)))
    return rows, start


def planted_pair(n=2000, dx=6, dy=6, n_mix=4, seed=21):
    """source rows from n_mix Gaussians and target rows that are a planted affine map of the source, one per mixture, plus noise
    -> joint rows [n, dx + dy]"""
    rng = np.random.default_rng(seed)
    centres = 4.0 * rng.normal(size=(n_mix, dx))
    which = rng.integers(0, n_mix, size=n)
    x = centres[which] + 0.6 * rng.normal(size=(n, dx))
    A = rng.normal(size=(n_mix, dy, dx)) / math.sqrt(dx)
    b = 2.0 * rng.normal(size=(n_mix, dy))
    y = np.einsum("nji,ni->nj", A[which], x) + b[which] + 0.05 * rng.normal(size=(n, dy))
    return np.concatenate([x, y], axis=1)
