"""GMM conversion in front of MLPG: 64 utterances of 2000 frames (10 s at 5 ms) whose mgc block (orders 2: statics and deltas, dx = dy =
2 * nd) converts in place in MLPG's layout, at (dx, dy, n_mix) = (50, 50, 64) and (120, 120, 64), and one push of 512 frames at
(50, 50, 64).  The model is seeded and well conditioned (Sxx = I + G G^T / dx), the frames lie around its means; the kernels' time does
not depend on the values.  Every call is host-timed around a device synchronisation after two warm-up calls; median and spread (min,
max) of the timed calls in one JSON line, per shape:
  convert_ms          wc_gmm_convert_device writing mean, variance and best (the table of ll in the scratch), its kernels alone by the
                      library's timing events, and the fraction of the floor: n * n_mix * dx * (dx + 1) separate multiplies and adds at
                      half the 78.6 TFLOP/s vector peak
  convert_loglik_ms   the same with d_loglik handed out as well
  torch_ms            the same arithmetic in torch float64 on the same device (einsum for z, bmm for the mean), and its ratio
  mlpg_ms             wc_mlpg_device(var_per_frame = 1) on the converted rows, the call that follows
    python tools/gmm_probe.py [reps]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # for the inputs; imported before the library is loaded so that both use one HIP runtime

import world_class_amd as w
from world_class_amd import features as ft, gmm

L = w.lib()
L.wc_set_device(0)
reps = max(7, int(sys.argv[1])) if len(sys.argv) > 1 else 9
n_ap, orders, n_mix = 5, 2, 64
PEAK_NO_FMA = 0.5 * 78.6e12


def timed(fn, warm=2):
    for _ in range(warm):
        fn()
    L.wc_synchronize()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        L.wc_synchronize()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts))}


def kernel_ms(fn, names):
    L.wc_set_kernel_timing(1)
    fn()
    L.wc_synchronize()
    out = {n: float(L.wc_last_kernel_ms(n.encode())) for n in names}
    L.wc_set_kernel_timing(0)
    return out


def model(dx, dy, seed):
    rng = np.random.default_rng(seed)
    mux, muy = rng.normal(size=(n_mix, dx)), rng.normal(size=(n_mix, dy))
    G = rng.normal(size=(n_mix, dx, dx))
    sxx = np.eye(dx)[None] + G @ G.transpose(0, 2, 1) / dx
    syx = 0.05 * rng.normal(size=(n_mix, dy, dx))
    syy = np.full((n_mix, dy), 1.0 + float(np.max(np.sum(syx * syx, axis=2))))     # (Sxx >= I: Syx Sxx^-1 Sxy <= Syx Sxy)
    mean, cov = gmm.joint_from_blocks(mux, muy, sxx, syx, syy)
    return rng.uniform(0.5, 1.5, size=n_mix), mean, cov


def torch_convert(c, Wm, B, cvar, mux, muy, x, step=16000):
    """the same arithmetic, a chunk of frames at a time: d, z = W d (einsum), q, ll, argmax, mean = muy + B z (bmm)"""
    means, bests = [], []
    for o in range(0, x.shape[0], step):
        d = x[o:o + step, None, :] - mux[None]
        zz = torch.einsum("mik,nmk->nmi", Wm, d)
        ll = c[None] - 0.5 * (zz * zz).sum(dim=2)
        best = ll.argmax(dim=1)
        zb = zz[torch.arange(zz.shape[0], device=zz.device), best]
        means.append(muy[best] + torch.bmm(B[best], zb[:, :, None])[:, :, 0])
        bests.append(best)
    best = torch.cat(bests)
    return torch.cat(means), cvar[best], best


def shape(nd, lengths, seed):
    dx = dy = orders * nd
    n = int(sum(lengths))
    weight, mean, cov = model(dx, dy, seed)
    g = gmm.Gmm(weight, mean, cov, dx)
    W, W1 = ft.width(nd, n_ap, orders), ft.width(nd, n_ap, 1)
    rng = np.random.default_rng(seed + 1)
    rows = rng.standard_normal((n, W))
    rows[:, :dx] = mean[rng.integers(0, n_mix, size=n), :dx] + 0.7 * rng.standard_normal((n, dx))
    d_rows = torch.from_numpy(rows.ravel()).cuda()
    d_mean, d_var = d_rows.clone(), torch.full((n * W,), 0.25, dtype=torch.float64, device="cuda")
    d_best = torch.empty(n, dtype=torch.int32, device="cuda")
    d_ll = torch.empty(n * n_mix, dtype=torch.float64, device="cuda")
    d_static = torch.empty(n * W1, dtype=torch.float64, device="cuda")
    res = {"workload": f"{len(lengths)} x {lengths[0]} frames, dx {dx}, dy {dy}, n_mix {n_mix}, rows of {W} doubles"}
    conv = lambda: g.convert(n, d_rows, W, d_mean, d_var, W, d_best=d_best)
    res["convert_ms"] = timed(conv)
    res["convert_kernels_ms"] = kernel_ms(conv, ("gmm_ll_kernel", "gmm_pick_kernel"))
    floor_ms = n * n_mix * dx * (dx + 1) / PEAK_NO_FMA * 1e3
    res["floor_ms"] = floor_ms
    res["fraction_of_floor"] = {"call": floor_ms / res["convert_ms"]["median"], "gmm_ll_kernel": floor_ms / res["convert_kernels_ms"]["gmm_ll_kernel"]}
    res["convert_loglik_ms"] = timed(lambda: g.convert(n, d_rows, W, d_mean, d_var, W, d_best=d_best, d_loglik=d_ll))
    c, Wm, B, cvar = (torch.from_numpy(a).cuda() for a in g.prepared())
    mux, muy = torch.from_numpy(mean[:, :dx].copy()).cuda(), torch.from_numpy(mean[:, dx:].copy()).cuda()
    x = d_rows.view(n, W)[:, :dx].contiguous()
    res["torch_ms"] = timed(lambda: torch_convert(c, Wm, B, cvar, mux, muy, x))
    res["torch_over_convert"] = res["torch_ms"]["median"] / res["convert_ms"]["median"]
    t_mean, t_var, t_best = torch_convert(c, Wm, B, cvar, mux, muy, x)
    conv()
    L.wc_synchronize()
    res["best_agrees_with_torch"] = float((t_best.to(torch.int32) == d_best).double().mean())
    res["mean_max_diff_to_torch"] = float((t_mean - d_mean.view(n, W)[:, :dx]).abs().max())
    res["mlpg_ms"] = timed(lambda: ft.mlpg(lengths, nd, n_ap, orders, d_mean, d_var, d_static, var_per_frame=True))
    res["finite"] = bool(torch.isfinite(d_static).all())
    g.close()
    return res


out = {"library": os.path.relpath(w.LIB_PATH), "reps": reps,
       "batch_50": shape(25, [2000] * 64, 1), "batch_120": shape(60, [2000] * 64, 2), "push_512_50": shape(25, [512], 3)}
L.wc_release_scratch()
print(json.dumps(out))
