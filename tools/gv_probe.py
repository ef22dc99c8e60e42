"""Global-variance parameter generation at the shape of tools/features_probe.py: 64 utterances of 2000 frames (10 s at 5 ms), nd 60,
n_ap 5, orders 3, one row of variances; the model is seeded noise (the kernels' time does not depend on the values: every column is on
and no utterance leaves early).  Every call is host-timed around a device synchronisation after warm-up calls; median and spread
(min, max) of the timed calls in one JSON line:
  mlpg_ms                    wc_mlpg_device, the call the refinement follows, from the same run
  gv_iter<k>_ms              wc_mlpg_gv_device at max_iter k (0: the variance-scaling post-filter alone; 5: the default), with its
                             ratio to mlpg_ms, and its kernels alone by the library's timing events
  gv_iter5_mask_ms           the same with a mask of 70 % of the frames
  stats_ms                   wc_gv_stats_device
    python tools/gv_probe.py [n_utt] [reps] [frames]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # for the inputs; imported before the library is loaded so that both use one HIP runtime

import world_class_amd as w
from world_class_amd import features as ft, gv

L = w.lib()
L.wc_set_device(0)
n_utt = int(sys.argv[1]) if len(sys.argv) > 1 else 64
reps = max(7, int(sys.argv[2])) if len(sys.argv) > 2 else 9
frames = int(sys.argv[3]) if len(sys.argv) > 3 else 2000
nd, n_ap, orders = 60, 5, 3


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


rng = np.random.default_rng(2000)
tot, lengths = n_utt * frames, [frames] * n_utt
S, W, W1 = nd + 1 + n_ap, ft.width(nd, n_ap, orders), ft.width(nd, n_ap, 1)
cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
d_mean = cuda(rng.standard_normal(tot * W))
d_var = torch.full((W,), 0.05, dtype=torch.float64, device="cuda")
d_gm, d_gvv = torch.full((S,), 1.5, dtype=torch.float64, device="cuda"), torch.full((S,), 0.2, dtype=torch.float64, device="cuda")
d_mask = cuda((rng.uniform(size=tot) < 0.7).astype(np.uint8))
d_ml = torch.empty(tot * W1, dtype=torch.float64, device="cuda")
d_static = torch.empty_like(d_ml)
d_m, d_v = torch.empty(n_utt * S, dtype=torch.float64, device="cuda"), torch.empty(n_utt * S, dtype=torch.float64, device="cuda")
res = {"library": os.path.relpath(w.LIB_PATH), "reps": reps, "workload": f"{n_utt} x {frames} frames, nd {nd}, n_ap {n_ap}, orders {orders}"}

mlpg = lambda: ft.mlpg(lengths, nd, n_ap, orders, d_mean, d_var, d_ml)
res["mlpg_ms"] = timed(mlpg)
res["mlpg_kernel_ms"] = kernel_ms(mlpg, ("mlpg_kernel",))["mlpg_kernel"]
res["copy_ms"] = timed(lambda: d_static.copy_(d_ml))   # every refinement below starts from MLPG's rows: this copy is inside its time


def refine(max_iter, mask=None):
    d_static.copy_(d_ml)
    torch.cuda.synchronize()
    gv.mlpg_gv(lengths, nd, n_ap, orders, d_mean, d_var, d_gm, d_gvv, d_static, mask, max_iter=max_iter)


for k in (0, 1, 5):
    res[f"gv_iter{k}_ms"] = timed(lambda: refine(k))
    res[f"gv_iter{k}_ms"]["less_copy_over_mlpg"] = (res[f"gv_iter{k}_ms"]["median"] - res["copy_ms"]["median"]) / res["mlpg_ms"]["median"]
    res[f"gv_iter{k}_kernels_ms"] = kernel_ms(lambda: refine(k), ("gv_system_kernel", "gv_refine_kernel"))
res["gv_iter5_mask_ms"] = timed(lambda: refine(5, d_mask))
res["stats_ms"] = timed(lambda: gv.stats(lengths, nd, n_ap, d_static, d_m, d_v))
res["stats_kernel_ms"] = kernel_ms(lambda: gv.stats(lengths, nd, n_ap, d_static, d_m, d_v), ("gv_stats_kernel",))["gv_stats_kernel"]
res["finite"] = bool(torch.isfinite(d_static).all())
res["gv_scratch_gb"] = 32 * tot * S / 1e9
L.wc_release_scratch()
print(json.dumps(res))
