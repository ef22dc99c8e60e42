"""Model features at the shape DESIGN.md section 10 reports: 64 utterances of 2000 frames (10 s at 5 ms), nd 60, n_ap 5, orders 3.  The
contour is voiced in seeded runs with unvoiced gaps between them; the coded rows are seeded noise (the kernels' time does not depend on
the values).  Every figure is the median of host-timed calls around a device synchronisation, after warm-up calls; prints one JSON line:
  pack_<fmt>_ms, pack_<fmt>_gbps     wc_pack_model_features_device and the bytes it must move (inputs read once, rows written once)
                                     per second -- to be held against the HBM rate and against copy_<fmt>_ms, a plain copy_ of as many
  lf0_/pack_kernel_ms                its two kernels in one more call, by the library's timing events
  mlpg_<global|per_frame>_ms         wc_mlpg_device with one row of variances and with one per frame, and its kernel alone
  unpack_ms                          wc_unpack_model_features_device of the static rows
    python tools/features_probe.py [n_utt] [reps] [frames]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # for the inputs and the plain copy; imported before the library is loaded so that both use one HIP runtime

import world_class_amd as w
from world_class_amd import features as ft

L = w.lib()
L.wc_set_device(0)
n_utt = int(sys.argv[1]) if len(sys.argv) > 1 else 64
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
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
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def kernel_ms(fn, names):
    L.wc_set_kernel_timing(1)
    fn()
    L.wc_synchronize()
    out = {n: float(L.wc_last_kernel_ms(n.encode())) for n in names}
    L.wc_set_kernel_timing(0)
    return out


rng = np.random.default_rng(2000)
tot, lengths = n_utt * frames, [frames] * n_utt
voiced = (np.cumsum(rng.uniform(size=tot) < 0.02) % 2) == 0   # runs of about 50 frames
f0 = np.where(voiced, rng.uniform(80.0, 400.0, tot), 0.0)
cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
d_f0, d_sp, d_ap = cuda(f0), cuda(rng.standard_normal(tot * nd)), cuda(-rng.uniform(0.0, 40.0, tot * n_ap))
W, W1 = ft.width(nd, n_ap, orders), ft.width(nd, n_ap, 1)
res = {"library": os.path.relpath(w.LIB_PATH), "reps": reps, "workload": f"{n_utt} x {frames} frames, nd {nd}, n_ap {n_ap}, orders {orders}",
       "voiced_share": float(voiced.mean())}

rows = {}
for fmt, tdt, esz in (("f64", torch.float64, 8), ("f32", torch.float32, 4)):
    rows[fmt] = torch.empty(tot * W, dtype=tdt, device="cuda")
    call = lambda: ft.pack(lengths, nd, n_ap, orders, d_f0, d_sp, d_ap, rows[fmt], 0.0, fmt)
    moved = 8 * tot * (1 + nd + n_ap) + esz * tot * W
    res[f"pack_{fmt}_ms"] = timed(call)
    res[f"pack_{fmt}_moved_gb"] = moved / 1e9
    res[f"pack_{fmt}_gbps"] = moved / 1e6 / res[f"pack_{fmt}_ms"]
    for k, v in kernel_ms(call, ("feat_lf0_kernel", "feat_pack_kernel")).items():
        res[f"{k}_{fmt}_ms"] = v
    c_src = torch.zeros(moved // 16, dtype=torch.float64, device="cuda")
    c_dst = torch.empty_like(c_src)
    res[f"copy_{fmt}_ms"] = timed(lambda: c_dst.copy_(c_src))
    del c_src, c_dst

d_static = torch.empty(tot * W1, dtype=torch.float64, device="cuda")
d_var_row = torch.full((W,), 0.5, dtype=torch.float64, device="cuda")
d_var = torch.full((tot * W,), 0.5, dtype=torch.float64, device="cuda")
for name, var, per_frame in (("global", d_var_row, False), ("per_frame", d_var, True)):
    call = lambda: ft.mlpg(lengths, nd, n_ap, orders, rows["f64"], var, d_static, per_frame)
    res[f"mlpg_{name}_ms"] = timed(call)
    res[f"mlpg_{name}_kernel_ms"] = kernel_ms(call, ("mlpg_kernel",))["mlpg_kernel"]
res["mlpg_scratch_gb"] = 24 * tot * (nd + 1 + n_ap) / 1e9
o = [torch.empty(tot * k, dtype=torch.float64, device="cuda") for k in (1, nd, n_ap)]
res["unpack_ms"] = timed(lambda: ft.unpack(tot, nd, n_ap, 1, d_static, o[0], o[1], o[2]))
L.wc_release_scratch()
print(json.dumps(res))
