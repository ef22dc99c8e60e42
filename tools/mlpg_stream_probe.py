"""MLPG streams at the shape DESIGN.md section 10 reports: 512 streams, nd 60, n_ap 5, orders 3; lags 8, 32 and 64; 1 and 4 rows per
push; one row of variances and variances per frame.  The rows are seeded noise (the kernels' time does not depend on the values).
Every stream is first fed past its lag, so that every timed push emits as many frames as it takes rows.  Every figure is the median
of host-timed calls around a device synchronisation, after warm-up calls; prints one JSON line:
  push_L<lag>_k<rows>_<global|per_frame>_ms   wc_mlpg_stream_push_device for all streams
  ..._forward_ms, ..._back_ms                 its two kernels in one more call, by the library's timing events
  ..._of_whole                                the push as a share of whole_<...>_ms
  ..._of_period                               the push as a share of the frame period it serves (5 ms per row)
  flush_L<lag>_ms                             wc_mlpg_stream_flush_device for all streams
  whole_<global|per_frame>_ms                 the only other way to the same values: wc_mlpg_device on the whole prefix at every
                                              push, timed for n_streams prefixes of `frames` rows
    python tools/mlpg_stream_probe.py [n_streams] [reps] [frames]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # for the inputs; imported before the library is loaded so that both use one HIP runtime

import world_class_amd as w
from world_class_amd import features as ft
from world_class_amd import mlpg_stream

L = w.lib()
L.wc_set_device(0)
n_streams = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
frames = int(sys.argv[3]) if len(sys.argv) > 3 else 2000
nd, n_ap, orders = 60, 5, 3
MAX_ROWS, MAX_LAG, PERIOD_MS = 4, 64, 5.0


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


W, W1 = ft.width(nd, n_ap, orders), ft.width(nd, n_ap, 1)
gen = torch.Generator(device="cuda").manual_seed(2000)
res = {"library": os.path.relpath(w.LIB_PATH), "reps": reps,
       "workload": f"{n_streams} streams, nd {nd}, n_ap {n_ap}, orders {orders}, at most {MAX_ROWS} rows per push; whole: {frames} rows"}

# the alternative: the whole call on every prefix
tot = n_streams * frames
d_mean = torch.randn(tot * W, dtype=torch.float64, device="cuda", generator=gen)
d_var_row = torch.full((W,), 0.5, dtype=torch.float64, device="cuda")
d_whole = torch.empty(tot * W1, dtype=torch.float64, device="cuda")
for name, per_frame in (("global", False), ("per_frame", True)):
    var = torch.full((tot * W,), 0.5, dtype=torch.float64, device="cuda") if per_frame else d_var_row
    res[f"whole_{name}_ms"] = timed(lambda: ft.mlpg([frames] * n_streams, nd, n_ap, orders, d_mean, var, d_whole, per_frame))
    del var
del d_whole
L.wc_release_scratch()

h = mlpg_stream.MlpgStream(n_streams, nd, n_ap, orders, MAX_ROWS, MAX_LAG)
d_var = torch.full((n_streams * MAX_ROWS * W,), 0.5, dtype=torch.float64, device="cuda")
d_static = torch.empty(n_streams * max(MAX_ROWS, MAX_LAG) * W1, dtype=torch.float64, device="cuda")
torch.cuda.synchronize()
for lag in (8, 32, 64):
    for k in (1, 4):
        for name, per_frame in (("global", False), ("per_frame", True)):
            for u in range(n_streams):
                h.reset(u, lag)
            for _ in range(lag // MAX_ROWS):   # past the lag: from here on every row emits a frame
                h.push_device([MAX_ROWS] * n_streams, d_mean, d_var, d_static, True)
            call = lambda: h.push_device([k] * n_streams, d_mean, d_var if per_frame else d_var_row, d_static, per_frame)
            assert call() == [k] * n_streams
            key = f"push_L{lag}_k{k}_{name}"
            res[key + "_ms"] = timed(call)
            for kn, v in kernel_ms(call, ("mlpg_stream_forward_kernel", "mlpg_stream_back_kernel")).items():
                res[key + ("_forward_ms" if "forward" in kn else "_back_ms")] = v
            res[key + "_of_whole"] = res[key + "_ms"] / res[f"whole_{name}_ms"]
            res[key + "_of_period"] = res[key + "_ms"] / (k * PERIOD_MS)
    flush_ms = []
    for _ in range(reps):   # a flush ends its streams: each one is timed on streams fed anew
        for u in range(n_streams):
            h.reset(u, lag)
        for _ in range(lag // MAX_ROWS):
            h.push_device([MAX_ROWS] * n_streams, d_mean, d_var, d_static, True)
        L.wc_synchronize()
        t0 = time.perf_counter()
        assert h.flush_device([1] * n_streams, d_static) == [lag] * n_streams
        L.wc_synchronize()
        flush_ms.append((time.perf_counter() - t0) * 1e3)
    res[f"flush_L{lag}_ms"] = float(np.median(flush_ms))
res["ring_mb"] = 8 * (4 * (nd + 1 + n_ap) + 1) * (MAX_LAG + MAX_ROWS + 1) * n_streams / 1e6
h.close()
print(json.dumps(res))
