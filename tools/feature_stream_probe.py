"""Feature streams at the shapes DESIGN.md section 10 reports: nd 60, n_ap 5, orders 3, lag 64; 512 streams x 1 row and 64 streams x
8 rows per push; rows of doubles and of floats.  The inputs are seeded noise with unvoiced gaps (the kernels' time does not depend
on the values).  Every stream is first fed past its lag, so that every timed push emits as many rows as it takes.  Every figure is
the median of host-timed windows of INNER calls that end in a device synchronisation, after warm-up calls, per call; prints one JSON
line:
  feat_<n>x<k>_<f64|f32>_ms             wc_feature_stream_push_device for all streams
  ..._scan_ms, ..._pack_ms              its two kernels in one more call, by the library's timing events
  ..._hbm_us                            the time HBM would take for the bytes the push moves, at the 6.3 TB/s a copy achieves
  ..._bytes                             those bytes, counted from the shapes (bytes_of_push below)
  mlpg_<n>x<k>_<global|per_frame>_ms    wc_mlpg_stream_push_device at the same shape, lag and timing, in the same session
  ..._of_mlpg                           the feature push over the MLPG push with one row of variances
    python tools/feature_stream_probe.py [reps]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # for the inputs; imported before the library is loaded so that both use one HIP runtime

import world_class_amd as w
from world_class_amd import feature_stream, mlpg_stream
from world_class_amd import features as ft

L = w.lib()
L.wc_set_device(0)
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
nd, n_ap, orders = 60, 5, 3
MAX_ROWS, LAG, INNER = 8, 64, 20
HBM = 6.3e12   # bytes per second a float4 copy achieves on the MI355X (8.0e12 is the specification)
S, W = nd + 1 + n_ap, ft.width(nd, n_ap, orders)


def timed(fn, warm=2):
    for _ in range(warm):
        fn()
    L.wc_synchronize()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(INNER):
            fn()
        L.wc_synchronize()
        ts.append((time.perf_counter() - t0) / INNER)
    return float(np.median(ts)) * 1e3


def kernel_ms(fn, names):
    L.wc_set_kernel_timing(1)
    fn()
    L.wc_synchronize()
    out = {n: float(L.wc_last_kernel_ms(n.encode())) for n in names}
    L.wc_set_kernel_timing(0)
    return out


def bytes_of_push(n, k, esz):
    """what a push of k rows to each of n streams past their lag moves: the descriptors up; the rows in and into the ring; the two
    scans over the parked logs of the window and the suffix scan's indices out and back; the triples out and back; for every
    emitted row its own and its two neighbours' ring rows in and the packed row out"""
    window = LAG + k + 1
    per_stream = 80 + 2 * 8 * k * S + 2 * 8 * window + 2 * 4 * window + 2 * 24 * k + k * (3 * 8 * S + esz * W)
    return n * per_stream


res = {"library": os.path.relpath(w.LIB_PATH), "reps": reps, "inner": INNER,
       "workload": f"nd {nd}, n_ap {n_ap}, orders {orders}, lag {LAG}, at most {MAX_ROWS} rows per push"}
gen = torch.Generator(device="cuda").manual_seed(2000)
for n, k in ((512, 1), (64, 8)):
    rows = n * MAX_ROWS
    d_f0 = torch.rand(rows, dtype=torch.float64, device="cuda", generator=gen) * 400.0 + 80.0
    d_f0[torch.rand(rows, dtype=torch.float64, device="cuda", generator=gen) < 0.3] = 0.0
    d_sp = torch.randn(rows * nd, dtype=torch.float64, device="cuda", generator=gen)
    d_ap = -torch.rand(rows * n_ap, dtype=torch.float64, device="cuda", generator=gen)
    h = feature_stream.FeatureStream(n, nd, n_ap, orders, MAX_ROWS, LAG)
    key = f"{n}x{k}"
    for fmt, esz, dtype in (("f64", 8, torch.float64), ("f32", 4, torch.float32)):
        d_rows = torch.empty(n * max(MAX_ROWS, LAG) * W, dtype=dtype, device="cuda")
        torch.cuda.synchronize()
        for u in range(n):
            h.reset(u, LAG, 0.0)
        for _ in range(LAG // MAX_ROWS + 1):   # past the lag: from here on every row emits a row
            h.push_device([MAX_ROWS] * n, d_f0, d_sp, d_ap, d_rows, fmt)
        call = lambda: h.push_device([k] * n, d_f0, d_sp, d_ap, d_rows, fmt)
        assert call() == [k] * n
        name = f"feat_{key}_{fmt}"
        res[name + "_ms"] = timed(call)
        for kn, v in kernel_ms(call, ("feat_stream_scan_kernel", "feat_stream_pack_kernel")).items():
            res[name + ("_scan_ms" if "scan" in kn else "_pack_ms")] = v
        res[name + "_bytes"] = bytes_of_push(n, k, esz)
        res[name + "_hbm_us"] = bytes_of_push(n, k, esz) / HBM * 1e6
        del d_rows
    h.close()
    # the MLPG stream's push at the same shape: tools/mlpg_stream_probe.py's set-up and calls, timed as above
    m = mlpg_stream.MlpgStream(n, nd, n_ap, orders, MAX_ROWS, LAG)
    d_mean = torch.randn(rows * W, dtype=torch.float64, device="cuda", generator=gen)
    d_var = torch.full((rows * W,), 0.5, dtype=torch.float64, device="cuda")
    d_var_row = torch.full((W,), 0.5, dtype=torch.float64, device="cuda")
    d_static = torch.empty(n * max(MAX_ROWS, LAG) * (S + 1), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for var_name, per_frame in (("global", False), ("per_frame", True)):
        for u in range(n):
            m.reset(u, LAG)
        for _ in range(LAG // MAX_ROWS + 1):
            m.push_device([MAX_ROWS] * n, d_mean, d_var, d_static, True)
        call = lambda: m.push_device([k] * n, d_mean, d_var if per_frame else d_var_row, d_static, per_frame)
        assert call() == [k] * n
        res[f"mlpg_{key}_{var_name}_ms"] = timed(call)
    m.close()
    for fmt in ("f64", "f32"):
        res[f"feat_{key}_{fmt}_of_mlpg"] = res[f"feat_{key}_{fmt}_ms"] / res[f"mlpg_{key}_global_ms"]
print(json.dumps(res))
