"""Feature alignment at the shape DESIGN.md section 10 reports: 64 pairs of 2001 x 2001 frames (10 s at 5 ms), dims = 60, dim_begin = 1,
band 0 and band 200.  The features are seeded random walks (a path that wanders, as between two utterances; the kernels' time does
not depend on the values).  Every figure is the median of host-timed calls around a device synchronisation, after warm-up calls;
prints one JSON line:
  align_band<b>_ms             wc_align_features_device with all five outputs
  cost_/accumulate_/path_kernel_band<b>_ms    the three kernels of one more call, by the library's timing events
  cost_copy_band<b>_ms         a plain copy_ that moves the bytes the cost pass must move (the features read, 8 bytes per stored
                               cell written: a copy of half their sum reads and writes as much)
  download_ms                  what a caller without the call does first: both sides' rows to the host (the host's own DTW is timed
                               by tools/host_dtw.cpp, a stand-alone program)
    python tools/align_probe.py [n_pairs] [reps] [frames]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # for the features and the plain copy; imported before the library is loaded so that both use one HIP runtime

import world_class_amd as w
from world_class_amd import io as wio

L = w.lib()
L.wc_set_device(0)
n_pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 64
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
frames = int(sys.argv[3]) if len(sys.argv) > 3 else 2001
dims, dim_begin = 60, 1


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


def stored_cells(n, m, band):
    """world_class_io.h: n * W, W the widest row the band can have"""
    if band < 1 or band >= max(n, m) or n == 1:
        return n * m
    return n * min(m, 2 * band * (max(n, m) - 1) // (n - 1) + 1)


torch.manual_seed(2001)
tot = n_pairs * frames
walk = lambda: torch.cumsum(0.1 * torch.randn(n_pairs, frames, dims, dtype=torch.float64, device="cuda"), dim=1).reshape(-1).contiguous()
d_a, d_b = walk(), walk()
fl = [frames] * n_pairs
d_cost = torch.empty(n_pairs, dtype=torch.float64, device="cuda")
d_len = torch.empty(n_pairs, dtype=torch.int32, device="cuda")
d_path = torch.empty(2 * n_pairs * (2 * frames - 1), dtype=torch.int32, device="cuda")
d_boa, d_aob = (torch.empty(tot, dtype=torch.float64, device="cuda") for _ in range(2))
torch.cuda.synchronize()
res = {"library": os.path.relpath(w.LIB_PATH), "reps": reps, "workload": f"{n_pairs} pairs of {frames} x {frames} frames, dims {dims}, from {dim_begin}"}

for band in (0, 200):
    call = lambda: wio.align_features_device(fl, d_a, fl, d_b, dims, dim_begin, dims, band, d_cost, d_len, d_path, d_boa, d_aob)
    res[f"align_band{band}_ms"] = timed(call)
    L.wc_set_kernel_timing(1)
    call()
    L.wc_synchronize()
    for k in ("cost", "accumulate", "path"):
        res[f"{k}_kernel_band{band}_ms"] = float(L.wc_last_kernel_ms(f"align_{k}_kernel".encode()))
    L.wc_set_kernel_timing(0)
    res[f"mean_path_length_band{band}"] = float(d_len.double().mean())
    cells = n_pairs * stored_cells(frames, frames, band)
    moved = 8 * cells + 2 * 8 * tot * (dims - dim_begin)
    res[f"stored_cells_band{band}"] = cells
    res[f"cost_moved_gb_band{band}"] = moved / 1e9
    c_src = torch.zeros(moved // 16, dtype=torch.float64, device="cuda")
    c_dst = torch.empty_like(c_src)
    res[f"cost_copy_band{band}_ms"] = timed(lambda: c_dst.copy_(c_src))
    del c_src, c_dst
    torch.cuda.empty_cache()

h_a, h_b = (torch.empty(tot * dims, dtype=torch.float64).pin_memory() for _ in range(2))


def download():
    h_a.copy_(d_a, non_blocking=True)
    h_b.copy_(d_b, non_blocking=True)


res["download_ms"] = timed(download)
L.wc_release_scratch()
print(json.dumps(res))
