"""Extended feature alignment at the shapes DESIGN.md section 10 reports, in the form of tools/align_probe.py.  The features are
seeded random walks (the kernels' time does not depend on the values).  Every call figure is the median of host-timed calls around
a device synchronisation, after warm-up calls; the kernels are those of one more call, by the library's timing events; prints one
JSON line:
  square shape   pairs of frames x frames, dims = 60, dim_begin = 1: step pattern 0 through wc_align_features_device (the
                 kernels of the plain call), step pattern 1 through wc_align_features_ex_device, both ends closed
  search shape   queries of `query` rows against tracks of `track` rows, both ends open, both patterns through
                 wc_align_features_ex_device with the span and both timelines
  <shape>_p<pattern>_ms, <shape>_p<pattern>_{cost,accumulate,path}_kernel_ms, <shape>_accumulate_p1_over_p0
Step pattern 1 takes 2^27 stored cells per call, half of pattern 0's: where n_pairs pairs are more (64 pairs of either default shape
are 2.56e8 cells), <shape> is the largest batch that fits, measured under both patterns, and <shape>_full is pattern 0 alone at
n_pairs pairs.
    python tools/align_ex_probe.py [n_pairs] [reps] [frames] [query] [track]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # for the features; imported before the library is loaded so that both use one HIP runtime

import world_class_amd as w
from world_class_amd import io as wio

L = w.lib()
L.wc_set_device(0)
arg = lambda k, v: int(sys.argv[k]) if len(sys.argv) > k else v
n_pairs, reps, frames, query, track = arg(1, 64), arg(2, 5), arg(3, 2001), arg(4, 200), arg(5, 20000)
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


def walk(pairs, rows):
    return torch.cumsum(0.1 * torch.randn(pairs, rows, dims, dtype=torch.float64, device="cuda"), dim=1).reshape(-1).contiguous()


def measure(res, shape, pairs, n, m, flags, patterns):
    d_a, d_b = walk(pairs, n), walk(pairs, m)
    al, bl = [n] * pairs, [m] * pairs
    entries = pairs * (n + m - 1)
    d_cost = torch.empty(pairs, dtype=torch.float64, device="cuda")
    d_len = torch.empty(pairs, dtype=torch.int32, device="cuda")
    d_path = torch.empty(2 * entries, dtype=torch.int32, device="cuda")
    d_boa, d_aob = torch.empty(pairs * n, dtype=torch.float64, device="cuda"), torch.empty(pairs * m, dtype=torch.float64, device="cuda")
    d_span = torch.empty(2 * pairs, dtype=torch.int32, device="cuda")
    d_ta, d_tb = (torch.empty(entries, dtype=torch.float64, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    res[f"{shape}_workload"] = f"{pairs} pairs of {n} x {m} frames, dims {dims}, from {dim_begin}, flags {flags}"
    res[f"{shape}_stored_cells"] = pairs * n * m
    for pattern in patterns:
        if pattern == 0 and flags == 0:
            call = lambda: wio.align_features_device(al, d_a, bl, d_b, dims, dim_begin, dims, 0, d_cost, d_len, d_path, d_boa, d_aob)
        else:
            call = lambda: wio.align_features_ex_device(al, d_a, bl, d_b, dims, dim_begin, dims, 0, pattern, flags, d_cost, d_len, d_path, d_boa,
                                                        d_aob, d_span, d_ta, d_tb)
        key = f"{shape}_p{pattern}"
        res[f"{key}_ms"] = timed(call)
        L.wc_set_kernel_timing(1)
        call()
        L.wc_synchronize()
        names = {"cost": "align_cost_kernel", "accumulate": "align_accumulate_slope_kernel" if pattern else "align_accumulate_kernel",
                 "path": "align_path_kernel"}
        for k, name in names.items():
            res[f"{key}_{k}_kernel_ms"] = float(L.wc_last_kernel_ms(name.encode()))
        L.wc_set_kernel_timing(0)
        res[f"{key}_mean_path_length"] = float(d_len.double().mean())
        res[f"{key}_finite"] = int(torch.isfinite(d_cost).sum())
    if len(patterns) == 2:
        res[f"{shape}_call_p1_over_p0"] = res[f"{shape}_p1_ms"] / res[f"{shape}_p0_ms"]
        res[f"{shape}_accumulate_p1_over_p0"] = res[f"{shape}_p1_accumulate_kernel_ms"] / res[f"{shape}_p0_accumulate_kernel_ms"]
    del d_a, d_b, d_path, d_boa, d_aob, d_ta, d_tb
    L.wc_release_scratch()
    torch.cuda.empty_cache()


def fitting(n, m):
    """the most pairs (at most n_pairs) that step pattern 1 takes in one call: 2^27 stored cells"""
    return max(1, min(n_pairs, (1 << 27) // (n * m)))


torch.manual_seed(2001)
res = {"library": os.path.relpath(w.LIB_PATH), "reps": reps}
for shape, n, m, flags in (("square", frames, frames, 0), ("search", query, track, 3)):
    part = fitting(n, m)
    if part < n_pairs:  # pattern 0 alone at the full batch (at flags 0 the figures of the plain call), both patterns at what pattern 1 takes
        measure(res, shape + "_full", n_pairs, n, m, flags, (0,))
    measure(res, shape, part, n, m, flags, (0, 1))
print(json.dumps(res))
