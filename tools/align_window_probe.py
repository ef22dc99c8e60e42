"""Alignment streams with a search window at the shape DESIGN.md section 10 reports: 512 streams, dims = 60, dim_begin = 1, eight
resident tracks of 2 000 and of 20 000 rows (the streams follow them in turn), pushes of 1 and of 8 rows per stream, windows of 128
and of 512 columns (back = a quarter of the width) at hop 1 and 8, and once the monotone flag.  The features are seeded random
walks.  The comparison is the unwindowed push of the same handle in the same process.  Every push figure is the median of
host-timed pushes around a device synchronisation, after warm-up pushes (so every stream has a row of state and a window that has
moved); prints one JSON line:
  plain_m<m>_k<k>_ms                      wc_align_stream_push_device without a window: k rows for each of the 512 streams, tracks of m rows
  win_m<m>_k<k>_w<width>_h<hop>[_mono]_ms the same push with the window set on every stream, ratio_...: plain over it
  kernel_...                              align_window_rows_kernel of one more push, by the library's timing events
    python tools/align_window_probe.py [n_streams] [reps]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # for the features; imported before the library is loaded so that both use one HIP runtime

import world_class_amd as w
from world_class_amd.stream import AlignStream

L = w.lib()
L.wc_set_device(0)
n_streams = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
dims, dim_begin, n_tracks = 60, 1, 8


def timed(fn, warm=3, reps=reps):
    for _ in range(warm):
        fn()
    L.wc_synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        L.wc_synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def walk(rows, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.cumsum(0.1 * torch.randn(rows, dims, dtype=torch.float64, device="cuda", generator=g), dim=0).contiguous()


res = {"library": os.path.relpath(w.LIB_PATH), "reps": reps, "workload": f"{n_streams} streams, dims {dims}, from {dim_begin}, {n_tracks} tracks"}
for m in (2000, 20000):
    tracks = [walk(m, 100 + t) for t in range(n_tracks)]
    torch.cuda.synchronize()
    for k in (1, 8):
        h = AlignStream(dims, n_streams, n_tracks, m, k, dim_begin=dim_begin)
        for t in range(n_tracks):
            h.set_track_device(t, m, tracks[t])
        d_rows = walk(n_streams * k, 200 + k).reshape(-1)
        d_pos, d_cost = (torch.empty(n_streams * k, dtype=torch.float64, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        counts = [k] * n_streams
        push = lambda: h.push_device(counts, d_rows, d_pos, d_cost)
        for u in range(n_streams):
            h.reset(u, u % n_tracks)
        plain = res[f"plain_m{m}_k{k}_ms"] = timed(push)
        for width, hop, mono in ((128, 1, False), (128, 8, False), (512, 1, False), (512, 8, False), (128, 8, True)):
            for u in range(n_streams):
                h.reset(u, u % n_tracks)
                h.set_window(u, width, width // 4, hop, monotone=mono)
            name = f"m{m}_k{k}_w{width}_h{hop}" + ("_mono" if mono else "")
            res[f"win_{name}_ms"] = timed(push)
            res[f"ratio_{name}"] = plain / res[f"win_{name}_ms"]
            L.wc_set_kernel_timing(1)
            push()
            L.wc_synchronize()
            res[f"kernel_{name}_ms"] = float(L.wc_last_kernel_ms(b"align_window_rows_kernel"))
            L.wc_set_kernel_timing(0)
        h.close()
        del d_rows, d_pos, d_cost
    del tracks
    torch.cuda.empty_cache()
print(json.dumps(res))
