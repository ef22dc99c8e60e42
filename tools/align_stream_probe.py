"""Alignment streams at the shape DESIGN.md section 10 reports: 512 streams, dims = 60, dim_begin = 1, eight resident tracks of 2 000 and
of 20 000 rows (the streams follow them in turn), pushes of 1 and of 8 rows per stream.  The features are seeded random walks (the
kernels' time does not depend on the values).  Every push figure is the median of host-timed pushes around a device synchronisation,
after warm-up pushes (so every stream has a row of state); prints one JSON line:
  push_m<m>_k<k>_ms                 wc_align_stream_push_device, k rows for each of the 512 streams against tracks of m rows
  cost_/rows_kernel_m<m>_k<k>_ms    the two kernels of one more push, by the library's timing events
  whole_m<m>_n<n>_ms, _batch        the only other route to the same numbers: wc_align_features_ex_device with an open end on the whole
                                    prefix of n rows, for as many pairs as its cap of 2^28 cells allows (at most 512), median of at most 5
  whole_m<m>_n<n>_ms_for_512        that time scaled to 512 streams, and ratio_m<m>_n<n>_k1: over the one-row push
    python tools/align_stream_probe.py [n_streams] [reps]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # for the features; imported before the library is loaded so that both use one HIP runtime

import world_class_amd as w
from world_class_amd import io as wio
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
        for u in range(n_streams):
            h.reset(u, u % n_tracks)
        d_rows = walk(n_streams * k, 200 + k).reshape(-1)
        d_pos, d_cost = (torch.empty(n_streams * k, dtype=torch.float64, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        counts = [k] * n_streams
        push = lambda: h.push_device(counts, d_rows, d_pos, d_cost)
        res[f"push_m{m}_k{k}_ms"] = timed(push)
        L.wc_set_kernel_timing(1)
        push()
        L.wc_synchronize()
        for name in ("cost", "rows"):
            res[f"{name}_kernel_m{m}_k{k}_ms"] = float(L.wc_last_kernel_ms(f"align_stream_{name}_kernel".encode()))
        L.wc_set_kernel_timing(0)
        h.close()
        del d_rows, d_pos, d_cost
    for n in (200, 2000):
        batch = int(min(n_streams, (1 << 28) // (n * m)))
        d_a = walk(batch * n, 300 + n).reshape(-1)
        d_b = torch.cat([tracks[p % n_tracks] for p in range(batch)]).reshape(-1).contiguous()
        d_c = torch.empty(batch, dtype=torch.float64, device="cuda")
        d_len = torch.empty(batch, dtype=torch.int32, device="cuda")
        d_span = torch.empty(2 * batch, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        whole = lambda: wio.align_features_ex_device([n] * batch, d_a, [m] * batch, d_b, dims, dim_begin, dims, 0, 0, wio.ALIGN_OPEN_END, d_c, d_len,
                                                     d_span=d_span)
        t = timed(whole, warm=2, reps=min(reps, 5))
        res[f"whole_m{m}_n{n}_ms"], res[f"whole_m{m}_n{n}_batch"] = t, batch
        res[f"whole_m{m}_n{n}_ms_for_512"] = t * n_streams / batch
        res[f"ratio_m{m}_n{n}_k1"] = t * n_streams / batch / res[f"push_m{m}_k1_ms"]
        del d_a, d_b, d_c, d_len, d_span
        L.wc_release_scratch()
    del tracks
    torch.cuda.empty_cache()
print(json.dumps(res))
