"""Settled positions of alignment streams (include/world_class_align_lag.h) on the followable voices of tests/align_window_rule.py:
one stream per voice (seeds 0 .. n_voices - 1: a track of 300 rows of 8, a voice of 150 rows sampled from it at slopes from
[0.6, 1.7] plus noise), each on a track slot of its own, pushed k rows at a time through wc_align_stream_push_settled_device;
without a window and under the window (60, 20, 8, monotone); at lags 0, 10 and 50.  Prints one JSON line:
  push_<win>_l<lag>_k<k>_ms   the kernels of one push (local costs, rows, settle) by the library's timing events, median over the
                              pushes behind row 50 (every walk has its full length there); ratio_...: the same push at lag 0 under it
  settle_<win>_l<lag>_k<k>_ms align_stream_settle_kernel alone
  falls_<win>_l<lag>          the share of rows whose settled position lies below its predecessor's (over all voices)
  err_settled_<win>_l<lag>    mean |settled - true position| of the row the value stands for (row i - lag; the last `lag` rows from
                              wc_align_stream_tail_device), err_position_<win>: mean |position - true position| of the raw position
    python tools/align_lag_probe.py [n_voices] [k]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import world_class_amd as w
from align_lag_rule import true_positions
from align_window_rule import followable
from world_class_amd.stream import AlignStream

L = w.lib()
L.wc_set_device(0)
n_voices = int(sys.argv[1]) if len(sys.argv) > 1 else 64
ks = [int(sys.argv[2])] if len(sys.argv) > 2 else [1, 8]
dims, m, n = 8, 300, 150
WINDOW = (60, 20, 8, True)
KERNELS = [b"align_stream_cost_kernel", b"align_stream_rows_kernel", b"align_window_rows_kernel", b"align_stream_settle_kernel"]

voices = [followable(s)[:2] for s in range(n_voices)]
true = np.stack([true_positions(s) for s in range(n_voices)])
res = {"library": os.path.relpath(w.LIB_PATH), "workload": f"{n_voices} followable voices of {n} rows on tracks of {m}, dims {dims}"}
for k in ks:
    h = AlignStream(dims, n_voices, n_voices, m, k, dim_begin=0)
    h.reserve_lag(50)
    for s, (voice, track) in enumerate(voices):
        h.set_track(s, track)
    d_out = [w.DeviceArray(n_voices * k) for _ in range(3)]
    for win in (None, WINDOW):
        wname = "plain" if win is None else "win"
        base = None
        for lag in (0, 10, 50):
            for s in range(n_voices):
                h.reset(s, s)
                if win is not None:
                    h.set_window(s, win[0], win[1], win[2], monotone=win[3])
                h.set_lag(s, lag)
            pos, settled = np.empty((n_voices, n)), np.empty((n_voices, n))
            push_ms, settle_ms = [], []
            L.wc_set_kernel_timing(1)
            for o in range(0, n, k):
                c = min(k, n - o)
                d_rows = w.DeviceArray.from_host(np.concatenate([v[o:o + c] for v, _ in voices]))
                h.push_settled_device([c] * n_voices, d_rows, *d_out)
                L.wc_synchronize()
                d_rows.free()
                if o >= 50:
                    rows_ms = sum(float(L.wc_last_kernel_ms(x)) for x in (KERNELS[:2] if win is None else KERNELS[2:3]))
                    settle_ms.append(float(L.wc_last_kernel_ms(KERNELS[3])))
                    push_ms.append(rows_ms + settle_ms[-1])
                pos[:, o:o + c] = d_out[0].to_host()[:n_voices * c].reshape(n_voices, c)
                settled[:, o:o + c] = d_out[2].to_host()[:n_voices * c].reshape(n_voices, c)
            L.wc_set_kernel_timing(0)
            name = f"{wname}_l{lag}_k{k}"
            res[f"push_{name}_ms"] = float(np.median(push_ms))
            res[f"settle_{name}_ms"] = float(np.median(settle_ms))
            if lag == 0:
                base = res[f"push_{name}_ms"]
            else:
                res[f"ratio_{name}"] = res[f"push_{name}_ms"] / base
            if k == ks[0]:
                # the value of row i stands for row i - lag; the last `lag` rows come from the tail
                per_row = settled if lag == 0 else np.concatenate([settled[:, lag:], np.stack(h.tail())[:, 1:]], axis=1)
                res[f"falls_{wname}_l{lag}"] = float((np.diff(settled, axis=1) < 0).mean())
                res[f"err_settled_{wname}_l{lag}"] = float(np.nanmean(np.abs(per_row - true)))
                res[f"err_position_{wname}"] = float(np.nanmean(np.abs(pos - true)))
    for x in d_out:
        x.free()
    h.close()
print(json.dumps(res))
