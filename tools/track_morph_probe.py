"""Track-morph streams at the shape of the live chain: 512 concurrent 24 kHz streams (fft 1024) on ONE resident track of 2 000 rows,
delay 20, pushes of 1 and of 50 rows per stream, positions that are half-integers and wander (a walk of -1 .. +2.5 rows per row
around the stream's own pace, in device memory as an alignment stream leaves them), weights that avoid the copy paths.  Every
figure is the median of host-timed pushes around a device synchronisation, after warm-up pushes, in the steady state (the ring is
full: every push forms as many frames as it takes rows).  Prints one JSON line with the rows that exist in the library it is given
(WC_LIB_PATH), so the same script runs on a build of the parent commit (tools/ab_build.py); per push size R:
  push_R_ms        wc_track_morph_push_device; push_R_host_ms: the part of it until the call returns (the counts, the records, the
                   enqueue); kernel_R_ms: track_morph_kernel alone in one more push (wc_last_kernel_ms)
  push_R_ratio_ms  the same with a spectral ratio per side on every stream (the variant with shared memory)
  morph_stream_R_ms / morph_stream_R_kernel_ms   wc_morph_stream_push_device in lockstep at speed 1 with R rows of both voices per
                   stream and push: the same number of formed frames (this row exists in the parent's library as well)
  copy_R_ms        a device-to-device copy that moves the bytes the kernel must move (per formed frame two rows of the voice and two
                   or four of the track read, two written; per kept row two read and two written: a copy of half their sum reads
                   and writes as much); moved_R_gb: those bytes
    python tools/track_morph_probe.py [n_streams] [pushes]"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # for the inputs and the plain copy; imported before the library is loaded so that both use one HIP runtime

import world_class_amd as w
from world_class_amd import stream as wstream

L = w.lib()
tables = [wstream.STREAM_SIGNATURES, getattr(wstream, "TRACK_MORPH_SIGNATURES", {})]
for table in tables:  # (a library of the parent commit lacks the newest symbols: bind what it has here)
    for name, (res_, args) in table.items():
        fn = getattr(L, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res_, args
wstream._bound = True
have = hasattr(C.CDLL(w.LIB_PATH), "wc_track_morph_push_device") and hasattr(wstream, "TrackMorph")
L.wc_set_device(0)
fs, fft, m, delay = 24000, 1024, 2000, 20
n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
pushes = int(sys.argv[2]) if len(sys.argv) > 2 else 12
warm = 3
bins = fft // 2 + 1
gen = torch.Generator(device="cuda").manual_seed(7)
res = {"library": os.path.relpath(w.LIB_PATH), "workload": f"{n} streams x 24 kHz, fft {fft}, one track of {m} rows, delay {delay}", "pushes": pushes, "warm": warm}


def rows(count):
    f0 = 120.0 + 60.0 * torch.rand(count, dtype=torch.float64, device="cuda", generator=gen)
    f0[torch.rand(count, device="cuda", generator=gen) < 0.2] = 0.0
    sp = 1e-4 + 1e-2 * torch.rand(count * bins, dtype=torch.float64, device="cuda", generator=gen)
    ap = 0.001 + 0.99 * torch.rand(count * bins, dtype=torch.float64, device="cuda", generator=gen)
    return f0, sp, ap


def median(ts):
    return float(np.median(ts[warm:])) * 1e3


def sync():
    L.wc_synchronize()
    torch.cuda.synchronize()


def timed(call, kernel, total):
    """`total` calls, the last `pushes + 1` timed, the very last with the timing events: (median ms, median host ms, kernel ms)"""
    ts, host = [], []
    for k in range(total):
        if k == total - 1:
            L.wc_set_kernel_timing(1)
        sync()
        t0 = time.perf_counter()
        call(k)
        t1 = time.perf_counter()
        sync()
        ts.append(time.perf_counter() - t0)
        host.append(t1 - t0)
    ms = float(L.wc_last_kernel_ms(kernel))
    L.wc_set_kernel_timing(0)
    ts, host = ts[-(pushes + 1):-1], host[-(pushes + 1):-1]
    return median(ts), median(host), ms


track = rows(m)
for per_push in (1, 50):
    R = str(per_push)
    tot = n * per_push
    a, b = rows(tot), rows(tot)
    o = [torch.empty(tot, dtype=torch.float64, device="cuda")] + [torch.empty(tot * bins, dtype=torch.float64, device="cuda") for _ in range(2)]
    fill = -(-delay // per_push)  # pushes until the ring is full
    total = fill + pushes + 1
    # positions: every stream at its own pace through the track, a wandering half-integer walk on top, one array per push
    rng = np.random.default_rng(11)
    pace = rng.uniform(0.6, 1.7, n)
    walk = np.cumsum(np.round(rng.uniform(-1.0, 2.5, (n, total * per_push)) * 2) / 2 - 0.75, axis=1)
    pos = np.clip(np.round((pace[:, None] * np.arange(total * per_push)[None, :] + walk) * 2) / 2, 0.0, m - 1.0)
    d_pos = [torch.from_numpy(np.ascontiguousarray(pos[:, k * per_push:(k + 1) * per_push]).ravel()).cuda() for k in range(total)]
    res["halves_" + R] = float((pos * 2 % 2 == 1).mean())
    if have:
        def run(ratio):
            h = wstream.TrackMorph(fs, fft, n, 1, m, per_push, delay)
            h.set_track_device(0, m, *track)
            for u in range(n):
                h.reset(u, 0, delay)
                h.set_weight(u, (0.25, 0.5, 0.75, 0.4)[u % 4])
                h.set_ratios(u, *((1.2, 0.8) if ratio else (0.0, 0.0)))
            counts = [per_push] * n
            got = timed(lambda k: h.push_device(counts, a[0], a[1], a[2], d_pos[k], *o), b"track_morph_kernel", total)
            assert h.frames_formed(0) == total * per_push - delay and h.pending(0) == delay
            h.close()
            return got

        res["push_" + R + "_ms"], res["push_" + R + "_host_ms"], res["kernel_" + R + "_ms"] = run(False)
        res["push_" + R + "_ratio_ms"], _, res["kernel_" + R + "_ratio_ms"] = run(True)
    if hasattr(wstream, "MorphStream"):
        h = wstream.MorphStream(fs, fft, n, per_push, 16)
        for u in range(n):
            h.set_weight(u, (0.25, 0.5, 0.75, 0.4)[u % 4])
        counts = [per_push] * n
        res["morph_stream_" + R + "_ms"], res["morph_stream_" + R + "_host_ms"], res["morph_stream_" + R + "_kernel_ms"] = timed(
            lambda k: h.push_device(counts, a[0], a[1], a[2], counts, b[0], b[1], b[2], *o), b"morph_stream_kernel", total)
        del h
    # the bytes the kernel must move in a steady push: per formed frame 2 rows of the voice, 2 or 4 of the track, 2 out; per kept row 2 + 2
    halves = res["halves_" + R]
    formed, kept = tot, n * min(delay, per_push)
    moved = 8 * bins * (formed * (2 + 2 * (1 + halves) + 2) + 4 * kept)
    res["moved_" + R + "_gb"] = moved / 1e9
    c_src = torch.zeros(int(moved // 16), dtype=torch.float64, device="cuda")
    c_dst = torch.empty_like(c_src)
    ts = []
    for _ in range(pushes + warm):
        sync()
        t0 = time.perf_counter()
        c_dst.copy_(c_src)
        sync()
        ts.append(time.perf_counter() - t0)
    res["copy_" + R + "_ms"] = median(ts)
print(json.dumps(res))
