"""BASELINE config 5's shape for the whole streaming loop: 512 concurrent 24 kHz streams, 1 ms frames, 200 ms per push -- chunked
Harvest + CheapTrick + D4C (incremental mode) feeding chunked Synthesis (include/world_class_stream.h), and Synthesis alone.  Each push
is timed on the host around a device synchronisation, after warm-up pushes; prints one JSON line with push_ms and real_time_factor.
With a speed the synthesis streams are retimed (wc_synth_stream_set_speed: 0.999 for the first push with frames, so that speed 1.0
is measured retimed too, the given speed from then on); the line then also carries the retiming kernel's own time in the last push
(wc_last_kernel_ms) and the time of a plain device-to-device copy of the bytes it must move (source rows read once, retimed rows
written once: a copy of half their sum reads and writes as much).  The script binds what the library it is given has (WC_LIB_PATH),
so without a speed it also runs on a build of the parent commit.
    python tools/synth_stream_probe.py [n_streams] [speed]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # for the plain device-to-device copy; imported before the library is loaded, so that both use one HIP runtime

import world_class_amd as w
from world_class_amd import DeviceArray
from world_class_amd import stream as wstream
from world_class_amd.stream import StreamAnalyzer, StreamSynthesizer
from world_class_amd.synth import make_utterance

L = w.lib()
for name, (res, args) in wstream.STREAM_SIGNATURES.items():  # (a library of the parent commit lacks the newest symbols: bind what
    fn = getattr(L, name, None)                              # it has here, the module's table stays as it is)
    if fn is not None:
        fn.restype, fn.argtypes = res, args
wstream._bound = True
L.wc_set_device(0)
fs, n, chunk_ms = 24000, int(sys.argv[1]) if len(sys.argv) > 1 else 512, 200
speed = float(sys.argv[2]) if len(sys.argv) > 2 else None
sig = [make_utterance(fs, 4.0, 5000 + u) for u in range(8)]
sa = StreamAnalyzer(fs, n, frame_period=1.0, chunk_ms=chunk_ms, lookback_ms=400, lookahead_ms=560, context_ms=160, aperiodicity=True)
ss = StreamSynthesizer(fs, sa.fft_size, 1.0, n, sa.max_frames if speed is None else int(sa.max_frames / min(speed, 0.999)) + 2)
cs, cap = sa.chunk_samples, n * sa.max_frames
d_t, d_f, d_sp = DeviceArray(cap), DeviceArray(cap), DeviceArray(cap * sa.bins)
d_ap = DeviceArray(cap * sa.bins)
d_y = DeviceArray(n * ss.max_samples)
n_push = len(sig[0]) // cs
chunks = [DeviceArray.from_host(np.concatenate([sig[u % 8][k * cs:(k + 1) * cs] for u in range(n)])) for k in range(n_push)]
warm = (400 + chunk_ms + 560) // chunk_ms + 1  # pushes until the analysis history is full
loop, synth, samples = [], [], []
begun, formed = False, 0
for k in range(n_push):
    t0 = time.perf_counter()
    counts = sa.push_device(chunks[k], None, None, d_t, d_f, d_sp, d_ap=d_ap)
    L.wc_synchronize()
    ta = time.perf_counter()
    if speed is not None:  # (the settings and the counts are outside the timed intervals: push_ms compares with a run without a speed)
        for u in range(n):
            ss.set_speed(u, speed if begun else 0.999)
        begun = begun or sum(counts) > 0
        formed = sum(ss.frames_for_push(u, counts[u]) for u in range(n))
        if k == n_push - 1:
            L.wc_set_kernel_timing(1)
    t1 = time.perf_counter()
    out = ss.push_device(counts, d_f, d_sp, d_ap, None, d_y)
    L.wc_synchronize()
    t2 = time.perf_counter()
    loop.append((ta - t0) + (t2 - t1))
    synth.append(t2 - t1)
    samples.append(sum(out) / n)
if speed is not None:
    loop, synth = loop[:-1], synth[:-1]  # (the last push ran with the timing events)
lm, sm = float(np.median(loop[warm:])) * 1e3, float(np.median(synth[warm:])) * 1e3
extra = {}
if speed is not None:
    moved = 8 * sa.bins * 2 * (sum(counts) + formed)
    extra = {"speed": speed, "synthesis_frames_last_push": formed, "retime_stream_kernel_ms": float(L.wc_last_kernel_ms(b"retime_stream_kernel")),
             "moved_gb": moved / 1e9}
    L.wc_set_kernel_timing(0)
    c_src = torch.zeros(moved // 16, dtype=torch.float64, device="cuda")
    c_dst = torch.empty_like(c_src)
    ts = []
    for _ in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c_dst.copy_(c_src)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    extra["copy_ms"] = float(np.median(ts[2:])) * 1e3
print(json.dumps({"workload": f"{n} streams x 24 kHz, 1 ms frames, {chunk_ms} ms pushes", "fft_size": sa.fft_size,
                  "samples_per_stream_per_push": samples[-1],
                  "loop": {"push_ms": lm, "real_time_factor": chunk_ms / lm, "note": "Harvest + CheapTrick + D4C (incremental) + Synthesis"},
                  "synthesis": {"push_ms": sm, "real_time_factor": chunk_ms / sm}, **extra}))
