"""BASELINE config 5's shape for the whole streaming loop: 512 concurrent 24 kHz streams, 1 ms frames, 200 ms per push -- chunked
Harvest + CheapTrick + D4C (incremental mode) feeding chunked Synthesis (include/world_class_stream.h), and Synthesis alone.  Each push
is timed on the host around a device synchronisation, after warm-up pushes; prints one JSON line with push_ms and real_time_factor.
    python tools/synth_stream_probe.py [n_streams]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import world_class_amd as w
from world_class_amd import DeviceArray
from world_class_amd.stream import StreamAnalyzer, StreamSynthesizer
from world_class_amd.synth import make_utterance

L = w.lib()
L.wc_set_device(0)
fs, n, chunk_ms = 24000, int(sys.argv[1]) if len(sys.argv) > 1 else 512, 200
sig = [make_utterance(fs, 4.0, 5000 + u) for u in range(8)]
sa = StreamAnalyzer(fs, n, frame_period=1.0, chunk_ms=chunk_ms, lookback_ms=400, lookahead_ms=560, context_ms=160, aperiodicity=True)
ss = StreamSynthesizer(fs, sa.fft_size, 1.0, n, sa.max_frames)
cs, cap = sa.chunk_samples, n * sa.max_frames
d_t, d_f, d_sp = DeviceArray(cap), DeviceArray(cap), DeviceArray(cap * sa.bins)
d_ap = DeviceArray(cap * sa.bins)
d_y = DeviceArray(n * ss.max_samples)
n_push = len(sig[0]) // cs
chunks = [DeviceArray.from_host(np.concatenate([sig[u % 8][k * cs:(k + 1) * cs] for u in range(n)])) for k in range(n_push)]
warm = (400 + chunk_ms + 560) // chunk_ms + 1  # pushes until the analysis history is full
loop, synth, samples = [], [], []
for k in range(n_push):
    t0 = time.perf_counter()
    counts = sa.push_device(chunks[k], None, None, d_t, d_f, d_sp, d_ap=d_ap)
    L.wc_synchronize()
    t1 = time.perf_counter()
    out = ss.push_device(counts, d_f, d_sp, d_ap, None, d_y)
    L.wc_synchronize()
    t2 = time.perf_counter()
    loop.append(t2 - t0)
    synth.append(t2 - t1)
    samples.append(sum(out) / n)
lm, sm = float(np.median(loop[warm:])) * 1e3, float(np.median(synth[warm:])) * 1e3
print(json.dumps({"workload": f"{n} streams x 24 kHz, 1 ms frames, {chunk_ms} ms pushes", "fft_size": sa.fft_size,
                  "samples_per_stream_per_push": samples[-1],
                  "loop": {"push_ms": lm, "real_time_factor": chunk_ms / lm, "note": "Harvest + CheapTrick + D4C (incremental) + Synthesis"},
                  "synthesis": {"push_ms": sm, "real_time_factor": chunk_ms / sm}}))
