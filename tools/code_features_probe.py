"""Feature coding on the device against the entry points it mirrors, old and new timed in the same process.  Every figure is the
median of host-timed calls around a device synchronisation, after warm-up calls; prints one JSON line:
  encode     wc_code_features_device against wc_code_spectral_envelope_device + wc_code_aperiodicity_device on 64 x 10 s at
             48 kHz (fft 2048, 128 064 frames, nd 60), the same at 24 kHz / fft 1024 (cached plan + the codec's kernels) and,
             with a quarter of the utterances, at 96 kHz / fft 4096
  pipeline   Pipeline.run_coded_device against run_device, and against run_device followed by the two old calls
  stream     512 x 24 kHz, 1 ms frames, 200 ms pushes, aperiodicity on: push_coded_device against push_device (_ex), and the
             bytes a host consumer then has to copy per push
  loop       analysis stream -> StreamSynthesizer.push_coded_device, coded rows never leaving the device, against the row loop
             of tools/synth_stream_probe.py
    python tools/code_features_probe.py [n_utt] [reps] [n_streams]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import world_class_amd as w
from world_class_amd import DeviceArray, codec
from world_class_amd.stream import StreamAnalyzer, StreamSynthesizer
from world_class_amd.synth import make_utterance
from oracle.gen_golden import synth_params

L = w.lib()
L.wc_set_device(0)
n_utt = int(sys.argv[1]) if len(sys.argv) > 1 else 64
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n_streams = int(sys.argv[3]) if len(sys.argv) > 3 else 512
nd, fp = 60, 5.0


def timed(fn, warm=2):
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


res = {"workload": f"{n_utt} x 10 s, nd {nd}; {n_streams} streams x 24 kHz, 1 ms frames, 200 ms pushes", "reps": reps}

# ---- encode ----
res["encode"] = {}
for fs, fft in ((48000, 2048), (24000, 1024), (96000, 4096)):
    frames = w.get_samples(fs, 10 * fs, fp)
    bins, n_ap = fft // 2 + 1, codec.number_of_aperiodicities(fs)
    base = [synth_params(fs, fft, frames, 7000 + k) for k in range(8)]
    n_here = n_utt if fft < 4096 else max(1, n_utt // 4)
    tot = frames * n_here
    d_sp, d_ap = DeviceArray(tot * bins), DeviceArray(tot * bins)
    for u in range(n_here):
        L.wc_memcpy_h2d(d_sp.ptr + u * frames * bins * 8, base[u % 8][1].ctypes.data, frames * bins * 8)
        L.wc_memcpy_h2d(d_ap.ptr + u * frames * bins * 8, base[u % 8][2].ctypes.data, frames * bins * 8)
    d_csp, d_cap = DeviceArray(tot * nd), DeviceArray(tot * n_ap)
    new = timed(lambda: codec.code_features_device(fs, fft, tot, nd, d_sp, d_ap, d_csp, d_cap))
    got = (d_csp.to_host(), d_cap.to_host())
    old = timed(lambda: (codec.code_spectral_envelope_device(fs, fft, tot, nd, d_sp, d_csp),
                         codec.code_aperiodicity_device(fs, fft, tot, d_ap, d_cap)))
    diff = max(float(np.abs(got[0] - d_csp.to_host()).max()), float(np.abs(got[1] - d_cap.to_host()).max()))
    res["encode"][f"{fs // 1000}k_fft{fft}"] = {"frames": tot, "code_features_ms": new, "two_coders_ms": old, "speedup": old / new,
                                               "row_gbytes": 2 * tot * bins * 8 / 1e9, "read_gbytes_per_s": 2 * tot * bins * 8 / 1e6 / new,
                                               "max_abs_diff_old_new": diff}
    for a in (d_sp, d_ap, d_csp, d_cap):
        a.free()

# ---- pipeline ----
fs = 48000
xs = [make_utterance(fs, 10.0, 100 + u) for u in range(8)]
xl = [len(xs[u % 8]) for u in range(n_utt)]
pipe = w.Pipeline(fs, fp)
fl, yl = pipe.lengths(xl)
nf, bins, n_ap = sum(fl), pipe.bins, codec.number_of_aperiodicities(fs)
d_x = DeviceArray.from_host(np.concatenate([xs[u % 8] for u in range(n_utt)]))
d_t, d_f, d_y = DeviceArray(nf), DeviceArray(nf), DeviceArray(sum(yl))
d_sp, d_ap = DeviceArray(nf * bins), DeviceArray(nf * bins)
d_csp, d_cap = DeviceArray(nf * nd), DeviceArray(nf * n_ap)
zero = [0] * n_utt
plain = timed(lambda: pipe.run_device(d_x, xl, d_t, d_f, d_sp, d_ap, d_y, rng_pos=zero))
coded = timed(lambda: pipe.run_coded_device(d_x, xl, d_t, d_f, d_csp, nd, d_cap, d_y, rng_pos=zero))
plain_then_old = timed(lambda: (pipe.run_device(d_x, xl, d_t, d_f, d_sp, d_ap, d_y, rng_pos=zero),
                                codec.code_spectral_envelope_device(fs, pipe.fft_size, nf, nd, d_sp, d_csp),
                                codec.code_aperiodicity_device(fs, pipe.fft_size, nf, d_ap, d_cap)))
res["pipeline"] = {"run_device_ms": plain, "run_coded_device_ms": coded, "run_device_then_two_coders_ms": plain_then_old,
                   "coded_over_plain": coded / plain, "bytes_out_rows": 2 * nf * bins * 8, "bytes_out_coded": nf * (nd + n_ap) * 8}
for a in (d_x, d_t, d_f, d_y, d_sp, d_ap, d_csp, d_cap):
    a.free()
del pipe

# ---- stream and loop (the shape of tools/synth_stream_probe.py) ----
fs, n, chunk_ms = 24000, n_streams, 200
n_ap = codec.number_of_aperiodicities(fs)
sig = [make_utterance(fs, 4.0, 5000 + u) for u in range(8)]
warm = (400 + chunk_ms + 560) // chunk_ms + 1  # pushes until the analysis history is full


def run_streams(coded_mode):
    sa = StreamAnalyzer(fs, n, frame_period=1.0, chunk_ms=chunk_ms, lookback_ms=400, lookahead_ms=560, context_ms=160, aperiodicity=True)
    ss = StreamSynthesizer(fs, sa.fft_size, 1.0, n, sa.max_frames)
    cs, cap = sa.chunk_samples, n * sa.max_frames
    d_t, d_f, d_y = DeviceArray(cap), DeviceArray(cap), DeviceArray(n * ss.max_samples)
    if coded_mode:
        d_a, d_b = DeviceArray(cap * nd), DeviceArray(cap * n_ap)
    else:
        d_a, d_b = DeviceArray(cap * sa.bins), DeviceArray(cap * sa.bins)
    n_push = len(sig[0]) // cs
    chunks = [DeviceArray.from_host(np.concatenate([sig[u % 8][k * cs:(k + 1) * cs] for u in range(n)])) for k in range(n_push)]
    ana, loop, frames = [], [], 0
    for k in range(n_push):
        t0 = time.perf_counter()
        if coded_mode:
            counts = sa.push_coded_device(chunks[k], d_a, nd, d_b, None, None, d_t, d_f)
        else:
            counts = sa.push_device(chunks[k], None, None, d_t, d_f, d_a, d_ap=d_b)
        L.wc_synchronize()
        t1 = time.perf_counter()
        if coded_mode:
            ss.push_coded_device(counts, d_f, d_a, nd, d_b, None, d_y)
        else:
            ss.push_device(counts, d_f, d_a, d_b, None, d_y)
        L.wc_synchronize()
        t2 = time.perf_counter()
        ana.append(t1 - t0)
        loop.append(t2 - t0)
        frames = sum(counts)
    per_frame = (nd + n_ap + 2) if coded_mode else (2 * sa.bins + 2)
    return {"analysis_push_ms": float(np.median(ana[warm:])) * 1e3, "loop_push_ms": float(np.median(loop[warm:])) * 1e3,
            "frames_per_push": frames, "host_bytes_per_push": frames * per_frame * 8, "fft_size": sa.fft_size}


rows, cod = run_streams(False), run_streams(True)
res["stream"] = {"push_device_ex_ms": rows["analysis_push_ms"], "push_coded_device_ms": cod["analysis_push_ms"],
                 "host_bytes_per_push_rows": rows["host_bytes_per_push"], "host_bytes_per_push_coded": cod["host_bytes_per_push"],
                 "frames_per_push": cod["frames_per_push"], "fft_size": cod["fft_size"]}
res["loop"] = {"row_loop_push_ms": rows["loop_push_ms"], "coded_loop_push_ms": cod["loop_push_ms"],
               "real_time_factor_coded": chunk_ms / cod["loop_push_ms"]}
print(json.dumps(res))
