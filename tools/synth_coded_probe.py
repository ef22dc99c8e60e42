"""Synthesis from coded features at the headline shape: 64 utterances x 10 s at 48 kHz (fft 2048, 5 ms frames: 128 064 frames),
60 mel-cepstral coefficients and 5 band aperiodicities per frame.  Every figure is the median of host-timed calls around a device
synchronisation, after warm-up calls; prints one JSON line:
  decode       wc_decode_features_device against wc_decode_spectral_envelope_device + wc_decode_aperiodicity_device
  device       wc_synthesis_compute_coded_device against wc_synthesis_compute_device on the decoded rows
  host         Synthesis.compute_batch_coded (float64 and int16 output) against Synthesis.compute_batch with full rows
    python tools/synth_coded_probe.py [n_utt] [reps]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import world_class_amd as w
from world_class_amd import DeviceArray, codec
from oracle.gen_golden import synth_params

L = w.lib()
L.wc_set_device(0)
fs, fft, nd, fp = 48000, 2048, 60, 5.0
n_utt = int(sys.argv[1]) if len(sys.argv) > 1 else 64
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
frames = w.get_samples(fs, 10 * fs, fp)
bins, n_ap = fft // 2 + 1, codec.number_of_aperiodicities(fs)
base = [synth_params(fs, fft, frames, 7000 + k) for k in range(8)]
f0 = np.concatenate([base[u % 8][0] for u in range(n_utt)])
tot = len(f0)
d_f0 = DeviceArray.from_host(f0)
d_sp, d_ap = DeviceArray(tot * bins), DeviceArray(tot * bins)
for u in range(n_utt):  # (uploaded utterance by utterance: the full-row matrices exist on the host only as the caller's rows, below)
    L.wc_memcpy_h2d(d_sp.ptr + u * frames * bins * 8, base[u % 8][1].ctypes.data, frames * bins * 8)
    L.wc_memcpy_h2d(d_ap.ptr + u * frames * bins * 8, base[u % 8][2].ctypes.data, frames * bins * 8)
d_csp, d_cap = DeviceArray(tot * nd), DeviceArray(tot * n_ap)
codec.code_spectral_envelope_device(fs, fft, tot, nd, d_sp, d_csp)
codec.code_aperiodicity_device(fs, fft, tot, d_ap, d_cap)
L.wc_synchronize()
syn = w.Synthesis(fs, fft, fp)
fl = [frames] * n_utt
ol = [syn.out_length(frames)] * n_utt
d_y = DeviceArray(sum(ol))


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


res = {"workload": f"{n_utt} x 10 s at 48 kHz, fft {fft}, {tot} frames, nd {nd}", "reps": reps}
dec_new = timed(lambda: codec.decode_features_device(fs, fft, tot, nd, d_csp, d_cap, d_sp, d_ap))
dec_old = timed(lambda: (codec.decode_spectral_envelope_device(fs, fft, tot, nd, d_csp, d_sp),
                         codec.decode_aperiodicity_device(fs, fft, tot, d_cap, d_ap)))
res["decode"] = {"decode_features_ms": dec_new, "two_decoders_ms": dec_old, "speedup": dec_old / dec_new}
codec.decode_features_device(fs, fft, tot, nd, d_csp, d_cap, d_sp, d_ap)
plain = timed(lambda: syn.compute_device(d_f0, fl, d_sp, d_ap, ol, d_y, rng_pos=[0] * n_utt))
coded = timed(lambda: syn.compute_coded_device(d_f0, fl, d_csp, nd, d_cap, ol, d_y, rng_pos=[0] * n_utt))
res["device"] = {"compute_device_ms": plain, "compute_coded_device_ms": coded, "ratio": coded / plain}
csp = np.empty(tot * nd)
cap = np.empty(tot * n_ap)
L.wc_memcpy_d2h(csp.ctypes.data, d_csp.ptr, csp.nbytes)
L.wc_memcpy_d2h(cap.ctypes.data, d_cap.ptr, cap.nbytes)
csp, cap = csp.reshape(tot, nd), cap.reshape(tot, n_ap)
f0s = [f0[u * frames:(u + 1) * frames] for u in range(n_utt)]
csps = [csp[u * frames:(u + 1) * frames] for u in range(n_utt)]
caps = [cap[u * frames:(u + 1) * frames] for u in range(n_utt)]
sps, aps = [base[u % 8][1] for u in range(n_utt)], [base[u % 8][2] for u in range(n_utt)]
host_coded = timed(lambda: syn.compute_batch_coded(f0s, csps, caps, rng_pos=[0] * n_utt), warm=1)
host_pcm = timed(lambda: syn.compute_batch_coded(f0s, csps, caps, y_pcm16=True, rng_pos=[0] * n_utt), warm=1)
host_rows = timed(lambda: syn.compute_batch(f0s, sps, aps, rng_pos=[0] * n_utt), warm=1)
res["host"] = {"compute_batch_coded_ms": host_coded, "compute_batch_coded_pcm16_ms": host_pcm, "compute_batch_rows_ms": host_rows,
               "speedup": host_rows / host_coded}
print(json.dumps(res))
