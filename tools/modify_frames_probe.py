"""Per-frame F0 / formant modification at the shape of tools/synth_coded_probe.py: 64 utterances x 10 s at 48 kHz (fft 2048, 5 ms
frames: 128 064 frames), 60 mel-cepstral coefficients and 5 band aperiodicities per frame.  Every figure is the median of host-timed
calls around a device synchronisation, after warm-up calls; prints one JSON line with the rows that exist in the library it is
given (WC_LIB_PATH), so the same script runs on a build of the parent commit (tools/ab_build.py):
  decode              wc_decode_features_device
  decode_then_scalar  wc_decode_features_device + wc_modify_parameters_device (one ratio, 0.9)
  modify_frames       wc_modify_parameters_frames_device on decoded rows (ratio array all 0.9; a mixed array)
  decode_then_frames  wc_decode_features_device + wc_modify_parameters_frames_device
  decode_modified     wc_decode_features_modified_device (WC_DECODE_MOD=route in the environment: the routed form)
  synthesis           wc_synthesis_compute_coded_device / wc_synthesis_compute_coded_modified_device
  stream              512 x 24 kHz streams, 1 ms frames, 200 ms pushes: the coded push neutral / with settings on all streams
    python tools/modify_frames_probe.py [n_utt] [reps] [n_streams]"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import world_class_amd as w
from world_class_amd import DeviceArray, codec, io as wio, stream as wstream

NEW = ("wc_modify_parameters_frames_device", "wc_decode_features_modified_device", "wc_synthesis_compute_coded_modified_device",
       "wc_synth_stream_set_modification")
_raw = C.CDLL(w.LIB_PATH)
have = {name: hasattr(_raw, name) for name in NEW}
for table in (w._SIGNATURES, wio.IO_SIGNATURES, codec.CODEC_SIGNATURES, wstream.STREAM_SIGNATURES):
    for name in NEW:
        if not have[name]:
            table.pop(name, None)  # (a library of the parent commit: bind what it has)

from oracle.gen_golden import synth_params

L = w.lib()
L.wc_set_device(0)
fs, fft, nd, fp = 48000, 2048, 60, 5.0
n_utt = int(sys.argv[1]) if len(sys.argv) > 1 else 64
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n_streams = int(sys.argv[3]) if len(sys.argv) > 3 else 512


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


def coded_rows(fs, fft, frames, seeds):
    """per seed: f0 and the coded rows of seeded parameters (coded on the device), as host arrays"""
    bins, n_ap = fft // 2 + 1, codec.number_of_aperiodicities(fs)
    out = []
    d_sp, d_ap, d_csp, d_cap = DeviceArray(frames * bins), DeviceArray(frames * bins), DeviceArray(frames * nd), DeviceArray(frames * n_ap)
    for seed in seeds:
        f0, sp, ap = synth_params(fs, fft, frames, seed)
        L.wc_memcpy_h2d(d_sp.ptr, sp.ctypes.data, sp.nbytes)
        L.wc_memcpy_h2d(d_ap.ptr, ap.ctypes.data, ap.nbytes)
        codec.code_spectral_envelope_device(fs, fft, frames, nd, d_sp, d_csp)
        codec.code_aperiodicity_device(fs, fft, frames, d_ap, d_cap)
        L.wc_synchronize()
        out.append((f0, d_csp.to_host().reshape(frames, nd), d_cap.to_host().reshape(frames, n_ap)))
    for a in (d_sp, d_ap, d_csp, d_cap):
        a.free()
    return out


res = {"library": os.path.relpath(w.LIB_PATH), "decode_mod": os.environ.get("WC_DECODE_MOD", "default"), "reps": reps,
       "workload": f"{n_utt} x 10 s at 48 kHz, fft {fft}, nd {nd}; {n_streams} streams x 24 kHz, 1 ms frames, 200 ms pushes"}

# ---- rows and decoders ----
frames = w.get_samples(fs, 10 * fs, fp)
bins, n_ap = fft // 2 + 1, codec.number_of_aperiodicities(fs)
base = coded_rows(fs, fft, frames, [7000 + k for k in range(8)])
tot = frames * n_utt
res["frames"] = tot
d_f0 = DeviceArray.from_host(np.concatenate([base[u % 8][0] for u in range(n_utt)]))
d_csp = DeviceArray.from_host(np.concatenate([base[u % 8][1] for u in range(n_utt)]).ravel())
d_cap = DeviceArray.from_host(np.concatenate([base[u % 8][2] for u in range(n_utt)]).ravel())
d_sp, d_ap = DeviceArray(tot * bins), DeviceArray(tot * bins)
mixed = np.array([0.0, 0.37, 0.8, 0.999, 1.0, 1.2, 2.5, 0.9])[np.arange(tot) % 8]
d_r09, d_mixed = DeviceArray.from_host(np.full(tot, 0.9)), DeviceArray.from_host(mixed)
decode = lambda: codec.decode_features_device(fs, fft, tot, nd, d_csp, d_cap, d_sp, d_ap)
res["decode_ms"] = timed(decode)
res["decode_then_scalar_ms"] = timed(lambda: (decode(), wio.modify_parameters_device(fs, fft, tot, 0, d_sp, 1.0, 0.9)))
if have["wc_modify_parameters_frames_device"]:
    # (each call stretches the rows the one before left: the work per call does not depend on the values)
    decode()
    res["modify_scalar_ms"] = timed(lambda: wio.modify_parameters_device(fs, fft, tot, 0, d_sp, 1.0, 0.9))
    decode()
    res["modify_frames_ms"] = timed(lambda: wio.modify_parameters_frames_device(fs, fft, tot, None, d_sp, None, d_r09))
    decode()
    res["modify_frames_mixed_ms"] = timed(lambda: wio.modify_parameters_frames_device(fs, fft, tot, None, d_sp, None, d_mixed))
    res["decode_then_frames_ms"] = timed(lambda: (decode(), wio.modify_parameters_frames_device(fs, fft, tot, None, d_sp, None, d_r09)))
if have["wc_decode_features_modified_device"]:
    res["decode_modified_ms"] = timed(lambda: codec.decode_features_modified_device(fs, fft, tot, nd, d_csp, d_cap, d_r09, d_sp, d_ap))
    res["decode_modified_mixed_ms"] = timed(lambda: codec.decode_features_modified_device(fs, fft, tot, nd, d_csp, d_cap, d_mixed, d_sp, d_ap))
    res["decode_modified_null_ms"] = timed(lambda: codec.decode_features_modified_device(fs, fft, tot, nd, d_csp, d_cap, None, d_sp, d_ap))
d_sp.free()
d_ap.free()

# ---- batch Synthesis ----
syn = w.Synthesis(fs, fft, fp)
fl = [frames] * n_utt
ol = [syn.out_length(frames)] * n_utt
d_y = DeviceArray(sum(ol))
zero = [0] * n_utt
res["compute_coded_ms"] = timed(lambda: syn.compute_coded_device(d_f0, fl, d_csp, nd, d_cap, ol, d_y, rng_pos=zero))
if have["wc_synthesis_compute_coded_modified_device"]:
    res["compute_coded_modified_ms"] = timed(lambda: syn.compute_coded_modified_device(d_f0, fl, d_csp, nd, d_cap, d_r09, ol, d_y, rng_pos=zero))
for a in (d_f0, d_csp, d_cap, d_r09, d_mixed, d_y):
    a.free()
del syn

# ---- streams ----
sfs, sfft, per_push, n_push = 24000, 1024, 200, 6
sbase = coded_rows(sfs, sfft, per_push * n_push, [5000 + k for k in range(8)])
pushes = []
for k in range(n_push):
    part = [tuple(a[k * per_push:(k + 1) * per_push] for a in sbase[u % 8]) for u in range(n_streams)]
    pushes.append(tuple(DeviceArray.from_host(np.concatenate([p[j] for p in part]).ravel()) for j in range(3)))


def run_streams(settings):
    ss = wstream.StreamSynthesizer(sfs, sfft, 1.0, n_streams, per_push)
    if settings:
        for u in range(n_streams):
            ss.set_modification(u, 1.0 + 0.2 * ((u % 5) - 2) / 2, 0.8 + 0.1 * (u % 5))
    d_y = DeviceArray(n_streams * ss.max_samples)
    ts = []
    for d_f, d_a, d_b in pushes:
        t0 = time.perf_counter()
        ss.push_coded_device([per_push] * n_streams, d_f, d_a, nd, d_b, None, d_y)
        L.wc_synchronize()
        ts.append(time.perf_counter() - t0)
    d_y.free()
    return float(np.median(ts[1:])) * 1e3


res["stream_push_coded_neutral_ms"] = run_streams(False)
if have["wc_synth_stream_set_modification"]:
    res["stream_push_coded_settings_ms"] = run_streams(True)
print(json.dumps(res))
