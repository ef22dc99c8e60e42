"""Time-scale modification at the shape of tools/modify_frames_probe.py: 64 utterances x 10 s at 48 kHz (fft 2048, 5 ms frames:
128 064 source frames), rows decoded on the device from 60 mel-cepstral coefficients and 5 band aperiodicities per frame.  Every
figure is the median of host-timed calls around a device synchronisation, after warm-up calls; prints one JSON line with the rows
that exist in the library it is given (WC_LIB_PATH), so the same script runs on a build of the parent commit (tools/ab_build.py):
  retime_<map>          wc_retime_parameters_device, F0 and both rows: identity, half (2x slower), fast15 (1.5x faster), ramp
  retime_<map>_mod      the same with an F0 scale and a spectral ratio per output frame (the mixed ratios of modify_frames_probe.py)
  routed_<map>_mod      the same as two calls: wc_retime_parameters_device, then wc_modify_parameters_frames_device on its outputs
                        (WC_RETIME_MOD=route in the environment makes retime_<map>_mod take that route inside the library)
  copy_<map>            a device-to-device copy that moves the bytes the kernel must move (the source rows read once, the output
                        rows written once: a copy of half their sum reads and writes as much)
  decode, modify_frames, compute_coded       what existed before, for the comparison with the parent build
  compute_coded_retimed                      wc_synthesis_compute_coded_retimed_device at the identity map / at half speed
    python tools/retime_probe.py [n_utt] [reps]"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # for the plain device-to-device copy the kernel is judged against (the C-ABI has none); imported before the library
# is loaded, as in the GPU tests, so that both use one HIP runtime

import world_class_amd as w
from world_class_amd import DeviceArray, codec, io as wio

NEW = ("wc_retime_parameters_device", "wc_synthesis_compute_coded_retimed_device")
_raw = C.CDLL(w.LIB_PATH)
have = {name: hasattr(_raw, name) for name in NEW}
for table in (w._SIGNATURES, wio.IO_SIGNATURES):
    for name in NEW:
        if not have[name]:
            table.pop(name, None)  # (a library of the parent commit: bind what it has)

from oracle.gen_golden import synth_params

L = w.lib()
L.wc_set_device(0)
fs, fft, nd, fp = 48000, 2048, 60, 5.0
n_utt = int(sys.argv[1]) if len(sys.argv) > 1 else 64
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5


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


def coded_rows(frames, seeds):
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


frames = w.get_samples(fs, 10 * fs, fp)
bins = fft // 2 + 1
tot = frames * n_utt
res = {"library": os.path.relpath(w.LIB_PATH), "retime_mod": os.environ.get("WC_RETIME_MOD", "default"), "reps": reps,
       "workload": f"{n_utt} x 10 s at 48 kHz, fft {fft}, nd {nd}", "frames": tot}
base = coded_rows(frames, [7000 + k for k in range(8)])
d_f0 = DeviceArray.from_host(np.concatenate([base[u % 8][0] for u in range(n_utt)]))
d_csp = DeviceArray.from_host(np.concatenate([base[u % 8][1] for u in range(n_utt)]).ravel())
d_cap = DeviceArray.from_host(np.concatenate([base[u % 8][2] for u in range(n_utt)]).ravel())
d_sp, d_ap = DeviceArray(tot * bins), DeviceArray(tot * bins)
decode = lambda: codec.decode_features_device(fs, fft, tot, nd, d_csp, d_cap, d_sp, d_ap)
res["decode_ms"] = timed(decode)

k144 = np.arange(frames + frames // 5)
maps = {"identity": np.arange(frames, dtype=np.float64), "half": np.arange(2 * frames - 1) / 2,
        "fast15": np.arange(int((frames - 1) / 1.5) + 1) * 1.5,
        "ramp": np.minimum(frames - 1, np.cumsum(0.5 + k144 / len(k144)) - 0.5)}
fl = [frames] * n_utt

if have["wc_retime_parameters_device"]:
    for name, pos in maps.items():
        m = len(pos)
        mt = m * n_utt
        ol = [m] * n_utt
        d_pos = DeviceArray.from_host(np.tile(pos, n_utt))
        mixed = np.array([0.0, 0.37, 0.8, 0.999, 1.0, 1.2, 2.5, 0.9])[np.arange(mt) % 8]
        d_ratio, d_scale = DeviceArray.from_host(mixed), DeviceArray.from_host(np.full(mt, 1.1))
        o_f0, o_sp, o_ap = DeviceArray(mt), DeviceArray(mt * bins), DeviceArray(mt * bins)
        res[f"frames_out_{name}"] = mt
        res[f"retime_{name}_ms"] = timed(lambda: wio.retime_parameters_device(fs, fft, fl, d_f0, d_sp, d_ap, ol, d_pos, None, None, o_f0, o_sp, o_ap))
        res[f"retime_{name}_mod_ms"] = timed(lambda: wio.retime_parameters_device(fs, fft, fl, d_f0, d_sp, d_ap, ol, d_pos, d_scale, d_ratio, o_f0, o_sp, o_ap))
        res[f"routed_{name}_mod_ms"] = timed(lambda: (wio.retime_parameters_device(fs, fft, fl, d_f0, d_sp, d_ap, ol, d_pos, None, None, o_f0, o_sp, o_ap),
                                                      wio.modify_parameters_frames_device(fs, fft, mt, o_f0, o_sp, d_scale, d_ratio)))
        # the bytes the kernel must move: 2 x tot source rows in, 2 x mt rows out; a copy of n bytes reads n and writes n
        moved = 8 * bins * 2 * (tot + mt)
        res[f"moved_gb_{name}"] = moved / 1e9
        for a in (o_sp, o_ap):
            a.free()
        c_src = torch.zeros(moved // 16, dtype=torch.float64, device="cuda")
        c_dst = torch.empty_like(c_src)
        res[f"copy_{name}_ms"] = timed(lambda: c_dst.copy_(c_src))
        del c_src, c_dst
        torch.cuda.empty_cache()
        for a in (d_pos, d_ratio, d_scale, o_f0):
            a.free()

# ---- what existed before ----
d_mixed = DeviceArray.from_host(np.array([0.0, 0.37, 0.8, 0.999, 1.0, 1.2, 2.5, 0.9])[np.arange(tot) % 8])
decode()
res["modify_frames_mixed_ms"] = timed(lambda: wio.modify_parameters_frames_device(fs, fft, tot, None, d_sp, None, d_mixed))
res["decode_again_ms"] = timed(decode)
d_sp.free()
d_ap.free()
d_mixed.free()

# ---- batch Synthesis ----
syn = w.Synthesis(fs, fft, fp)
zero = [0] * n_utt
ol = [syn.out_length(frames)] * n_utt
d_y = DeviceArray(sum(ol))
res["compute_coded_ms"] = timed(lambda: syn.compute_coded_device(d_f0, fl, d_csp, nd, d_cap, ol, d_y, rng_pos=zero))
if have["wc_synthesis_compute_coded_retimed_device"]:
    d_pos = DeviceArray.from_host(np.tile(maps["identity"], n_utt))
    res["compute_coded_retimed_identity_ms"] = timed(lambda: syn.compute_coded_retimed_device(d_f0, fl, d_csp, nd, d_cap, fl, d_pos, None, None, ol, d_y, rng_pos=zero))
    d_pos.free()
    res["compute_coded_again_ms"] = timed(lambda: syn.compute_coded_device(d_f0, fl, d_csp, nd, d_cap, ol, d_y, rng_pos=zero))
    d_y.free()
    m = len(maps["half"])
    ol2 = [syn.out_length(m)] * n_utt
    d_y = DeviceArray(sum(ol2))
    d_pos = DeviceArray.from_host(np.tile(maps["half"], n_utt))
    res["compute_coded_retimed_half_ms"] = timed(lambda: syn.compute_coded_retimed_device(d_f0, fl, d_csp, nd, d_cap, [m] * n_utt, d_pos, None, None, ol2, d_y, rng_pos=zero))
    d_pos.free()
d_y.free()
print(json.dumps(res))
