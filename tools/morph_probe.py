"""Voice morphing at the shape of tools/retime_probe.py: 64 pairs x 10 s at 48 kHz (fft 2048, 5 ms frames: 128 064 source frames a
side), rows of both voices decoded on the device from 60 mel-cepstral coefficients and 5 band aperiodicities per frame.  Every
figure is the median of host-timed calls around a device synchronisation, after warm-up calls; prints one JSON line with the rows
that exist in the library it is given (WC_LIB_PATH), so the same script runs on a build of the parent commit:
  morph_<maps>          wc_morph_parameters_device, F0 and both rows: identity (both voices along their identity maps), ramp_half (A
                        along the ramp from speed 0.5 to 1.5, B at half speed, truncated to the ramp's length)
  morph_<maps>_ratio    the same with a spectral ratio per output frame and source (the mixed ratios of modify_frames_probe.py)
  routed_<maps>[_ratio] what a caller builds without the call: wc_retime_parameters_device twice (with the ratios), then in torch
                        exp((1 - w) * log(a) + w * log(b)) for sp, (1 - w) * a + w * b for ap and the contour's rule
  copy_<maps>           a device-to-device copy that moves the bytes the kernel must move (eight source rows read, two rows
                        written per output frame: a copy of half their sum reads and writes as much)
  compute_coded_retimed_identity, compute_coded_morphed_identity    the two coded Synthesis calls at the identity map(s)
    python tools/morph_probe.py [n_pairs] [reps]"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # for the routed form and the plain copy; imported before the library is loaded so that both use one HIP runtime

import world_class_amd as w
from world_class_amd import DeviceArray, codec, io as wio

NEW = ("wc_morph_parameters_device", "wc_synthesis_compute_coded_morphed_device")
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
n_pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 64
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


def tensor(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).ravel()).cuda()


frames = w.get_samples(fs, 10 * fs, fp)
bins = fft // 2 + 1
tot = frames * n_pairs
res = {"library": os.path.relpath(w.LIB_PATH), "reps": reps, "workload": f"{n_pairs} pairs x 10 s at 48 kHz, fft {fft}, nd {nd}", "frames_per_side": tot}
base = coded_rows(frames, [7000 + k for k in range(8)])
side = lambda first: tuple(tensor(np.concatenate([base[(first + u) % 8][q] for u in range(n_pairs)])) for q in range(3))
(a_f0, a_csp, a_cap), (b_f0, b_csp, b_cap) = side(0), side(3)
a_sp, a_ap, b_sp, b_ap = (torch.empty(tot * bins, dtype=torch.float64, device="cuda") for _ in range(4))
codec.decode_features_device(fs, fft, tot, nd, a_csp, a_cap, a_sp, a_ap)
codec.decode_features_device(fs, fft, tot, nd, b_csp, b_cap, b_sp, b_ap)
L.wc_synchronize()
fl = [frames] * n_pairs

k144 = np.arange(frames + frames // 5)
ramp = np.minimum(frames - 1, np.cumsum(0.5 + k144 / len(k144)) - 0.5)
maps = {"identity": (np.arange(frames, dtype=np.float64), np.arange(frames, dtype=np.float64)), "ramp_half": (ramp, (np.arange(2 * frames - 1) / 2)[:len(ramp)])}


def routed(m, ol, d_pa, d_pb, d_w, d_ra, d_rb, r, o):
    """two retime calls and the blend in torch: r = (f0, sp, ap) scratch of A and of B, o = the outputs"""
    wio.retime_parameters_device(fs, fft, fl, a_f0, a_sp, a_ap, ol, d_pa, None, d_ra, *r[0])
    wio.retime_parameters_device(fs, fft, fl, b_f0, b_sp, b_ap, ol, d_pb, None, d_rb, *r[1])
    wr = d_w.repeat_interleave(bins)
    torch.exp((1.0 - wr) * torch.log(r[0][1]) + wr * torch.log(r[1][1]), out=o[1])
    torch.add((1.0 - wr) * r[0][2], wr * r[1][2], out=o[2])
    fa, fb = r[0][0], r[1][0]
    glide = torch.exp((1.0 - d_w) * torch.log(fa) + d_w * torch.log(fb))
    o[0].copy_(torch.where((fa != 0) & (fb != 0), glide, torch.where(fa != 0, torch.where(d_w < 0.5, fa, 0.0), torch.where(d_w > 0.5, fb, 0.0))))


for name, (pa, pb) in maps.items():
    m = len(pa)
    mt = m * n_pairs
    ol = [m] * n_pairs
    d_pa, d_pb = tensor(np.tile(pa, n_pairs)), tensor(np.tile(pb, n_pairs))
    d_w = tensor(np.array([0.25, 0.5, 0.75, 0.4, 0.6, 0.3, 0.7, 0.5])[np.arange(mt) % 8])  # (no frame takes the copy paths of w = 0 / 1)
    mixed = np.array([0.0, 0.37, 0.8, 0.999, 1.0, 1.2, 2.5, 0.9])
    d_ra, d_rb = tensor(mixed[np.arange(mt) % 8]), tensor(mixed[(np.arange(mt) + 3) % 8])
    o = [torch.empty(mt, dtype=torch.float64, device="cuda")] + [torch.empty(mt * bins, dtype=torch.float64, device="cuda") for _ in range(2)]
    res[f"frames_out_{name}"] = mt
    if have["wc_morph_parameters_device"]:
        call = lambda ra, rb: wio.morph_parameters_device(fs, fft, fl, a_f0, a_sp, a_ap, fl, b_f0, b_sp, b_ap, ol, d_pa, d_pb, d_w, None, ra, rb, *o)
        res[f"morph_{name}_ms"] = timed(lambda: call(None, None))
        res[f"morph_{name}_ratio_ms"] = timed(lambda: call(d_ra, d_rb))
    r = [[torch.empty_like(t) for t in o] for _ in range(2)]
    res[f"routed_{name}_ms"] = timed(lambda: routed(m, ol, d_pa, d_pb, d_w, None, None, r, o))
    res[f"routed_{name}_ratio_ms"] = timed(lambda: routed(m, ol, d_pa, d_pb, d_w, d_ra, d_rb, r, o))
    del r, o
    torch.cuda.empty_cache()
    # the bytes the kernel must move: eight source rows in, two rows out per output frame; a copy of n bytes reads n and writes n
    moved = 8 * bins * 10 * mt
    res[f"moved_gb_{name}"] = moved / 1e9
    c_src = torch.zeros(moved // 16, dtype=torch.float64, device="cuda")
    c_dst = torch.empty_like(c_src)
    res[f"copy_{name}_ms"] = timed(lambda: c_dst.copy_(c_src))
    del c_src, c_dst, d_pa, d_pb, d_w, d_ra, d_rb
    torch.cuda.empty_cache()

del a_sp, a_ap, b_sp, b_ap
torch.cuda.empty_cache()

# ---- batch Synthesis ----
syn = w.Synthesis(fs, fft, fp)
zero = [0] * n_pairs
ol = [syn.out_length(frames)] * n_pairs
d_y = torch.empty(sum(ol), dtype=torch.float64, device="cuda")
d_id = tensor(np.tile(maps["identity"][0], n_pairs))
res["compute_coded_ms"] = timed(lambda: syn.compute_coded_device(a_f0, fl, a_csp, nd, a_cap, ol, d_y, rng_pos=zero))
res["compute_coded_retimed_identity_ms"] = timed(lambda: syn.compute_coded_retimed_device(a_f0, fl, a_csp, nd, a_cap, fl, d_id, None, None, ol, d_y, rng_pos=zero))
if have["wc_synthesis_compute_coded_morphed_device"]:
    d_half = tensor(np.full(tot, 0.5))
    res["compute_coded_morphed_identity_ms"] = timed(lambda: syn.compute_coded_morphed_device(a_f0, fl, a_csp, a_cap, b_f0, fl, b_csp, b_cap, nd, fl, d_id, d_id, d_half,
                                                                                             None, None, None, ol, d_y, rng_pos=zero))
    res["compute_coded_retimed_identity_again_ms"] = timed(lambda: syn.compute_coded_retimed_device(a_f0, fl, a_csp, nd, a_cap, fl, d_id, None, None, ol, d_y,
                                                                                                   rng_pos=zero))
print(json.dumps(res))
