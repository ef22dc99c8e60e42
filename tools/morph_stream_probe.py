"""Morph streams at the shape of tools/synth_stream_probe.py: 512 concurrent 24 kHz streams (fft 1024), 1 ms frames, 200 source
frames of each voice per stream and push, both voices at speed 0.97 (fractional positions: four source rows per voice and frame,
about 206 frames formed per stream and push), weights that avoid the copy paths.  Every figure is the median of host-timed pushes
around a device synchronisation, after warm-up pushes; prints one JSON line with the rows that exist in the library it is given
(WC_LIB_PATH), so the same script runs on a build of the parent commit (tools/ab_build.py):
  push_ms          wc_morph_stream_push_device, full rows; push_host_ms: the part of it until the call returns (the rule, the
                   records, the enqueue); kernel_ms: morph_stream_kernel alone in one more push (wc_last_kernel_ms)
  push_ratio_ms    the same with a spectral ratio per voice on every stream (the variant with shared memory)
  push_coded_ms    wc_morph_stream_push_coded_device, 40 coefficients and the bands per frame (decode in front of the same launch)
  routed_ms        what a caller builds without the handle: torch copies that glue every stream's kept rows in front of its new rows
                   and keep the rows of the next push, the positions uploaded, then one wc_morph_parameters_device call with one pair
                   per stream; routed_ratio_ms: the same with ratios
  copy_ms          a device-to-device copy that moves the bytes the kernel must move (per formed frame eight source rows read and two
                   written, per kept row two read and two written: a copy of half their sum reads and writes as much)
    python tools/morph_stream_probe.py [n_streams] [pushes]"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # for the routed form and the plain copy; imported before the library is loaded so that both use one HIP runtime

import world_class_amd as w
from world_class_amd import codec, io as wio
from world_class_amd import stream as wstream

L = w.lib()
for name, (res, args) in wstream.STREAM_SIGNATURES.items():  # (a library of the parent commit lacks the newest symbols: bind what
    fn = getattr(L, name, None)                              # it has here, the module's table stays as it is)
    if fn is not None:
        fn.restype, fn.argtypes = res, args
wstream._bound = True
have = hasattr(C.CDLL(w.LIB_PATH), "wc_morph_stream_push_device")
L.wc_set_device(0)
fs, fft, nd, per_push, speed = 24000, 1024, 40, 200, 0.97
n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
pushes = int(sys.argv[2]) if len(sys.argv) > 2 else 9
warm = 3
bins, n_ap = fft // 2 + 1, codec.number_of_aperiodicities(fs)
max_frames = int(per_push / speed) + 2
tot = n * per_push
gen = torch.Generator(device="cuda").manual_seed(5)


def voice():
    """one push of a voice for every stream: F0 (a fifth unvoiced), coded rows, and the rows the decoder makes of them"""
    f0 = 120.0 + 60.0 * torch.rand(tot, dtype=torch.float64, device="cuda", generator=gen)
    f0[torch.rand(tot, device="cuda", generator=gen) < 0.2] = 0.0
    sp = 1e-4 + 1e-2 * torch.rand(tot * bins, dtype=torch.float64, device="cuda", generator=gen)
    ap = 0.001 + 0.99 * torch.rand(tot * bins, dtype=torch.float64, device="cuda", generator=gen)
    csp, cap = torch.empty(tot * nd, dtype=torch.float64, device="cuda"), torch.empty(tot * n_ap, dtype=torch.float64, device="cuda")
    codec.code_spectral_envelope_device(fs, fft, tot, nd, sp, csp)
    codec.code_aperiodicity_device(fs, fft, tot, ap, cap)
    codec.decode_features_device(fs, fft, tot, nd, csp, cap, sp, ap)
    L.wc_synchronize()
    return f0, sp, ap, csp, cap


a, b = voice(), voice()
cap_rows = n * max_frames
o = [torch.empty(cap_rows, dtype=torch.float64, device="cuda")] + [torch.empty(cap_rows * bins, dtype=torch.float64, device="cuda") for _ in range(2)]
res = {"library": os.path.relpath(w.LIB_PATH), "workload": f"{n} streams x 24 kHz, fft {fft}, {per_push} source frames per voice, stream and push, speed {speed}",
       "pushes": pushes, "warm": warm}


def median(ts):
    return float(np.median(ts[warm:])) * 1e3


def sync():
    L.wc_synchronize()
    torch.cuda.synchronize()


# ---- the rule on the host (every stream moves in lockstep): positions, rows kept ----
def plan():
    """per push: the positions of the frames formed (absolute), the first row kept before and after it"""
    out, F, last, formed, keep = [], 0, 0.0, False, 0
    for _ in range(pushes):
        F += per_push
        pos = []
        while True:
            p = last + speed if formed else 0.0
            if not p <= F - 1:
                break
            pos.append(p)
            last, formed = p, True
        keep_new = int(np.floor(last))
        out.append((np.array(pos), keep, keep_new, F))
        keep = keep_new
    return out


steps = plan()
res["frames_formed_per_stream_and_push"] = len(steps[-1][0])

if have:
    from world_class_amd.stream import MorphStream

    def stream_run(ratio, coded):
        h = MorphStream(fs, fft, n, max_frames, 16)
        for u in range(n):
            h.set_speeds(u, speed, speed)
            h.set_weight(u, (0.25, 0.5, 0.75, 0.4)[u % 4])
            h.set_ratios(u, *((1.2, 0.8) if ratio else (0.0, 0.0)))
        counts, ts, host = [per_push] * n, [], []
        for k in range(pushes + 1):
            if k == pushes:  # one more push with the timing events: the kernel alone
                L.wc_set_kernel_timing(1)
            sync()
            t0 = time.perf_counter()
            if coded:
                h.push_coded_device(counts, a[0], a[3], a[4], counts, b[0], b[3], b[4], nd, *o)
            else:
                h.push_device(counts, a[0], a[1], a[2], counts, b[0], b[1], b[2], *o)
            t1 = time.perf_counter()
            sync()
            ts.append(time.perf_counter() - t0)
            host.append(t1 - t0)
        kernel = float(L.wc_last_kernel_ms(b"morph_stream_kernel"))
        L.wc_set_kernel_timing(0)
        return median(ts[:-1]), median(host[:-1]), kernel

    res["push_ms"], res["push_host_ms"], res["kernel_ms"] = stream_run(False, False)
    res["push_ratio_ms"], _, res["kernel_ratio_ms"] = stream_run(True, False)
    res["push_coded_ms"], _, _ = stream_run(False, True)


# ---- the routed form: glue, keep, upload, one wc_morph_parameters_device call ----
def routed_run(ratio):
    kept = [[torch.empty(0, dtype=torch.float64, device="cuda") for _ in range(3)] for _ in range(2)]  # per voice: f0, sp, ap of the kept rows
    widths = (1, bins, bins)
    d_w = torch.tensor([(0.25, 0.5, 0.75, 0.4)[u % 4] for u in range(n)], dtype=torch.float64, device="cuda")
    ts = []
    for pos, keep, keep_new, F in steps:
        sync()
        t0 = time.perf_counter()
        have_rows = F - per_push - keep  # rows every stream kept
        glued = []
        for x, v in enumerate((a, b)):
            g = []
            for q, wd in enumerate(widths):
                t = torch.empty((n, have_rows + per_push, wd), dtype=torch.float64, device="cuda")
                if have_rows:
                    t[:, :have_rows] = kept[x][q].view(n, have_rows, wd)
                t[:, have_rows:] = v[q].view(n, per_push, wd)
                kept[x][q] = t[:, keep_new - keep:].contiguous()
                g.append(t)
            glued.append(g)
        m = len(pos)
        rel = torch.from_numpy(np.tile(pos - keep, n)).cuda()
        wt = d_w.repeat_interleave(m)
        ra = torch.full((n * m,), 1.2, dtype=torch.float64, device="cuda") if ratio else None
        rb = torch.full((n * m,), 0.8, dtype=torch.float64, device="cuda") if ratio else None
        ln = [have_rows + per_push] * n
        wio.morph_parameters_device(fs, fft, ln, *glued[0], ln, *glued[1], [m] * n, rel, rel, wt, None, ra, rb, *o)
        sync()
        ts.append(time.perf_counter() - t0)
    return median(ts)


res["routed_ms"] = routed_run(False)
res["routed_ratio_ms"] = routed_run(True)
# the bytes the kernel must move: per formed frame eight source rows in and two out, per kept row two in and two out
formed, keeps = n * len(steps[-1][0]), 2 * n * (steps[-1][3] - steps[-1][2])
moved = 8 * bins * (10 * formed + 4 * keeps)
res["moved_gb"] = moved / 1e9
c_src = torch.zeros(moved // 16, dtype=torch.float64, device="cuda")
c_dst = torch.empty_like(c_src)
ts = []
for _ in range(pushes):
    sync()
    t0 = time.perf_counter()
    c_dst.copy_(c_src)
    sync()
    ts.append(time.perf_counter() - t0)
res["copy_ms"] = median(ts)
print(json.dumps(res))
