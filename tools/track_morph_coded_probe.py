"""Coded track-morph streams at the shape of the live chain, beside the full-row handle in the same process: 512 concurrent streams
on ONE resident track of 2 000 rows, delay 20, the ring full, pushes of 1 and of 50 rows per stream, nd = 60, positions that are
half-integers and wander (tools/track_morph_probe.py's walk, in device memory as an alignment stream leaves them), weights that avoid
the copy paths -- at 24 kHz / fft 1024 (the workgroup decoders) and at 48 kHz / fft 2048 (the one-wavefront decoder).  Every figure
is the median of host-timed pushes around a device synchronisation, after warm-up pushes, in the steady state.  Prints one JSON line
with the rows that exist in the library it is given (WC_LIB_PATH), so the same script gives the full-row line on a build of the
parent commit (tools/ab_build.py); per size S = fft and push size R:
  S_coded_R_ms       wc_track_morph_coded_push_device; S_coded_R_host_ms: the part of it until the call returns; S_gather_R_ms /
                     S_decode_R_ms / S_blend_R_ms: track_gather_coded_kernel, the decoder over the 3 x frames scratch slots and
                     track_morph_coded_kernel alone in one more push (wc_last_kernel_ms)
  S_full_R_ms        wc_track_morph_push_device at the same counts, positions and weights on full rows (S_full_R_host_ms,
                     S_full_R_kernel_ms as in tools/track_morph_probe.py)
  S_coded_bytes_R    wc_track_morph_coded_device_bytes; S_coded_resident_R: its tracks + ring; S_full_resident_R: the full-row
                     handle's tracks + ring by its create's arithmetic, 8 (T + S) (1 + 2 bins)
    python tools/track_morph_coded_probe.py [n_streams] [pushes]"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # for the inputs; imported before the library is loaded so that both use one HIP runtime

import world_class_amd as w
from world_class_amd import codec, stream as wstream

L = w.lib()
codec._L()
tables = [wstream.STREAM_SIGNATURES, getattr(wstream, "TRACK_MORPH_SIGNATURES", {}), getattr(wstream, "TRACK_MORPH_CODED_SIGNATURES", {})]
for table in tables:  # (a library of the parent commit lacks the newest symbols: bind what it has here)
    for name, (res_, args) in table.items():
        fn = getattr(L, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res_, args
wstream._bound = True
raw = C.CDLL(w.LIB_PATH)
have_coded = hasattr(raw, "wc_track_morph_coded_push_device") and hasattr(wstream, "CodedTrackMorph")
have_full = hasattr(raw, "wc_track_morph_push_device") and hasattr(wstream, "TrackMorph")
L.wc_set_device(0)
m, delay, nd = 2000, 20, 60
n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
pushes = int(sys.argv[2]) if len(sys.argv) > 2 else 12
warm = 3
gen = torch.Generator(device="cuda").manual_seed(7)
res = {"library": os.path.relpath(w.LIB_PATH), "workload": f"{n} streams, one track of {m} rows, delay {delay}, nd {nd}", "pushes": pushes, "warm": warm}


def median(ts):
    return float(np.median(ts[warm:])) * 1e3


def sync():
    L.wc_synchronize()
    torch.cuda.synchronize()


def timed(call, kernels, total):
    """`total` calls, the last `pushes + 1` timed, the very last with the timing events: (median ms, median host ms, kernel ms ...)"""
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
    ms = [float(L.wc_last_kernel_ms(name)) for name in kernels]
    L.wc_set_kernel_timing(0)
    ts, host = ts[-(pushes + 1):-1], host[-(pushes + 1):-1]
    return [median(ts), median(host)] + ms


for fs, fft in ((24000, 1024), (48000, 2048)):
    bins, n_ap = fft // 2 + 1, codec.number_of_aperiodicities(fs)
    S = str(fft) + "_"

    def rows(count):
        """smooth envelopes (what a coder is for) and aperiodicities below 1: full rows, and their coded rows where the library codes"""
        f0 = 120.0 + 60.0 * torch.rand(count, dtype=torch.float64, device="cuda", generator=gen)
        f0[torch.rand(count, device="cuda", generator=gen) < 0.2] = 0.0
        x = torch.linspace(0.0, 1.0, bins, dtype=torch.float64, device="cuda")[None, :]
        a = torch.rand(count, 4, dtype=torch.float64, device="cuda", generator=gen)
        sp = (1e-4 * torch.exp(3.0 * a[:, 0:1] * torch.cos(6.0 * x + 6.0 * a[:, 1:2]) - 4.0 * x * a[:, 2:3])).reshape(-1).contiguous()
        ap = (0.001 + 0.99 * (0.1 + 0.8 * a[:, 3:4]) * (0.2 + 0.8 * x)).reshape(-1).contiguous()
        csp = torch.empty(count * nd, dtype=torch.float64, device="cuda")
        cap = torch.empty(count * n_ap, dtype=torch.float64, device="cuda")
        sync()
        codec.code_features_device(fs, fft, count, nd, sp, ap, csp, cap)
        sync()
        return (f0, sp, ap), (f0, csp, cap)

    track, ctrack = rows(m)
    for per_push in (1, 50):
        R = str(per_push)
        tot = n * per_push
        a, ca = rows(tot)
        o = [torch.empty(tot, dtype=torch.float64, device="cuda")] + [torch.empty(tot * bins, dtype=torch.float64, device="cuda") for _ in range(2)]
        fill = -(-delay // per_push)  # pushes until the ring is full
        total = fill + pushes + 1
        rng = np.random.default_rng(11)
        pace = rng.uniform(0.6, 1.7, n)
        walk = np.cumsum(np.round(rng.uniform(-1.0, 2.5, (n, total * per_push)) * 2) / 2 - 0.75, axis=1)
        pos = np.clip(np.round((pace[:, None] * np.arange(total * per_push)[None, :] + walk) * 2) / 2, 0.0, m - 1.0)
        d_pos = [torch.from_numpy(np.ascontiguousarray(pos[:, k * per_push:(k + 1) * per_push]).ravel()).cuda() for k in range(total)]
        res[S + "halves_" + R] = float((pos * 2 % 2 == 1).mean())
        counts = [per_push] * n

        def run(cls, extra, trk, voice, kernels):
            h = cls(fs, fft, *extra, n, 1, m, per_push, delay)
            h.set_track_device(0, m, *trk)
            for u in range(n):
                h.reset(u, 0, delay)
                h.set_weight(u, (0.25, 0.5, 0.75, 0.4)[u % 4])
            got = timed(lambda k: h.push_device(counts, voice[0], voice[1], voice[2], d_pos[k], *o), kernels, total)
            assert h.frames_formed(0) == total * per_push - delay and h.pending(0) == delay
            extra_bytes = h.device_bytes() if hasattr(h, "device_bytes") else None
            h.close()
            return got, extra_bytes

        # the two handles alternately, twice each: first / second run
        for turn in ("", "_again"):
            if have_coded:
                got, nbytes = run(wstream.CodedTrackMorph, (nd,), ctrack, ca, (b"track_gather_coded_kernel", b"track_morph_coded_decode", b"track_morph_coded_kernel"))
                for key, v in zip(("coded_%s_ms", "coded_%s_host_ms", "gather_%s_ms", "decode_%s_ms", "blend_%s_ms"), got):
                    res[S + key % R + turn] = v
                res[S + "coded_bytes_" + R] = nbytes
            if have_full:
                got, _ = run(wstream.TrackMorph, (), track, a, (b"track_morph_kernel",))
                for key, v in zip(("full_%s_ms", "full_%s_host_ms", "full_%s_kernel_ms"), got):
                    res[S + key % R + turn] = v
        cap_ = delay + min(delay, per_push)
        res[S + "coded_resident_" + R] = 8 * (m + n * cap_) * (1 + nd + n_ap)  # (each of its six arrays rounded up to 256 bytes)
        res[S + "full_resident_" + R] = 8 * (m + n * cap_) * (1 + 2 * bins)
        del a, ca, o, d_pos
        torch.cuda.empty_cache()
print(json.dumps(res))
