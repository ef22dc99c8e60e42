"""Warping along maps at the shapes DESIGN.md section 10 reports ("Warp streams"), all in one run and one process.  The samples are
seeded noise (the kernels' time does not depend on the values).  Every figure is the median of host-timed calls around a device
synchronisation, after warm-up calls; prints one JSON line:
  (a) <case>_chain_ms, _chain_again_ms   wc_warp_map_positions_device + wc_warp_device, before and behind the fused call: 64 utterances
                                         of 10 s at 44.1 kHz on maps of 2001 frames at a hop of 220.5 samples (441 001 outputs each), on
                                         the handle of section 10's first row (step_of(48000 / 44100))
      <case>_fused_ms                    wc_warp_along_map_device on the same batch and handle, between the two
      <case>_warp_alone_ms               wc_warp_device alone on the positions the chain has left
      <case>_fused_over_chain            against the mean of the chain's two runs; <case>_chain_spread: the chain's two runs apart,
                                         over their mean
      cases: forward (the map 0.97 i), reverse (the same played backwards), i16 (the forward map, int16 in and out)
  (b) stream_push_ms                     one push of 512 warp streams on 64 resident tracks of 10 s at 48 kHz (double), 4 entries per
                                         stream and push at a hop of 240 (960 outputs a stream, 20 ms of audio); stream_x_real_time:
                                         the audio of one push over the time of the push; _kernels_ms: its launches alone
    python tools/warp_stream_probe.py [reps]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # for the samples; imported before the library is loaded so that both use one HIP runtime

import world_class_amd as w
from world_class_amd import vresample as vr, warp, warp_stream as ws

L = w.lib()
L.wc_set_device(0)
args = [a for a in sys.argv[1:] if not a.startswith("--")]
reps = int(args[0]) if args else 20
WARM = 3


def timed(fn, warm=WARM, reps=reps):
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


def kernels_ms(fn, label):
    L.wc_set_kernel_timing(1)
    fn()
    L.wc_synchronize()
    t = float(L.wc_last_kernel_ms(label))
    L.wc_set_kernel_timing(0)
    return t


def noise(n, seed, dtype=torch.float64):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand(n, dtype=torch.float64, device="cuda", generator=g) * 2 - 1
    return (x * 32767).to(torch.int16) if dtype == torch.int16 else x


res = {"library": os.path.relpath(w.LIB_PATH), "reps": reps}

# ---- (a) the fused call against the chain it replaces ----
n_utt, n_in, frames, hop = 64, 441000, 2001, 220.5
step = vr.step_of(48000 / 44100)
r = vr.VResampler(step, step)
n_out = warp.map_out_length(frames, hop)
lengths, map_lengths, outs = [n_in] * n_utt, [frames] * n_utt, [n_out] * n_utt
d_x, d_x16 = noise(n_utt * n_in, 44100), noise(n_utt * n_in, 44100, torch.int16)
forward = torch.arange(frames, dtype=torch.float64, device="cuda") * 0.97
d_pos = torch.empty(n_utt * n_out, dtype=torch.int64, device="cuda")
d_y, d_y16 = torch.empty(n_utt * n_out, dtype=torch.float64, device="cuda"), torch.empty(n_utt * n_out, dtype=torch.int16, device="cuda")
for case, one_map, x, y, fmt in (("forward", forward, d_x, d_y, "f64"), ("reverse", torch.flip(forward, [0]), d_x, d_y, "f64"),
                                 ("i16", forward, d_x16, d_y16, "i16")):
    d_map = one_map.repeat(n_utt).contiguous()
    torch.cuda.synchronize()

    def chain():
        warp.map_positions_device(r, d_map, map_lengths, hop, hop, outs, d_pos)
        warp.warp_device(r, x, lengths, d_pos, outs, y, fmt, fmt)

    fused = lambda: ws.warp_along_map_device(r, x, lengths, d_map, map_lengths, hop, hop, outs, y, fmt, fmt)
    res[case + "_chain_ms"] = timed(chain)
    res[case + "_fused_ms"] = timed(fused)
    res[case + "_chain_again_ms"] = timed(chain)
    res[case + "_warp_alone_ms"] = timed(lambda: warp.warp_device(r, x, lengths, d_pos, outs, y, fmt, fmt))
    mean = (res[case + "_chain_ms"] + res[case + "_chain_again_ms"]) / 2
    res[case + "_fused_over_chain"] = res[case + "_fused_ms"] / mean
    res[case + "_chain_spread"] = abs(res[case + "_chain_ms"] - res[case + "_chain_again_ms"]) / mean
    res[case + "_fused_kernels_ms"] = kernels_ms(fused, b"warp_map_kernels")
    res[case + "_warp_kernels_ms"] = kernels_ms(chain, b"warp_kernels")
    del d_map
res["plan"] = list(vr.plan(step, step)) + list(warp.tiling(step, step))
r.close()
del d_x, d_x16, d_pos, d_y, d_y16

# ---- (b) 512 streams ----
n_streams, n_tracks, fs, hop, per_push = 512, 64, 48000, 240, 4
track_len = 10 * fs
h = ws.WarpStream(vr.ONE, vr.ONE, n_streams, n_tracks, track_len, per_push, 0, float(hop))
d_track = noise(track_len, 48000)
for t in range(n_tracks):
    h.set_track_device(t, track_len, d_track)
for u in range(n_streams):
    h.reset(u, u % n_tracks, 0, float(hop), float(hop))
d_out = torch.empty(n_streams * h.max_out_per_push, dtype=torch.float64, device="cuda")
rows = [per_push] * n_streams
# the maps of the pushes to come: every stream walks its track at 0.97 of its own rate, the streams a frame apart
at = torch.arange(per_push, dtype=torch.float64, device="cuda").repeat(n_streams) + torch.arange(n_streams, dtype=torch.float64, device="cuda").repeat_interleave(per_push)
maps = [((at + per_push * k) * 0.97).contiguous() for k in range(WARM + reps + 1)]
torch.cuda.synchronize()
k = [0]


def push():
    got = h.push_device(rows, maps[k[0]], d_out)
    k[0] += 1
    return got


res["stream_push_ms"] = timed(push)
res["stream_outputs_per_push"] = sum(push())
res["stream_x_real_time"] = (per_push * hop / fs * 1e3) / res["stream_push_ms"]
k[0] -= 1
res["stream_push_kernels_ms"] = kernels_ms(push, b"warp_map_kernels")
h.close()
print(json.dumps(res))
