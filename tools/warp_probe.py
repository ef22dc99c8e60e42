"""Warping at the shapes DESIGN.md section 10 reports, beside the variable-ratio converter on the same batch and handle, all in one
run.  The samples are seeded noise (the kernels' time does not depend on the values).  Every figure is the median of host-timed calls
around a device synchronisation, after warm-up calls; prints one JSON line:
  arith_<name>_ms          wc_warp_device, 64 utterances of 10 s at 44.1 kHz, double in and out, at the positions n x step for
                           up = step_of(48000 / 44100) and half = 2^33; _kernels_ms: its launches alone, by the library's timing
                           events; _vresample_ms and _vresample_kernels_ms: wc_vresample_device on the same batch and handle;
                           _over_vresample: the ratio of the two calls; _i16_ms: int16 in and out
  far_ms, near_ms          the up batch with every utterance's positions in a random order (every tile far: its inputs come from
                           global memory) and in their own order (every tile near); far_over_near
  reverse_ms               the up batch played backwards (near tiles whose positions fall)
  map_ms                   wc_warp_map_positions_device, 64 maps of 2001 frames at a hop of 220.5 samples (441001 positions each);
                           map_copy_ms: a device-to-device copy of as many bytes as the positions
    python tools/warp_probe.py [reps]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # for the samples; imported before the library is loaded so that both use one HIP runtime

import world_class_amd as w
from world_class_amd import vresample as vr, warp

L = w.lib()
L.wc_set_device(0)
args = [a for a in sys.argv[1:] if not a.startswith("--")]
reps = int(args[0]) if args else 20


def timed(fn, warm=3, reps=reps):
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


def copy_ms(n_bytes):
    """a device-to-device copy that moves n_bytes in all: n_bytes / 2 read and as many written"""
    a = torch.empty(n_bytes // 2, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)

    def copy():
        b.copy_(a)
        torch.cuda.synchronize()

    t = timed(copy)
    del a, b
    return t


res = {"library": os.path.relpath(w.LIB_PATH), "reps": reps}
n_utt, seconds, fs_in = 64, 10, 44100
n_in = fs_in * seconds
d_x, d_x16 = noise(n_utt * n_in, fs_in), noise(n_utt * n_in, fs_in, torch.int16)
lengths = [n_in] * n_utt
for name, step in (("up", vr.step_of(48000 / 44100)), ("half", 1 << 33)):
    key = "arith_" + name
    n_out = vr.out_length(step, n_in)
    steps, outs = [step] * n_utt, [n_out] * n_utt
    r = vr.VResampler(step, step)
    d_pos = (torch.arange(n_out, dtype=torch.int64, device="cuda") * step).repeat(n_utt)
    d_y, d_y16 = torch.empty(n_utt * n_out, dtype=torch.float64, device="cuda"), torch.empty(n_utt * n_out, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    run_v = lambda: r.run_device(d_x, lengths, steps, d_y)
    run_w = lambda: warp.warp_device(r, d_x, lengths, d_pos, outs, d_y)
    res[key + "_vresample_ms"] = timed(run_v)
    res[key + "_ms"] = timed(run_w)
    res[key + "_vresample_again_ms"] = timed(run_v)   # (the converter before and behind the warp: the run's own drift)
    res[key + "_over_vresample"] = 2 * res[key + "_ms"] / (res[key + "_vresample_ms"] + res[key + "_vresample_again_ms"])
    res[key + "_vresample_kernels_ms"] = kernels_ms(run_v, b"vresample_kernels")
    res[key + "_kernels_ms"] = kernels_ms(run_w, b"warp_kernels")
    res[key + "_i16_ms"] = timed(lambda: warp.warp_device(r, d_x16, lengths, d_pos, outs, d_y16, "i16", "i16"))
    res[key + "_plan"] = list(vr.plan(step, step)) + list(warp.tiling(step, step))
    if name == "up":
        g = torch.Generator(device="cuda").manual_seed(5)
        d_far = torch.cat([d_pos[:n_out][torch.randperm(n_out, device="cuda", generator=g)] for _ in range(n_utt)])
        d_rev = torch.flip(d_pos[:n_out], [0]).repeat(n_utt)
        torch.cuda.synchronize()
        res["near_ms"] = res[key + "_ms"]
        res["far_ms"] = timed(lambda: warp.warp_device(r, d_x, lengths, d_far, outs, d_y))
        res["far_kernels_ms"] = kernels_ms(lambda: warp.warp_device(r, d_x, lengths, d_far, outs, d_y), b"warp_kernels")
        res["far_over_near"] = res["far_ms"] / res["near_ms"]
        res["reverse_ms"] = timed(lambda: warp.warp_device(r, d_x, lengths, d_rev, outs, d_y))
        del d_far, d_rev
        frames, hop = 2001, 220.5
        n_map = warp.map_out_length(frames, hop)
        d_map = (torch.arange(frames, dtype=torch.float64, device="cuda") * 0.97).repeat(n_utt)
        d_mp = torch.empty(n_utt * n_map, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        res["map_ms"] = timed(lambda: warp.map_positions_device(r, d_map, [frames] * n_utt, hop, hop, [n_map] * n_utt, d_mp))
        res["map_copy_ms"] = copy_ms(2 * 8 * n_utt * n_map)
        del d_map, d_mp
    r.close()
    del d_pos, d_y, d_y16
print(json.dumps(res))
