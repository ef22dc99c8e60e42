"""Variable-ratio sample-rate conversion at the shapes DESIGN.md section 10 reports, beside the rational converter at the nearest
rational conversion and a device-to-device copy of the same bytes, all in one run.  The samples are seeded noise (the kernels' time
does not depend on the values).  Every figure is the median of host-timed calls around a device synchronisation, after warm-up calls;
prints one JSON line:
  batch_<name>_ms                wc_vresample_device, 64 utterances of 10 s at 44.1 kHz, double in and out, at the steps
                                 up = step_of(48000 / 44100), one_plus = 2^32 + 1 (one segment holds a whole tile) and half = 2^33;
                                 _kernels_ms: its launches alone, by the library's timing events; _i16_ms: int16 in and int16 out;
                                 _rational_ms: wc_resample_device at 44.1 -> 48 kHz (up, one_plus: as many taps and about as many
                                 outputs) and 48 -> 24 kHz (half); _copy_ms: a device-to-device copy of as many bytes as the call
                                 reads and writes together; _over_rational: the ratio of the two calls
  batch_up_<B>_<D>_ms            the same call at up with the other tables: (4, 5), (2, 7) and (8, 3) against the default (3, 5)
  push_ms, push_short_ms         wc_vresample_stream_push_device, 512 streams at step_of(24000 / 44100 x 1.00002), 200 ms
                                 (8820 samples) and 10 ms (441 samples, the plain mapping) each; _rational_ms:
                                 wc_resample_stream_push_device at 44.1 -> 24 kHz; push_copy_ms as above
With WC_LIB_PATH at a variant built with -DWC_VR_FORCE_PLAIN=1 (tools/ab_build.py) the same run measures the plain mapping alone.
    python tools/vresample_probe.py [reps]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # for the samples; imported before the library is loaded so that both use one HIP runtime

import world_class_amd as w
from world_class_amd import resample as rs, vresample as vr

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


def rational_batch_ms(fs_in, fs_out, n_utt, seconds):
    n_in = fs_in * seconds
    r = rs.Resampler(fs_in, fs_out)
    d_x, d_y = noise(n_utt * n_in, fs_in), torch.empty(n_utt * rs.out_length(fs_in, fs_out, n_in), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    lengths = [n_in] * n_utt
    t = timed(lambda: r.run_device(d_x, lengths, d_y))
    r.close()
    return t


res = {"library": os.path.relpath(w.LIB_PATH), "reps": reps}
n_utt, seconds, fs_in = 64, 10, 44100
n_in = fs_in * seconds
d_x, d_x16 = noise(n_utt * n_in, fs_in), noise(n_utt * n_in, fs_in, torch.int16)
lengths = [n_in] * n_utt
rational = {}
# name -> (the step, its handle's range, the rational conversion beside it)
BATCH = {"up": (vr.step_of(48000 / 44100), (44100, 48000)), "one_plus": (vr.ONE + 1, (44100, 48000)), "half": (1 << 33, (48000, 24000))}
for name, (step, conv) in BATCH.items():
    key = "batch_" + name
    n_out = vr.out_length(step, n_in)
    steps = [step] * n_utt
    r = vr.VResampler(step, step)
    d_y, d_y16 = torch.empty(n_utt * n_out, dtype=torch.float64, device="cuda"), torch.empty(n_utt * n_out, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    res[key + "_ms"] = timed(lambda: r.run_device(d_x, lengths, steps, d_y))
    L.wc_set_kernel_timing(1)
    r.run_device(d_x, lengths, steps, d_y)
    L.wc_synchronize()
    res[key + "_kernels_ms"] = float(L.wc_last_kernel_ms(b"vresample_kernels"))
    L.wc_set_kernel_timing(0)
    res[key + "_i16_ms"] = timed(lambda: r.run_device(d_x16, lengths, steps, d_y16, "i16", "i16"))
    res[key + "_plan"] = list(vr.plan(step, step)) + list(vr.tiling(step, step))
    r.close()
    del d_y, d_y16
    if conv not in rational:
        rational[conv] = rational_batch_ms(*conv, n_utt, seconds)
    res[key + "_rational_ms"] = rational[conv]
    res[key + "_over_rational"] = res[key + "_ms"] / rational[conv]
    res[key + "_copy_ms"] = copy_ms(8 * n_utt * (n_in + n_out))

step = BATCH["up"][0]
steps = [step] * n_utt
d_y = torch.empty(n_utt * vr.out_length(step, n_in), dtype=torch.float64, device="cuda")
for bits, degree in ((3, 5), (4, 5), (2, 7), (8, 3)):
    r = vr.VResampler(step, step, phase_bits=bits, degree=degree)
    res["batch_up_%d_%d_ms" % (bits, degree)] = timed(lambda: r.run_device(d_x, lengths, steps, d_y))
    r.close()
del d_x, d_x16, d_y

fs_out, n_streams = 24000, 512
step = vr.step_of(fs_out / fs_in * 1.00002)
for key, n_new in (("push", 8820), ("push_short", 441)):
    s = vr.VResampleStream(step, step, n_streams, n_new)
    d_c = noise(n_streams * n_new, 7)
    d_y = torch.empty(n_streams * s.max_out_per_push, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    counts = [n_new] * n_streams
    res[key + "_ms"] = timed(lambda: s.push_device(counts, d_c, None, d_y))
    s.close()
    q = rs.ResampleStream(fs_in, fs_out, n_streams, n_new)
    res[key + "_rational_ms"] = timed(lambda: q.push_device(counts, d_c, None, d_y))
    q.close()
    res[key + "_over_rational"] = res[key + "_ms"] / res[key + "_rational_ms"]
    if n_new == 8820:
        res["push_copy_ms"] = copy_ms(8 * n_streams * (n_new + vr.out_length(step, n_new)))
    del d_c, d_y
print(json.dumps(res))
