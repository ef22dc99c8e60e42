"""Sample-rate conversion at the shapes DESIGN.md section 10 reports.  The samples are seeded noise (the kernels' time does not depend
on the values).  Every figure is the median of host-timed calls around a device synchronisation, after warm-up calls; prints one JSON
line:
  batch_<in>_<out>_ms            wc_resample_device, 64 utterances of 10 s, double in and out, at 44.1 -> 48, 48 -> 24 and 48 -> 44.1 kHz
                                 (the last: M = 160, the padded tile); _kernels_ms: its launches alone, by the
                                 library's timing events; _copy_ms: a device-to-device copy of as many bytes as the call reads and
                                 writes together (half of them read, half written); _i16_ms: int16 in and int16 out
  push_44100_24000_ms            wc_resample_stream_push_device, 512 streams, 200 ms (8820 samples) each, double in and out;
                                 _copy_ms as above; _short_ms: the same streams with 10 ms pushes (the plain mapping)
  pipeline_step_ms               ms_per_step of `bench.py --gpus 1` (the flagship workload, 64 x 10 s at 48 kHz), in a process of its own
  stream_push_ms                 the push of bench.py's config 5 (512 analysis streams at 24 kHz, 200 ms, whole windows)
  ratio_*                        the conversions over those two
    python tools/resample_probe.py [reps] [--no-bench]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # for the samples; imported before the library is loaded so that both use one HIP runtime

import world_class_amd as w
from world_class_amd import resample as rs

L = w.lib()
L.wc_set_device(0)
args = [a for a in sys.argv[1:] if not a.startswith("--")]
reps = int(args[0]) if args else 20
with_bench = "--no-bench" not in sys.argv


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


res = {"library": os.path.relpath(w.LIB_PATH), "reps": reps}
n_utt, seconds = 64, 10
for fs_in, fs_out in ((44100, 48000), (48000, 24000), (48000, 44100)):
    key = f"batch_{fs_in}_{fs_out}"
    n_in = fs_in * seconds
    n_out = rs.out_length(fs_in, fs_out, n_in)
    r = rs.Resampler(fs_in, fs_out)
    d_x, d_y = noise(n_utt * n_in, fs_in), torch.empty(n_utt * n_out, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    lengths = [n_in] * n_utt
    res[key + "_ms"] = timed(lambda: r.run_device(d_x, lengths, d_y))
    L.wc_set_kernel_timing(1)
    r.run_device(d_x, lengths, d_y)
    L.wc_synchronize()
    res[key + "_kernels_ms"] = float(L.wc_last_kernel_ms(b"resample_kernels"))
    L.wc_set_kernel_timing(0)
    res[key + "_copy_ms"] = copy_ms(8 * n_utt * (n_in + n_out))
    d_x16, d_y16 = noise(n_utt * n_in, fs_in, torch.int16), torch.empty(n_utt * n_out, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    res[key + "_i16_ms"] = timed(lambda: r.run_device(d_x16, lengths, d_y16, "i16", "i16"))
    res[key + "_plan"] = list(rs.plan(fs_in, fs_out)) + list(rs.tiling(fs_in, fs_out))
    r.close()
    del d_x, d_y, d_x16, d_y16

fs_in, fs_out, n_streams = 44100, 24000, 512
for key, n_new in (("push_44100_24000", 8820), ("push_44100_24000_short", 441)):
    s = rs.ResampleStream(fs_in, fs_out, n_streams, n_new)
    d_c = noise(n_streams * n_new, 7)
    d_y = torch.empty(n_streams * s.max_out_per_push, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    counts = [n_new] * n_streams
    res[key + "_ms"] = timed(lambda: s.push_device(counts, d_c, None, d_y))
    if n_new == 8820:
        res[key + "_copy_ms"] = copy_ms(8 * n_streams * (n_new + rs.out_length(fs_in, fs_out, n_new)))
    s.close()
    del d_c, d_y
torch.cuda.empty_cache()

if with_bench:
    sys.path.insert(0, ROOT)
    import bench
    c5 = bench.stage_config5(w, L, torch, torch.device("cuda:0"))
    res["stream_push_ms"] = c5["whole_windows"]["push_ms"]
    L.wc_release_scratch()
    torch.cuda.empty_cache()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3"], check=True,
                         stdout=subprocess.PIPE, text=True).stdout
    res["pipeline_step_ms"] = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])["ms_per_step"]
    for k in ("batch_44100_48000", "batch_48000_24000"):
        res["ratio_" + k + "_over_pipeline_step"] = res[k + "_ms"] / res["pipeline_step_ms"]
    res["ratio_push_over_stream_push"] = res["push_44100_24000_ms"] / res["stream_push_ms"]
print(json.dumps(res))
