"""Frame filtering: 64 utterances of 10 s with one row of power gains per 5 ms frame, at 48 kHz (fft_size 2048) and at 16 kHz (1024).
The gains are exp of a smooth random log envelope (+-12 dB), made on the device; the kernels' time does not depend on the values.
Every call is host-timed around a device synchronisation after two warm-up calls; median and spread (min, max) of the timed calls
in one JSON line, per rate:
  run_ms      wc_frame_filter_run_device (WC_FILTER_POWER) into a separate output, and its two kernels alone by the library's timing
              events; block_ms the same under WC_FILTER_KERNEL=block
  torch_ms    the same rule written with torch.fft on the same device, which is what a caller without the call has to do: the weighted
              segments gathered in one indexing step, rfft, the minimum phase by two more transforms and exp, the product, irfft, and an
              index_add_ for the overlap-add; a few utterances at a time, so that its temporaries stay below 4 GB.  Its ratio to run_ms,
              and the largest difference between the two results
    python tools/filter_probe.py [reps]"""
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # for the inputs; imported before the library is loaded so that both use one HIP runtime

import world_class_amd as w
from world_class_amd import filter as ff

L = w.lib()
L.wc_set_device(0)
reps = max(5, int(sys.argv[1])) if len(sys.argv) > 1 else 7
n_utt, seconds, fp = 64, 10.0, 5.0


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
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts))}


def kernel_ms(fn, names):
    L.wc_set_kernel_timing(1)
    fn()
    L.wc_synchronize()
    out = {n: float(L.wc_last_kernel_ms(n.encode())) for n in names}
    L.wc_set_kernel_timing(0)
    return out


def centre(t, fs):
    return int(math.floor((float(t) * fp) * float(fs) / 1000.0 + 0.5))


def torch_plan(n, S, fs, N):
    """the gather of the rule for utterances of n samples: for every segment and j < 2 ceil(h) - 1 the sample a_t + j (clamped), its
    weight (0.0 outside the span), and the outputs a_t + j, j < N, with those at or beyond n sent to a bin behind the signal"""
    lmax = 2 * math.ceil(fp * fs / 1000.0) - 1
    c = np.array([centre(t, fs) for t in range(-1, S + 1)], dtype=np.int64)   # c[t + 1] = c_t
    cm, c0, cp = c[:-2], c[1:-1], c[2:]
    a = np.where(np.arange(S) > 0, cm + 1, 0)
    b = np.minimum(n - 1, cp - 1)
    k = a[:, None] + np.arange(lmax)[None]
    up = (k - cm[:, None]) / np.maximum(c0 - cm, 1)[:, None].astype(np.float64)
    down = 1.0 - (k - c0[:, None]) / (cp - c0)[:, None].astype(np.float64)
    wgt = np.where(k < c0[:, None], up, np.where(k == c0[:, None], 1.0, down)) * (k <= b[:, None])
    out = a[:, None] + np.arange(N)[None]
    out = np.where(out < n, out, n)
    dev = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v, dtype=dt)).cuda()
    return dev(np.minimum(k, n - 1), np.int64), dev(wgt, np.float64), dev(out, np.int64)


def torch_filter(x, gains, plan, N, n, S, step):
    """x [U, n], gains [U, S, N/2+1] -> y [U, n] by the rule with torch.fft"""
    idx, wgt, out = plan
    m = N // 2
    ys = []
    for o in range(0, x.shape[0], step):
        xs, g = x[o:o + step], gains[o:o + step]
        U = xs.shape[0]
        seg = xs[:, idx] * wgt[None]                                     # [U, S, lmax]
        ls = torch.log(g) / 2.0
        cep = torch.fft.irfft(ls.to(torch.complex128), n=N, dim=-1)      # the real even sequence's transform, / N
        cep[..., 1:m] *= 2.0
        cep[..., m + 1:] = 0.0
        resp = torch.exp(torch.fft.rfft(cep, n=N, dim=-1))               # the minimum-phase spectrum in the e^{-i} convention
        r = torch.fft.irfft(torch.fft.rfft(seg, n=N, dim=-1) * resp, n=N, dim=-1)
        y = torch.zeros((U, n + 1), dtype=torch.float64, device=x.device)
        y.view(-1).index_add_(0, (out[None] + (n + 1) * torch.arange(U, device=x.device)[:, None, None]).reshape(-1), r.reshape(-1))
        ys.append(y[:, :n])
    return torch.cat(ys)


def rate(fs, N, step):
    n = int(seconds * fs)
    h = ff.FrameFilter(fs, N, fp)
    S = h.segments(n)
    gen = torch.Generator(device="cuda").manual_seed(fs)
    x = torch.randn((n_utt, n), dtype=torch.float64, device="cuda", generator=gen)
    knots = torch.randn((n_utt * S, 1, 17), dtype=torch.float64, device="cuda", generator=gen)
    ls = torch.nn.functional.interpolate(knots, size=N // 2 + 1, mode="linear", align_corners=True)[:, 0] * 0.7   # nepers: +-12 dB at 2 sigma
    gains = torch.exp(2.0 * ls).contiguous()
    del knots, ls
    lengths, f_lengths = [n] * n_utt, [S] * n_utt
    d_y = torch.empty(n_utt * n, dtype=torch.float64, device="cuda")
    res = {"workload": f"{n_utt} x {seconds:g} s at {fs} Hz, {S} segments each, fft_size {N}, rows of {N // 2 + 1} doubles",
           "response_rows_mb": n_utt * S * N * 8 / 2 ** 20}
    run = lambda: h.run(x, lengths, gains, f_lengths, d_y, "power")
    res["run_ms"] = timed(run)
    names = ("filter_segment_wave_kernel", "filter_overlap_add_kernel")
    res["run_kernels_ms"] = kernel_ms(run, names)
    os.environ["WC_FILTER_KERNEL"] = "block"
    hb = ff.FrameFilter(fs, N, fp)
    os.environ.pop("WC_FILTER_KERNEL")
    runb = lambda: hb.run(x, lengths, gains, f_lengths, d_y, "power")
    res["block_ms"] = timed(runb)
    res["block_kernels_ms"] = kernel_ms(runb, ("filter_segment_kernel", "filter_overlap_add_kernel"))
    hb.close()
    plan = torch_plan(n, S, fs, N)
    g3 = gains.view(n_utt, S, N // 2 + 1)
    res["torch_ms"] = timed(lambda: torch_filter(x, g3, plan, N, n, S, step))
    res["torch_over_run"] = res["torch_ms"]["median"] / res["run_ms"]["median"]
    run()
    L.wc_synchronize()
    y_t = torch_filter(x, g3, plan, N, n, S, step)
    res["max_diff_to_torch"] = float((y_t.reshape(-1) - d_y).abs().max())
    res["max_abs_y"] = float(d_y.abs().max())
    res["finite"] = bool(torch.isfinite(d_y).all())
    h.close()
    return res


out = {"library": os.path.relpath(w.LIB_PATH), "reps": reps, "48k": rate(48000, 2048, 4), "16k": rate(16000, 1024, 16)}
print(json.dumps(out))
