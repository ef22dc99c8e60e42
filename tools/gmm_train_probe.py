"""One EM iteration of the GMM trainer over 100 000 joint rows at D = 48, 96 and 160 and n_mix = 32 and 128, against the way a caller
without the trainer has to do it on the same device: wc_gmm_convert_device's d_loglik on the joint rows (a Gmm of dx = D next to one
dimension of its own), then torch float64 softmax and, per mixture, the weighted sums as matrix products (torch.einsum over all
mixtures at once would hold n * n_mix * D doubles).  The model is seeded and well conditioned, the rows lie around its means; the
kernels' time does not depend on the values.  Every call is host-timed around a device synchronisation after two warm-up calls; median
and spread (min, max) in one JSON line, per shape:
  accumulate_ms       wc_gmm_trainer_accumulate_device (E-step and statistics), its kernels alone by the library's timing events, and
                      the statistics kernel's fraction of the floor: n * n_mix * D(D+1)/2 multiply-add pairs, D multiplies by gamma,
                      at half the 78.6 TFLOP/s vector peak
  update_ms           stats to the host, the M-step, the model back on the device
  torch_ms            the caller's way: ll by convert, softmax, and the statistics by matmul; and the einsum-side alone
    python tools/gmm_train_probe.py [reps]
    python tools/gmm_train_probe.py --ulp     the largest distance in ulp between the device library's exp and log (torch float64 on the
                                              device calls the same functions) and libm's, on the arguments the trainer's tests use"""
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # for the inputs; imported before the library is loaded so that both use one HIP runtime

import world_class_amd as w
from world_class_amd import gmm, gmm_train

L = w.lib()
L.wc_set_device(0)
PEAK_NO_FMA = 0.5 * 78.6e12


def ulp_distance(got, want):
    a, b = got.view(np.int64), want.view(np.int64)
    return int(np.abs(a - b).max())


def ulp():
    rng = np.random.default_rng(0)
    args = np.concatenate([-rng.uniform(0.0, 745.0, size=400000), -np.exp(rng.uniform(-40.0, 6.6, size=400000)), [0.0, -0.0, -745.0, -1e-300]])
    s = np.concatenate([rng.uniform(1.0, 1024.0, size=400000), 1.0 + np.exp(rng.uniform(-40.0, 0.0, size=400000)), [1.0, 2.0, 1024.0]])
    dev_exp = torch.exp(torch.from_numpy(args).cuda()).cpu().numpy()
    dev_log = torch.log(torch.from_numpy(s).cuda()).cpu().numpy()
    host_exp = np.array([math.exp(v) for v in args])
    host_log = np.array([math.log(v) for v in s])
    normal = host_exp >= 2.0 ** -1022
    print(json.dumps({"exp_max_ulp": ulp_distance(dev_exp[normal], host_exp[normal]), "exp_subnormal_max_ulp": ulp_distance(dev_exp[~normal], host_exp[~normal]),
                      "log_max_ulp": ulp_distance(dev_log, host_log), "arguments": int(args.size + s.size)}))


def timed(fn, reps, warm=2):
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


def model(n_mix, D, seed):
    rng = np.random.default_rng(seed)
    G = rng.normal(size=(n_mix, D, D))
    return rng.uniform(0.5, 1.5, size=n_mix), rng.normal(size=(n_mix, D)), np.eye(D)[None] + G @ G.transpose(0, 2, 1) / D


def torch_statistics(post, x, mean):
    """per mixture: N, S1 and S2 centred on the model's mean, as two matrix products"""
    out = []
    for m in range(mean.shape[0]):
        d = x - mean[m][None]
        g = post[:, m, None] * d
        out.append((post[:, m].sum(), g.sum(dim=0), g.T @ d))
    return out


def shape(n, D, n_mix, reps, seed):
    weight, mean, cov = model(n_mix, D, seed)
    rng = np.random.default_rng(seed + 1)
    rows = mean[rng.integers(0, n_mix, size=n)] + 0.7 * rng.standard_normal((n, D))
    d_rows = torch.from_numpy(rows.ravel()).cuda()
    t = gmm_train.GmmTrainer(n_mix, D // 2, D - D // 2)
    t.set_model(weight, mean, cov)
    res = {"workload": f"{n} frames, D {D}, n_mix {n_mix}"}

    def acc():
        t.reset_stats()
        t.accumulate(n, d_rows, D)

    res["accumulate_ms"] = timed(acc, reps)
    t.set_segments_per_launch((n + 1023) // 1024)      # one launch, so that the timing events cover the whole call
    res["accumulate_kernels_ms"] = kernel_ms(acc, ("gmm_ll_kernel", "gmm_post_kernel", "gmm_stats_kernel"))
    res["accumulate_one_launch_ms"] = timed(acc, reps)
    t.set_segments_per_launch(0)
    floor_ms = n * n_mix * (D * (D + 1) + D) / PEAK_NO_FMA * 1e3
    res["stats_floor_ms"] = floor_ms
    res["stats_fraction_of_floor"] = floor_ms / res["accumulate_kernels_ms"]["gmm_stats_kernel"]
    res["kernels_share_of_call"] = sum(res["accumulate_kernels_ms"].values()) / res["accumulate_one_launch_ms"]["median"]

    def iteration():
        t.accumulate(n, d_rows, D)
        t.update()
        t.set_model(weight, mean, cov)      # (the same model every time)

    res["iteration_ms"] = timed(iteration, max(3, reps // 3), warm=1)
    # the caller's way
    big = np.zeros((n_mix, D + 1, D + 1))
    big[:, :D, :D], big[:, D, D] = cov, 1.0
    g = gmm.Gmm(weight, np.concatenate([mean, np.zeros((n_mix, 1))], axis=1), big, D)
    d_ll = torch.empty(n * n_mix, dtype=torch.float64, device="cuda")
    t_mean = torch.from_numpy(mean).cuda()
    x = d_rows.view(n, D)

    def caller():
        g.convert(n, d_rows, D, None, None, 1, d_loglik=d_ll)
        L.wc_synchronize()
        post = torch.softmax(d_ll.view(n, n_mix), dim=1)
        return torch_statistics(post, x, t_mean)

    res["torch_ms"] = timed(caller, reps)
    post = torch.softmax(d_ll.view(n, n_mix), dim=1)
    res["torch_statistics_ms"] = timed(lambda: torch_statistics(post, x, t_mean), reps)
    res["torch_statistics_over_stats_kernel"] = res["torch_statistics_ms"]["median"] / res["accumulate_kernels_ms"]["gmm_stats_kernel"]
    res["torch_over_accumulate"] = res["torch_ms"]["median"] / res["accumulate_ms"]["median"]
    acc()
    N, S1, S2, info = t.stats()
    ref = torch_statistics(post, x, t_mean)
    full = np.zeros((D, D))
    full[np.tril_indices(D)] = S2[0]
    res["S2_max_rel_diff_to_torch"] = float(np.abs(np.tril(full) - np.tril(ref[0][2].cpu().numpy())).max() / np.abs(full).max())
    res["N_max_diff_to_torch"] = float(max(abs(N[m] - float(ref[m][0])) for m in range(n_mix)))
    g.close()
    t.close()
    return res


if "--ulp" in sys.argv:
    ulp()
else:
    reps = max(5, int(sys.argv[1])) if len(sys.argv) > 1 else 7
    out = {"library": os.path.relpath(w.LIB_PATH), "reps": reps}
    for D in (48, 96, 160):
        for n_mix in (32, 128):
            out[f"D{D}_M{n_mix}"] = shape(100000, D, n_mix, reps, D + n_mix)
            L.wc_release_scratch()
            torch.cuda.empty_cache()
    print(json.dumps(out))
