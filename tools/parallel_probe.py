"""Times the three calls of include/world_class_parallel.h on a corpus-sized batch against what a caller does without them for the same
joint rows: synchronise, copy the path, its lengths and both speakers' rows to the host, gather in numpy, upload.

    python tools/parallel_probe.py [--pairs 64] [--frames 2000] [--dx 120] [--dy 120] [--reps 7] [--out profiles/parallel_probe.txt]

Both sides are timed by a host clock around work that ends in a device synchronise, after a warm-up of every shape, alternating, and
the spread of the repetitions is printed with the median.  Needs a GPU: there is no fall-back."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def monotone_path(rng, a, b):
    """a path from (0, 0) to (a - 1, b - 1) of diagonal, up and left steps"""
    cells, i, j = [(0, 0)], 0, 0
    while (i, j) != (a - 1, b - 1):
        r = rng.random()
        if i < a - 1 and j < b - 1 and r < 0.6:
            i, j = i + 1, j + 1
        elif i < a - 1 and (j == b - 1 or r < 0.8):
            i += 1
        else:
            j += 1
        cells.append((i, j))
    return np.array(cells, dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--dx", type=int, default=120)
    ap.add_argument("--dy", type=int, default=120)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "parallel_probe.txt"))
    args = ap.parse_args()
    import world_class_amd as w
    from world_class_amd import parallel as par
    w.lib().wc_set_device(0)
    rng = np.random.default_rng(0)
    al_ = [int(args.frames * rng.uniform(0.9, 1.1)) for _ in range(args.pairs)]
    bl = [int(args.frames * rng.uniform(0.9, 1.1)) for _ in range(args.pairs)]
    fa, fb, n_slots = sum(al_), sum(bl), par.slots(al_, bl)
    dx, dy = args.dx, args.dy
    path, path_length, p = np.full((n_slots, 2), -1, dtype=np.int32), np.zeros(args.pairs, dtype=np.int32), 0
    for u, (a, b) in enumerate(zip(al_, bl)):
        cells = monotone_path(rng, a, b)
        path[p:p + len(cells)], path_length[u] = cells, len(cells)
        p += a + b - 1
    rows_a, rows_b = rng.normal(size=(fa, dx)), rng.normal(size=(fb, dy))
    rows_a[:, 0] = rng.normal(size=fa) * 3.0
    d_a, d_b = w.DeviceArray.from_host(rows_a), w.DeviceArray.from_host(rows_b)
    d_len, d_path = w.DeviceArray.from_host(path_length, np.int32), w.DeviceArray.from_host(path, np.int32)
    d_ma, d_mb = w.DeviceArray(fa, np.uint8), w.DeviceArray(fb, np.uint8)
    d_joint, d_jm = w.DeviceArray(n_slots * (dx + dy)), w.DeviceArray(n_slots, np.uint8)
    d_sum, d_cnt = w.DeviceArray(args.pairs), w.DeviceArray(args.pairs, np.int64)
    sync = w.lib().wc_synchronize

    def device_calls():
        par.speech_mask(al_, d_a, dx, d_ma, 0, 9.2)
        par.speech_mask(bl, d_b, dy, d_mb, 0, 9.2)
        par.joint_rows(al_, bl, d_a, dx, dx, d_b, dy, dy, d_len, d_path, d_joint, dx + dy, d_jm, d_mask_a=d_ma, d_mask_b=d_mb)
        par.path_distortion(al_, bl, d_a, dx, d_b, dy, min(dx, dy), d_len, d_path, d_sum, d_cnt, None, 0, 0, d_ma, d_mb)
        sync()

    kept = {}

    def host_gather():
        sync()
        K, cells = d_len.to_host(), d_path.to_host((n_slots, 2))
        xa, xb = d_a.to_host((fa, dx)), d_b.to_host((fb, dy))
        parts, p, oa, ob = [], 0, 0, 0
        for a, b, k in zip(al_, bl, K):
            c = cells[p:p + k]
            parts.append(np.concatenate([xa[oa + c[:, 0]], xb[ob + c[:, 1]]], axis=1))
            p, oa, ob = p + a + b - 1, oa + a, ob + b
        joint = np.concatenate(parts)
        d = w.DeviceArray.from_host(joint)
        sync()
        kept["rows"] = joint
        d.free()

    for _ in range(2):          # every shape once before the clock runs
        device_calls()
        host_gather()
    t_dev, t_host = [], []
    for _ in range(args.reps):          # alternating
        t0 = time.perf_counter()
        device_calls()
        t1 = time.perf_counter()
        host_gather()
        t2 = time.perf_counter()
        t_dev.append(t1 - t0)
        t_host.append(t2 - t1)
    on_path = d_jm.to_host() != 0          # (the masks of the timed calls drop rows; the host gather keeps every cell)
    got = d_joint.to_host((n_slots, dx + dy))
    every = np.concatenate([np.arange(p, p + k) for p, k in zip(np.cumsum([0] + [a + b - 1 for a, b in zip(al_, bl)][:-1]), path_length)])
    assert np.array_equal(got[every], kept["rows"]), "the two sides gather different rows"
    moved = (n_slots * (dx + dy) * 8 + int(path_length.sum()) * (dx + dy) * 8 + n_slots * 9) / 1e6
    lines = [
        "parallel_probe: %d pairs of about %d frames, dx = %d, dy = %d, float64; %d path slots, %d on the path, %d live under the speech masks"
        % (args.pairs, args.frames, dx, dy, n_slots, int(path_length.sum()), int(on_path.sum())),
        "host clock around work that ends in a device synchronise; %d alternating repetitions after 2 warm-up rounds; median [min .. max]" % args.reps,
        "device calls (2 speech masks + joint rows + path distortion over %d columns): %.3f ms [%.3f .. %.3f]"
        % (min(dx, dy), 1e3 * np.median(t_dev), 1e3 * min(t_dev), 1e3 * max(t_dev)),
        "host gather (synchronise, path and both row sets to the host, numpy gather, upload): %.3f ms [%.3f .. %.3f]"
        % (1e3 * np.median(t_host), 1e3 * min(t_host), 1e3 * max(t_host)),
        "the gather reads and writes about %.0f MB on the device; both sides produce the same rows on the path (checked)" % moved,
    ]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
