"""Filter streams (include/world_class_filter_stream.h) push by push against the batch call on the same total samples: 512 streams at
24 kHz (fft_size 1024) and 64 streams at 48 kHz (fft_size 2048), every push one 5 ms frame -- one hop of samples and one row -- per
stream.  The pushes are enqueued back to back and timed on the host around one device synchronisation at the end (throughput: what a
server that keeps the queue filled pays per push), and once more with a synchronisation behind every push (latency: what a caller that
waits for each push's outputs pays).  The timed pushes call the library with count arrays made once ("library"); the Python mirror's
push, which converts the counts of every stream on every call, is timed beside them ("mirror").  Beside them the batch call wc_frame_filter_run_device on the same samples and rows as n_streams
utterances, on the same library: the floor a push-by-push form can be held against.  Prints one JSON line per workload.
    python tools/filter_stream_probe.py [pushes]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import world_class_amd as w
from world_class_amd import DeviceArray, _ints
from world_class_amd.filter import FrameFilter
from world_class_amd.filter_stream import FilterStream

L = w.lib()
L.wc_set_device(0)
pushes = int(sys.argv[1]) if len(sys.argv) > 1 else 400
FRAME_MS, WARM, REPEATS, CYCLE = 5.0, 40, 5, 8


def probe(fs, fft_size, n_streams):
    hop, width = int(FRAME_MS * fs / 1000), fft_size // 2 + 1
    rng = np.random.default_rng(fs)
    total = pushes + WARM
    # push k holds stream u's hop of samples at ((k % CYCLE) * n_streams + u) * hop, its row at (k % CYCLE) * n_streams + u
    x = DeviceArray.from_host(rng.normal(size=CYCLE * n_streams * hop))
    rows = DeviceArray.from_host(np.exp(rng.normal(size=(CYCLE * n_streams, width)) * 0.5))
    y = DeviceArray(n_streams * 4 * hop)
    st = FilterStream(fs, fft_size, FRAME_MS, "power", n_streams, 4 * hop, 2)
    ns, nr = [hop] * n_streams, [1] * n_streams

    c_ns, c_nr, c_out, push = _ints(ns), _ints(nr), _ints([0] * n_streams), L.wc_filter_stream_push_device

    def run(first, count, wait, mirror=False):
        t0 = time.perf_counter()
        for k in range(first, first + count):
            d_x, d_r = x.ptr + 8 * (k % CYCLE) * n_streams * hop, rows.ptr + 8 * (k % CYCLE) * n_streams * width
            if mirror:
                st.push(ns, d_x, nr, d_r, y)
            else:
                assert push(st._h, c_ns, d_x, c_nr, d_r, None, y.ptr, c_out) == 0
            if wait:
                L.wc_synchronize()
        L.wc_synchronize()
        return (time.perf_counter() - t0) / count

    run(0, WARM, False)
    third = pushes // 3
    queued, waited, mirror = run(WARM, third, False), run(WARM + third, third, True), run(WARM + 2 * third, pushes - 2 * third, False, True)
    for u in range(n_streams):
        assert st.samples_received(u) == total * hop and st.segments_done(u) == total
    st.close()
    # the batch on the same total: n_streams utterances of pushes * hop samples; CYCLE rows each, the last one held (every segment
    # forms its row's minimum phase anew, so the work is that of a row per segment)
    n = pushes * hop
    ff = FrameFilter(fs, fft_size, FRAME_MS)
    assert ff.segments(n) == pushes + 1
    bx, brows = DeviceArray.from_host(rng.normal(size=n_streams * n)), DeviceArray.from_host(np.exp(rng.normal(size=(n_streams * CYCLE, width)) * 0.5))
    by = DeviceArray(n_streams * n)
    times = []
    for _ in range(REPEATS + 2):
        t0 = time.perf_counter()
        ff.run(bx, [n] * n_streams, brows, [CYCLE] * n_streams, by)
        L.wc_synchronize()
        times.append(time.perf_counter() - t0)
    batch = float(np.median(times[2:]))
    ff.close()
    for d in (x, rows, y, bx, brows, by):
        d.free()
    return {"workload": "%d streams x %g kHz, fft_size %d, one %g ms frame per push, %d pushes" % (n_streams, fs / 1000, fft_size, FRAME_MS, pushes),
            "push_us_queued": queued * 1e6, "real_time_factor_queued": FRAME_MS * 1e-3 / queued,
            "push_us_waited": waited * 1e6, "real_time_factor_waited": FRAME_MS * 1e-3 / waited,
            "push_us_queued_mirror": mirror * 1e6,
            "batch_ms_same_samples": batch * 1e3, "batch_us_per_frame_of_all_streams": batch / pushes * 1e6,
            "push_over_batch": queued / (batch / pushes)}


for setting in ((24000, 1024, 512), (48000, 2048, 64)):
    print(json.dumps(probe(*setting)), flush=True)
