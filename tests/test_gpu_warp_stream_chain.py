"""GPU test of the live chain (include/world_class_warp_stream.h): alignment streams with lag 3 follow 40-row live voices through a
60-frame coded track, every push's d_settled goes straight into a warp stream that holds the track's 60 x 240 samples, and the tail
into its flush; nothing is read on the host in between.  Afterwards the settled values and the tail are read back once, and the
stream's audio must be wc_warp_along_map_device's on that map, bit for bit."""
import numpy as np
import pytest

import vresample_rule as R
import warp_stream_rule as S
from test_gpu_vresample import GUARD, PATTERN
from world_class_amd import DeviceArray, lib, stream, vresample as vr, warp_stream as ws

pytestmark = pytest.mark.gpu

DIMS, LAG, FRAMES, ROWS, HOP = 8, 3, 60, 40, 240


def test_settled_positions_and_the_tail_drive_the_warp_stream():
    rng = np.random.default_rng(31300)
    coded = rng.standard_normal((FRAMES, DIMS))
    voices = [coded[np.minimum(np.arange(ROWS) * 3 // 2, FRAMES - 1)] + 0.05 * rng.standard_normal((ROWS, DIMS)), rng.standard_normal((ROWS, DIMS))]
    audio = rng.uniform(-1, 1, FRAMES * HOP)
    cuts = [[1, 2], [2, 1], [5, 0], [7, 12], [25, 25]]
    assert [sum(c[u] for c in cuts) for u in range(2)] == [ROWS, ROWS]
    a = stream.AlignStream(DIMS, 2, 1, FRAMES, 32)
    w = ws.WarpStream(R.ONE, R.ONE, 2, 1, FRAMES * HOP, 32, LAG, float(HOP))
    r = vr.VResampler(R.ONE, R.ONE)
    held = []
    keep = lambda d: held.append(d) or d
    try:
        a.reserve_lag(LAG)
        a.set_track(0, coded)
        w.set_track(0, audio)
        for u in range(2):
            a.reset(u, 0)
            a.set_lag(u, LAG)
            w.reset(u, 0, LAG, float(HOP), float(HOP))
        cap = 2 * w.max_out_per_push
        fill = np.full(cap + GUARD, PATTERN, dtype=np.uint64).view(np.float64)
        taken, settled, outs = [0, 0], [], []
        for counts in cuts:
            rows = np.concatenate([voices[u][taken[u]:taken[u] + c] for u, c in enumerate(counts)])
            d_rows, d_pos, d_cost = keep(DeviceArray.from_host(rows)), keep(DeviceArray(sum(counts))), keep(DeviceArray(sum(counts)))
            d_settled, d_y = keep(DeviceArray(sum(counts))), keep(DeviceArray.from_host(fill))
            a.push_settled_device(counts, d_rows, d_pos, d_cost, d_settled)
            n = w.push_device(counts, d_settled, d_y)   # (the counts come from the counts)
            settled.append((counts, d_settled))
            outs.append((n, d_y))
            taken = [t + c for t, c in zip(taken, counts)]
        d_tail, d_last = keep(DeviceArray(2 * (LAG + 1))), keep(DeviceArray.from_host(fill))
        a.tail_device([1, 1], d_tail)
        outs.append((w.flush_device([1, 1], d_tail, d_last), d_last))
        assert lib().wc_synchronize() == 0
        # ---- one read of everything ----
        rows_of = [[], []]
        for counts, d in settled:
            for u, part in enumerate(np.split(d.to_host(), np.cumsum(counts)[:-1])):
                rows_of[u].append(part)
        tail = np.split(d_tail.to_host(), [LAG + 1])
        got = [[], []]
        for n, d in outs:
            y = d.to_host()
            assert np.array_equal(y[sum(n):].view(np.uint8), fill[sum(n):].view(np.uint8))
            for u, part in enumerate(np.split(y[:sum(n)], np.cumsum(n)[:-1])):
                got[u].append(part)
        for u in range(2):
            entries = np.concatenate([np.concatenate(rows_of[u])[LAG:], tail[u][1:]])   # row i >= lag is entry i - lag; the tail's last `lag`
            assert len(entries) == ROWS and np.isfinite(entries).all() and tail[u][0] == entries[ROWS - LAG - 1]
            n_out = S.committed(ROWS, float(HOP))
            d_map, d_x, d_ref = keep(DeviceArray.from_host(entries)), keep(DeviceArray.from_host(audio)), keep(DeviceArray(n_out))
            ws.warp_along_map_device(r, d_x, [len(audio)], d_map, [ROWS], float(HOP), float(HOP), [n_out], d_ref)
            y = np.concatenate(got[u])
            assert len(y) == n_out == (ROWS - 1) * HOP + 1 and np.array_equal(y.view(np.uint8), d_ref.to_host().view(np.uint8)), u
            assert (w.rows_received(u), w.entries_consumed(u), w.samples_committed(u)) == (ROWS, ROWS, n_out) and y.any()
    finally:
        for d in held:
            d.free()
        for h in (a, w, r):
            h.close()
