"""TEST INFRASTRUCTURE ONLY -- generates tests/golden/frame_periods.npz from the REAL reference (oracle/_ref/libworld_ref.so) at
frame periods that are no whole number of samples or not representable in seconds (tests/frame_periods.py):

  - Synthesis alone (reference src/synthesis.cpp:77-177) on every contour of every case, each in a process of its own (noise stream
    at its seed state): the waveform in full where it is short, otherwise windows of 192 samples -- around the pulses that sit on
    nominal frame-boundary samples for the boundary contours, evenly spaced for the others -- and the sums of 480-sample blocks;
  - Harvest's F0 on one 0.6 s utterance per frame period.

Run in the build container only:

    make -C oracle ref && python oracle/gen_golden_frame_periods.py

Only data travels: the parameters and signals are regenerated from their seeds by the tests and checked against the stored sums."""
import hashlib
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)
sys.path.insert(0, os.path.join(_ROOT, "tests"))
import frame_periods as fpm  # noqa: E402
from oracle import port, ref  # noqa: E402


def main():
    P = port.Port()
    out = {}
    for name in fpm.NAMES:
        fs, fft, fp, _, _ = fpm.CASES[name]
        for kind in fpm.contours(name):
            f0, sp, ap = fpm.contour(name, kind)
            n, cap = P.synthesis_pulses(f0, fft, fs, fp)
            assert n <= cap, (name, kind, n, cap)  # (the reference writes past its pulse arrays otherwise)
            y = ref.run_fresh("at", 0, "synthesis", f0, sp, ap, fs, fp)
            k = "%s/%s/" % (name, kind)
            out[k + "y_len"] = np.array([len(y)])
            out[k + "param_sums"] = np.array([f0.sum(), sp.sum(), ap.sum()])
            if len(y) <= fpm.FULL_LIMIT:
                out[k + "y"] = y
            else:
                below, at = fpm.boundary_pulses(P, f0, fs, fft, fp) if kind in ("boundary", "steep") else ([], [])
                centres = [c for pair in zip(below, at) for c in pair] + below[len(at):] + at[len(below):]
                starts = fpm.windows(len(y), centres)
                nb = len(y) // fpm.BLOCK
                out[k + "y_blocksum"] = y[:nb * fpm.BLOCK].reshape(nb, fpm.BLOCK).sum(1)
                out[k + "y_win_start"] = np.array(starts)
                out[k + "y_win"] = np.stack([y[s:s + fpm.WIN] for s in starts])
            print(k, "frames", len(f0), "pulses", n, "y", len(y), "max", float(np.abs(y).max()))
    for name, fs, fp in fpm.HARVEST_PERIODS:
        x = fpm.harvest_signal(fs)
        tpos, f0 = ref.run_fresh("harvest", x, fs, frame_period=fp)
        assert np.array_equal(tpos, np.arange(len(f0)) * fp / 1000.0)
        out["harvest/%s/f0" % name] = f0
        out["harvest/%s/x_sha256" % name] = np.frombuffer(hashlib.sha256(x.tobytes()).digest(), dtype=np.uint8)
        print("harvest", name, "frames", len(f0), "voiced", int((f0 > 0).sum()))
    path = fpm.fixture_path()
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
