"""TEST INFRASTRUCTURE ONLY -- generates tests/golden/minphase_sizes.npz from the REAL reference
(oracle/_ref/libworld_ref.so): MinimumPhaseAnalysis at 512, 1024, 2048 and 4096 points on three log spectra per size (a log
envelope with formants, a -6 tilt and noise; a notch of depth 35 five bins wide; 0.5 N(0, 1) -- tests/minimum_phase_rule.py).
Run in the build container only:

    make -C oracle ref && python oracle/gen_golden_minphase.py

Only data (inputs + expected outputs) is written; no reference source travels.
"""
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)
sys.path.insert(0, os.path.join(_ROOT, "tests"))
from oracle import ref  # noqa: E402
import minimum_phase_rule as rule  # noqa: E402


def main():
    R = ref.Ref()
    out = {}
    for n in rule.SIZES:
        for kind in rule.KINDS:
            ls = rule.fixture_input(kind, n)
            M = R.minimum_phase(ls, n)
            out[f"{kind}/in_{n}"] = ls
            out[f"{kind}/out_{n}"] = np.stack([M.real, M.imag], 1)
            mine = rule.minimum_phase(ls, n)
            print(n, kind, "max |rule - ref| / |ref| = %.3g" % (np.abs(mine - M) / np.abs(M)).max())
    np.savez_compressed(rule.FIXTURE, **out)
    print(rule.FIXTURE, os.path.getsize(rule.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
