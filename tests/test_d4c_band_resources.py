"""Without a GPU: the resource figures of the D4C band kernels in the built library's gfx950 code object (tools/kernel_resources.py).
The three-wavefront form holds three wavefronts per SIMD only without scratch memory, within 168 VGPRs (512 / 3, in blocks of 8) and
within the LDS that twelve wavefronts per CU leave each (160 KB / 12 = 13 653 B)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _figures():
    from world_class_amd import build
    env = dict(os.environ, WC_LIB_PATH=build.build())
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "d4c2_band_kernel"], env=env, check=True,
                         stdout=subprocess.PIPE, text=True).stdout
    rows = {}
    for line in out.splitlines()[1:]:
        name, vgpr, sgpr, scratch, lds = line.split()
        rows[name] = dict(vgpr=int(vgpr), sgpr=int(sgpr), scratch=int(scratch), lds=int(lds))
    return rows


def test_three_wavefront_band_kernel_fits_three_wavefronts_per_simd():
    rows = _figures()
    print(rows)
    three, two = rows["d4c2_band_kernel<3>"], rows["d4c2_band_kernel<2>"]
    assert three["scratch"] == 0
    assert three["vgpr"] <= 168
    assert three["lds"] <= 13312
    assert two["scratch"] == 0 and two["lds"] == 9216  # the twin: as it was
