"""Without a GPU: the resource figures of the D4C frames kernels at N = 4096 in the built library's gfx950 code object
(tools/kernel_resources.py).  Two wavefronts per SIMD need at most 256 VGPRs and 20 480 B of LDS (160 KB / 8); the launch over the
long-window frames kept 376 B of scratch while it formed a window per half and transform with both transforms' registers and the
running products live together (its twin, d4c2_frames_halves_kernel, still does), and must keep no more now that it forms each
window once."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _figures():
    from world_class_amd import build
    env = dict(os.environ, WC_LIB_PATH=build.build())
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "d4c2_frames"], env=env, check=True,
                         stdout=subprocess.PIPE, text=True).stdout
    rows = {}
    for line in out.splitlines()[1:]:
        name, vgpr, sgpr, scratch, lds = line.split()
        rows[name] = dict(vgpr=int(vgpr), sgpr=int(sgpr), scratch=int(scratch), lds=int(lds))
    return rows


def test_long_window_frames_kernel_keeps_two_wavefronts_per_simd_and_no_more_scratch():
    rows = _figures()
    print(rows)
    long_ = rows["d4c2_frames_kernel<true>"]
    assert long_["scratch"] <= 376
    assert long_["vgpr"] <= 256
    assert long_["lds"] <= 20480
    for name in ("d4c2_frames_kernel<false>", "d4c2_frames_halves_kernel"):  # the short frames' launch and the twin: two per SIMD too
        assert rows[name]["vgpr"] <= 256 and rows[name]["lds"] <= 20480
