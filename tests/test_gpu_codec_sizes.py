"""-m gpu: the feature codec at every fft size (512 .. 4096: code_sp_kernel / decode_sp_kernel <256> .. <2048>) and every band count
(0 .. 5) against the real reference's rows in tests/golden/io/codec_sizes.npz (oracle/gen_golden_codec_sizes.py), through the
device-resident calls and the reference-named host functions, at the tolerances of test_gpu_codec.py::test_codec_golden."""
import os

import numpy as np
import pytest

from oracle.gen_golden_codec_sizes import CASES, RAMP_ONLY, case_data, close_ap, code_nds, name, sp_decode_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def env():
    import torch
    import world_class_amd as w
    from world_class_amd import codec
    w.lib().wc_set_device(0)
    return w, codec, torch, np.load(os.path.join(ROOT, "tests", "golden", "io", "codec_sizes.npz"))


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).ravel()).cuda()


@pytest.mark.parametrize("fs,fft,seed", CASES)
def test_codec_sizes_device(env, fs, fft, seed):
    """wc_{code,decode}_{spectral_envelope,aperiodicity}_device on device-resident rows"""
    w, codec, torch, g = env
    sp, ap, only, cap, k = case_data(g, fs, fft, seed)
    n_ap, bins = int(g[k + "n_ap"]), fft // 2 + 1

    def run(fn, *args, n, width):
        out = torch.full((n * width,), np.nan, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()  # (torch's fill runs on its own stream, the library's kernels on another)
        fn(*args, out)
        w.lib().wc_synchronize()
        return out.cpu().numpy().reshape(n, width)

    if n_ap:
        assert np.abs(run(codec.code_aperiodicity_device, fs, fft, len(ap), _dev(torch, ap), n=len(ap), width=n_ap)
                      - g[k + "ap_coded"]).max() < 1e-11
    d_cap = _dev(torch, cap) if n_ap else torch.zeros(1, dtype=torch.float64, device="cuda")  # (no band: not read)
    assert close_ap(run(codec.decode_aperiodicity_device, fs, fft, len(cap), d_cap, n=len(cap), width=bins), g[k + "ap_decoded"])
    if fs in RAMP_ONLY:
        return
    d_sp = _dev(torch, sp)
    for nd in code_nds(fft):
        c = run(codec.code_spectral_envelope_device, fs, fft, len(sp), nd, d_sp, n=len(sp), width=nd)
        assert np.abs(c - g[k + "sp_coded"][:, :nd]).max() < 1e-11, nd  # values are O(10): log of two math libraries + FFT order
    for nd, coded, ref in sp_decode_cases(g, k, fft, only):
        d = run(codec.decode_spectral_envelope_device, fs, fft, len(coded), nd, _dev(torch, coded), n=len(coded), width=bins)
        assert np.abs(d / ref - 1).max() < 1e-11, nd


@pytest.mark.parametrize("fs,fft,seed", CASES)
def test_codec_sizes_host(env, fs, fft, seed):
    """the reference-named host functions (include/codec.hpp signatures, row-pointer tables)"""
    w, codec, torch, g = env
    sp, ap, only, cap, k = case_data(g, fs, fft, seed)
    if int(g[k + "n_ap"]):
        assert np.abs(codec.code_aperiodicity(ap, fs, fft) - g[k + "ap_coded"]).max() < 1e-11
    assert close_ap(codec.decode_aperiodicity(cap, fs, fft), g[k + "ap_decoded"])
    if fs in RAMP_ONLY:
        return
    for nd in code_nds(fft):
        assert np.abs(codec.code_spectral_envelope(sp, fs, fft, nd) - g[k + "sp_coded"][:, :nd]).max() < 1e-11, nd
    for nd, coded, ref in sp_decode_cases(g, k, fft, only):
        assert np.abs(codec.decode_spectral_envelope(coded, fs, fft) / ref - 1).max() < 1e-11, nd


@pytest.mark.parametrize("fs", [8000, 11025])
def test_no_band_rates(env, fs):
    """below 12 kHz there is no band: DecodeAperiodicity fills every row with the reference's line from -60 dB at 0 Hz to -1e-12 dB
    at fs/2 (its mean of zero bands is NaN, so every frame is voiced) and reads no coded row; CodeAperiodicity writes nothing"""
    w, codec, torch, g = env
    fft, bins = 512, 257
    assert codec.number_of_aperiodicities(fs) == 0
    ramp = 10.0 ** ((-60.0 + np.arange(bins) / (bins - 1.0) * (60.0 - 1e-12)) / 20.0)
    for row in g[name(fs, fft) + "/ap_decoded"]:
        assert row[0] == 0.001 and np.abs(row - ramp).max() < 1e-15 and abs(row[-1] - 1.0) < 1e-12
    dec = codec.decode_aperiodicity(np.zeros((5, 0)), fs, fft)
    assert np.abs(dec - ramp).max() < 1e-13
    ap = np.full((5, bins), 0.5)
    cap = np.full((5, 3), 7.0)  # rows of three doubles that nothing may touch
    codec._L().CodeAperiodicity(codec._rows(ap), 5, fs, fft, codec._rows(cap))
    assert (cap == 7.0).all()
    with pytest.raises(w.WorldClassError):  # the device coder keeps refusing: it has no row to write
        d = torch.zeros(4 * bins, dtype=torch.float64, device="cuda")
        codec.code_aperiodicity_device(fs, fft, 4, d, d)
