"""TEST INFRASTRUCTURE ONLY (build container).  Runs the reference's codec (src/codec.cpp compiled from where it lies into
oracle/_ref/libworld_ref_tools.so) at every fft size and at every band count, and writes tests/golden/io/codec_sizes.npz:

    make -C oracle ref && python oracle/gen_golden_codec_sizes.py

Only outputs are stored.  The input rows are regenerated from their seeds by inputs() below (oracle/gen_golden.synth_params, a flat
spectral envelope, aperiodicity rows at exactly 1 and 1 - 1e-12, seeded decode-only coefficient rows and hand-made coded
aperiodicity rows); a SHA-256 of them is stored and checked by the tests.  Per case (key prefix "fs<fs>_fft<fft>/"):

  sp_coded           the reference's coded rows at nd = fft/4+1.  A coded row at a smaller nd is the prefix of this one (the
                     reference computes the whole transform and keeps the first nd coefficients); the generator asserts that
                     for every nd of code_nds(), bit for bit, so the tests compare each nd with the prefix
  sp_decoded_<nd>    the reference's decoded rows of sp_coded[:, :nd] for nd in decode_nds(); of the seeded decode-only
                     coefficient rows for nd in decode_only_nds() (fft/4+2 .. fft/2: decoding accepts more than coding makes)
  ap_coded           the reference's coded aperiodicity of the aperiodicity rows
  ap_decoded         the reference's decoded rows of [ap_coded; hand_coded_ap()]; below 12 kHz (no band) of two empty rows
  n_ap               GetNumberOfAperiodicities(fs)
  inputs_sha256      digest of inputs()

Every row is stored whole (bin-level errors stay visible).  The file stays under 1 MiB: three frames per decoded spectral envelope.
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
_dp = C.POINTER(C.c_double)

# (fs, fft_size, seed).  Band counts 0, 0, 1, 1, 2, 4, 5, 5; fft 512 and 4096 take the codec's workgroup kernels
# (code_sp_kernel / decode_sp_kernel <256> and <2048>), fft 2048 the one-wavefront decoder of Synthesis from coded features
CASES = [
    (8000, 512, 801),      # no band: the spectral-envelope codec only, and the decoded aperiodicity ramp
    (11025, 512, 1101),    # no band: the ramp alone
    (12000, 512, 1201),    # 1 band: the lowest rate that coded Synthesis accepts
    (16000, 2048, 1601),   # 1 band; fs/2 below the codec's 20 kHz ceiling
    (22050, 1024, 2201),   # 2 bands; non-integer bin spacing
    (32000, 2048, 3201),   # 4 bands; ceiling = fs/2
    (44100, 2048, 4401),   # 5 bands; ceiling 20 kHz < fs/2
    (96000, 4096, 9601),   # 5 bands; the largest size
]
RAMP_ONLY = (11025,)


def name(fs, fft):
    return f"fs{fs}_fft{fft}"


def code_nds(fft):
    return sorted({1, 2, 64, 65, 255, 256, 257, fft // 4 + 1} & set(range(1, fft // 4 + 2)))


def decode_nds(fft):
    """coded rows of the reference decoded at these nd: 256 / 257 are either side of the one-wavefront decoder's pruned stage"""
    return sorted({1, 256, 257, fft // 4 + 1} & set(range(1, fft // 4 + 2)))


def decode_only_nds(fft):
    return [fft // 4 + 2, fft // 2]


def hand_coded_ap(n_ap):
    """coded aperiodicity rows made by hand (n_ap >= 1): the edges of the voiced/unvoiced test on the band mean and of the
    interpolation"""
    rows = [np.full(n_ap, -0.5)]        # mean exactly -0.5: not above it, so voiced
    up = np.full(n_ap, -0.5)            # the last band raised by the fewest ulps that lift the sequential mean above -0.5: unvoiced
    while True:
        up[-1] = np.nextafter(up[-1], 0.0)
        t = 0.0
        for v in up:
            t += v
        if t / n_ap > -0.5:
            break
    rows.append(up)
    rows.append(np.full(n_ap, -60.0))   # every band at -60 dB
    hot = np.full(n_ap, -40.0)          # a band above 0 dB: the decoded aperiodicity exceeds 1 (the reference does not clamp)
    hot[0] = 6.0
    rows.append(hot)
    nan = np.full(n_ap, -20.0)          # one NaN band: the mean is NaN, so voiced; NaN only in the bins next to that band
    nan[n_ap // 2] = np.nan
    rows.append(nan)
    return np.array(rows)


def inputs(fs, fft, seed):
    """(sp rows, ap rows, {nd: decode-only coefficient rows}, coded ap rows made by hand), regenerated from the seed"""
    from oracle.gen_golden import synth_params
    _, sp, ap = synth_params(fs, fft, 8, seed)  # (8 frames: synth_params sets frame 5)
    bins = fft // 2 + 1
    sp = np.concatenate([sp[:2], np.full((1, bins), 3e-3)])                           # two seeded rows and a flat one
    ap = np.concatenate([ap[:3], np.ones((1, bins)), np.full((1, bins), 1.0 - 1e-12)])  # three seeded rows, exactly 1, 1 - 1e-12
    rng = np.random.default_rng(seed + 7)
    only = {}
    for nd in decode_only_nds(fft):  # N(0, 1) e^{-i/30} around a c0 of a typical log spectrum (the mean log of sp is about -8)
        c = rng.normal(size=(3, nd)) * np.exp(-np.arange(nd) / 30.0)
        c[:, 0] -= 8.0
        only[nd] = c
    from oracle.port_codec import number_of_aperiodicities
    n_ap = number_of_aperiodicities(fs)
    return sp, ap, only, hand_coded_ap(n_ap) if n_ap > 0 else np.zeros((2, 0))


def inputs_digest(fs, fft, seed):
    sp, ap, only, hand = inputs(fs, fft, seed)
    h = hashlib.sha256()
    for a in [sp, ap, hand] + [only[nd] for nd in sorted(only)]:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def case_data(g, fs, fft, seed):
    """for the tests, from the written file g: the regenerated inputs of a case (checked against the stored digest), the coded
    aperiodicity rows to decode (the reference's coded rows, then the hand-made ones) and the case's key prefix"""
    k = name(fs, fft) + "/"
    assert np.array_equal(inputs_digest(fs, fft, seed), g[k + "inputs_sha256"]), "input generator drifted"
    sp, ap, only, hand = inputs(fs, fft, seed)
    cap = np.concatenate([g[k + "ap_coded"], hand]) if int(g[k + "n_ap"]) else hand
    return sp, ap, only, cap, k


def sp_decode_cases(g, k, fft, only):
    """[(nd, coded rows, the reference's decoded rows)]: its own coded rows cut to nd, then the decode-only rows (nd > fft/4+1)"""
    out = [(nd, np.ascontiguousarray(g[k + "sp_coded"][:, :nd]), g[k + f"sp_decoded_{nd}"]) for nd in decode_nds(fft)]
    return out + [(nd, only[nd], g[k + f"sp_decoded_{nd}"]) for nd in decode_only_nds(fft)]


def close_ap(a, ref, tol=1e-13):
    """NaN where the reference has NaN (a NaN band reaches only its neighbouring bins), within tol elsewhere"""
    return np.array_equal(np.isnan(a), np.isnan(ref)) and np.nanmax(np.abs(a - ref)) < tol


def rows(mat):
    arr = (_dp * mat.shape[0])()
    for i in range(mat.shape[0]):
        arr[i] = mat[i].ctypes.data_as(_dp)
    return arr


def main():
    L = C.CDLL(os.path.join(HERE, "_ref", "libworld_ref_tools.so"))
    R = C.POINTER(_dp)
    L.CodeSpectralEnvelope.argtypes = [R, C.c_int, C.c_int, C.c_int, C.c_int, R]
    L.DecodeSpectralEnvelope.argtypes = [R, C.c_int, C.c_int, C.c_int, C.c_int, R]
    L.CodeAperiodicity.argtypes = [R, C.c_int, C.c_int, C.c_int, R]
    L.DecodeAperiodicity.argtypes = [R, C.c_int, C.c_int, C.c_int, R]

    def decode_sp(coded, fs, fft):
        coded = np.ascontiguousarray(coded)
        dec = np.full((coded.shape[0], fft // 2 + 1), np.nan)
        L.DecodeSpectralEnvelope(rows(coded), coded.shape[0], fs, fft, coded.shape[1], rows(dec))
        return dec

    g = {}
    for fs, fft, seed in CASES:
        k = name(fs, fft) + "/"
        sp, ap, only, hand = inputs(fs, fft, seed)
        n_ap = L.GetNumberOfAperiodicities(fs)
        bins = fft // 2 + 1
        g[k + "fs"], g[k + "fft"], g[k + "seed"], g[k + "n_ap"] = fs, fft, seed, n_ap
        g[k + "inputs_sha256"] = inputs_digest(fs, fft, seed)
        if n_ap > 0:
            cap = np.full((ap.shape[0], n_ap), np.nan)
            L.CodeAperiodicity(rows(ap), ap.shape[0], fs, fft, rows(cap))
            g[k + "ap_coded"] = cap
            cap = np.concatenate([cap, hand])
        else:
            cap = hand  # two rows of no band
        dap = np.full((cap.shape[0], bins), np.nan)
        L.DecodeAperiodicity(rows(cap), cap.shape[0], fs, fft, rows(dap))
        g[k + "ap_decoded"] = dap
        if n_ap > 0:  # the exact-mean row is voiced, the row an ulp above it is not
            assert not np.all(dap[-5] == 1.0 - 1e-12) and np.all(dap[-4] == 1.0 - 1e-12)
        if fs in RAMP_ONLY:
            continue
        full = fft // 4 + 1
        coded = np.full((sp.shape[0], full), np.nan)
        L.CodeSpectralEnvelope(rows(sp), sp.shape[0], fs, fft, full, rows(coded))
        for nd in code_nds(fft):
            c = np.full((sp.shape[0], nd), np.nan)
            L.CodeSpectralEnvelope(rows(sp), sp.shape[0], fs, fft, nd, rows(c))
            assert np.array_equal(c, coded[:, :nd]), (fs, fft, nd)
        g[k + "sp_coded"] = coded
        for nd in decode_nds(fft):
            g[k + f"sp_decoded_{nd}"] = decode_sp(coded[:, :nd], fs, fft)
        for nd in decode_only_nds(fft):
            g[k + f"sp_decoded_{nd}"] = decode_sp(only[nd], fs, fft)
    out = os.path.join(ROOT, "tests", "golden", "io", "codec_sizes.npz")
    np.savez_compressed(out, **g)
    print("wrote", out, f"{os.path.getsize(out) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
