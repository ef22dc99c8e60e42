"""-m gpu: the gated frames of D4C whose windows exceed 2048 samples at N = 4096 (F0 at or below 93.79 Hz at 48 kHz, 86.17 Hz at
44.1 kHz, 62.53 Hz at 32 kHz: 2 round(4 fs / f0 / 2) + 1 > 2048).  d4c2_frames_kernel<true> forms each of a frame's three windows
once, parks the mean-removed samples of all 32 slots in a row owned by its block and forms every transform's input from them; its
twin (WC_D4C_LONG=halves, d4c2_frames_halves_kernel) forms the window again for every half and transform.  The same bits in ap, the
same noise positions, and the length of the list the long launch walked (wc_debug_d4c_long_count) as the contour says.

Everything is a D4C stage call on a given contour (D4C.compute_device) at threshold 0.0, so that every voiced frame reaches the
frames stage, but for one case at the default gate."""
import ctypes as C

import numpy as np
import pytest

from world_class_amd.synth import make_utterance

pytestmark = pytest.mark.gpu

SENTINEL = 1.0 - 1e-12
AP_ABS = 1e-7  # tests/test_gpu_d4c.py, the two-wavefront kernels against the block kernels


@pytest.fixture(scope="module")
def wca():
    import world_class_amd as w
    L = w.lib()
    L.wc_debug_d4c_long_count.restype = C.c_int
    L.wc_debug_d4c_long_count.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    return w


def _handle(wca, fs, threshold, env):
    """a handle created under the environment switches it reads at creation"""
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("WC_D4C_LONG", raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        return wca.D4C(fs, threshold)


def _stage(wca, d, fs, utts, start, hop):
    """one D4C.compute_device call on the batch [(x, f0), ...]: the aperiodicity matrices and the noise positions it ends at"""
    import torch
    fft = wca.cheaptrick_fft_size(fs)
    bins = fft // 2 + 1
    xs = [np.ascontiguousarray(x, dtype=np.float64) for x, _ in utts]
    f0s = [np.ascontiguousarray(f, dtype=np.float64) for _, f in utts]
    dev = lambda v: torch.from_numpy(np.concatenate(v)).to("cuda")
    d_x, d_f0, d_t = dev(xs), dev(f0s), dev([np.arange(len(f)) * hop for f in f0s])
    total = sum(len(f) for f in f0s)
    d_ap = torch.full((total * bins + 1,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    end = d.compute_device(d_x, [len(x) for x in xs], d_t, d_f0, [len(f) for f in f0s], fft, d_ap, rng_pos=list(start))
    wca.lib().wc_synchronize()
    ap = d_ap.cpu().numpy()
    assert np.isnan(ap[-1])  # (nothing written behind the last row)
    return ap[:-1].reshape(total, bins), list(end)


def _long_count(wca, d):
    n = C.c_int(-2)
    assert wca.lib().wc_debug_d4c_long_count(d._h, C.byref(n)) == 0
    return n.value


def _window(fs, f0):
    """the length of a gated frame's three windows (reference src/d4c.cpp: 2 matlab_round(4 fs / max(47, f0) / 2) + 1)"""
    return 2 * np.floor(4.0 * fs / np.maximum(f0, 47.0) / 2.0 + 0.5).astype(np.int64) + 1


def _is_long(fs, f0):
    return (f0 > 0.0) & (_window(fs, np.where(f0 > 0.0, f0, 1000.0)) > 2048)


def _cyc(n, vals):
    return np.array([vals[i % len(vals)] for i in range(n)], dtype=np.float64)


# the highest long F0 and the lowest short one, to 0.01 Hz (test_the_cut_between_short_and_long_windows checks them)
# (the cut itself is 2 fs / 1023.5: 93.796, 86.175 and 62.531 Hz)
CUT = {48000: (93.79, 93.80), 44100: (86.17, 86.18), 32000: (62.53, 62.54)}


def _ragged(fs):
    lo, hi = CUT[fs]
    return [_cyc(101, [47.0, lo, hi, 0.0, 150.0, 60.0 if fs > 32000 else 50.0]), _cyc(61, [hi, lo, 0.0, 47.0])]


def _cases():
    """name -> (fs, contours, threshold, start positions, hop in s, the long frames the contours hold)"""
    c = {}
    n = 81  # 0.4 s at a 5 ms hop
    c["cut_48k"] = (48000, [_cyc(n, [93.80, 93.79, 0.0, 200.0])], 0.0, [0], 0.005, 20)
    c["all_long"] = (48000, [_cyc(n, [47.0, 40.0, 60.0, 80.0, 93.79])], 0.0, [5], 0.005, 81)
    one = np.full(n, 150.0)
    one[40] = 80.0
    c["one_long"] = (48000, [one], 0.0, [0], 0.005, 1)
    c["none_long"] = (48000, [_cyc(n, [150.0, 93.80, 0.0])], 0.0, [0], 0.005, 0)
    edges = np.full(n, 150.0)
    edges[0] = edges[-1] = 47.0  # windows of 4087 samples: 2043 before the first sample, 2043 behind the last
    c["edges"] = (48000, [edges], 0.0, [0], 0.005, 2)
    for fs in (48000, 44100, 32000):
        f = _ragged(fs)
        c["ragged_%d" % fs] = (fs, f, 0.0, [0, 31337], 0.005, int(sum(_is_long(fs, v).sum() for v in f)))
    c["default_gate"] = (48000, _ragged(48000), 0.85, [0, 31337], 0.005, None)  # (what passes the gate: see the test)
    # more long frames than the long launch has blocks (4 096): blocks take a second frame and reuse their row
    c["more_than_blocks"] = (48000, [np.full(4200, 60.0)], 0.0, [0], 0.001, 4200)
    return c


def _utts(name):
    fs, f0s, _, _, hop, _ = _cases()[name]
    return [(make_utterance(fs, hop * (len(f) - 1), 6100 + 7 * u + fs % 13), f) for u, f in enumerate(f0s)]


@pytest.fixture(scope="module")
def runs(wca):
    """every case once through the default form and once through its twin; shared by the tests below and left unchanged"""
    out = {}

    def get(name):
        if name not in out:
            fs, f0s, thr, start, hop, _ = _cases()[name]
            utts = _utts(name)
            dn = _handle(wca, fs, thr, {})
            new = _stage(wca, dn, fs, utts, start, hop)
            n_new = _long_count(wca, dn)
            dh = _handle(wca, fs, thr, {"WC_D4C_LONG": "halves"})
            old = _stage(wca, dh, fs, utts, start, hop)
            out[name] = dict(new=new, old=old, n_new=n_new, n_old=_long_count(wca, dh), handle=dn, utts=utts)
        return out[name]
    return get


def test_the_cut_between_short_and_long_windows():
    assert _window(48000, np.array([93.80, 93.79, 47.0, 40.0])).tolist() == [2047, 2049, 4087, 4087]
    for fs, (lo, hi) in CUT.items():
        w = _window(fs, np.array([lo, hi]))
        assert w[0] == 2049 and w[1] == 2047


@pytest.mark.parametrize("name", list(_cases()))
def test_windows_formed_once_give_the_bits_of_the_per_half_twin(wca, runs, name):
    fs, f0s, thr, start, hop, want = _cases()[name]
    r = runs(name)
    (a, pa), (b, pb) = r["new"], r["old"]
    f0 = np.concatenate(f0s)
    gated = (b != SENTINEL).any(axis=1)  # frames that went through the frames stage
    long_gated = int((_is_long(fs, f0) & gated).sum())
    if want is None:  # the default gate decides which of the contour's long frames are listed
        want = long_gated
        assert 0 < want < int(_is_long(fs, f0).sum())
    print(name, "frames", len(f0), "voiced", int((f0 > 0).sum()), "gated", int(gated.sum()), "long in the contour", int(_is_long(fs, f0).sum()),
          "long and gated", long_gated, "listed", r["n_new"], "(twin", r["n_old"], ") expected", want)
    assert r["n_new"] == want and r["n_old"] == want
    if thr == 0.0:
        assert want == int(_is_long(fs, f0).sum()) == long_gated
    assert pa == pb
    assert np.isfinite(b).all()
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert (b[f0 == 0.0] == SENTINEL).all()


def test_a_second_call_on_the_handle_reuses_its_rows(wca, runs):
    """the parked rows of the first call are stale input to nothing: the same bits again, and the list starts empty again"""
    name = "ragged_48000"
    fs, _, _, start, hop, want = _cases()[name]
    r = runs(name)
    a2, p2 = _stage(wca, r["handle"], fs, r["utts"], start, hop)
    assert _long_count(wca, r["handle"]) == want
    assert p2 == r["new"][1] and np.array_equal(a2.view(np.uint64), r["new"][0].view(np.uint64))


def test_long_windows_against_the_block_kernels(wca, runs):
    name = "all_long"
    fs, _, thr, start, hop, _ = _cases()[name]
    r = runs(name)
    db = _handle(wca, fs, thr, {"WC_D4C_IMPL": "block"})
    b, pb = _stage(wca, db, fs, r["utts"], start, hop)
    a, pa = r["new"]
    print("against the block kernels: max |difference|", np.abs(a - b).max())
    assert _long_count(wca, db) == -1  # (the block kernels list nothing)
    assert pa == pb
    assert np.abs(a - b).max() < AP_ABS
