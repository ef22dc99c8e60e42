"""-m gpu: F0 and formant modification per frame (the demo's ParameterModification, reference test/test.cpp:201-243, with one
scale and one ratio per frame): wc_modify_parameters_frames_device against the real reference's modification and bit for bit
against the scalar call, the decoder with the stretch inside (wc_decode_features_modified_device) against the two calls it
stands for and against the reference, the coded Synthesis batch call, the per-stream settings of the synthesis streams, and the
refused calls.  Outputs are NaN-filled with a guard row behind them that must stay NaN."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IO = os.path.join(ROOT, "tests", "golden", "io")
Y_ABS = 1e-8        # the project's Synthesis tolerance (test_gpu_synth_coded.py)
ATOMIC_ABS = 1e-12  # the FP64-atomic overlap-add at fft 512 / 4096 (test_gpu_synth_coded.py)
FUSED_REL = 1e-12   # the fused decoder against the composition: log / exp of two math libraries (derivation: test 4's docstring)
REF_REL = 1.2e-11   # the fused decoder against the reference: 1e-11 (decoder) + 1e-12 (modification) + 1e-13 (port_io)
SIZES = [(16000, 512), (24000, 1024), (48000, 2048), (96000, 4096)]


def ratios_of(fft):
    return [0.0, 0.37, 0.8, 0.999, 1.0, 1.2, 2.5, 2.0 / fft]


def cycled(fft, n, first=0):
    r = ratios_of(fft)
    return np.array([r[(first + i) % len(r)] for i in range(n)])


@pytest.fixture(scope="module")
def env():
    import torch
    import world_class_amd as w
    from world_class_amd import codec, io as wio
    w.lib().wc_set_device(0)
    return w, codec, wio, torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).ravel()).cuda()


def _guarded(torch, rows, n, bins):
    """rows (or NaN where rows is None) with a guard row of NaN behind them"""
    a = np.full((n + 1, bins), np.nan)
    if rows is not None:
        a[:n] = rows
    return _dev(torch, a)


def _rows(t, n, bins):
    a = t.cpu().numpy().reshape(n + 1, bins)
    assert np.isnan(a[n]).all(), "the guard row was written"
    return a[:n]


def _modify_frames(env, fs, fft, sp, ratio, f0=None, scale=None):
    w, codec, wio, torch = env
    n, bins = sp.shape[0], fft // 2 + 1
    d_sp = _guarded(torch, sp, n, bins)
    d_f0 = None if f0 is None else _guarded(torch, np.asarray(f0)[:, None], n, 1)
    wio.modify_parameters_frames_device(fs, fft, n, d_f0, d_sp, None if scale is None else _dev(torch, scale),
                                        None if ratio is None else _dev(torch, ratio))
    w.lib().wc_synchronize()
    return _rows(d_sp, n, bins), None if f0 is None else _rows(d_f0, n, 1)[:, 0]


def _modify_scalar(env, fs, fft, sp, ratio):
    w, codec, wio, torch = env
    n = sp.shape[0]
    d_sp = _dev(torch, sp)
    wio.modify_parameters_device(fs, fft, n, 0, d_sp, 1.0, ratio)
    w.lib().wc_synchronize()
    return d_sp.cpu().numpy().reshape(n, -1)


def _by_scalar_calls(env, fs, fft, sp, ratio):
    """the rows of one scalar call per distinct ratio"""
    out = np.empty_like(sp)
    for r in np.unique(ratio):
        out[ratio == r] = _modify_scalar(env, fs, fft, sp, float(r))[ratio == r]
    return out


# ---- 1. the reference's own modification ------------------------------------------------------------------------------------

def test_frames_against_the_reference_modification(env):
    """tests/golden/io/io_golden.npz: the real reference's ParameterModification of six rows (16 kHz, fft 1024) for four argument
    sets; one call on the six rows tiled four times with the per-frame arrays built from the argument sets (no ratio = 0): F0
    exactly, sp within the 1e-12 that test_gpu_io.py::test_parameter_modification_golden holds the scalar kernel to"""
    g = np.load(os.path.join(IO, "io_golden.npz"))
    fs, fft = int(g["mod_fs"]), int(g["mod_fft"])
    tags = ("scale_only", "up", "down", "down_small")
    scale, ratio = [], []
    for tag in tags:
        n_args, shift, r = g[f"mod_{tag}_args"]
        scale += [shift] * 6
        ratio += [r if n_args >= 2 else 0.0] * 6
    sp, f0 = _modify_frames(env, fs, fft, np.tile(g["mod_sp"], (4, 1)), np.array(ratio), np.tile(g["mod_f0"], 4), np.array(scale))
    for t, tag in enumerate(tags):
        assert np.array_equal(f0[6 * t:6 * t + 6], g[f"mod_{tag}_f0"]), tag
        rel = np.abs(sp[6 * t:6 * t + 6] / g[f"mod_{tag}_sp"] - 1).max()
        print("modify_frames against the reference, %s: %.3e" % (tag, rel))
        assert rel < 1e-12, tag


# ---- 2. row by row against the scalar call ----------------------------------------------------------------------------------

@pytest.mark.parametrize("fs,fft", SIZES)
def test_frames_equal_the_scalar_call_bit_for_bit(env, fs, fft):
    w, codec, wio, torch = env
    from oracle.gen_golden import synth_params
    n, bins = 131, fft // 2 + 1
    f0, sp, _ = synth_params(fs, fft, n, 2100 + fft)
    ratio = cycled(fft, n)
    scale = 0.5 + np.arange(n) / 64.0
    want = _by_scalar_calls(env, fs, fft, sp, ratio)
    got, got_f0 = _modify_frames(env, fs, fft, sp, ratio, f0, scale)
    assert np.array_equal(got, want)
    assert np.array_equal(got_f0, f0 * scale)
    assert np.array_equal(got[ratio == 0.0], sp[ratio == 0.0])
    rev, _ = _modify_frames(env, fs, fft, sp[::-1], ratio[::-1])
    assert np.array_equal(rev, want[::-1])
    # n_frames = 0 and both arrays NULL change nothing; d_sp NULL with a scale array is accepted
    d_sp, d_f0 = _guarded(torch, sp, n, bins), _dev(torch, f0)
    wio.modify_parameters_frames_device(fs, fft, 0, d_f0, d_sp, _dev(torch, scale), _dev(torch, ratio))
    wio.modify_parameters_frames_device(fs, fft, n, d_f0, d_sp, None, None)
    w.lib().wc_synchronize()
    assert np.array_equal(_rows(d_sp, n, bins), sp) and np.array_equal(d_f0.cpu().numpy(), f0)
    wio.modify_parameters_frames_device(fs, fft, n, d_f0, None, _dev(torch, scale), _dev(torch, ratio))
    w.lib().wc_synchronize()
    assert np.array_equal(d_f0.cpu().numpy(), f0 * scale)
    f0n = f0.copy()
    f0n[3] = np.nan  # the scale is a plain product
    _, got_f0 = _modify_frames(env, fs, fft, sp, None, f0n, scale)
    assert np.array_equal(got_f0, f0n * scale, equal_nan=True) and np.isnan(got_f0[3])


# ---- 3. bad per-frame values ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fs,fft", SIZES)
def test_bad_ratios_make_their_own_rows_nan(env, fs, fft):
    from oracle.gen_golden import synth_params
    n = 67
    _, sp, _ = synth_params(fs, fft, n, 3100 + fft)
    good = cycled(fft, n, 3)
    bad = good.copy()
    at = [0, 13, 40, 66]
    bad[at] = [-1.0, np.nan, np.inf, 1.0 / fft]
    want, _ = _modify_frames(env, fs, fft, sp, good)
    got, _ = _modify_frames(env, fs, fft, sp, bad)
    keep = np.ones(n, bool)
    keep[at] = False
    assert np.isnan(got[at]).all()
    assert np.array_equal(got[keep], want[keep])


# ---- 4. the fused decoder against the composition ---------------------------------------------------------------------------

def _decode(env, fs, fft, nd, csp, cap, ratio=None, modified=True):
    """decode_features_modified_device (or decode_features_device) into NaN-filled, guarded outputs"""
    w, codec, wio, torch = env
    n, bins = csp.shape[0], fft // 2 + 1
    d_sp, d_ap = _guarded(torch, None, n, bins), _guarded(torch, None, n, bins)
    if modified:
        codec.decode_features_modified_device(fs, fft, n, nd, _dev(torch, csp), _dev(torch, cap), None if ratio is None else _dev(torch, ratio),
                                              d_sp, d_ap)
    else:
        codec.decode_features_device(fs, fft, n, nd, _dev(torch, csp), _dev(torch, cap), d_sp, d_ap)
    w.lib().wc_synchronize()
    return _rows(d_sp, n, bins), _rows(d_ap, n, bins)


def _composition(env, fs, fft, nd, csp, cap, ratio):
    sp, ap = _decode(env, fs, fft, nd, csp, cap, modified=False)
    return _modify_frames(env, fs, fft, sp, ratio)[0], ap, sp


def _sizes_cases():
    from oracle.gen_golden_codec_sizes import CASES
    return [c for c in CASES if c[0] >= 12000]


@pytest.mark.parametrize("fs,fft,seed", _sizes_cases())
def test_fused_decoder_against_the_composition(env, fs, fft, seed):
    """every case of tests/golden/io/codec_sizes.npz from 12 kHz up, every nd of test_decode_features_every_size, the ratios of test
    2 cycled over the frames (each nd starts the cycle three places on, so that every size meets all eight).  d_sp within 1e-12
    relative of decode_features_device -> modify_parameters_frames_device, d_ap that of decode_features_device; a NULL ratio is
    decode_features_device.  The bound: the fused kernel interpolates the log values v the decoder holds before its exp, the
    composition interpolates log(exp(v)); on the golden rows (|v| <= 13.5) the two differ by at most 2.2e-16 absolute (checked in
    numpy), the interpolation is a convex combination (for a ratio below 1 the bins that would extrapolate are the ones filled
    from bin cut - 1, which copy one such value), so the exponents agree within 2.2e-16 and the results within that relative --
    1e-12 is the project's allowance for the log / exp of two math libraries and leaves three orders of margin."""
    from oracle.gen_golden_codec_sizes import case_data, sp_decode_cases
    g = np.load(os.path.join(IO, "codec_sizes.npz"))
    sp, ap, only, cap_all, k = case_data(g, fs, fft, seed)
    for i, (nd, csp, ref) in enumerate(sp_decode_cases(g, k, fft, only)):
        rows = [(3 * i + j) % len(cap_all) for j in range(len(csp))]
        cap = cap_all[rows]
        ratio = cycled(fft, len(csp), 3 * i)
        want_sp, want_ap, plain_sp = _composition(env, fs, fft, nd, csp, cap, ratio)
        got_sp, got_ap = _decode(env, fs, fft, nd, csp, cap, ratio)
        rel = np.abs(got_sp / want_sp - 1).max()
        print("fused decoder against the composition, fs %d fft %d nd %d: %.3e" % (fs, fft, nd, rel))
        assert rel < FUSED_REL, (fs, nd)
        assert np.array_equal(got_ap, want_ap, equal_nan=True), (fs, nd)
        null_sp, null_ap = _decode(env, fs, fft, nd, csp, cap, None)
        assert np.array_equal(null_sp, plain_sp) and np.array_equal(null_ap, want_ap, equal_nan=True), (fs, nd)


# ---- 5. the fused decoder against the reference -----------------------------------------------------------------------------

def _port_frames(fs, fft, sp, ratio):
    """oracle.port_io.parameter_modification frame by frame, with that frame's ratio (0 = none)"""
    from oracle import port_io
    out = np.array(sp, dtype=np.float64)
    for i, r in enumerate(ratio):
        if r != 0.0:
            out[i] = port_io.parameter_modification(fs, fft, np.zeros(1), sp[i:i + 1], None, float(r))[1][0]
    return out


@pytest.mark.parametrize("nd", [25, 60, 513])
def test_fused_decoder_against_the_reference(env, nd):
    """case m48k_1s of tests/golden/io/codec_golden.npz (fft 2048, the one-wavefront path): expected = the CPU restatement of the
    reference's modification applied frame by frame to the real reference's decoded rows.  1.2e-11 = 1e-11 (the decoder against
    those rows, test_gpu_synth_coded.py::test_decode_features_golden) + 1e-12 (the modification, test 1) + 1e-13 (port_io against
    the real reference, tests/test_io_formats.py); the stretch does not amplify: a 1e-11 relative perturbation of those rows
    changes port_io's output by at most 1.0001e-11 for every ratio used here (checked on the CPU), and the reference's rows stay
    finite for all of them."""
    g = np.load(os.path.join(IO, "codec_golden.npz"))
    case = "m48k_1s"
    fs, fft = int(g[case + "/fs"]), int(g[case + "/fft"])
    assert fft == 2048
    csp, cap = g[f"{case}/sp_coded_{nd}"], g[case + "/ap_coded"]
    n = csp.shape[0]
    ratio = cycled(fft, n)
    want = _port_frames(fs, fft, g[f"{case}/sp_decoded_{nd}"], ratio)
    assert np.isfinite(want).all()
    got_sp, got_ap = _decode(env, fs, fft, nd, csp, cap, ratio)
    rel = np.abs(got_sp / want - 1).max()
    print("fused decoder against the reference, nd %d: %.3e" % (nd, rel))
    assert rel < REF_REL
    assert np.abs(got_ap - g[case + "/ap_decoded"]).max() < 1e-13


# ---- 6. a frame's rows depend on that frame alone ---------------------------------------------------------------------------

def _coded_rows(env, fs, fft, n, seed, nd):
    """seeded rows (oracle/gen_golden.synth_params) coded on the device: f0, coded sp, coded ap as host arrays"""
    w, codec, wio, torch = env
    from oracle.gen_golden import synth_params
    f0, sp, ap = synth_params(fs, fft, n, seed)
    n_ap = codec.number_of_aperiodicities(fs)
    d_csp = torch.empty(n * nd, dtype=torch.float64, device="cuda")
    d_cap = torch.empty(n * n_ap, dtype=torch.float64, device="cuda")
    codec.code_spectral_envelope_device(fs, fft, n, nd, _dev(torch, sp), d_csp)
    codec.code_aperiodicity_device(fs, fft, n, _dev(torch, ap), d_cap)
    w.lib().wc_synchronize()
    return f0, d_csp.cpu().numpy().reshape(n, nd), d_cap.cpu().numpy().reshape(n, n_ap)


@pytest.mark.parametrize("fs,fft", [(48000, 2048), (24000, 1024)])
def test_fused_rows_depend_on_their_frame_alone(env, fs, fft):
    nd, n = 40, 131
    _, csp, cap = _coded_rows(env, fs, fft, n, 6100, nd)
    _, csp2, cap2 = _coded_rows(env, fs, fft, 87, 6200, nd)
    ratio = cycled(fft, n, 1)
    sp, ap = _decode(env, fs, fft, nd, csp, cap, ratio)
    assert np.isfinite(sp).all() and np.isfinite(ap).all()
    rsp, rap = _decode(env, fs, fft, nd, csp[::-1], cap[::-1], ratio[::-1])
    assert np.array_equal(rsp, sp[::-1]) and np.array_equal(rap, ap[::-1])
    for i in (0, 1, 63, 64, 65, 130):
        osp, oap = _decode(env, fs, fft, nd, csp[i:i + 1], cap[i:i + 1], ratio[i:i + 1])
        assert np.array_equal(osp[0], sp[i]) and np.array_equal(oap[0], ap[i]), i
    r2 = cycled(fft, 87, 5)
    esp, eap = _decode(env, fs, fft, nd, np.concatenate([csp2[:37], csp, csp2[37:]]), np.concatenate([cap2[:37], cap, cap2[37:]]),
                       np.concatenate([r2[:37], ratio, r2[37:]]))
    assert np.array_equal(esp[37:37 + n], sp) and np.array_equal(eap[37:37 + n], ap)


# ---- 7. ordering on the caller's stream -------------------------------------------------------------------------------------

def test_fused_decoder_is_ordered_on_the_callers_stream(env):
    """a long torch kernel in front on a torch stream handed over by wc_set_stream; the coded rows and the ratio array written by
    torch kernels on that stream; four (fs, fft) combinations interleaved, twice; one synchronisation at the end"""
    w, codec, wio, torch = env
    from oracle import port_codec as pc
    from oracle.gen_golden import synth_params
    nd, n = 60, 64
    combos = [(48000, 2048), (24000, 1024), (44100, 2048), (16000, 1024)]
    data, want = [], []
    for fs, fft in combos:
        _, sp, ap = synth_params(fs, fft, n, 7100 + fs // 100)
        csp, cap = pc.code_spectral_envelope(sp, fs, fft, nd), pc.code_aperiodicity(ap, fs, fft)
        ratio = cycled(fft, n, 2)
        data.append((csp, cap, ratio))
        want.append(_composition(env, fs, fft, nd, csp, cap, ratio)[:2])
    host = [tuple(torch.from_numpy(np.ascontiguousarray(a).ravel().copy()).pin_memory() for a in d) for d in data]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert w.lib().wc_set_stream(s.cuda_stream) == 0
    try:
        outs = []
        with torch.cuda.stream(s):
            junk = torch.randn(2048, 2048, device="cuda")
            for _ in range(20):  # a long-running kernel in front: the decoder must wait for it and for the uploads behind it
                junk = junk @ junk * 1e-3
            for rnd in range(2):
                for (fs, fft), (h_csp, h_cap, h_ratio) in zip(combos, host):
                    bins = fft // 2 + 1
                    d_csp, d_cap, d_ratio = (torch.zeros(len(h), dtype=torch.float64, device="cuda") for h in (h_csp, h_cap, h_ratio))
                    d_sp = torch.full(((n + 1) * bins,), np.nan, dtype=torch.float64, device="cuda")
                    d_ap = torch.full(((n + 1) * bins,), np.nan, dtype=torch.float64, device="cuda")
                    d_csp.copy_(h_csp, non_blocking=True)
                    d_cap.copy_(h_cap, non_blocking=True)
                    d_ratio.copy_(h_ratio, non_blocking=True)
                    d_csp.mul_(1.0)    # torch kernels on the stream write the coded rows
                    d_ratio.mul_(1.0)  # and the ratio array
                    codec.decode_features_modified_device(fs, fft, n, nd, d_csp, d_cap, d_ratio, d_sp, d_ap)
                    outs.append((d_sp, d_ap, d_csp, d_cap, d_ratio))
        s.synchronize()  # once
    finally:
        assert w.lib().wc_set_stream(None) == 0
    for i, (d_sp, d_ap, _, _, _) in enumerate(outs):
        fft = combos[i % 4][1]
        want_sp, want_ap = want[i % 4]
        sp, ap = _rows(d_sp, n, fft // 2 + 1), _rows(d_ap, n, fft // 2 + 1)
        assert np.abs(sp / want_sp - 1).max() < FUSED_REL, i
        assert np.array_equal(ap, want_ap, equal_nan=True), i
    for i in range(4):
        m = n * (combos[i][1] // 2 + 1)  # (without the guard row)
        assert torch.equal(outs[i][0][:m], outs[i + 4][0][:m]) and torch.equal(outs[i][1][:m], outs[i + 4][1][:m])


# ---- 8. batch Synthesis -----------------------------------------------------------------------------------------------------

def _ragged_batch(env, fs, fft, nd, seed):
    """3 ragged utterances, per-frame ratios that differ per utterance and ramp inside one"""
    frames = [61, 97, 74]
    parts = [_coded_rows(env, fs, fft, n, seed + u, nd) for u, n in enumerate(frames)]
    ratio = np.concatenate([np.full(frames[0], 1.15), np.linspace(0.8, 1.25, frames[1]), np.where(np.arange(frames[2]) % 9 < 4, 0.0, 0.9)])
    return frames, np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]), ratio


@pytest.mark.parametrize("fs,fft", [(24000, 1024), (48000, 2048), (12000, 512), (96000, 4096)])
def test_compute_coded_modified_equals_decode_then_synthesis(env, fs, fft):
    """compute_coded_modified_device == decode_features_modified_device -> compute_device with the same noise positions (bit for
    bit at fft 1024 / 2048, within ATOMIC_ABS at 512 / 4096, where Synthesis adds with FP64 atomics), and with a NULL ratio
    compute_coded_device"""
    w, codec, wio, torch = env
    nd = 40
    frames, f0, csp, cap, ratio = _ragged_batch(env, fs, fft, nd, 8100)
    same = (lambda a, b: np.array_equal(a, b)) if fft in (1024, 2048) else (lambda a, b: len(a) == len(b) and np.abs(a - b).max() < ATOMIC_ABS)
    syn = w.Synthesis(fs, fft, 5.0)
    ol = [syn.out_length(n) for n in frames]
    start = [1000 * u + 7 for u in range(len(frames))]
    tot, bins = sum(frames), fft // 2 + 1
    d_f0, d_csp, d_cap, d_ratio = (_dev(torch, a) for a in (f0, csp, cap, ratio))
    d_sp = torch.empty(tot * bins, dtype=torch.float64, device="cuda")
    d_ap = torch.empty(tot * bins, dtype=torch.float64, device="cuda")

    def run(fn):
        y = torch.full((sum(ol) + 1,), np.nan, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        end = fn(y)
        w.lib().wc_synchronize()
        y = y.cpu().numpy()
        assert np.isnan(y[-1])
        return y[:-1], end

    codec.decode_features_modified_device(fs, fft, tot, nd, d_csp, d_cap, d_ratio, d_sp, d_ap)
    y_ref, end_ref = run(lambda y: syn.compute_device(d_f0, frames, d_sp, d_ap, ol, y, rng_pos=start))
    y, end = run(lambda y: syn.compute_coded_modified_device(d_f0, frames, d_csp, nd, d_cap, d_ratio, ol, y, rng_pos=start))
    assert end == end_ref
    assert np.isfinite(y).all() and same(y, y_ref)
    y_plain, end_plain = run(lambda y: syn.compute_coded_device(d_f0, frames, d_csp, nd, d_cap, ol, y, rng_pos=start))
    y_null, end_null = run(lambda y: syn.compute_coded_modified_device(d_f0, frames, d_csp, nd, d_cap, None, ol, y, rng_pos=start))
    assert end_null == end_plain and same(y_null, y_plain)
    assert np.abs(y - y_plain).max() > 1e-6  # (the ratios do change the waveform)


@pytest.mark.parametrize("fs,fft,nd", [(16000, 1024, 60), (48000, 2048, 60)])
def test_compute_coded_modified_matches_the_reference_chain(env, port, checker, fs, fft, nd):
    """seeded rows (synth_params, 70 frames) coded and decoded by the reference's codec (oracle/port_codec), stretched frame by
    frame by port_io.parameter_modification, synthesised from noise position 0 by the reference (the real one where oracle/_ref is
    built): the device call on the coded rows and the ratio array within 1e-8, ending at the same noise position"""
    w, codec, wio, torch = env
    from oracle import port_codec as pc
    from oracle.gen_golden import synth_params
    n = 70
    f0, sp, ap = synth_params(fs, fft, n, 4000 + fs // 1000)
    csp, cap = pc.code_spectral_envelope(sp, fs, fft, nd), pc.code_aperiodicity(ap, fs, fft)
    sp_d, ap_d = pc.decode_spectral_envelope(csp, fs, fft), pc.decode_aperiodicity(cap, fs, fft)
    ratio = np.linspace(0.8, 1.25, n)
    ratio[::11] = 0.0
    sp_m = _port_frames(fs, fft, sp_d, ratio)
    port.rng_seek(0)
    y_ref = port.synthesis(f0, sp_m, ap_d, fs, 5.0)
    end = port.rng_position()
    if checker is not None:
        y_ref = checker.stage_at(0, "synthesis", f0, sp_m, ap_d, fs, 5.0)
    syn = w.Synthesis(fs, fft, 5.0)
    ol = syn.out_length(n)
    assert ol == len(y_ref)
    y = torch.full((ol + 1,), np.nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    pos = syn.compute_coded_modified_device(_dev(torch, f0), [n], _dev(torch, csp), nd, _dev(torch, cap), _dev(torch, ratio), [ol], y, rng_pos=[0])
    w.lib().wc_synchronize()
    y = y.cpu().numpy()
    assert np.isnan(y[-1]) and pos == [end]
    err = np.abs(y[:-1] - y_ref).max()
    print("compute_coded_modified against the reference chain, fs %d: %.3e" % (fs, err))
    assert err < Y_ABS


# ---- 9. streams -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fs,fft,fp", [(24000, 1024, 1.0), (48000, 2048, 5.0)])
def test_stream_settings(env, fs, fft, fp):
    """four ragged streams pushed with the irregular pattern of the coded-push test: stream 0 at (1.2, 0.9), stream 1 neutral,
    stream 2 at (0.8, 1.15) changed to (1.0, 0.8) between two pushes, stream 3 with a setting and reset in mid-signal (back to
    neutral).  Every push's committed samples equal, bit for bit, those of a second StreamSynthesizer fed by push_device with rows
    from decode_features_modified_device (per-frame ratios = the settings in force) and f0 * scale; stream 1 equals an unmodified
    coded push; refused settings and a refused push_device leave everything as it was"""
    w, codec, wio, torch = env
    from world_class_amd.stream import StreamSynthesizer
    nd, n = 30, 4
    frames = [150, 103, 171, 126]
    parts = [_coded_rows(env, fs, fft, m, 9100 + u, nd) for u, m in enumerate(frames)]
    bins = fft // 2 + 1
    pattern = [[1, 7, 40], [33, 0, 1], [7, 0, 0, 40], [50]]
    A, B, P = (StreamSynthesizer(fs, fft, fp, n, 50) for _ in range(3))  # settings | full rows | stream 1 alone, no settings
    setting = [(1.2, 0.9), (1.0, 0.0), (0.8, 1.15), (1.1, 1.05)]
    for u in (0, 2, 3):
        A.set_modification(u, *setting[u])
    state = lambda S: [(S.frames_received(u), S.samples_committed(u), S.rng_position(u)) for u in range(n)]
    y_of = lambda d_y, counts: np.split(d_y.cpu().numpy()[:sum(counts)], np.cumsum(counts)[:-1])
    new_y = lambda S: torch.full((n * S.max_samples,), np.nan, dtype=torch.float64, device="cuda")
    pos, k, done = [0] * n, [0] * n, [False] * n
    got1, plain1, pushes, changed, was_reset = [], [], 0, False, False
    while not all(done):
        if not changed and pos[2] >= 60:  # between two pushes in mid-signal
            setting[2] = (1.0, 0.8)
            A.set_modification(2, *setting[2])
            changed = True
        if not was_reset and pos[3] >= 50:  # the rest of stream 3 is a new signal: from frame 0, noise position 0, neutral
            A.reset(3)
            B.reset(3)
            setting[3] = (1.0, 0.0)
            was_reset = True
        cnt, flush = [], []
        for u in range(n):
            c = 0 if done[u] else min(pattern[u][k[u] % len(pattern[u])], frames[u] - pos[u])
            k[u] += 1
            cnt.append(c)
            flush.append(1 if not done[u] and pos[u] + c >= frames[u] else 0)
        take = lambda j: np.concatenate([parts[u][j][pos[u]:pos[u] + cnt[u]] for u in range(n)]) if sum(cnt) else np.zeros((1, (1, nd, parts[0][2].shape[1])[j]))
        f0, csp, cap = take(0).ravel(), take(1), take(2)
        scale = np.concatenate([np.full(cnt[u], setting[u][0]) for u in range(n)]) if sum(cnt) else np.ones(1)
        ratio = np.concatenate([np.full(cnt[u], setting[u][1]) for u in range(n)]) if sum(cnt) else np.zeros(1)
        d_f0, d_csp, d_cap = _dev(torch, f0), _dev(torch, csp), _dev(torch, cap)
        if pushes == 2:
            for bad in ((0.0, 0.9), (np.nan, 0.9), (np.inf, 0.9), (-1.0, 0.9), (1.2, -0.5), (1.2, 1.0 / fft), (1.2, np.nan), (1.2, np.inf)):
                with pytest.raises(w.WorldClassError):
                    A.set_modification(0, *bad)
            with pytest.raises(w.WorldClassError):
                A.set_modification(n, 1.0, 0.0)
        if cnt[0] > 0 and pushes >= 2:  # full rows for a stream with a setting: refused, every stream as it was
            before = state(A)
            rows = torch.ones(sum(cnt) * bins, dtype=torch.float64, device="cuda")
            d_y = new_y(A)
            torch.cuda.synchronize()
            with pytest.raises(w.WorldClassError):
                A.push_device(cnt, d_f0, rows, rows, flush, d_y)
            assert state(A) == before and bool(torch.isnan(d_y).all())
        ya, yb, yp = new_y(A), new_y(B), new_y(P)
        d_sp = torch.full((sum(cnt) * bins + 1,), np.nan, dtype=torch.float64, device="cuda")
        d_ap = torch.full((sum(cnt) * bins + 1,), np.nan, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ca = A.push_coded_device(cnt, d_f0, d_csp, nd, d_cap, flush, ya)
        codec.decode_features_modified_device(fs, fft, sum(cnt), nd, d_csp, d_cap, _dev(torch, ratio), d_sp, d_ap)
        cb = B.push_device(cnt, _dev(torch, f0 * scale[:len(f0)]), d_sp, d_ap, flush, yb)
        assert ca == cb and state(A) == state(B), pushes
        for u, (a, b) in enumerate(zip(y_of(ya, ca), y_of(yb, cb))):
            assert np.array_equal(a, b), (pushes, u)
        got1.append(y_of(ya, ca)[1])
        only1 = [c if u == 1 else 0 for u, c in enumerate(cnt)]
        o1 = sum(cnt[:1])
        cp = P.push_coded_device(only1, _dev(torch, f0[o1:o1 + cnt[1]] if cnt[1] else np.zeros(1)), _dev(torch, csp[o1:o1 + cnt[1]] if cnt[1] else csp[:1]),
                                 nd, _dev(torch, cap[o1:o1 + cnt[1]] if cnt[1] else cap[:1]), [f if u == 1 else 0 for u, f in enumerate(flush)], yp)
        plain1.append(y_of(yp, cp)[1])
        for u in range(n):
            pos[u] += cnt[u]
            done[u] = done[u] or bool(flush[u])
        pushes += 1
    assert changed and was_reset and pushes > 4
    assert np.array_equal(np.concatenate(got1), np.concatenate(plain1))
    assert A.samples_committed(1) == P.samples_committed(1) == len(np.concatenate(got1)) > 0
    assert A.rng_position(1) == P.rng_position(1)


# ---- 10. refused calls ------------------------------------------------------------------------------------------------------

def test_refused_calls_leave_the_outputs_untouched(env):
    w, codec, wio, torch = env
    L = w.lib()
    fs, fft, nd, n = 48000, 2048, 20, 8
    bins = fft // 2 + 1
    f0, csp, cap = _coded_rows(env, fs, fft, n, 10100, nd)
    d_f0, d_csp, d_cap, d_ratio = _dev(torch, f0), _dev(torch, csp), _dev(torch, cap), _dev(torch, np.full(n, 0.9))
    d_sp = torch.full((n * bins,), np.nan, dtype=torch.float64, device="cuda")
    d_ap = torch.full((n * bins,), np.nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for a_fs, a_fft, a_n, a_nd, a_csp, a_sp in ((fs, 3000, n, nd, d_csp, d_sp), (fs, fft, n, 0, d_csp, d_sp), (fs, fft, n, fft // 2 + 1, d_csp, d_sp),
                                              (fs, fft, n, nd, 0, d_sp), (fs, fft, n, nd, d_csp, 0), (fs, fft, -1, nd, d_csp, d_sp),
                                              (8000, 1024, n, nd, d_csp, d_sp)):
        with pytest.raises(w.WorldClassError):
            codec.decode_features_modified_device(a_fs, a_fft, a_n, a_nd, a_csp, d_cap, d_ratio, a_sp, d_ap)
    for a_fs, a_fft, a_n in ((fs, fft, -1), (fs, fft, 1 << 32), (fs, 8192, n), (0, fft, n)):
        with pytest.raises(w.WorldClassError):
            wio.modify_parameters_frames_device(a_fs, a_fft, a_n, d_ap, d_sp, d_ratio, d_ratio)
    syn, syn8 = w.Synthesis(fs, fft, 5.0), w.Synthesis(8000, 1024, 5.0)
    ol = [syn.out_length(n)]
    y = torch.full((ol[0],), np.nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ints = lambda v: (C.c_int * len(v))(*v)
    ptr = lambda a: a if isinstance(a, int) else a.data_ptr()
    for h, a_csp, a_nd, a_cap in ((syn, d_csp, 0, d_cap), (syn, d_csp, fft // 2 + 1, d_cap), (syn8, d_csp, nd, d_cap), (syn, 0, nd, d_cap),
                                  (syn, d_csp, nd, 0)):
        pos = (C.c_uint64 * 1)(5)
        rc = L.wc_synthesis_compute_coded_modified_device(h._h, 1, d_f0.data_ptr(), ints([n]), ptr(a_csp), a_nd, ptr(a_cap), d_ratio.data_ptr(),
                                                          ints(ol), y.data_ptr(), pos)
        assert rc == -1 and w.last_error()
        assert list(pos) == [5]
    L.wc_synchronize()
    assert bool(torch.isnan(d_sp).all()) and bool(torch.isnan(d_ap).all()) and bool(torch.isnan(y).all())
