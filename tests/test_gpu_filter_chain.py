"""-m gpu: the frame filter behind the conversion chain.  Two voices through the device's coded pipeline step; voice A filtered by
decode(code(B) - code(A)) is held to tests/filter_rule.py on the downloaded rows and, analysed again, lies closer to B's envelope than
A did in every frame; and pack -> GMM convert -> MLPG -> unpack -> run_coded(to = converted, from = source) runs end to end on device
arrays with a one-mixture model whose conditional mean is the identity plus a constant offset."""
import numpy as np
import pytest

import features_rule as ftr
import filter_rule as fr

pytestmark = pytest.mark.gpu

FS, N, ND, FP = 16000, 1024, 60, 5.0
BOUND = fr.K


@pytest.fixture(scope="module")
def voices():
    """make_utterance seeds 1 and 2, 0.6 s at 16 kHz, through the coded pipeline step with 60 dimensions"""
    import torch
    import world_class_amd as w
    from world_class_amd import codec, filter as ff
    from world_class_amd.synth import make_utterance
    w.lib().wc_set_device(0)
    xs = [make_utterance(FS, 0.6, 1), make_utterance(FS, 0.6, 2)]
    xl = [len(x) for x in xs]
    p = w.Pipeline(FS)
    assert p.fft_size == N
    fl, yl = p.lengths(xl)
    T, n_ap = sum(fl), codec.number_of_aperiodicities(FS)
    z = lambda n: torch.full((n,), np.nan, dtype=torch.float64, device="cuda")
    d_x = torch.from_numpy(np.concatenate(xs)).cuda()
    tpos, f0, csp, cap, y0 = z(T), z(T), z(T * ND), z(T * n_ap), z(sum(yl))
    torch.cuda.synchronize()
    p.run_coded_device(d_x, xl, tpos, f0, csp, ND, cap, y0, rng_pos=[0, 0])
    w.lib().wc_synchronize()
    h = ff.FrameFilter(FS, N, FP)
    assert [h.segments(n) for n in xl] == fl    # one row per segment here
    yield dict(w=w, torch=torch, codec=codec, xs=xs, xl=xl, fl=fl, T=T, n_ap=n_ap, d_x=d_x, tpos=tpos, f0=f0, csp=csp, cap=cap, z=z, h=h)
    h.close()


def decoded(s, d):
    """rows of the spectral-envelope decoder on the host array d, through the device's public call"""
    torch = s["torch"]
    d_d = torch.from_numpy(np.ascontiguousarray(d).ravel()).cuda()
    d_sp = s["z"](len(d) * (N // 2 + 1))
    s["codec"].decode_spectral_envelope_device(FS, N, len(d), ND, d_d, d_sp)
    s["w"].lib().wc_synchronize()
    return d_sp.cpu().numpy().reshape(len(d), N // 2 + 1)


def test_a_voice_filtered_towards_another(voices):
    s = voices
    w, torch = s["w"], s["torch"]
    na, fa = s["xl"][0], s["fl"][0]
    d_xa, c_a, c_b = s["d_x"][:na], s["csp"][:fa * ND], s["csp"][fa * ND:]
    d_y = s["z"](na)
    s["h"].run_coded(d_xa, [na], c_b, c_a, ND, [fa], d_y)
    w.lib().wc_synchronize()
    y = d_y.cpu().numpy()
    # the numbers: the rule on the downloaded rows
    csp = s["csp"].cpu().numpy().reshape(s["T"], ND)
    rows = decoded(s, csp[fa:] - csp[:fa])
    want = fr.frame_filter(s["xs"][0], rows, fr.POWER, FS, N, FP)
    ratio = float(np.abs(y - want).max() / fr.unit(s["xs"][0], rows, fr.POWER, FS, N, FP))
    print("chain: max |device - rule| / u = %.4f (K = %s)" % (ratio, fr.K))
    assert np.isfinite(y).all() and ratio <= BOUND
    # what it is for: CheapTrick of the result on A's contour against B's envelope
    tpos, f0 = s["tpos"].cpu().numpy(), s["f0"].cpu().numpy()
    ct = w.CheapTrick(FS)
    sp_a = ct.compute(s["xs"][0], tpos[:fa], f0[:fa])
    sp_b = ct.compute(s["xs"][1], tpos[fa:], f0[fa:])
    sp_y = ct.compute(y, tpos[:fa], f0[:fa])
    lsd = lambda p, q: np.sqrt(np.mean((10.0 * np.log10(p / q)) ** 2, axis=1))
    before, after = lsd(sp_a, sp_b), lsd(sp_y, sp_b)
    print("chain: mean log-spectral distance to B %.3f dB -> %.3f dB, ratio %.4f, worst frame %.4f"
          % (before.mean(), after.mean(), after.mean() / before.mean(), (after / before).max()))
    assert (after < before).all() and after.mean() / before.mean() <= 0.5


def test_pack_convert_mlpg_unpack_filter_on_the_device(voices):
    """one mixture with Syx = Sxx: the conditional mean is x - mux + muy, the identity plus the offset; its variance Syy - Sxx"""
    from world_class_amd import features as ft, gmm
    s = voices
    w, torch, z = s["w"], s["torch"], s["z"]
    na, fa, n_ap = s["xl"][0], s["fl"][0], s["n_ap"]
    W2, W1, dx = ftr.width(ND, n_ap, 2), ftr.width(ND, n_ap, 1), 2 * ND
    f0, c_a, cap = s["f0"][:fa], s["csp"][:fa * ND], s["cap"][:fa * n_ap]
    rows = z(fa * W2)
    ft.pack([fa], ND, n_ap, 2, f0, c_a, cap, rows)
    w.lib().wc_synchronize()
    block = rows.cpu().numpy().reshape(fa, W2)[:, :dx]
    sxx = block.var(axis=0) + 1e-3
    offset = np.concatenate([0.3 / (1.0 + np.arange(ND)), np.zeros(ND)])     # on the statics; a constant has no delta
    mux = block.mean(axis=0)
    mean, cov = gmm.joint_from_blocks(mux[None], (mux + offset)[None], np.diag(sxx)[None], np.diag(sxx)[None], 2.0 * sxx[None])
    g = gmm.Gmm([1.0], mean, cov, dx)
    d_mean = rows.clone()
    d_var = torch.full((fa * W2,), 0.25, dtype=torch.float64, device="cuda")
    static, f0_m, csp_m, cap_m, d_y = z(fa * W1), z(fa), z(fa * ND), z(fa * n_ap), z(na)
    torch.cuda.synchronize()
    g.convert(fa, rows, W2, d_mean, d_var, W2)
    ft.mlpg([fa], ND, n_ap, 2, d_mean, d_var, static, var_per_frame=True)
    ft.unpack(fa, ND, n_ap, 1, static, f0_m, csp_m, cap_m)
    s["h"].run_coded(s["d_x"][:na], [na], csp_m, c_a, ND, [fa], d_y)
    w.lib().wc_synchronize()
    g.close()
    y, to, frm = d_y.cpu().numpy(), csp_m.cpu().numpy().reshape(fa, ND), c_a.cpu().numpy().reshape(fa, ND)
    # (the generation answers the offset only in the middle: pack's deltas count a neighbour outside the utterance as 0.0, so a constant
    # has a delta at the two ends, which the model's offset row does not carry)
    print("chain through the model: converted - source - offset, median %.2e, worst %.2e"
          % (np.median(np.abs((to - frm) - offset[:ND])), np.abs((to - frm) - offset[:ND]).max()))
    assert np.isfinite(to).all() and np.abs(to - frm).max() > 0.1
    gains = decoded(s, to - frm)
    want = fr.frame_filter(s["xs"][0], gains, fr.POWER, FS, N, FP)
    ratio = float(np.abs(y - want).max() / fr.unit(s["xs"][0], gains, fr.POWER, FS, N, FP))
    print("chain through the model: max |device - rule| / u = %.4f (K = %s)" % (ratio, fr.K))
    assert np.isfinite(y).all() and ratio <= BOUND and np.abs(y - s["xs"][0]).max() > 1e-3
