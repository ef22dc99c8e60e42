"""-m gpu: the chain pipeline-coded -> pack -> MLPG -> unpack -> coded Synthesis with no host copy between its steps."""
import numpy as np
import pytest

import features_rule as fr
from test_gpu_features import env  # noqa: F401

pytestmark = pytest.mark.gpu

Y_ABS = 1e-8   # the project's Synthesis tolerance, which the morph tests hold their chain to (tests/test_gpu_retime.py)


@pytest.mark.parametrize("fs,nd", [(16000, 25), (48000, 60)])
def test_chain_on_the_device(env, fs, nd):
    """A 0.5 s utterance through the coded pipeline call, pack(orders=3), MLPG with equal variances, unpack, coded Synthesis: every
    step enqueued on device arrays, one synchronisation at the end.  The voicing is the pipeline's; the coded rows come back within
    1e-12 of max|x| (the bound of the consistent-means tests); the waveform is finite and within Y_ABS of the Synthesis of the rows
    unpacked without MLPG, from the same noise position.  Derivation: rows that move by d = 1e-12 max|x| move the log envelope by at
    most nd d (every basis function of the decoder is bounded by 1), 60 x 1e-12 x 10 = 6e-10 relative in the spectrum and in a
    waveform of amplitude below 1 -- under Y_ABS with room, above the 1e-12 of a bit-compatible composition."""
    w, ft, torch = env
    from world_class_amd import codec
    from world_class_amd.synth import make_utterance
    x = make_utterance(fs, 0.5, 2024)
    p = w.Pipeline(fs)
    syn = w.Synthesis(fs, p.fft_size, 5.0)
    fl, yl = p.lengths([len(x)])
    nf, n_ap = fl[0], codec.number_of_aperiodicities(fs)
    W3, W1 = fr.width(nd, n_ap, 3), fr.width(nd, n_ap, 1)
    z = lambda n: torch.full((n,), np.nan, dtype=torch.float64, device="cuda")
    d_x = torch.from_numpy(x).cuda()
    tpos, f0, csp, cap, y0 = z(nf), z(nf), z(nf * nd), z(nf * n_ap), z(yl[0])
    rows, var, static = z(nf * W3), torch.full((W3,), 0.3, dtype=torch.float64, device="cuda"), z(nf * W1)
    f0_m, csp_m, cap_m, y_m = z(nf), z(nf * nd), z(nf * n_ap), z(yl[0] + 1)
    f0_p, csp_p, cap_p, y_p = z(nf), z(nf * nd), z(nf * n_ap), z(yl[0] + 1)
    torch.cuda.synchronize()
    p.run_coded_device(d_x, [len(x)], tpos, f0, csp, nd, cap, y0, rng_pos=[0])
    ft.pack([nf], nd, n_ap, 3, f0, csp, cap, rows)
    ft.mlpg([nf], nd, n_ap, 3, rows, var, static)
    ft.unpack(nf, nd, n_ap, 1, static, f0_m, csp_m, cap_m)
    syn.compute_coded_device(f0_m, [nf], csp_m, nd, cap_m, yl, y_m, rng_pos=[0])
    ft.unpack(nf, nd, n_ap, 3, rows, f0_p, csp_p, cap_p)   # the pack's own statics, without MLPG
    syn.compute_coded_device(f0_p, [nf], csp_p, nd, cap_p, yl, y_p, rng_pos=[0])
    w.lib().wc_synchronize()
    h = lambda t, *shape: t.cpu().numpy().reshape(*shape) if shape else t.cpu().numpy()
    f0_h = h(f0)
    on = f0_h > 0
    assert on.any()
    for got in (h(f0_m), h(f0_p)):   # the voicing is the pipeline's; F0 is the exp of a log that moved by 1e-12 of max|lf0| at most
        assert np.array_equal(got > 0, on) and np.array_equal(got == 0, ~on)
        assert (np.abs(got[on] - f0_h[on]) / f0_h[on]).max() < 1e-12 * np.abs(np.log(f0_h[on])).max() + 1e-12
    assert np.array_equal(h(csp_p), h(csp)) and np.array_equal(h(cap_p), h(cap))   # the statics travel as they are
    e_sp = np.abs(h(csp_m) - h(csp)).max() / np.abs(h(csp)).max()
    e_ap = np.abs(h(cap_m) - h(cap)).max() / max(np.abs(h(cap)).max(), 1e-300)
    ym, yp = h(y_m), h(y_p)
    assert np.isnan(ym[-1]) and np.isnan(yp[-1])
    e_y = np.abs(ym[:-1] - yp[:-1]).max()
    print("chain fs %d: coded sp %.3e, coded ap %.3e of max|x|; waveform %.3e (max|y| %.3f)" % (fs, e_sp, e_ap, e_y, np.abs(yp[:-1]).max()))
    assert e_sp <= 1e-12 and e_ap <= 1e-12
    assert np.isfinite(ym[:-1]).all() and np.abs(yp[:-1]).max() > 1e-3
    assert e_y < Y_ABS
