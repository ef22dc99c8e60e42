"""-m gpu: the chain pipeline-coded -> pack -> (an over-smoothing model) -> MLPG -> GV -> unpack -> coded Synthesis on device arrays."""
import numpy as np
import pytest

import features_rule as fr

pytestmark = pytest.mark.gpu


def test_chain_with_global_variance_on_the_device():
    """Two utterances through the coded pipeline call; the "model" is their coded rows blurred by a moving average of 5 frames, packed
    with deltas, with variances a hundredth of the natural variance of each column; the global variance is the natural one: the
    mean over the two utterances of each column's variance over the voiced frames (the mask), a tenth of its square for its variance,
    a column that does not vary switched off by +inf.  MLPG, the refinement, unpack and coded Synthesis follow on the device.  The
    waveform is finite, and in every column that is on the variance of each utterance over its masked frames lies closer to gv_mean
    after the refinement than MLPG's"""
    import torch
    import world_class_amd as w
    from world_class_amd import codec, features as ft, gv
    from world_class_amd.synth import make_utterance
    w.lib().wc_set_device(0)
    fs, nd = 16000, 25
    xs = [make_utterance(fs, 0.5, 2024), make_utterance(fs, 0.4, 7)]
    xl = [len(x) for x in xs]
    p = w.Pipeline(fs)
    syn = w.Synthesis(fs, p.fft_size, 5.0)
    fl, yl = p.lengths(xl)
    T, n_ap = sum(fl), codec.number_of_aperiodicities(fs)
    S, W3, W1 = nd + 1 + n_ap, fr.width(nd, n_ap, 3), fr.width(nd, n_ap, 1)
    z = lambda n: torch.full((n,), np.nan, dtype=torch.float64, device="cuda")
    sync = lambda: (w.lib().wc_synchronize(), torch.cuda.synchronize())
    d_x = torch.from_numpy(np.concatenate(xs)).cuda()
    tpos, f0, csp, cap, y0, nat = z(T), z(T), z(T * nd), z(T * n_ap), z(sum(yl)), z(T * W1)
    g_mean, g_var = z(2 * S), z(2 * S)
    torch.cuda.synchronize()
    p.run_coded_device(d_x, xl, tpos, f0, csp, nd, cap, y0, rng_pos=[0, 0])
    ft.pack(fl, nd, n_ap, 1, f0, csp, cap, nat)
    sync()
    mask = (f0 > 0).to(torch.uint8)
    torch.cuda.synchronize()
    gv.stats(fl, nd, n_ap, nat, g_mean, g_var, mask)
    sync()
    assert int(mask[:fl[0]].sum()) >= 2 and int(mask[fl[0]:].sum()) >= 2
    gv_mean = g_var.cpu().numpy().reshape(2, S).mean(axis=0)
    on = gv_mean > 0.0
    assert on[:nd + 1].all()
    gv_var = np.where(on, 0.1 * gv_mean * gv_mean, np.inf)
    gv_mean = np.where(on, gv_mean, 1.0)

    def blur(t, cols):   # a moving average of 5 frames inside every utterance, the ends repeated
        out, o = [], 0
        for n in fl:
            x = t[o * cols:(o + n) * cols].view(n, cols)
            xp = torch.cat([x[:1].repeat(2, 1), x, x[-1:].repeat(2, 1)])
            out.append(sum(xp[i:i + n] for i in range(5)) / 5.0)
            o += n
        return torch.cat(out).reshape(-1).contiguous()

    csp_b, cap_b = blur(csp, nd), blur(cap, n_ap)
    cols, vuv_col = fr.columns(nd, n_ap, 3)
    var_row = np.ones(W3)
    for c, ks in enumerate(cols):
        var_row[ks] = 0.01 * gv_mean[c]
    rows, static = z(T * W3), z(T * W1)
    d_var, d_gm, d_gvv = (torch.from_numpy(a).cuda() for a in (var_row, gv_mean, gv_var))
    v_ml, v_gv, unused = z(2 * S), z(2 * S), z(2 * S)
    f0_m, csp_m, cap_m, y_m = z(T), z(T * nd), z(T * n_ap), z(sum(yl) + 1)
    torch.cuda.synchronize()
    ft.pack(fl, nd, n_ap, 3, f0, csp_b, cap_b, rows)
    ft.mlpg(fl, nd, n_ap, 3, rows, d_var, static)
    gv.stats(fl, nd, n_ap, static, unused, v_ml, mask)
    gv.mlpg_gv(fl, nd, n_ap, 3, rows, d_var, d_gm, d_gvv, static, mask)
    gv.stats(fl, nd, n_ap, static, unused, v_gv, mask)
    ft.unpack(T, nd, n_ap, 1, static, f0_m, csp_m, cap_m)
    syn.compute_coded_device(f0_m, fl, csp_m, nd, cap_m, yl, y_m, rng_pos=[0, 0])
    sync()
    y = y_m.cpu().numpy()
    assert np.isnan(y[-1]) and np.isfinite(y[:-1]).all() and np.abs(y[:-1]).max() > 1e-3
    v_ml, v_gv = v_ml.cpu().numpy().reshape(2, S), v_gv.cpu().numpy().reshape(2, S)
    far_ml, far_gv = np.abs(v_ml - gv_mean)[:, on], np.abs(v_gv - gv_mean)[:, on]
    print("chain with GV: |v - gv_mean| / gv_mean, worst column: MLPG %.3f, refined %.3f; %d of %d columns on"
          % ((far_ml / gv_mean[on]).max(), (far_gv / gv_mean[on]).max(), on.sum(), S))
    assert (far_gv < far_ml).all()
    assert np.array_equal(v_gv[:, ~on], v_ml[:, ~on], equal_nan=True)
    assert np.array_equal(f0_m.cpu().numpy() > 0, f0.cpu().numpy() > 0)      # the voicing is the pipeline's
