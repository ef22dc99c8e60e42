"""-m gpu: the chain pipeline-coded -> pack -> GMM conversion -> MLPG (one row of variances per frame) -> unpack -> coded Synthesis on
device arrays, and the same conversion push by push in front of an MLPG stream."""
import numpy as np
import pytest

import features_rule as fr
import gmm_rule as gm
import mlpg_stream_rule as ms

pytestmark = pytest.mark.gpu

PICKS = (3, 20, 41, 60, 77, 95, 120, 150)     # the frames whose mgc blocks are the mixtures' source means
SHIFT = 0.05


@pytest.fixture(scope="module")
def chain():
    """Two short 16 kHz utterances through the coded pipeline call and pack(orders = 2).  The model is built from the packed rows:
    8 mixtures whose source means are 8 rows of the mgc block (statics and deltas, 2 * nd columns from 0), Sxx the diagonal of the
    block's natural variance, Syx = 0.5 Sxx, Syy = Sxx, target means the source means plus a fixed shift"""
    import torch
    import world_class_amd as w
    from world_class_amd import codec, features as ft, gmm
    from world_class_amd.synth import make_utterance
    w.lib().wc_set_device(0)
    fs, nd = 16000, 25
    xs = [make_utterance(fs, 0.5, 2024), make_utterance(fs, 0.4, 7)]
    xl = [len(x) for x in xs]
    p = w.Pipeline(fs)
    fl, yl = p.lengths(xl)
    T, n_ap = sum(fl), codec.number_of_aperiodicities(fs)
    W2, W1, dx = fr.width(nd, n_ap, 2), fr.width(nd, n_ap, 1), 2 * nd
    z = lambda n: torch.full((n,), np.nan, dtype=torch.float64, device="cuda")
    d_x = torch.from_numpy(np.concatenate(xs)).cuda()
    tpos, f0, csp, cap, y0, rows = z(T), z(T), z(T * nd), z(T * n_ap), z(sum(yl)), z(T * W2)
    torch.cuda.synchronize()
    p.run_coded_device(d_x, xl, tpos, f0, csp, nd, cap, y0, rng_pos=[0, 0])
    ft.pack(fl, nd, n_ap, 2, f0, csp, cap, rows)
    w.lib().wc_synchronize()
    host = rows.cpu().numpy().reshape(T, W2)
    assert np.isfinite(host).all() and T > max(PICKS)
    block = host[:, :dx]
    sxx = block.var(axis=0)
    assert (sxx > 0).all()
    mux = block[list(PICKS)]
    mean, cov = gmm.joint_from_blocks(mux, mux + SHIFT, np.tile(np.diag(sxx), (8, 1, 1)), np.tile(np.diag(0.5 * sxx), (8, 1, 1)), np.tile(sxx, (8, 1)))
    weight = np.full(8, 0.125)
    g = gmm.Gmm(weight, mean, cov, dx)
    c, Wm, B, cvar = g.prepared()
    own = dict(c=c, W=Wm, B=B, cvar=cvar, mux=mean[:, :dx].copy(), muy=mean[:, dx:].copy())
    yield dict(w=w, ft=ft, torch=torch, fs=fs, nd=nd, n_ap=n_ap, fl=fl, yl=yl, T=T, W2=W2, W1=W1, dx=dx, rows=rows, host=host, g=g, own=own, z=z,
               syn=w.Synthesis(fs, p.fft_size, 5.0))
    g.close()


def test_chain_with_gmm_conversion_on_the_device(chain):
    """convert writes the mgc block into mean and variance rows that were initialised from the packed rows and a constant variance;
    MLPG with one row of variances per frame, unpack and coded Synthesis follow.  Mean, variance and best equal the rule bit for bit on
    the device's own packed rows, every best lies in [0, 8), the static mgc columns equal features_rule.mlpg on those means and
    variances, and the waveform is finite and not silent"""
    s = chain
    w, ft, torch, z, g = s["w"], s["ft"], s["torch"], s["z"], s["g"]
    nd, n_ap, fl, yl, T, W2, W1, dx = s["nd"], s["n_ap"], s["fl"], s["yl"], s["T"], s["W2"], s["W1"], s["dx"]
    d_mean = s["rows"].clone()
    d_var = torch.full((T * W2,), 0.25, dtype=torch.float64, device="cuda")
    d_best = torch.full((T + 1,), -7, dtype=torch.int32, device="cuda")
    static, f0_m, csp_m, cap_m, y_m = z(T * W1), z(T), z(T * nd), z(T * n_ap), z(sum(yl) + 1)
    torch.cuda.synchronize()
    g.convert(T, s["rows"], W2, d_mean, d_var, W2, d_best=d_best)
    ft.mlpg(fl, nd, n_ap, 2, d_mean, d_var, static, var_per_frame=True)
    ft.unpack(T, nd, n_ap, 1, static, f0_m, csp_m, cap_m)
    s["syn"].compute_coded_device(f0_m, fl, csp_m, nd, cap_m, yl, y_m, rng_pos=[0, 0])
    w.lib().wc_synchronize()
    torch.cuda.synchronize()
    mean, var, best = d_mean.cpu().numpy().reshape(T, W2), d_var.cpu().numpy().reshape(T, W2), d_best.cpu().numpy()
    want_mean, want_var, want_best, _ = gm.convert(s["own"], s["host"][:, :dx])
    assert np.array_equal(mean[:, :dx], want_mean) and np.array_equal(var[:, :dx], want_var) and np.array_equal(best[:T], want_best)
    assert best[T] == -7 and ((best[:T] >= 0) & (best[:T] < 8)).all() and len(set(best[:T].tolist())) > 1
    assert np.array_equal(best[list(PICKS)], np.arange(8))                       # a source mean belongs to its own mixture
    assert np.array_equal(mean[:, dx:], s["host"][:, dx:]) and (var[:, dx:] == 0.25).all()   # every other column is as it was
    assert (var[:, :dx] > 0).all() and not np.array_equal(mean[:, :dx], s["host"][:, :dx])
    got = static.cpu().numpy().reshape(T, W1)
    want = fr.mlpg(fl, nd, n_ap, 2, mean, var, True)
    assert np.isfinite(got).all() and np.array_equal(got[:, :nd], want[:, :nd])
    y = y_m.cpu().numpy()
    assert np.isnan(y[-1]) and np.isfinite(y[:-1]).all() and np.abs(y[:-1]).max() > 1e-3


def test_conversion_in_pushes_in_front_of_an_mlpg_stream(chain):
    """the first utterance's rows through convert in pushes of 4, each push handed on to an MLPG stream with a lag of 8 and one row of
    variances per frame: the converted rows equal those of one call, and the stream emits its rule's rows on them"""
    from world_class_amd import mlpg_stream
    s = chain
    w, torch, z, g = s["w"], s["torch"], s["z"], s["g"]
    nd, n_ap, W2, W1, dx, nf, lag = s["nd"], s["n_ap"], s["W2"], s["W1"], s["dx"], s["fl"][0], 8
    cuts = [4] * (nf // 4) + ([nf % 4] if nf % 4 else [])
    d_mean = s["rows"][:nf * W2].clone()
    d_var = torch.full((nf * W2,), 0.25, dtype=torch.float64, device="cuda")
    d_static = z(9 * W1)
    h = mlpg_stream.MlpgStream(1, nd, n_ap, 2, 8, 128)
    torch.cuda.synchronize()
    h.reset(0, lag)
    o, emitted = 0, []
    for k in cuts:
        g.convert(k, s["rows"][o * W2:], W2, d_mean[o * W2:], d_var[o * W2:], W2)
        n, = h.push_device([k], d_mean[o * W2:(o + k) * W2], d_var[o * W2:(o + k) * W2], d_static, var_per_frame=True)
        o += k
        assert n == ms.emitted(o, lag) - ms.emitted(o - k, lag)
        w.lib().wc_synchronize()
        emitted.append(d_static.cpu().numpy()[:n * W1].reshape(n, W1).copy())
    n, = h.flush_device([1], d_static)
    w.lib().wc_synchronize()
    tail = d_static.cpu().numpy()[:n * W1].reshape(n, W1).copy()
    h.close()
    mean, var = d_mean.cpu().numpy().reshape(nf, W2), d_var.cpu().numpy().reshape(nf, W2)
    want_mean, want_var, _, _ = gm.convert(s["own"], s["host"][:nf, :dx])
    assert np.array_equal(mean[:, :dx], want_mean) and np.array_equal(var[:, :dx], want_var)
    want, want_tail = ms.stream(nd, n_ap, 2, lag, mean, var, True, cuts)
    assert n == lag and sum(len(a) for a in emitted) + n == nf
    for got, rule_rows in zip(emitted + [tail], want + [want_tail]):
        assert got.shape == rule_rows.shape and np.array_equal(got, rule_rows)
