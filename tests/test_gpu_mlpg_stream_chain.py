"""-m gpu: the streaming chain MLPG stream -> unpack(orders=1) -> wc_synth_stream_push_coded_device with n_frames = frames_out, no
host copy between its steps, against the whole-utterance chain wc_mlpg_device -> unpack -> the same synthesis stream."""
import numpy as np
import pytest

import features_rule as fr
import mlpg_stream_rule as ms
from test_gpu_features import env  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup(env):
    """a 0.5 s utterance at 16 kHz through the coded pipeline call and pack(orders=3): the rows a model would predict; one row of
    variances (1, 0.1, 0.05) for statics, deltas and delta-deltas"""
    w, ft, torch = env
    from world_class_amd import codec, mlpg_stream
    from world_class_amd.stream import StreamSynthesizer
    from world_class_amd.synth import make_utterance
    fs, nd = 16000, 25
    x = make_utterance(fs, 0.5, 2024)
    p = w.Pipeline(fs)
    fl, yl = p.lengths([len(x)])
    nf, n_ap = fl[0], codec.number_of_aperiodicities(fs)
    W3 = fr.width(nd, n_ap, 3)
    z = lambda n: torch.full((n,), np.nan, dtype=torch.float64, device="cuda")
    d_x = torch.from_numpy(x).cuda()
    tpos, f0, csp, cap, y0, rows = z(nf), z(nf), z(nf * nd), z(nf * n_ap), z(yl[0]), z(nf * W3)
    torch.cuda.synchronize()
    p.run_coded_device(d_x, [len(x)], tpos, f0, csp, nd, cap, y0, rng_pos=[0])
    ft.pack([nf], nd, n_ap, 3, f0, csp, cap, rows)
    w.lib().wc_synchronize()
    cols, _ = fr.columns(nd, n_ap, 3)
    var = np.ones(W3)
    for ks in cols:
        var[ks[1]], var[ks[2]] = 0.1, 0.05
    syn = StreamSynthesizer(fs, p.fft_size, 5.0, 1, 200)
    h = mlpg_stream.MlpgStream(1, nd, n_ap, 3, 8, 128)
    assert 8 < nf <= 128 and (f0.cpu().numpy() > 0).any()
    yield dict(nd=nd, n_ap=n_ap, nf=nf, rows=rows, var=torch.from_numpy(var).cuda(), var_host=var, syn=syn, h=h, z=z)
    h.close()


def synthesise(env, s, statics_of_push, last):
    """Resets the synthesis stream to noise position 0 and feeds it push by push: statics_of_push(p) -> (device static rows, their
    count) for p = 0 .. last, the last one flushing.  Returns the samples and the count of every push"""
    w, ft, torch = env
    syn, nd, n_ap, z = s["syn"], s["nd"], s["n_ap"], s["z"]
    syn.reset(0)
    syn.set_rng_position(0, 0)
    ys, counts = [], []
    d_f0, d_sp, d_ap, d_y = z(200), z(200 * nd), z(200 * n_ap), z(syn.max_samples)
    torch.cuda.synchronize()
    for p in range(last + 1):
        d_static, k = statics_of_push(p)
        torch.cuda.synchronize()   # (rows that came up on torch's stream)
        ft.unpack(k, nd, n_ap, 1, d_static, d_f0, d_sp, d_ap)
        got = syn.push_coded_device([k], d_f0, d_sp, nd, d_ap, flush=[1 if p == last else 0], d_y=d_y)
        w.lib().wc_synchronize()
        ys.append(d_y.cpu().numpy()[:got[0]].copy())
        counts.append(got[0])
    return np.concatenate(ys), counts


def test_a_lag_beyond_the_utterance_is_the_whole_call(env, setup):
    """with L >= n everything comes from the flush, and the samples are, bit for bit, those of wc_mlpg_device -> unpack -> the same
    synthesis stream"""
    w, ft, torch = env
    s = setup
    nd, n_ap, nf, h, z = s["nd"], s["n_ap"], s["nf"], s["h"], s["z"]
    W3, S1 = fr.width(nd, n_ap, 3), nd + 2 + n_ap
    whole, streamed = z(nf * S1), z((nf + 1) * S1)
    torch.cuda.synchronize()
    ft.mlpg([nf], nd, n_ap, 3, s["rows"], s["var"], whole)
    h.reset(0, 128)
    for o in range(0, nf, 8):
        k = min(8, nf - o)
        assert h.push_device([k], s["rows"][o * W3:(o + k) * W3], s["var"], streamed) == [0]
    assert h.flush_device([1], streamed) == [nf]
    w.lib().wc_synchronize()
    a, b = whole.cpu().numpy(), streamed.cpu().numpy()
    assert np.isfinite(a).all() and np.array_equal(a, b[:nf * S1]) and np.isnan(b[nf * S1:]).all()
    y_whole, _ = synthesise(env, s, lambda p: (whole, nf), 0)
    y_stream, _ = synthesise(env, s, lambda p: (streamed, nf), 0)
    assert len(y_whole) > 0 and np.isfinite(y_whole).all() and np.abs(y_whole).max() > 1e-3
    assert np.array_equal(y_stream, y_whole)


def test_the_lagged_chain_runs_push_by_push(env, setup):
    """L = 8 in pushes of 4: every push hands frames_out frames on to the synthesis stream, the flush the last 8; the frame and sample
    totals match, and the samples equal those of the synthesis stream fed the rule's statics in the same cut"""
    w, ft, torch = env
    s = setup
    nd, n_ap, nf, h, z, syn = s["nd"], s["n_ap"], s["nf"], s["h"], s["z"], s["syn"]
    W3, S1, lag = fr.width(nd, n_ap, 3), nd + 2 + n_ap, 8
    cuts = [4] * (nf // 4) + ([nf % 4] if nf % 4 else [])
    rows_host = s["rows"].cpu().numpy().reshape(nf, W3)
    want, want_tail = ms.stream(nd, n_ap, 3, lag, rows_host, s["var_host"], False, cuts)
    want.append(want_tail)
    d_static = z(9 * S1)
    torch.cuda.synchronize()
    h.reset(0, lag)
    fed, statics = [0], []

    def device_push(p):
        if p < len(cuts):
            o, k = fed[0], cuts[p]
            n, = h.push_device([k], s["rows"][o * W3:(o + k) * W3], s["var"], d_static)
            fed[0] += k
            assert n == ms.emitted(o + k, lag) - ms.emitted(o, lag)
        else:
            n, = h.flush_device([1], d_static)
            assert n == lag
        w.lib().wc_synchronize()
        statics.append(d_static.cpu().numpy()[:n * S1].reshape(n, S1).copy())
        return d_static, n

    y_dev, counts_dev = synthesise(env, s, device_push, len(cuts))
    assert syn.frames_received(0) == nf == sum(len(a) for a in statics) and syn.samples_committed(0) == len(y_dev)
    for got, rule_rows in zip(statics, want):
        assert got.shape == rule_rows.shape and np.array_equal(got, rule_rows)
    y_rule, counts_rule = synthesise(env, s, lambda p: (torch.from_numpy(np.ascontiguousarray(want[p]).ravel().copy()).cuda(), len(want[p])), len(cuts))
    assert syn.frames_received(0) == nf and counts_rule == counts_dev
    assert len(y_dev) > 0 and np.isfinite(y_dev).all() and np.array_equal(y_dev, y_rule)
