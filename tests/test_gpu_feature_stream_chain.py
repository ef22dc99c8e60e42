"""-m gpu: the live loop on one set of frames, 0.5 s at 16 kHz: wc_stream_push_coded_device -> feature stream -> identity model ->
MLPG stream -> wc_unpack_model_features_device -> wc_synth_stream_push_coded_device.  Every count that passes from one step to the
next is the frames_out of the step before; between the first push and the last sample nothing is synchronised and nothing comes
back to the host.  Against the batch chain on the same committed frames: pack -> wc_mlpg_device -> unpack -> coded synthesis."""
import numpy as np
import pytest

import features_rule as fr
from test_gpu_features import env  # noqa: F401

pytestmark = pytest.mark.gpu

LAG = 16        # of the feature stream: above the signal's longest unvoiced run, which the test asserts on the committed F0
MLPG_LAG = 128  # at least the frames of the utterance: the MLPG stream's flush is then wc_mlpg_device itself, bit for bit
                # (tests/test_gpu_mlpg_stream_chain.py holds stream against batch on this path at this lag and with no tolerance)


def longest_run(voiced):
    """the longest unvoiced run that consequence 7 counts: the leading run counts, the trailing run does not"""
    idx = [i for i, v in enumerate(voiced) if v]
    if not idx:
        return 0
    return max([idx[0]] + [b - a - 1 for a, b in zip(idx, idx[1:])])


def test_longest_run_counts_the_leading_run_and_not_the_trailing_one():
    b = lambda s: [c == "1" for c in s]
    assert longest_run(b("0001101000")) == 3 and longest_run(b("1100100000")) == 2 and longest_run(b("0000")) == 0
    assert longest_run(b("1111")) == 0 and longest_run(b("")) == 0 and longest_run(b("10001")) == 3


def test_the_live_loop_equals_the_batch_chain(env):
    w, ft, torch = env
    from world_class_amd import codec, feature_stream, mlpg_stream
    from world_class_amd.stream import StreamAnalyzer, StreamSynthesizer
    from world_class_amd.synth import make_utterance
    fs, nd = 16000, 25
    x = make_utterance(fs, 0.5, 2024)
    n_ap = codec.number_of_aperiodicities(fs)
    W3, S1 = fr.width(nd, n_ap, 3), nd + 2 + n_ap
    an = StreamAnalyzer(fs, 1, frame_period=5.0, chunk_ms=160, lookback_ms=400, lookahead_ms=400, aperiodicity=True)
    most = 200   # frames of the utterance at most: the analysis pushes commit about 100
    feat = feature_stream.FeatureStream(1, nd, n_ap, 3, an.max_frames, LAG)
    ml = mlpg_stream.MlpgStream(1, nd, n_ap, 3, max(an.max_frames, LAG), MLPG_LAG)
    syn = StreamSynthesizer(fs, an.fft_size, 5.0, 1, most)
    z = lambda n: torch.full((n,), np.nan, dtype=torch.float64, device="cuda")
    tpos, f0, csp, cap, rows = z(most), z(most), z(most * nd), z(most * n_ap), z(most * W3)
    statics, g_f0, g_sp, g_ap, y = z(most * S1), z(most), z(most * nd), z(most * n_ap), z(syn.max_samples)
    cols, _ = fr.columns(nd, n_ap, 3)
    var_host = np.ones(W3)
    for ks in cols:
        var_host[ks[1]], var_host[ks[2]] = 0.1, 0.05
    var = torch.from_numpy(var_host).cuda()   # the identity model: the packed rows as means, one row of variances
    step = an.chunk_samples
    chunks = [torch.from_numpy(x[o:o + step].copy()).cuda() for o in range(0, len(x), step)]
    torch.cuda.synchronize()

    # ---- the live loop: enqueue only; a count goes from a frames_out into the next call as it is ----
    feat.reset(0, LAG, 0.0)
    ml.reset(0, MLPG_LAG)
    syn.reset(0)
    syn.set_rng_position(0, 0)
    frames = packed = 0
    counts = []
    for p, chunk in enumerate(chunks):
        last = p == len(chunks) - 1
        got = an.push_coded_device(chunk, csp[frames * nd:], nd, cap[frames * n_ap:], n_new=[len(chunk)], flush=[1 if last else 0],
                                   d_tpos=tpos[frames:], d_f0=f0[frames:])
        out = feat.push_device(got, f0[frames:], csp[frames * nd:], cap[frames * n_ap:], rows[packed * W3:])
        assert out == [feature_stream.emitted(frames + got[0], LAG) - feature_stream.emitted(frames, LAG)]
        assert ml.push_device(out, rows[packed * W3:], var, statics) == [0]
        counts.append((got[0], out[0]))
        frames += got[0]
        packed += out[0]
    out = feat.flush_device([1], rows[packed * W3:])
    assert ml.push_device(out, rows[packed * W3:], var, statics) == [0]
    packed += out[0]
    n_static, = ml.flush_device([1], statics)
    ft.unpack(n_static, nd, n_ap, 1, statics, g_f0, g_sp, g_ap)
    n_y, = syn.push_coded_device([n_static], g_f0, g_sp, nd, g_ap, flush=[1], d_y=y)
    w.lib().wc_synchronize()   # the first synchronisation since the first push: the results are read now

    nf = frames
    assert 8 < nf <= MLPG_LAG and packed == nf == n_static and n_y > 0
    assert sum(1 for c in counts if c[0]) >= 2 and sum(1 for c in counts if c[1]) >= 1   # rows arrive and rows leave push by push
    f0_host = f0.cpu().numpy()[:nf]
    voiced = fr.voiced(f0_host)
    run = longest_run(list(voiced))
    print("feature stream chain: %d frames, %d voiced, longest counted unvoiced run %d, lag %d, per push (committed, packed) %s"
          % (nf, int(voiced.sum()), run, LAG, counts))
    assert voiced.any() and (~voiced[np.flatnonzero(voiced)[0]:np.flatnonzero(voiced)[-1]]).any()   # there is a gap to interpolate
    assert run < LAG   # the precondition of consequence 7: the test cannot pass by leaving frames out

    # ---- the batch chain on the same committed frames ----
    rows_batch, statics_batch, y_batch = z(nf * W3), z(nf * S1), z(syn.max_samples)
    torch.cuda.synchronize()
    ft.pack([nf], nd, n_ap, 3, f0, csp, cap, rows_batch, 0.0)
    ft.mlpg([nf], nd, n_ap, 3, rows_batch, var, statics_batch)
    ft.unpack(nf, nd, n_ap, 1, statics_batch, g_f0, g_sp, g_ap)
    syn.reset(0)
    syn.set_rng_position(0, 0)
    m_y, = syn.push_coded_device([nf], g_f0, g_sp, nd, g_ap, flush=[1], d_y=y_batch)
    w.lib().wc_synchronize()
    a, b = rows.cpu().numpy(), rows_batch.cpu().numpy()
    assert np.isfinite(b).all() and np.array_equal(a[:nf * W3], b) and np.isnan(a[nf * W3:]).all()   # consequence 7, bit for bit
    sa, sb = statics.cpu().numpy(), statics_batch.cpu().numpy()
    assert np.array_equal(sa[:nf * S1], sb) and np.isnan(sa[nf * S1:]).all()
    ya, yb = y.cpu().numpy()[:n_y], y_batch.cpu().numpy()[:m_y]
    assert n_y == m_y and np.isfinite(yb).all() and np.abs(yb).max() > 1e-3
    diff = np.abs(ya - yb).max()
    print("feature stream chain: %d samples, max |live - batch| = %.3e" % (n_y, diff))
    assert np.array_equal(ya, yb)
    for hdl in (feat, ml):
        hdl.close()
