"""-m gpu: coded pushes of a filter stream (include/world_class_filter_stream.h) against wc_frame_filter_run_coded_device, bit for bit
-- `to` another voice's coded rows, `from` the source's, with skip_energy on and off -- and the live loop: an analysis stream's coded
push commits rows, they go with a fixed offset as `to` and unchanged as `from` to a filter stream together with the samples pushed so
far, the flush comes at the end, and the result is the batch coded call's on the concatenated rows, bit for bit."""
import numpy as np
import pytest

import filter_stream_rule as fsr

pytestmark = pytest.mark.gpu

FS, N, ND, FP = 16000, 1024, 60, 5.0


@pytest.fixture(scope="module")
def voices():
    """make_utterance seeds 1 and 2, 0.6 s at 16 kHz, through the coded pipeline step with 60 dimensions"""
    import torch
    import world_class_amd as w
    from world_class_amd import codec, filter as ff, filter_stream as fs_
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
    csp = csp.cpu().numpy().reshape(T, ND)
    yield dict(w=w, fs_=fs_, xs=xs, fl=fl, h=h, a=csp[:fl[0]], b=csp[fl[0]:])
    h.close()


@pytest.mark.parametrize("how", ("hop_and_row", "random", "all_at_once"))
@pytest.mark.parametrize("skip_energy", (False, True))
@pytest.mark.parametrize("with_from", (True, False))
def test_coded_pushes_are_the_coded_call_bit_for_bit(voices, with_from, skip_energy, how):
    s = voices
    x, to = s["xs"][0], s["b"][:s["fl"][0]]
    to = np.concatenate([to, np.repeat(to[-1:], max(s["fl"][0] - len(to), 0), axis=0)])
    frm = s["a"] if with_from else None
    want = s["h"].filter_coded(x, to, frm, skip_energy)
    assert np.isfinite(want).all() and np.abs(want - x).max() > 1e-3
    st = s["fs_"].FilterStream(FS, N, FP, "power", 2, len(x), len(to))
    got, i, j = [], 0, 0
    for ns, nr, flush in fsr.cut(how, len(x), len(to), FP, FS, seed=7):
        out = st.push_coded_host([None, x[i:i + ns]], [None, to[j:j + nr]], None if frm is None else [None, frm[j:j + nr]], skip_energy, [0, flush])
        assert len(out[0]) == 0
        got.append(out[1])
        i, j = i + ns, j + nr
    st.close()
    got = np.concatenate(got)
    assert got.shape == want.shape and np.array_equal(got, want)


def test_the_live_loop(voices):
    """analysis stream (coded push) -> rows + offset -> filter stream (coded push), chunk by chunk"""
    from world_class_amd import stream
    s = voices
    x = s["xs"][0]
    an = stream.StreamAnalyzer(FS, 1, frame_period=FP, chunk_ms=120, lookback_ms=200, lookahead_ms=200)
    assert an.fft_size == N
    offset = 0.3 / (1.0 + np.arange(ND))
    st = s["fs_"].FilterStream(FS, N, FP, "power", 1, len(x) + an.chunk_samples, an.max_frames + 2)
    got, rows = [], []
    for i in range(0, len(x), an.chunk_samples):
        chunk = x[i:i + an.chunk_samples]
        last = i + an.chunk_samples >= len(x)
        csp = an.push_coded([chunk], ND, flush=[1] if last else None)[0]["csp"]
        rows.append(csp)
        got.append(st.push_coded_host([chunk], [csp + offset], [csp], True, [1 if last else 0])[0])
        if not last:      # committed as far as the rows allow: a_T of the counts
            assert st.samples_committed(0) == fsr.committed(fsr.segments_done(i + len(chunk), st.rows_received(0), FP, FS), FP, FS)
    an.close()
    st.close()
    rows = np.concatenate(rows)
    assert len(rows) >= 2
    want = s["h"].filter_coded(x, rows + offset, rows, True)
    got = np.concatenate(got)
    assert got.shape == want.shape and np.array_equal(got, want) and np.abs(want - x).max() > 1e-3
