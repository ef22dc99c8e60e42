"""-m gpu: morph streams (wc_morph_stream, include/world_class_stream.h).  One handle of five streams driven together -- streams
0-3 run the cases a-d of tests/morph_stream_rule.py, stream 4 never receives a frame -- with max_frames = 12 and max_backlog = 16,
the weights changing before every push.  The frames against one whole-utterance wc_morph_parameters_device pair per stream bit
for bit (also with ratios per push), against the numpy rule, coded pushes against decode + full-row pushes, a stream alone against
itself among the five, refusals that leave everything as it was, the frames through a synthesis stream against the batch call and
against the reference chain, and ordering on the caller's stream.  Outputs are NaN-filled with a guard row behind them that must
stay NaN."""
import math

import numpy as np
import pytest

import morph_rule as mr
import morph_stream_rule as ms
import retime_rule as rr
from test_gpu_morph import LOG_EXP_REL, _morph, _rel, reference_case
from test_gpu_retime import ATOMIC_ABS, SIZES, Y_ABS, _dev, _guarded, _rows, _same, env  # noqa: F401

pytestmark = pytest.mark.gpu
CASE = ["a", "b", "c", "d", None]  # the case of stream u; None: never receives a frame
MAXF, MAXB = 12, 16
_SRC, _RUNS = {}, {}


def _sources(fs, fft):
    """per stream with a case: (voice A, voice B), each (f0, sp, ap) of oracle/gen_golden.synth_params"""
    from oracle.gen_golden import synth_params
    if (fs, fft) not in _SRC:
        _SRC[fs, fft] = [tuple(synth_params(fs, fft, n, 9100 + fft + 2 * u + x) for x, n in enumerate(ms.CASES[c]["frames"])) for u, c in enumerate(CASE[:4])]
    return _SRC[fs, fft]


def _settings(u, k, fft, ratios, n_pushes=64):
    """weight, F0 weight, ratio of A, ratio of B of stream u at push k: the weights cycle morph_rule.WEIGHTS, the F0 weight three
    places on; the ratios retime_rule.cycled"""
    w, wf = mr.WEIGHTS[(k + u) % len(mr.WEIGHTS)], mr.WEIGHTS[(k + u + 3) % len(mr.WEIGHTS)]
    if not ratios:
        return w, wf, 0.0, 0.0
    return w, wf, float(rr.cycled(fft, n_pushes, u)[k]), float(rr.cycled(fft, n_pushes, u + 3)[k])


def _drive(env, fs, fft, ids, full=None, coded=None, nd=40, ratios=False, mode="full", handle=None, hook=None, check=True, on_frames=None):
    """Drives the streams ids (indices into CASE) together on one handle, push by push along the rule.  full[i] / coded[i]: the
    sources (A, B) of the i-th stream as full rows / coded rows; mode: "full", "coded" or "alternate" (coded pushes at even k).
    hook(k, handle): called before push k.  on_frames(k, counts, f0, sp, ap): the device outputs of push k.  Returns per stream a
    dict: f0, sp, ap of the formed frames and pos_a, pos_b, w, wf, ra, rb per frame."""
    w, codec, wio, torch = env
    from world_class_amd.stream import MorphStream
    bins, n = fft // 2 + 1, len(ids)
    h = handle or MorphStream(fs, fft, n, MAXF, MAXB)
    runs = [ms.run(CASE[u]) if CASE[u] else [] for u in ids]
    sims = [ms.Stream() for _ in ids]
    K = max(len(r) for r in runs)
    off = [[0, 0] for _ in ids]
    out = [dict(f0=[], sp=[], ap=[], pos_a=[], pos_b=[], w=[], wf=[], ra=[], rb=[]) for _ in ids]
    n_ap = codec.number_of_aperiodicities(fs)
    for k in range(K):
        if hook is not None:
            hook(k, h)
        use_coded = mode == "coded" or (mode == "alternate" and k % 2 == 0)
        src, widths = (coded, (1, nd, n_ap)) if use_coded else (full, (1, bins, bins))
        counts, parts, want = [[], []], [[[], [], []], [[], [], []]], []
        for i, u in enumerate(ids):
            rec = runs[i][k] if k < len(runs[i]) else dict(n=(0, 0), pos=[], speeds=(1.0, 1.0))
            wt, wf, ra, rb = _settings(u, k, fft, ratios)
            h.set_speeds(i, *rec["speeds"])
            h.set_weight(i, wt, wf)
            h.set_ratios(i, ra, rb)
            sims[i].speed = list(rec["speeds"])
            if check:
                assert h.frames_for_push(i, *rec["n"]) == len(rec["pos"]) == sims[i].count(*rec["n"], MAXF)
            sims[i].push(*rec["n"])
            for x in (0, 1):
                counts[x].append(rec["n"][x])
                for q in range(3):
                    if rec["n"][x]:
                        parts[x][q].append(np.asarray(src[i][x][q][off[i][x]:off[i][x] + rec["n"][x]]).reshape(rec["n"][x], widths[q]))
                off[i][x] += rec["n"][x]
            want.append(len(rec["pos"]))
            o = out[i]
            o["pos_a"] += [p[0] for p in rec["pos"]]
            o["pos_b"] += [p[1] for p in rec["pos"]]
            for key, v in (("w", wt), ("wf", wf), ("ra", ra), ("rb", rb)):
                o[key] += [v] * len(rec["pos"])
        ins = [[_dev(torch, np.concatenate(p)) if p else None for p in parts[x]] for x in (0, 1)]
        m = sum(want)
        outs = [_guarded(torch, m, 1), _guarded(torch, m, bins), _guarded(torch, m, bins)]
        torch.cuda.synchronize()
        if use_coded:
            got = h.push_coded_device(counts[0], *ins[0], counts[1], *ins[1], nd, *outs)
        else:
            got = h.push_device(counts[0], *ins[0], counts[1], *ins[1], *outs)
        assert got == want, (k, got, want)
        if on_frames is not None:
            on_frames(k, got, *outs)
        w.lib().wc_synchronize()
        rows = [_rows(t, m, wd) for t, wd in zip(outs, (1, bins, bins))]
        at = 0
        for i, c in enumerate(got):
            out[i]["f0"].append(rows[0][at:at + c, 0])
            out[i]["sp"].append(rows[1][at:at + c])
            out[i]["ap"].append(rows[2][at:at + c])
            at += c
            if check:
                _check_counters(h, i, sims[i])
    for o in out:
        for key in ("f0", "sp", "ap"):
            o[key] = np.concatenate(o[key])
        for key in ("pos_a", "pos_b", "w", "wf", "ra", "rb"):
            o[key] = np.array(o[key], dtype=np.float64)
    return out


def _check_counters(h, i, sim):
    assert h.frames_formed(i) == sim.frames
    for x in (0, 1):
        assert h.frames_received(i, x) == sim.F[x] and h.backlog(i, x) == sim.backlog(x)
        p = h.source_position(i, x)
        assert (math.isnan(p) and not sim.formed) or p == sim.position(x)


def _five(env, fs, fft, ratios):
    """the five streams driven together, once per (size, ratios) and module: the run the other tests compare with"""
    if (fs, fft, ratios) not in _RUNS:
        _RUNS[fs, fft, ratios] = _drive(env, fs, fft, range(5), _sources(fs, fft) + [None], ratios=ratios)
    return _RUNS[fs, fft, ratios]


def _whole(env, fs, fft, src, o, ratios):
    """one wc_morph_parameters_device pair over the whole sources at the stream's positions and per-frame values"""
    d = dict(a_lengths=[len(src[0][0])], b_lengths=[len(src[1][0])], out_lengths=[len(o["w"])], a=src[0], b=src[1], pos_a=o["pos_a"], pos_b=o["pos_b"],
             weight=o["w"], f0_weight=o["wf"])
    return _morph(env, fs, fft, d, o["ra"] if ratios else None, o["rb"] if ratios else None)


# ---- 1. the frames of every stream equal the whole-utterance call -------------------------------------------------------------

@pytest.mark.parametrize("ratios", [False, True])
@pytest.mark.parametrize("fs,fft", SIZES)
def test_frames_equal_the_whole_call_bit_for_bit(env, fs, fft, ratios):
    """per stream the concatenated frames are those of ONE pair over the whole sources; the counters follow the rule at every push
    (checked inside the drive), the idle stream reports zeros and NaN throughout"""
    runs = _five(env, fs, fft, ratios)
    for u, c in enumerate(CASE[:4]):
        o = runs[u]
        assert len(o["w"]) == sum(len(p["pos"]) for p in ms.run(c)) > 0
        want = _whole(env, fs, fft, _sources(fs, fft)[u], o, ratios)
        for g, w_, key in zip((o["f0"], o["sp"], o["ap"]), want, ("f0", "sp", "ap")):
            assert np.isfinite(g).all() and _same(g, w_), (c, key)
    assert len(runs[4]["f0"]) == 0
    if ratios:  # (the ratios do change rows, and leave the contour and the ap rows alone)
        plain = _five(env, fs, fft, False)
        assert _same(runs[1]["f0"], plain[1]["f0"]) and _same(runs[1]["ap"], plain[1]["ap"]) and not _same(runs[1]["sp"], plain[1]["sp"])


# ---- 2. against the numpy rule ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fs,fft", SIZES)
def test_frames_agree_with_the_numpy_rule(env, fs, fft):
    runs = _five(env, fs, fft, False)
    for u, c in enumerate(CASE[:4]):
        o, (a, b) = runs[u], _sources(fs, fft)[u]
        f0, sp, ap = mr.morph(a, b, o["pos_a"], o["pos_b"], o["w"], o["wf"])
        assert _same(o["ap"], ap)
        ends = (o["w"] == 0) | (o["w"] == 1)
        assert _same(o["sp"][ends], sp[ends])
        e_sp = _rel(o["sp"][~ends], sp[~ends])
        voiced = f0 != 0
        assert _same(o["f0"] == 0, f0 == 0)
        e_f0 = _rel(o["f0"][voiced], f0[voiced])
        print("morph stream against the numpy rule, fs %d fft %d case %s: sp %.3e, F0 %.3e (relative)" % (fs, fft, c, e_sp, e_f0))
        assert e_sp < LOG_EXP_REL and e_f0 < LOG_EXP_REL


# ---- 3. coded pushes ----------------------------------------------------------------------------------------------------------

def _coded_sources(env, fs, fft, nd):
    """the sources coded on the device, and their rows as wc_decode_features_device decodes them"""
    w, codec, wio, torch = env
    n_ap = codec.number_of_aperiodicities(fs)
    bins = fft // 2 + 1
    coded, full = [], []
    for pair in _sources(fs, fft):
        cs, fs_ = [], []
        for f0, sp, ap in pair:
            n = len(f0)
            d_csp, d_cap = torch.empty(n * nd, dtype=torch.float64, device="cuda"), torch.empty(n * n_ap, dtype=torch.float64, device="cuda")
            d_sp, d_ap = torch.empty(n * bins, dtype=torch.float64, device="cuda"), torch.empty(n * bins, dtype=torch.float64, device="cuda")
            codec.code_spectral_envelope_device(fs, fft, n, nd, _dev(torch, sp), d_csp)
            codec.code_aperiodicity_device(fs, fft, n, _dev(torch, ap), d_cap)
            codec.decode_features_device(fs, fft, n, nd, d_csp, d_cap, d_sp, d_ap)
            w.lib().wc_synchronize()
            cs.append((f0, d_csp.cpu().numpy().reshape(n, nd), d_cap.cpu().numpy().reshape(n, n_ap)))
            fs_.append((f0, d_sp.cpu().numpy().reshape(n, bins), d_ap.cpu().numpy().reshape(n, bins)))
        coded.append(tuple(cs))
        full.append(tuple(fs_))
    return coded, full


@pytest.mark.parametrize("fs,fft", SIZES)
def test_coded_pushes_equal_decode_then_full_row_pushes(env, fs, fft):
    nd = 40
    coded, full = _coded_sources(env, fs, fft, nd)
    coded.append(None)
    full.append(None)
    base = _drive(env, fs, fft, range(5), full, ratios=True)
    for mode in ("coded", "alternate"):
        got = _drive(env, fs, fft, range(5), full, coded, nd, ratios=True, mode=mode, check=False)
        for u in range(4):
            for key in ("f0", "sp", "ap"):
                assert _same(got[u][key], base[u][key]), (mode, u, key)
    assert np.isfinite(base[1]["sp"]).all() and len(base[1]["f0"]) == 107


# ---- 4. isolation -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fs,fft", SIZES)
def test_a_stream_alone_gives_the_bits_it_gives_among_the_five(env, fs, fft):
    alone = _drive(env, fs, fft, [1], [_sources(fs, fft)[1]], ratios=True)[0]
    among = _five(env, fs, fft, True)[1]
    for key in ("f0", "sp", "ap"):
        assert _same(alone[key], among[key]), key


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------

def _refused(w, fn, *args):
    with pytest.raises(w.WorldClassError) as e:
        fn(*args)
    assert "error -1:" in str(e.value), str(e.value)


@pytest.mark.parametrize("fs,fft", [SIZES[1], SIZES[3]])
def test_refusals_leave_everything_as_it_was(env, fs, fft):
    w, codec, wio, torch = env
    from world_class_amd.stream import MorphStream
    bins = fft // 2 + 1
    src = _sources(fs, fft)
    nan, inf = float("nan"), float("inf")

    def state(h):
        return [(h.frames_formed(u),) + tuple((h.frames_received(u, x), h.backlog(u, x), repr(h.source_position(u, x))) for x in (0, 1)) for u in range(5)]

    def hook(k, h):
        if k not in (0, 7, 20):
            return
        before = state(h)
        rows = 13
        d_in = [_dev(torch, v[:rows]) for v in src[1][0]]
        outs = [_guarded(torch, 5 * MAXF, 1), _guarded(torch, 5 * MAXF, bins), _guarded(torch, 5 * MAXF, bins)]
        torch.cuda.synchronize()
        zero = [0] * 5
        at = lambda u, v: [v if i == u else 0 for i in range(5)]
        push = lambda na, nb, a=d_in, b=d_in, o=outs: h.push_device(na, *a, nb, *b, *o)
        _refused(w, push, at(0, 13), zero)                    # over max_frames
        _refused(w, push, zero, at(2, 13))
        _refused(w, push, at(1, -1), zero)                    # a negative count
        _refused(w, push, at(0, 2), at(0, 2), [None] * 3)     # NULL arrays with frames to read
        _refused(w, push, at(0, 2), at(0, 2), d_in, [None] * 3)
        _refused(w, push, at(3, 12), at(3, 12), d_in, d_in, [None] * 3)  # ... and to write (both voices in: frames form)
        # a push that would form more than max_frames: the idle stream at a hundredth of the speed (refused, so it stays idle)
        h.set_speeds(4, 0.01, 0.01)
        assert h.frames_for_push(4, 2, 2) == MAXF + 1
        _refused(w, push, at(4, 2), at(4, 2))
        h.set_speeds(4, 1e-300, 1e-300)
        assert h.frames_for_push(4, 2, 2) == MAXF + 1
        _refused(w, push, at(4, 2), at(4, 2))
        h.set_speeds(4, 1.0, 1.0)
        for bad in ((0.0, 1.0), (1.0, 0.0), (-1.0, 1.0), (1.0, nan), (inf, 1.0), (1.0, -inf)):
            _refused(w, h.set_speeds, 1, *bad)
        for bad in ((nan, 0.5), (0.5, nan), (inf, 0.5), (0.5, -inf)):
            _refused(w, h.set_weight, 1, *bad)
        _refused(w, h.set_weight, 1, nan)
        for bad in ((-1.0, 0.0), (0.0, -1.0), (nan, 1.0), (1.0, inf), (1.0 / fft, 1.0), (1.0, 1.9 / fft)):
            _refused(w, h.set_ratios, 1, *bad)
        for u in (-1, 5):
            _refused(w, h.set_speeds, u, 1.0, 1.0)
            _refused(w, h.set_weight, u, 0.5)
            _refused(w, h.set_ratios, u, 1.0, 1.0)
            _refused(w, h.reset, u)
            _refused(w, h.frames_for_push, u, 1, 1)
            assert math.isnan(h.source_position(u, 0)) and h.frames_received(u, 0) == -1 and h.backlog(u, 1) == -1 and h.frames_formed(u) == -1
        _refused(w, h.frames_for_push, 0, -1, 0)
        assert math.isnan(h.source_position(0, 2)) and h.frames_received(0, -1) == -1 and h.backlog(0, 2) == -1
        w.lib().wc_synchronize()
        assert all(bool(torch.isnan(o).all()) for o in outs)
        assert state(h) == before

    h = MorphStream(fs, fft, 5, MAXF, MAXB)
    got = _drive(env, fs, fft, range(5), src + [None], ratios=True, handle=h, hook=hook)
    want = _five(env, fs, fft, True)
    for u in range(4):
        for key in ("f0", "sp", "ap"):
            assert _same(got[u][key], want[u][key]), (u, key)
    # (a refused setter kept the settings of the drive: nothing above changed stream 1's frames)
    # reset: the stream's first-push behaviour and its default settings -- speeds 1, weight 0: voice A's rows as they are
    assert h.frames_formed(0) == 65
    h.reset(0)
    assert (h.frames_formed(0), h.frames_received(0, 0), h.frames_received(0, 1), h.backlog(0, 0), h.backlog(0, 1)) == (0, 0, 0, 0, 0)
    assert math.isnan(h.source_position(0, 0)) and h.frames_for_push(0, 3, 2) == 2
    a, b = src[0]
    res = h.push([tuple(v[:3] for v in a)] + [tuple(v[:0] for v in a)] * 4, [tuple(v[:2] for v in b)] + [tuple(v[:0] for v in b)] * 4)
    assert [len(r[0]) for r in res] == [2, 0, 0, 0, 0]
    assert _same(res[0][0], a[0][:2]) and _same(res[0][1], a[1][:2]) and _same(res[0][2], a[2][:2])
    assert (h.source_position(0, 0), h.source_position(0, 1), h.backlog(0, 0), h.backlog(0, 1), h.frames_formed(1)) == (1.0, 1.0, 2, 1, 107)


@pytest.mark.parametrize("fs,fft", [SIZES[0], SIZES[2]])
def test_case_c_on_a_backlog_of_six_is_refused_where_the_rule_says(env, fs, fft):
    """max_backlog = 6: the rule (tests/test_morph_stream_rule.py) admits case c's first two pushes -- six rows of A wait, which is
    not above the bound -- and is over it at the third, which would leave seven.  That push is refused, the stream goes on as if
    it had not been made.  The settings are the defaults (weight 0): the frames are voice A's rows."""
    w, codec, wio, torch = env
    from world_class_amd.stream import MorphStream
    assert [p is None for p in ms.run("c", max_backlog=6)] == [False, False, True]
    a, b = _sources(fs, fft)[2]
    cut = lambda v, i, j: tuple(x[i:j] for x in v)
    h = MorphStream(fs, fft, 1, MAXF, 6)
    assert [len(r[0]) for r in h.push([cut(a, 0, 6)], [cut(b, 0, 0)])] == [0] and h.backlog(0, 0) == 6
    res = h.push([cut(a, 6, 6)], [cut(b, 0, 6)])
    assert _same(res[0][1], a[1][:6]) and _same(res[0][2], a[2][:6]) and _same(res[0][0], a[0][:6])
    assert h.frames_for_push(0, 6, 0) == 0  # (no frame forms: the refusal below is the backlog's)
    _refused(w, h.push, [cut(a, 6, 12)], [cut(b, 6, 6)])
    assert (h.frames_formed(0), h.frames_received(0, 0), h.frames_received(0, 1), h.backlog(0, 0), h.backlog(0, 1)) == (6, 6, 6, 1, 1)
    res = h.push([cut(a, 6, 11)], [cut(b, 6, 8)])  # five rows of A fit: six wait
    assert _same(res[0][1], a[1][6:8]) and _same(res[0][0], a[0][6:8]) and (h.backlog(0, 0), h.backlog(0, 1)) == (4, 1)
    h.set_weight(0, 1.0)
    res = h.push([cut(a, 11, 11)], [cut(b, 8, 10)])  # weight 1: voice B's rows, A's kept rows untouched
    assert _same(res[0][1], b[1][8:10]) and _same(res[0][2], b[2][8:10]) and _same(res[0][0], b[0][8:10])


# ---- 6. through Synthesis -----------------------------------------------------------------------------------------------------

def _through_synthesis(env, fs, fft, coded_pair, full_pair, nd, ratios):
    """case a on a one-stream handle, coded pushes; every push's frames go into a synthesis stream as they are on the device, a
    flush behind the last push.  Returns the samples, the final noise position and the drive's per-frame arrays."""
    w, codec, wio, torch = env
    from world_class_amd.stream import StreamSynthesizer
    syn = StreamSynthesizer(fs, fft, 5.0, 1, MAXF)
    y = []

    def on_frames(k, counts, d_f0, d_sp, d_ap):
        c = syn.push_device(counts, d_f0, d_sp, d_ap)
        w.lib().wc_synchronize()
        y.append(syn._d_y.to_host()[:c[0]].copy())

    o = _drive(env, fs, fft, [0], [full_pair], [coded_pair], nd, ratios=ratios, mode="coded", on_frames=on_frames)[0]
    d_none = torch.zeros(8, dtype=torch.float64, device="cuda")
    c = syn.push_device([0], d_none, d_none, d_none, flush=[1])
    y.append(syn._d_y.to_host()[:c[0]].copy())
    return np.concatenate(y), syn.rng_position(0), o


@pytest.mark.parametrize("fs,fft", [(24000, 1024), (48000, 2048), (16000, 512), (96000, 4096)])
def test_frames_through_a_synthesis_stream_equal_the_batch_call(env, fs, fft):
    """stream a's frames, push by push into a StreamSynthesizer, against ONE compute_coded_morphed_device call over the whole
    coded sources at the rule's positions: bit for bit at fft 1024 / 2048, within ATOMIC_ABS at 512 / 4096 (FP64 atomics)"""
    w, codec, wio, torch = env
    nd = 40
    coded, full = _coded_sources(env, fs, fft, nd)
    y, end, o = _through_synthesis(env, fs, fft, coded[0], full[0], nd, True)
    (fa, cspa, capa), (fb, cspb, capb) = coded[0]
    m = len(o["w"])
    assert m == 65
    syn = w.Synthesis(fs, fft, 5.0)
    ol = syn.out_length(m)
    d_y = torch.full((ol + 1,), np.nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    want_end = syn.compute_coded_morphed_device(_dev(torch, fa), [len(fa)], _dev(torch, cspa), _dev(torch, capa), _dev(torch, fb), [len(fb)], _dev(torch, cspb),
                                                _dev(torch, capb), nd, [m], _dev(torch, o["pos_a"]), _dev(torch, o["pos_b"]), _dev(torch, o["w"]),
                                                _dev(torch, o["wf"]), _dev(torch, o["ra"]), _dev(torch, o["rb"]), [ol], d_y, rng_pos=[0])
    w.lib().wc_synchronize()
    want = d_y.cpu().numpy()
    assert np.isnan(want[-1]) and np.isfinite(want[:-1]).all() and np.abs(want[:-1]).max() > 1e-3
    assert len(y) == ol and [end] == want_end
    err = np.abs(y - want[:-1]).max()
    print("morph stream through a synthesis stream against the batch call, fs %d fft %d: %.3e" % (fs, fft, err))
    assert np.array_equal(y, want[:-1]) if fft in (1024, 2048) else err < ATOMIC_ABS


# ---- 7. against the reference chain -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fs,fft", [(16000, 1024), (48000, 2048)])
def test_lockstep_stream_matches_the_reference_chain(env, port, checker, fs, fft):
    """the sources of test_gpu_morph.reference_case, speeds (1, 1), lockstep pushes of 8 frames, the weights per push: the reference
    codec's decode, the numpy rule with those per-frame weights and the reference's Synthesis from noise position 0 (the real one
    where oracle/_ref is built, oracle/port.py otherwise) against coded pushes -> synthesis stream, within Y_ABS, with equal length
    and final noise position"""
    w, codec, wio, torch = env
    from oracle import port_codec as pc
    from world_class_amd.stream import MorphStream, StreamSynthesizer
    nd, step = 60, 8
    a, b = reference_case(fs, fft, nd)[:2]
    n, bins = len(a[0]), fft // 2 + 1
    rows = [(v[0], pc.decode_spectral_envelope(v[1], fs, fft), pc.decode_aperiodicity(v[2], fs, fft)) for v in (a, b)]
    wt = np.repeat([mr.WEIGHTS[k % 8] for k in range(n // step)], step)
    wf = np.repeat([mr.WEIGHTS[(k + 3) % 8] for k in range(n // step)], step)
    pos = np.arange(n, dtype=np.float64)
    f0_m, sp_m, ap_m = mr.morph(rows[0], rows[1], pos, pos, wt, wf)
    assert n == 120 and np.isfinite(f0_m).all() and (f0_m == 0).any()
    port.rng_seek(0)
    y_ref = port.synthesis(f0_m, sp_m, ap_m, fs, 5.0)
    end = port.rng_position()
    if checker is not None:
        y_ref = checker.stage_at(0, "synthesis", f0_m, sp_m, ap_m, fs, 5.0)
    assert np.isfinite(y_ref).all()
    h, syn = MorphStream(fs, fft, 1, step, MAXB), StreamSynthesizer(fs, fft, 5.0, 1, step)
    outs = [torch.empty(step, dtype=torch.float64, device="cuda"), torch.empty(step * bins, dtype=torch.float64, device="cuda"),
            torch.empty(step * bins, dtype=torch.float64, device="cuda")]
    d = [[_dev(torch, q) for q in v] for v in (a, b)]
    widths = (1, nd, codec.number_of_aperiodicities(fs))
    y = []
    for k in range(n // step):
        h.set_weight(0, wt[k * step], wf[k * step])
        ins = [[t[k * step * wd:(k + 1) * step * wd] for t, wd in zip(v, widths)] for v in d]
        c = h.push_coded_device([step], *ins[0], [step], *ins[1], nd, *outs)
        assert c == [step]
        s = syn.push_device(c, *outs, flush=[1 if k == n // step - 1 else 0])
        y.append(syn._d_y.to_host()[:s[0]].copy())
    y = np.concatenate(y)
    assert len(y) == len(y_ref) and syn.rng_position(0) == end
    err = np.abs(y - y_ref).max()
    print("morph stream -> synthesis stream against the reference chain, fs %d: %.3e (peak %.2f)" % (fs, err, np.abs(y_ref).max()))
    assert err < Y_ABS
    assert checker is None or not checker.fell_back


# ---- 8. ordering on the caller's stream ---------------------------------------------------------------------------------------

def test_pushes_are_ordered_on_the_callers_stream(env):
    """a long torch kernel in front on a torch stream handed over by wc_set_stream, the rows written by torch kernels on that
    stream, no synchronisation before the pushes: the first two pushes return while the kernel in front still runs (the staging is a
    pair), and every push reads its inputs behind it; one synchronisation at the end"""
    w, codec, wio, torch = env
    from world_class_amd.stream import MorphStream
    fs, fft = 24000, 1024
    bins = fft // 2 + 1
    a, b = _sources(fs, fft)[3]
    want = _five(env, fs, fft, False)[3]
    runs = ms.run("d")
    h = MorphStream(fs, fft, 1, MAXF, MAXB)
    warm = MorphStream(fs, fft, 1, MAXF, MAXB)
    warm.push([tuple(v[:2] for v in a)], [tuple(v[:2] for v in b)])  # (the kernel's code is on the device before the clock matters)
    host = [[torch.from_numpy(np.ascontiguousarray(v).ravel().copy()).pin_memory() for v in src] for src in (a, b)]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert w.lib().wc_set_stream(s.cuda_stream) == 0
    try:
        outs, running = [], []
        with torch.cuda.stream(s):
            junk = torch.randn(4096, 4096, device="cuda")
            for _ in range(40):  # a long-running kernel in front: the pushes must wait for it and for the uploads behind it
                junk = junk @ junk * 1e-3
            done = torch.cuda.Event()
            done.record(s)
            dev = [[torch.zeros(len(t), dtype=torch.float64, device="cuda") for t in src] for src in host]
            for dsts, srcs in zip(dev, host):
                for dst, src in zip(dsts, srcs):
                    dst.copy_(src, non_blocking=True)
                    dst.mul_(1.0)  # torch kernels on the stream write every input
            off = [0, 0]
            for k, rec in enumerate(runs):
                wt, wf, _, _ = _settings(3, k, fft, False)
                h.set_weight(0, wt, wf)
                ins = [[t[off[x] * wd:(off[x] + rec["n"][x]) * wd] if rec["n"][x] else None for t, wd in zip(dev[x], (1, bins, bins))] for x in (0, 1)]
                m = len(rec["pos"])
                o = [_guarded(torch, m, 1), _guarded(torch, m, bins), _guarded(torch, m, bins)]
                assert h.push_device([rec["n"][0]], *ins[0], [rec["n"][1]], *ins[1], *o) == [m]
                running.append(not done.query())
                off = [off[0] + rec["n"][0], off[1] + rec["n"][1]]
                outs.append((o, m))
        s.synchronize()  # once
    finally:
        assert w.lib().wc_set_stream(None) == 0
    assert running[0] and running[1], running
    got = [np.concatenate([_rows(o[q], m, wd) for o, m in outs]) for q, wd in enumerate((1, bins, bins))]
    assert _same(got[0][:, 0], want["f0"]) and _same(got[1], want["sp"]) and _same(got[2], want["ap"])
