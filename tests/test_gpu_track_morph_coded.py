"""-m gpu: coded track-morph streams (wc_track_morph_coded, include/world_class_track_morph_coded.h), in the layout of
tests/test_gpu_track_morph.py and on its tables: one handle of five streams and two tracks (slot 0: m = 1, slot 1: m = 40) with
max_frames = 6 and max_delay = 5, streams 0-3 at delays 0, 1, 3 and 5 with about 60 rows each, the counts per push cycling through
0, 1 and 6, the weights changing before every push, stream 4 never attached; outputs NaN-filled with a guard row behind them.

The coded rows are codec.code_features_device of oracle.gen_golden.synth_params rows.  The reference is the existing full-row
TrackMorph, driven by the same driver with the same counts, positions, delays, weights and ratios, whose tracks and live rows are
codec.decode_features_device of those coded rows.  Nothing here has a tolerance: every comparison is np.array_equal on bits.
"""
import ctypes as C

import numpy as np
import pytest

import track_morph_rule as tm
from test_gpu_morph import _morph
from test_gpu_retime import _dev, _guarded, _rows, _same, env  # noqa: F401
from test_gpu_track_morph import (DELAY, FIRST, M, MAXD, MAXF, ROWS, _cuts, _drive, _lane, _refused, _settings, _tracks, _used, _voice)

pytestmark = pytest.mark.gpu
SIZES = [(16000, 512, 25, False), (24000, 1024, 40, True), (48000, 2048, 60, True)]  # fs, fft, nd, ratios
_CODED, _RUNS = {}, {}


def _code(env, fs, fft, nd, rows):
    """(f0, sp, ap) full rows -> ((f0, coded sp, coded ap), (f0, decoded sp, decoded ap)): coded and decoded on the device, once"""
    w, codec, wio, torch = env
    n, bins, n_ap = len(rows[0]), fft // 2 + 1, codec.number_of_aperiodicities(fs)
    new = lambda k: torch.full((k,), np.nan, dtype=torch.float64, device="cuda")
    d_sp, d_ap, d_csp, d_cap, d_sp2, d_ap2 = _dev(torch, rows[1]), _dev(torch, rows[2]), new(n * nd), new(n * n_ap), new(n * bins), new(n * bins)
    torch.cuda.synchronize()
    codec.code_features_device(fs, fft, n, nd, d_sp, d_ap, d_csp, d_cap)
    codec.decode_features_device(fs, fft, n, nd, d_csp, d_cap, d_sp2, d_ap2)
    w.lib().wc_synchronize()
    f0 = np.ascontiguousarray(rows[0], dtype=np.float64)
    coded = (f0, d_csp.cpu().numpy().reshape(n, nd), d_cap.cpu().numpy().reshape(n, n_ap))
    decoded = (f0, d_sp2.cpu().numpy().reshape(n, bins), d_ap2.cpu().numpy().reshape(n, bins))
    assert np.isfinite(coded[1]).all() and np.isfinite(coded[2]).all() and np.isfinite(decoded[1]).all() and np.isfinite(decoded[2]).all()
    return coded, decoded


def _cvoice(env, fs, fft, nd, u):
    if ("v", fs, fft, nd, u) not in _CODED:
        _CODED["v", fs, fft, nd, u] = _code(env, fs, fft, nd, _voice(fs, fft, u))
    return _CODED["v", fs, fft, nd, u]


def _ctracks(env, fs, fft, nd):
    """[(coded, decoded) of slot 0, of slot 1]"""
    if ("t", fs, fft, nd) not in _CODED:
        _CODED["t", fs, fft, nd] = [_code(env, fs, fft, nd, b) for b in _tracks(fs, fft)]
    return _CODED["t", fs, fft, nd]


def _pair(env, fs, fft, nd, u, **kw):
    """the lane of tests/test_gpu_track_morph.py for stream u twice: with the coded rows of its voice, and with the decoded ones"""
    ln = _lane(fs, fft, u, **kw)
    n = len(ln["pos"])
    coded, decoded = _cvoice(env, fs, fft, nd, u)
    return dict(ln, voice=tuple(v[:n] for v in coded)), dict(ln, voice=tuple(v[:n] for v in decoded))


def _pairs(env, fs, fft, nd, cutting="cycle"):
    both = [_pair(env, fs, fft, nd, u, cutting=cutting) for u in range(4)]
    return [c for c, _ in both] + [None], [d for _, d in both] + [None]


def _new_coded(env, fs, fft, nd, n_streams, max_frames=MAXF, max_delay=MAXD):
    from world_class_amd.stream import CodedTrackMorph
    h = CodedTrackMorph(fs, fft, nd, n_streams, 2, M[1], max_frames, max_delay)
    for t, (coded, _) in enumerate(_ctracks(env, fs, fft, nd)):
        h.set_track(t, *coded)
    assert [h.track_length(t) for t in (0, 1)] == M
    return h


def _new_full(env, fs, fft, nd, n_streams, max_frames=MAXF, max_delay=MAXD):
    """the reference: the full-row handle of the same shape on the decoded tracks"""
    from world_class_amd.stream import TrackMorph
    h = TrackMorph(fs, fft, n_streams, 2, M[1], max_frames, max_delay)
    for t, (_, decoded) in enumerate(_ctracks(env, fs, fft, nd)):
        h.set_track(t, *decoded)
    return h


def _five(env, fs, fft, nd, ratios, fixed=False):
    """the five streams driven together on the coded handle, once per case and module: the run the other tests compare with"""
    key = (fs, fft, nd, ratios, fixed)
    if key not in _RUNS:
        _RUNS[key] = _drive(env, fs, fft, _pairs(env, fs, fft, nd)[0], ratios=ratios, fixed=fixed, handle=_new_coded(env, fs, fft, nd, 5))
    return _RUNS[key]


def _identical(got, want, what):
    for key in ("f0", "sp", "ap", "w", "wf", "ra", "rb"):
        assert _same(got[key], want[key]), (what, key)


# ---- 9. (first, as in the full-row file) the cases cover what they should -----------------------------------------------------

def test_the_cases_cover_what_they_should():
    """(no GPU work: the tables) at least 40 % of the positions consumed are fractional, every special value is among them, every
    delay has a push that straddles i = D, and the ring wraps"""
    assert tm.ring_cap(MAXD, MAXF) == 10 and DELAY[:4] == [0, 1, 3, 5] and ROWS[4] == 0
    for u in range(4):  # (the positions and the cuts depend on the stream alone, not on the size)
        ln = _lane(16000, 512, u)
        m = M[ln["slot"]]
        used = _used(ln)
        assert len(used) == ROWS[u]
        fin = used[np.isfinite(used)]
        assert np.isnan(used).any() and (used == np.inf).any() and (used == -np.inf).any() and (fin < 0).any() and (fin > m - 1).any()
        assert (np.diff(fin) < 0).any() and (np.diff(used) == 0).any()  # they fall and repeat
        if m > 1:
            assert (fin != np.floor(fin)).mean() >= 0.4 and (fin * 2 % 2 == 1).any() and (fin == np.floor(fin)).any()
        at = np.cumsum([0] + ln["cuts"])
        assert sorted(set(ln["cuts"][:-1])) == [0, 1, 6]
        if ln["delay"]:
            assert any(s < ln["delay"] < e for s, e in zip(at, at[1:])), u
            s = tm.Stream(ln["delay"], MAXD, MAXF)
            assert sum(len(s.push(c)[1]) for c in ln["cuts"]) > (1 if u == 1 else 3) * s.cap
    assert [FIRST[u] for u in range(4)] == [0, 2, 1, 0]


# ---- 1. bit identity with the full-row handle on the decoded rows -------------------------------------------------------------

@pytest.mark.parametrize("fs,fft,nd,ratios", SIZES)
def test_frames_equal_the_full_row_handle_on_the_decoded_rows(env, fs, fft, nd, ratios):
    """(16000, 512, 25): n_ap = 1 and nd odd, coded rows on 8-byte boundaries only; (24000, 1024, 40) with ratios, one push with
    stream 2 alone having them; (48000, 2048, 60): the one-wavefront decoder"""
    w, codec, wio, torch = env
    assert codec.number_of_aperiodicities(fs) == {16000: 1, 24000: 3, 48000: 5}[fs]
    coded, decoded = _pairs(env, fs, fft, nd)
    got = _five(env, fs, fft, nd, ratios)
    want = _drive(env, fs, fft, decoded, ratios=ratios, handle=_new_full(env, fs, fft, nd, 5))
    for u in range(4):
        assert len(got[u]["f0"]) == ROWS[u]
        _identical(got[u], want[u], u)
        gone = ~np.isfinite(_used(coded[u]))  # the frames that are NaN throughout, and no others
        o = got[u]
        assert gone.any() and _same(np.isnan(o["f0"]), gone) and _same(np.isnan(o["sp"]).all(axis=1), gone) and _same(np.isnan(o["ap"]).any(axis=1), gone)
    assert len(got[4]["f0"]) == 0
    if ratios:
        assert len({(a, b) for a, b in zip(got[2]["ra"], got[2]["rb"])}) > 4 and (got[0]["ra"] == 0).any()
    if (fs, fft) == (24000, 1024):  # by the full-row handle's contract: wc_morph_parameters_device on the decoded pair
        ln, o = decoded[3], got[3]
        n = ROWS[3]
        d = dict(a_lengths=[n], b_lengths=[M[ln["slot"]]], out_lengths=[n], a=ln["voice"], b=_ctracks(env, fs, fft, nd)[ln["slot"]][1],
                 pos_a=np.arange(n, dtype=np.float64), pos_b=_used(ln), weight=o["w"], f0_weight=o["wf"])
        whole = _morph(env, fs, fft, d, o["ra"], o["rb"])
        assert _same(o["f0"], whole[0]) and _same(o["sp"], whole[1]) and _same(o["ap"], whole[2])


@pytest.mark.parametrize("fs,fft,nd", [(48000, 4096, 60), (48000, 2048, 300)])
def test_a_dozen_frames_at_fft_4096_and_at_the_unpruned_first_stage(env, fs, fft, nd):
    """fft 4096: the workgroup decoders at the largest size and both LDS rows full; fft 2048 with nd = 300 > 256: the one-wavefront
    decoder's unpruned first stage.  Delay 3, ratios on both sides"""
    coded, decoded = _pair(env, fs, fft, nd, 2, cutting="five_two", rows=12)
    got = _drive(env, fs, fft, [coded], ratios=True, handle=_new_coded(env, fs, fft, nd, 1))[0]
    want = _drive(env, fs, fft, [decoded], ratios=True, handle=_new_full(env, fs, fft, nd, 1))[0]
    assert len(got["f0"]) == 12 and (got["ra"] != 0).any() and (got["rb"] != 0).any() and np.isfinite(got["sp"]).any()
    _identical(got, want, (fft, nd))


# ---- 2. cuttings and isolation ------------------------------------------------------------------------------------------------

def test_the_same_rows_under_other_cuttings_give_identical_bits(env):
    """one setting per stream (a weight that blends, ratios on), the rows cut along 0-1-6, six by six and one by one -- the last
    two on ONE handle, the small pushes behind the large ones: no scratch slot of an earlier, larger push shows"""
    fs, fft, nd = 24000, 1024, 40
    base = _five(env, fs, fft, nd, True, fixed=True)
    h = _new_coded(env, fs, fft, nd, 5)
    for cutting in ("sixes", "ones"):
        got = _drive(env, fs, fft, _pairs(env, fs, fft, nd, cutting)[0], ratios=True, fixed=True, handle=h)
        for u in range(4):
            for key in ("f0", "sp", "ap"):
                assert _same(got[u][key], base[u][key]), (cutting, u, key)
    want = _drive(env, fs, fft, _pairs(env, fs, fft, nd)[1], ratios=True, fixed=True, handle=_new_full(env, fs, fft, nd, 5))
    _identical(base[3], want[3], "fixed")


def test_a_stream_alone_gives_the_bits_it_gives_among_the_five(env):
    fs, fft, nd = 24000, 1024, 40
    alone = _drive(env, fs, fft, [_pair(env, fs, fft, nd, 3)[0]], ratios=True, handle=_new_coded(env, fs, fft, nd, 1))[0]
    among = _five(env, fs, fft, nd, True)[3]
    for key in ("f0", "sp", "ap"):
        assert _same(alone[key], among[key]), key


# ---- 3. the flush, through the numpy front-ends -------------------------------------------------------------------------------

def test_flush_at_few_rows_one_past_the_delay_and_many(env):
    """D = 5 with n = 2 (n < D), n = 6 (n = D + 1: the first tail entry is skipped) and n = 30, through CodedTrackMorph.push /
    .flush, against TrackMorph.push / .flush on the decoded rows"""
    fs, fft, nd = 16000, 512, 25
    both = [_pair(env, fs, fft, nd, 3, rows=n, delay=5) for n in (2, 6, 30)]
    hc, hf = _new_coded(env, fs, fft, nd, 3), _new_full(env, fs, fft, nd, 3)
    runs = []
    for h, lanes in ((hc, [c for c, _ in both]), (hf, [d for _, d in both])):
        got = [[[], [], []] for _ in lanes]
        for i, ln in enumerate(lanes):
            h.reset(i, ln["slot"], 5)
            h.set_weight(i, 0.25, 0.75)
        for k in range(5):
            rows = [tuple(v[6 * k:6 * k + 6] for v in ln["voice"]) for ln in lanes]
            res = h.push(rows, [ln["pos"][6 * k:6 * k + 6] for ln in lanes])
            assert [len(r[0]) for r in res] == [max(min(len(ln["pos"]), 6 * k + 6) - 5, 0) - max(min(len(ln["pos"]), 6 * k) - 5, 0) for ln in lanes]
            for i, r in enumerate(res):
                for q in range(3):
                    got[i][q].append(r[q])
        assert [h.pending(i) for i in range(3)] == [2, 5, 5] and [h.frames_formed(i) for i in range(3)] == [0, 1, 25]
        assert [len(ln["tail"]) for ln in lanes] == [2, 6, 6]
        res = h.flush([ln["tail"] for ln in lanes])
        assert [len(r[0]) for r in res] == [2, 5, 5]
        assert [h.pending(i) for i in range(3)] == [0, 0, 0] and [h.frames_formed(i) for i in range(3)] == [2, 6, 30]
        runs.append([[np.concatenate(got[i][q] + [r[q]]) for q in range(3)] for i, r in enumerate(res)])
    for i, n in enumerate((2, 6, 30)):
        for q in range(3):
            assert len(runs[0][i][q]) == n and _same(runs[0][i][q], runs[1][i][q]), (n, q)
    assert np.isfinite(runs[0][2][1]).any()
    lanes = [c for c, _ in both]
    none = tuple(v[:0] for v in lanes[0]["voice"])
    with pytest.raises(env[0].WorldClassError):  # ended: rows are refused until the next reset
        hc.push([tuple(v[:1] for v in lanes[0]["voice"]), none, none], [np.zeros(1), np.zeros(0), np.zeros(0)])
    with pytest.raises(env[0].WorldClassError):
        hc.flush([lanes[0]["tail"], None, None])
    hc.close()
    hc.close()


# ---- 4. a stream reused on the other track ------------------------------------------------------------------------------------

def test_a_stream_is_reused_after_reset_onto_the_other_track(env):
    """stream 3 of a handle that has run the five is attached again, at delay 5, and takes twelve coded rows of NaN: every one of
    its ten ring slots holds NaN.  Reset onto slot 0 (m = 1) at delay 3 it runs 40 rows of its voice: no stale row shows"""
    w, codec, wio, torch = env
    fs, fft, nd = 16000, 512, 25
    bins, n_ap = fft // 2 + 1, codec.number_of_aperiodicities(fs)
    h = _new_coded(env, fs, fft, nd, 5)
    first = _drive(env, fs, fft, _pairs(env, fs, fft, nd)[0], handle=h)
    _identical(first[3], _five(env, fs, fft, nd, False)[3], "first")

    def poison(h):
        h.reset(3, 1, 5)
        nan = [torch.full((6 * wd,), np.nan, dtype=torch.float64, device="cuda") for wd in (1, nd, n_ap)]
        outs = [_guarded(torch, 6, wd) for wd in (1, bins, bins)]
        zero = torch.zeros(6, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert h.push_device([0, 0, 0, 6, 0], *nan, zero, *outs) == [0, 0, 0, 1, 0]
        assert h.push_device([0, 0, 0, 6, 0], *nan, zero, *outs) == [0, 0, 0, 6, 0]
        w.lib().wc_synchronize()
        assert h.pending(3) == 5

    coded, decoded = _pair(env, fs, fft, nd, 3, rows=40, slot=0, delay=3)
    o = _drive(env, fs, fft, [None, None, None, coded, None], handle=h, pre=poison)[3]
    want = _drive(env, fs, fft, [None, None, None, decoded, None], handle=_new_full(env, fs, fft, nd, 5))[3]
    _identical(o, want, "reused")
    assert _same(np.isnan(o["sp"]).any(axis=1), ~np.isfinite(_used(coded)))


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------

def test_refusals_leave_everything_as_it_was(env):
    w, codec, wio, torch = env
    from world_class_amd.stream import CodedTrackMorph, _lib
    fs, fft, nd = 24000, 1024, 40
    bins = fft // 2 + 1
    nan, inf = float("nan"), float("inf")
    L = _lib()
    src = _cvoice(env, fs, fft, nd, 1)[0]
    track = _ctracks(env, fs, fft, nd)[1][0]

    def state(h):
        return [(h.frames_received(u), h.frames_formed(u), h.pending(u), h.get_delay(u)) for u in range(5)] + [h.track_length(t) for t in (0, 1)] + [h.device_bytes()]

    def hook(k, h):
        if k not in (0, 7, 20):
            return
        before = state(h)
        d_in = [_dev(torch, v[:7]) for v in src]
        d_pos = torch.zeros(7, dtype=torch.float64, device="cuda")
        outs = [_guarded(torch, 5 * MAXF, 1), _guarded(torch, 5 * MAXF, bins), _guarded(torch, 5 * MAXF, bins)]
        torch.cuda.synchronize()
        at = lambda u, v: [v if i == u else 0 for i in range(5)]
        push = lambda n_a, a=d_in, p=d_pos, o=outs: h.push_device(n_a, *a, p, *o)
        flush = lambda want, t=d_pos, o=outs: h.flush_device(want, t, *o)
        _refused(w, push, at(0, 7))                         # over max_frames
        _refused(w, push, at(2, -1))                        # a negative count
        _refused(w, push, at(4, 1))                         # a stream that is not attached
        _refused(w, push, at(0, 2), [None] * 3)             # NULL arrays with rows to read ...
        _refused(w, push, at(0, 2), [d_in[0], None, d_in[2]])
        _refused(w, push, at(0, 2), [d_in[0], d_in[1], None])
        _refused(w, push, at(0, 2), d_in, None)             # ... with positions to read (delay 0: both rows form frames) ...
        _refused(w, push, at(0, 2), d_in, d_pos, [None] * 3)  # ... and with frames to write
        _refused(w, lambda: w._check(L.wc_track_morph_coded_push_device(h._h, None, None, None, None, None, None, None, None, (C.c_int * 5)())))
        _refused(w, lambda: w._check(L.wc_track_morph_coded_push_device(h._h, (C.c_int * 5)(), None, None, None, None, None, None, None, None)))
        _refused(w, flush, at(0, 1))                        # no delay
        _refused(w, flush, at(4, 1))                        # not attached
        if k == 0:
            _refused(w, flush, at(2, 1))                    # no rows
            h.set_track(1, *track)                          # (no stream has rows yet: allowed, and the same rows)
        else:
            _refused(w, flush, at(2, 1), None)              # NULL tail / outputs with frames to form
            _refused(w, flush, at(2, 1), d_pos, [None] * 3)
            _refused(w, h.set_track_device, 1, 40, *[_dev(torch, v) for v in track])  # streams with rows are attached
        _refused(w, lambda: w._check(L.wc_track_morph_coded_flush_device(h._h, None, None, None, None, None, (C.c_int * 5)())))
        _refused(w, lambda: w._check(L.wc_track_morph_coded_flush_device(h._h, (C.c_int * 5)(), None, None, None, None, None)))
        d_t = [_dev(torch, v) for v in track]
        for bad in ((-1, 1), (2, 1), (0, 0), (0, 41)):      # a bad slot, m out of range
            _refused(w, h.set_track_device, bad[0], bad[1], *d_t)
        for hole in range(3):                               # a NULL array
            _refused(w, h.set_track_device, 0, 1, *[None if q == hole else t for q, t in enumerate(d_t)])
        for bad in ((-1, 0, 0), (5, 0, 0), (4, -1, 0), (4, 2, 0), (4, 0, -1), (4, 0, 6)):  # stream, slot, delay
            _refused(w, h.reset, *bad)
        for bad in ((nan, 0.5), (0.5, nan), (inf, 0.5), (0.5, -inf)):
            _refused(w, h.set_weight, 1, *bad)
        for bad in ((-1.0, 0.0), (0.0, -1.0), (nan, 1.0), (1.0, inf), (1.0 / fft, 1.0), (1.0, 1.9 / fft)):
            _refused(w, h.set_ratios, 1, *bad)
        for u in (-1, 5):
            _refused(w, h.set_weight, u, 0.5)
            _refused(w, h.set_ratios, u, 1.0, 1.0)
            assert (h.frames_received(u), h.frames_formed(u), h.pending(u), h.get_delay(u)) == (-1, -1, -1, -1)
        assert h.track_length(-1) == -1 and h.track_length(2) == -1
        assert h.push_device([0] * 5, None, None, None, None, None, None, None) == [0] * 5  # no rows: nothing to read or to write
        w.lib().wc_synchronize()
        assert all(bool(torch.isnan(o).all()) for o in outs)
        assert state(h) == before

    h = _new_coded(env, fs, fft, nd, 5)
    got = _drive(env, fs, fft, _pairs(env, fs, fft, nd)[0], ratios=True, handle=h, hook=hook)
    want = _five(env, fs, fft, nd, True)
    for u in range(4):  # (the refused setters kept the settings of the drive, the refused pushes the ring)
        _identical(got[u], want[u], u)
    # create: what the full-row handle refuses, and the decoder's: nd outside 1 .. fft / 2, fs below 12 kHz
    for bad in ((fs, 1000, nd, 1, 1, 4, 2, 1), (0, fft, nd, 1, 1, 4, 2, 1), (fs, fft, nd, 0, 1, 4, 2, 1), (fs, fft, nd, 1, 0, 4, 2, 1), (fs, fft, nd, 1, 1, 0, 2, 1),
                (fs, fft, nd, 1, 1, 4, 0, 1), (fs, fft, nd, 1, 1, 4, 2, -1), (fs, fft, 0, 1, 1, 4, 2, 1), (fs, fft, -3, 1, 1, 4, 2, 1),
                (fs, fft, fft // 2 + 1, 1, 1, 4, 2, 1), (8000, fft, nd, 1, 1, 4, 2, 1), (11999, fft, nd, 1, 1, 4, 2, 1)):
        with pytest.raises(w.WorldClassError):
            CodedTrackMorph(*bad)
    assert L.wc_track_morph_coded_device_bytes(None) == -1
    g = CodedTrackMorph(fs, fft, nd, 1, 2, 4, 2, 0)  # max_delay = 0: no ring; a reset onto a slot that has not been set
    _refused(w, g.reset, 0, 1, 0)
    g.set_track(1, *[v[:3] for v in track])
    _refused(w, g.reset, 0, 0, 0)
    _refused(w, g.reset, 0, 1, 1)
    g.reset(0, 1, 0)
    coded, decoded = _cvoice(env, fs, fft, nd, 0)
    res = g.push([tuple(v[:2] for v in coded)], [np.array([0.0, 1.5])])  # weight 0 after the reset: the voice's decoded rows as they are
    assert _same(res[0][0], decoded[0][:2]) and _same(res[0][1], decoded[1][:2]) and _same(res[0][2], decoded[2][:2]) and g.pending(0) == 0
    g.close()
    CodedTrackMorph(12000, fft, fft // 2, 1, 1, 1, 1, 0).close()  # the edges that are taken


# ---- 6. ordering on the caller's stream ---------------------------------------------------------------------------------------

def test_calls_are_ordered_on_the_callers_stream(env):
    """a long torch kernel in front on a torch stream handed over by wc_set_stream, the coded rows and the positions written by
    torch kernels on that stream, no synchronisation before the calls: the first two pushes return while the kernel in front still
    runs (the staging is a pair, the decoding plan was built by create), and every call reads its rows and its positions behind it;
    one synchronisation at the end"""
    w, codec, wio, torch = env
    fs, fft, nd = 24000, 1024, 40
    bins, n_ap = fft // 2 + 1, codec.number_of_aperiodicities(fs)
    ln, dec = _pair(env, fs, fft, nd, 2, cutting="sixes", rows=24)
    want = _drive(env, fs, fft, [dec], handle=_new_full(env, fs, fft, nd, 1))[0]
    h, warm = _new_coded(env, fs, fft, nd, 1), _new_coded(env, fs, fft, nd, 1)
    warm.reset(0, 1, 0)
    warm.push([tuple(v[:2] for v in ln["voice"])], [np.zeros(2)])  # (the kernels' code is on the device before the clock matters)
    h.reset(0, ln["slot"], ln["delay"])
    host = [torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64).ravel().copy()).pin_memory() for v in ln["voice"] + (ln["pos"], ln["tail"])]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert w.lib().wc_set_stream(s.cuda_stream) == 0
    try:
        outs, running = [], []
        with torch.cuda.stream(s):
            junk = torch.randn(4096, 4096, device="cuda")
            for _ in range(40):  # a long-running kernel in front: the calls must wait for it and for the uploads behind it
                junk = junk @ junk * 1e-3
            done = torch.cuda.Event()
            done.record(s)
            dev = [torch.zeros(len(t), dtype=torch.float64, device="cuda") for t in host]
            for dst, src in zip(dev, host):
                dst.copy_(src, non_blocking=True)
                dst.mul_(1.0)  # torch kernels on the stream write every input
            off = 0
            sim = tm.Stream(ln["delay"], MAXD, MAXF)
            for k, c in enumerate(ln["cuts"] + [None]):
                st = _settings(2, k, fft, False)
                h.set_weight(0, st[0], st[1])
                m = sim.pending() if c is None else sim.count(c)
                o = [_guarded(torch, m, 1), _guarded(torch, m, bins), _guarded(torch, m, bins)]
                if c is None:
                    assert h.flush_device([1], dev[4], *o) == [m]
                else:
                    ins = [t[off * wd:(off + c) * wd] for t, wd in zip(dev[:4], (1, nd, n_ap, 1))]
                    assert h.push_device([c], *ins, *o) == [m]
                    sim.push(c)
                    off += c
                running.append(not done.query())
                outs.append((o, m))
        s.synchronize()  # once
    finally:
        assert w.lib().wc_set_stream(None) == 0
    assert running[0] and running[1], running
    got = [np.concatenate([_rows(o[q], m, wd) for o, m in outs]) for q, wd in enumerate((1, bins, bins))]
    assert _same(got[0][:, 0], want["f0"]) and _same(got[1], want["sp"]) and _same(got[2], want["ap"]) and np.isfinite(got[1]).any()


# ---- 7. memory ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(24000, 1024, 60, 8, 2, 100, 5, 20), (48000, 2048, 60, 3, 1, 77, 50, 7), (16000, 512, 25, 2, 1, 9, 4, 0)])
def test_device_bytes_is_the_headers_formula(env, shape):
    """every array once and exactly, each rounded up to 256 bytes; tracks + ring take (1 + nd + n_ap) / (1 + 2 bins) of what the
    full-row handle's arrays hold (8 (T + S) (1 + 2 bins) bytes by its create's arithmetic), the rounding of six arrays apart"""
    w, codec, wio, torch = env
    from world_class_amd.stream import CodedTrackMorph
    fs, fft, nd, n, n_tracks, max_m, mf, md = shape
    bins, n_ap = fft // 2 + 1, codec.number_of_aperiodicities(fs)
    A = lambda x: (x + 255) // 256 * 256 if x else 0
    T, S, F = n_tracks * max_m, n * (md + min(md, mf)), n * max(mf, md)
    tracks = A(8 * T) + A(8 * T * nd) + A(8 * T * n_ap)
    ring = A(8 * S) + A(8 * S * nd) + A(8 * S * n_ap)
    scratch = A(24 * F * nd) + A(24 * F * n_ap) + 2 * A(24 * F * bins)
    records = A(48 * n + 16 * F + 8 * n * min(md, mf))
    h = CodedTrackMorph(fs, fft, nd, n, n_tracks, max_m, mf, md)
    assert h.device_bytes() == tracks + ring + scratch + records
    h.close()
    full = 8 * (T + S) * (1 + 2 * bins)
    exact = 8 * (T + S) * (1 + nd + n_ap)  # = full x (1 + nd + n_ap) / (1 + 2 bins)
    assert exact * (1 + 2 * bins) == full * (1 + nd + n_ap) and exact <= tracks + ring < exact + 6 * 256
    assert (md > 0) == (ring > 0) and 15 * exact < full  # (a fifteenth or less at these sizes, the rounding apart)


# ---- 8. the live chain on coded rows alone ------------------------------------------------------------------------------------

def test_one_set_of_coded_rows_through_alignment_the_morph_and_a_synthesis_stream(env):
    """fft 1024, lag 3.  Every push codes the new rows once (wc_code_features_device); the SAME coded sp array goes to
    AlignStream.push_settled_device and, with its coded ap rows, to CodedTrackMorph.push_device, which reads d_settled where it
    lies; the same coded track arrays went to both set_track_device calls; a synthesis stream takes the frames and tail_device
    feeds flush_device -- nothing is downloaded in between.  Afterwards the frames equal wc_morph_parameters_device on the decoded
    voice and the decoded track at the settled and tail values read back, and the samples equal the batch Synthesis of those
    frames bit for bit (fft 1024: no FP64 atomics)."""
    w, codec, wio, torch = env
    from oracle.gen_golden import synth_params
    from world_class_amd.stream import AlignStream, CodedTrackMorph, StreamSynthesizer
    fs, fft, nd, lag, n, m = 24000, 1024, 40, 3, 30, 40
    bins, n_ap = fft // 2 + 1, codec.number_of_aperiodicities(fs)
    track = synth_params(fs, fft, m, 8101)
    at = (np.arange(n) * 1.2).astype(np.int64)  # the voice runs through the track 1.2 times as fast, a little louder and higher
    voice = (track[0][at] * 1.1, track[1][at] * 1.21, track[2][at].copy())
    d_track, d_voice = [_dev(torch, v) for v in track], [_dev(torch, v) for v in voice]
    new = lambda k, fill=np.nan: torch.full((k,), fill, dtype=torch.float64, device="cuda")
    d_ctrack, d_ctrack_ap, d_csp, d_cap = new(m * nd), new(m * n_ap), new(n * nd), new(n * n_ap)
    torch.cuda.synchronize()
    codec.code_features_device(fs, fft, m, nd, d_track[1], d_track[2], d_ctrack, d_ctrack_ap)
    al = AlignStream(nd, 1, 1, m, MAXF)
    al.reserve_lag(lag)
    al.set_track_device(0, m, d_ctrack)
    al.reset(0, 0)
    al.set_lag(0, lag)
    h = CodedTrackMorph(fs, fft, nd, 1, 1, m, MAXF, lag)
    h.set_track_device(0, m, d_track[0], d_ctrack, d_ctrack_ap)
    h.reset(0, 0, lag)
    h.set_weight(0, 0.5, 0.25)
    syn = StreamSynthesizer(fs, fft, 5.0, 1, MAXF)
    d_pos, d_cost, d_settled, d_tail = new(n + 1), new(n + 1), new(n + 1), new(lag + 2)
    frames, y, off = [], [], 0
    torch.cuda.synchronize()

    def synthesise(counts, o, flush):
        c = syn.push_device(counts, *o, flush=[flush])
        w.lib().wc_synchronize()
        y.append(syn._d_y.to_host()[:c[0]].copy())

    for c in _cuts(n, 1, "cycle"):
        rows = [t[off * wd:(off + c) * wd] for t, wd in zip(d_voice, (1, bins, bins))]
        csp, cap = d_csp[off * nd:], d_cap[off * n_ap:]
        if c:
            codec.code_features_device(fs, fft, c, nd, rows[1], rows[2], csp, cap)  # once: what both consumers read
        al.push_settled_device([c], csp, d_pos[off:], d_cost[off:], d_settled[off:])
        want = max(off + c - lag, 0) - max(off - lag, 0)
        o = [_guarded(torch, want, 1), _guarded(torch, want, bins), _guarded(torch, want, bins)]
        torch.cuda.synchronize()  # (the outputs' NaN fill is torch's, on its own stream)
        assert h.push_device([c], rows[0], csp, cap, d_settled[off:], *o) == [want]
        synthesise([want], o, 0)
        frames.append((o, want))
        off += c
    al.tail_device([1], d_tail)
    o = [_guarded(torch, lag, 1), _guarded(torch, lag, bins), _guarded(torch, lag, bins)]
    torch.cuda.synchronize()
    assert h.flush_device([1], d_tail, *o) == [lag]
    synthesise([lag], o, 1)
    frames.append((o, lag))
    settled, tail = d_settled.cpu().numpy(), d_tail.cpu().numpy()
    assert np.isnan(settled[n]) and np.isnan(tail[lag + 1]) and np.isfinite(settled[:n]).all() and np.isfinite(tail[:lag + 1]).all()
    used = tm.consumed(settled[:n], tail[:lag + 1], lag)
    assert (used * 2 == np.floor(used * 2)).all() and used.min() >= 0 and used.max() <= m - 1 and len(set(used)) > 5
    got = [np.concatenate([_rows(f[q], c, wd) for f, c in frames]) for q, wd in enumerate((1, bins, bins))]
    # the decoded voice and the decoded track: one wc_decode_features_device call each over the coded arrays the chain used
    d_dec = [new(n * bins), new(n * bins), new(m * bins), new(m * bins)]
    torch.cuda.synchronize()
    codec.decode_features_device(fs, fft, n, nd, d_csp, d_cap, d_dec[0], d_dec[1])
    codec.decode_features_device(fs, fft, m, nd, d_ctrack, d_ctrack_ap, d_dec[2], d_dec[3])
    w.lib().wc_synchronize()
    dec = [t.cpu().numpy() for t in d_dec]
    d = dict(a_lengths=[n], b_lengths=[m], out_lengths=[n], a=(voice[0], dec[0].reshape(n, bins), dec[1].reshape(n, bins)),
             b=(track[0], dec[2].reshape(m, bins), dec[3].reshape(m, bins)), pos_a=np.arange(n, dtype=np.float64), pos_b=used, weight=np.full(n, 0.5),
             f0_weight=np.full(n, 0.25))
    want = _morph(env, fs, fft, d)
    assert _same(got[0][:, 0], want[0]) and _same(got[1], want[1]) and _same(got[2], want[2]) and np.isfinite(got[1]).all()
    batch = w.Synthesis(fs, fft, 5.0)
    ol = batch.out_length(n)
    d_y = torch.full((ol + 1,), np.nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    end = batch.compute_device(_dev(torch, want[0]), [n], _dev(torch, want[1]), _dev(torch, want[2]), [ol], d_y, rng_pos=[0])
    w.lib().wc_synchronize()
    ref = d_y.cpu().numpy()
    y = np.concatenate(y)
    assert np.isnan(ref[-1]) and np.isfinite(ref[:-1]).all() and np.abs(ref[:-1]).max() > 1e-3
    assert len(y) == ol and [syn.rng_position(0)] == end
    print("coded track morph chain through a synthesis stream against the batch call: %.3e" % np.abs(y - ref[:-1]).max())
    assert np.array_equal(y, ref[:-1])
