"""-m gpu: track-morph streams (wc_track_morph, include/world_class_track_morph.h).  One handle of five streams and two tracks
(slot 0: m = 1, slot 1: m = 40) with max_frames = 6 and max_delay = 5, so cap = 10: streams 0-3 run about 60 rows each at delays
0, 1, 3 and 5, the counts per push cycling through 0, 1 and 6, the weights changing before every push; stream 4 never receives a row.
The frames against ONE whole-utterance wc_morph_parameters_device pair per stream bit for bit (also with ratios per push, and at
fft 4096), against the numpy rule, other cuttings, a stream alone, the flush at n < D, n = D + 1 and n >> D, a stream reused on
the other track over a ring left full of NaN, refusals that leave everything as it was, ordering on the caller's stream, and the
whole live chain: coded rows -> alignment stream -> track morph -> synthesis stream, no download in between.  Outputs are NaN-filled
with a guard row behind them that must stay NaN.

Timings and figures of a run are not asserted; nothing here has a tolerance of its own: bit identity, LOG_EXP_REL of
tests/test_gpu_morph.py against the numpy rule."""
import ctypes as C

import numpy as np
import pytest

import morph_rule as mr
import retime_rule as rr
import track_morph_rule as tm
from test_gpu_morph import LOG_EXP_REL, _morph, _rel
from test_gpu_retime import _dev, _guarded, _rows, _same, env  # noqa: F401

pytestmark = pytest.mark.gpu
MAXF, MAXD = 6, 5
M = [1, 40]                  # rows of the two tracks
DELAY = [0, 1, 3, 5, 0]      # per stream
SLOT = [1, 0, 1, 1, 1]       # the track of stream u
ROWS = [60, 57, 61, 59, 0]   # rows of the live voice of stream u; stream 4 never receives a row
PATTERN = (0, 1, 6)
FIRST = [0, 2, 1, 0, 0]      # where in the pattern stream u starts: one push of every stream with a delay straddles i = D
ONLY_ONE = 4                 # the push at which stream 2 alone has ratios
_SRC, _RUNS = {}, {}


def _voice(fs, fft, u):
    from oracle.gen_golden import synth_params
    if ("v", fs, fft, u) not in _SRC:
        _SRC["v", fs, fft, u] = synth_params(fs, fft, max(ROWS[u], 8), 7100 + fft + u)
    return _SRC["v", fs, fft, u]


def _tracks(fs, fft):
    from oracle.gen_golden import synth_params
    if ("t", fs, fft) not in _SRC:
        one = tuple(v[3:4].copy() for v in synth_params(fs, fft, 8, 7200 + fft))
        _SRC["t", fs, fft] = [one, synth_params(fs, fft, M[1], 7201 + fft)]
    return _SRC["t", fs, fft]


def _positions(n, m, delay, seed):
    """n positions in a track of m rows -- whole, half-integer and arbitrary fractions, falling, repeated, below 0, above m - 1,
    NaN and both infinities; the entries of the rows i < delay, which nothing may read, are NaN -- and the 6 tail entries"""
    rng = np.random.default_rng(seed)
    pos = np.round(rng.uniform(-2.0, m + 1.0, n + 6) * 2) / 2
    pos[1::5] = rng.uniform(0.0, m - 1.0, len(pos[1::5]))
    pos[2::9] = pos[1::9][:len(pos[2::9])]
    if n > 32:
        pos[20:26] = np.linspace(m - 1.0, 0.0, 6)
        pos[[13, 31, 17]] = [np.nan, np.inf, -np.inf]
    pos[:delay] = np.nan
    return pos[:n], pos[n:]


def _cuts(n, first, cutting):
    pat = {"cycle": PATTERN[first % 3:] + PATTERN[:first % 3], "ones": (1,), "sixes": (6,), "five_two": (5, 2, 0)}[cutting]
    return tm.cuttings(n, [pat])[0]


def _lane(fs, fft, u, cutting="cycle", rows=None, slot=None, delay=None):
    """what stream u of the tables is fed; rows / slot / delay replace the tables' values"""
    n = ROWS[u] if rows is None else rows
    slot = SLOT[u] if slot is None else slot
    delay = DELAY[u] if delay is None else delay
    pos, tail = _positions(n, M[slot], delay, 7300 + 10 * u + slot)
    return dict(u=u, voice=tuple(v[:n] for v in _voice(fs, fft, u)), slot=slot, delay=delay, pos=pos, tail=tail[:min(delay + 1, n)], cuts=_cuts(n, FIRST[u], cutting))


def _used(lane):
    return tm.consumed(lane["pos"], lane["tail"] if lane["delay"] else None, lane["delay"])


def _settings(u, k, fft, ratios, fixed=False):
    """weight, F0 weight, ratio of A, ratio of B of stream u at call k: the weights cycle morph_rule.WEIGHTS, the F0 weight three
    places on, the ratios retime_rule.cycled; at call ONLY_ONE stream 2 alone has ratios.  fixed: one setting per stream"""
    if fixed:
        k = 2
    w, wf = mr.WEIGHTS[(k + u) % len(mr.WEIGHTS)], mr.WEIGHTS[(k + u + 3) % len(mr.WEIGHTS)]
    if not ratios:
        return w, wf, 0.0, 0.0
    if k == ONLY_ONE and not fixed:
        return (w, wf, 0.8, 1.2) if u == 2 else (w, wf, 0.0, 0.0)
    return w, wf, float(rr.cycled(fft, 64, u)[k % 64]), float(rr.cycled(fft, 64, u + 3)[k % 64])


def _new(env, fs, fft, n_streams):
    from world_class_amd.stream import TrackMorph
    h = TrackMorph(fs, fft, n_streams, 2, M[1], MAXF, MAXD)
    for t, b in enumerate(_tracks(fs, fft)):
        h.set_track(t, *b)
    assert [h.track_length(t) for t in (0, 1)] == M
    return h


def _drive(env, fs, fft, lanes, ratios=False, fixed=False, handle=None, pre=None, hook=None, on_frames=None):
    """Drives the lanes (None: a stream that is never attached) together on one handle, call by call along the rule; the call behind
    the last push is the flush of every stream with a delay and rows.  pre(handle): before the resets.  hook(k, handle): before
    call k, behind its settings.  on_frames(k, counts, f0, sp, ap): the device outputs of call k.  Returns per stream a dict: f0,
    sp, ap of the formed frames and w, wf, ra, rb per frame."""
    w, codec, wio, torch = env
    bins, n = fft // 2 + 1, len(lanes)
    h = handle or _new(env, fs, fft, n)
    if pre is not None:
        pre(h)
    for i, ln in enumerate(lanes):
        if ln is not None:
            h.reset(i, ln["slot"], ln["delay"])
            assert (h.get_delay(i), h.frames_received(i), h.frames_formed(i), h.pending(i)) == (ln["delay"], 0, 0, 0)
    sims = [tm.Stream(ln["delay"] if ln else 0, MAXD, MAXF) for ln in lanes]
    counters = lambda i: (h.frames_received(i), h.frames_formed(i), h.pending(i))
    idle = {i: counters(i) for i, ln in enumerate(lanes) if ln is None}  # (a stream without a lane stays as it is)
    K = max(len(ln["cuts"]) for ln in lanes if ln)
    off = [0] * n
    out = [dict(f0=[], sp=[], ap=[], w=[], wf=[], ra=[], rb=[]) for _ in lanes]
    for k in range(K + 1):
        sets = [_settings(ln["u"], k, fft, ratios, fixed) if ln else None for ln in lanes]
        for i, s in enumerate(sets):
            if s is not None:
                h.set_weight(i, s[0], s[1])
                h.set_ratios(i, s[2], s[3])
        if hook is not None:
            hook(k, h)
        if k < K:
            counts = [ln["cuts"][k] if ln and k < len(ln["cuts"]) else 0 for ln in lanes]
            want = [sims[i].count(c) for i, c in enumerate(counts)]
            parts = [[], [], [], []]
            for i, (ln, c) in enumerate(zip(lanes, counts)):
                if c:
                    for q in range(3):
                        parts[q].append(np.asarray(ln["voice"][q][off[i]:off[i] + c]).reshape(c, -1))
                    parts[3].append(ln["pos"][off[i]:off[i] + c].reshape(c, 1))
                sims[i].push(c)
                off[i] += c
            ins = [_dev(torch, np.concatenate(p)) if p else None for p in parts]
            call = lambda outs: h.push_device(counts, *ins, *outs)
        else:
            wanted = [1 if ln and ln["delay"] > 0 and len(ln["pos"]) > 0 else 0 for ln in lanes]
            if not any(wanted):
                break
            want = [sims[i].pending() if f else 0 for i, f in enumerate(wanted)]
            ins = [_dev(torch, np.concatenate([ln["tail"] for ln, f in zip(lanes, wanted) if f]))]
            for i, f in enumerate(wanted):
                if f:
                    sims[i].flush()
            call = lambda outs: h.flush_device(wanted, *ins, *outs)
        m = sum(want)
        outs = [_guarded(torch, m, 1), _guarded(torch, m, bins), _guarded(torch, m, bins)]
        torch.cuda.synchronize()
        got = call(outs)
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
            if sets[i] is not None:
                for key, v in zip(("w", "wf", "ra", "rb"), sets[i]):
                    out[i][key] += [v] * c
            assert counters(i) == (idle[i] if i in idle else (sims[i].n, sims[i].formed(), sims[i].pending())), (k, i)
    for o in out:
        for key in ("f0", "sp", "ap"):
            o[key] = np.concatenate(o[key])
        for key in ("w", "wf", "ra", "rb"):
            o[key] = np.array(o[key], dtype=np.float64)
    return out


def _lanes(fs, fft, cutting="cycle"):
    return [_lane(fs, fft, u, cutting) for u in range(4)] + [None]


def _five(env, fs, fft, ratios, fixed=False):
    """the five streams driven together, once per (size, ratios, fixed) and module: the run the other tests compare with"""
    if (fs, fft, ratios, fixed) not in _RUNS:
        _RUNS[fs, fft, ratios, fixed] = _drive(env, fs, fft, _lanes(fs, fft), ratios=ratios, fixed=fixed)
    return _RUNS[fs, fft, ratios, fixed]


def _whole(env, fs, fft, lane, o, ratios):
    """one wc_morph_parameters_device pair (all rows of the voice, the track) at d_position_a = the frame's index, d_position_b =
    the entry consumed and the per-frame settings of the run"""
    a, b = lane["voice"], _tracks(fs, fft)[lane["slot"]]
    n = len(a[0])
    assert len(o["w"]) == n
    d = dict(a_lengths=[n], b_lengths=[len(b[0])], out_lengths=[n], a=a, b=b, pos_a=np.arange(n, dtype=np.float64), pos_b=_used(lane), weight=o["w"],
             f0_weight=o["wf"])
    return _morph(env, fs, fft, d, o["ra"] if ratios else None, o["rb"] if ratios else None)


def _equal(got, want, what):
    for key, w_ in zip(("f0", "sp", "ap"), want):
        assert _same(got[key], w_), (what, key)


# ---- 1. the frames of every stream equal the whole-utterance call ------------------------------------------------------------

def test_the_cases_cover_what_they_should():
    """(no GPU work: the tables above) the ring wraps several times, one push straddles i = D for every delay, and the positions
    consumed hold every kind"""
    assert tm.ring_cap(MAXD, MAXF) == 10
    for u in range(1, 4):
        ln = _lane(16000, 512, u)
        at = np.cumsum([0] + ln["cuts"])
        assert any(s < ln["delay"] < e for s, e in zip(at, at[1:])), u
        assert sorted(set(ln["cuts"][:-1])) == [0, 1, 6]
        s = tm.Stream(ln["delay"], MAXD, MAXF)
        assert sum(len(s.push(c)[1]) for c in ln["cuts"]) > (1 if u == 1 else 3) * s.cap  # (numbers taken: the ring wraps)
    used = _used(_lane(16000, 512, 2))
    m = M[1]
    fin = used[np.isfinite(used)]
    assert np.isnan(used).any() and (used == np.inf).any() and (used == -np.inf).any() and (fin < 0).any() and (fin > m - 1).any()
    assert (fin == np.floor(fin)).any() and (fin * 2 % 2 == 1).any() and (fin * 2 != np.floor(fin * 2)).any()
    assert (np.diff(fin) < 0).any() and (np.diff(used) == 0).any()


@pytest.mark.parametrize("fs,fft,ratios", [(16000, 512, False), (16000, 1024, True)])
def test_frames_equal_the_whole_call_bit_for_bit(env, fs, fft, ratios):
    """per stream the concatenated frames of all pushes and the flush are those of ONE pair; the counters follow the rule at every
    call (checked inside the drive); the idle stream forms nothing"""
    runs = _five(env, fs, fft, ratios)
    for u, ln in enumerate(_lanes(fs, fft)[:4]):
        o = runs[u]
        assert len(o["f0"]) == ROWS[u]
        want = _whole(env, fs, fft, ln, o, ratios)
        _equal(o, want, u)
        gone = ~np.isfinite(_used(ln))  # the frames that are NaN throughout, and no others
        assert gone.any() and _same(np.isnan(o["f0"]), gone) and _same(np.isnan(o["sp"]).all(axis=1), gone) and _same(np.isnan(o["ap"]).any(axis=1), gone)
    assert len(runs[4]["f0"]) == 0
    if ratios:  # (the ratios do change rows, and leave the contour and the ap rows alone; one push had them on stream 2 alone)
        assert len({(a, b) for a, b in zip(runs[2]["ra"], runs[2]["rb"])}) > 4 and (runs[0]["ra"] == 0).any()
        plain = _five(env, fs, fft, False)
        assert _same(runs[2]["f0"], plain[2]["f0"]) and _same(runs[2]["ap"], plain[2]["ap"]) and not _same(runs[2]["sp"], plain[2]["sp"])


def test_lds_rows_at_fft_4096(env):
    """a dozen frames at the largest size, where the log rows fill both LDS arrays: delay 3, ratios on both sides"""
    fs, fft = 96000, 4096
    ln = _lane(fs, fft, 2, cutting="five_two", rows=12)
    o = _drive(env, fs, fft, [ln], ratios=True)[0]
    assert len(o["f0"]) == 12 and (o["ra"] != 0).any() and (o["rb"] != 0).any() and np.isfinite(o["sp"]).any()
    _equal(o, _whole(env, fs, fft, ln, o, True), "4096")


# ---- 2. against the numpy rule ------------------------------------------------------------------------------------------------

def test_frames_agree_with_the_numpy_rule(env):
    fs, fft = 16000, 512
    runs = _five(env, fs, fft, False)
    for u, ln in enumerate(_lanes(fs, fft)[:4]):
        o, n = runs[u], ROWS[u]
        f0, sp, ap = mr.morph(ln["voice"], _tracks(fs, fft)[ln["slot"]], np.arange(n, dtype=np.float64), _used(ln), o["w"], o["wf"])
        assert _same(o["ap"], ap)
        ok = np.isfinite(_used(ln))
        ends = ((o["w"] == 0) | (o["w"] == 1)) & ok
        assert _same(o["sp"][ends], sp[ends]) and _same(np.isnan(o["sp"]), np.isnan(sp))
        e_sp = _rel(o["sp"][ok & ~ends], sp[ok & ~ends])
        assert _same(np.isnan(o["f0"]), np.isnan(f0)) and _same(o["f0"] == 0, f0 == 0)
        voiced = ok & (f0 != 0)
        e_f0 = _rel(o["f0"][voiced], f0[voiced])
        print("track morph against the numpy rule, fs %d fft %d stream %d: sp %.3e, F0 %.3e (relative)" % (fs, fft, u, e_sp, e_f0))
        assert e_sp < LOG_EXP_REL and e_f0 < LOG_EXP_REL


# ---- 3. cuttings and isolation ------------------------------------------------------------------------------------------------

def test_the_same_rows_under_other_cuttings_give_identical_bits(env):
    """one setting per stream (a weight that blends, ratios on), the rows cut along 0-1-6, one by one and six by six"""
    fs, fft = 16000, 1024
    base = _five(env, fs, fft, True, fixed=True)
    _equal(base[3], _whole(env, fs, fft, _lanes(fs, fft)[3], base[3], True), "fixed")
    for cutting in ("ones", "sixes"):
        got = _drive(env, fs, fft, _lanes(fs, fft, cutting), ratios=True, fixed=True)
        for u in range(4):
            for key in ("f0", "sp", "ap"):
                assert _same(got[u][key], base[u][key]), (cutting, u, key)


def test_a_stream_alone_gives_the_bits_it_gives_among_the_five(env):
    fs, fft = 16000, 1024
    alone = _drive(env, fs, fft, [_lane(fs, fft, 3)], ratios=True)[0]
    among = _five(env, fs, fft, True)[3]
    for key in ("f0", "sp", "ap"):
        assert _same(alone[key], among[key]), key


# ---- 4. the flush, through the numpy front-ends -------------------------------------------------------------------------------

def test_flush_at_few_rows_one_past_the_delay_and_many(env):
    """D = 5 with n = 2 (n < D: the tail has n entries, all used), n = 6 (n = D + 1: six entries, the first skipped) and n = 30,
    through TrackMorph.push / TrackMorph.flush"""
    fs, fft = 16000, 512
    lanes = [_lane(fs, fft, 3, rows=n, delay=5) for n in (2, 6, 30)]
    h = _new(env, fs, fft, 3)
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
    for i, (ln, r) in enumerate(zip(lanes, res)):
        n = len(ln["pos"])
        o = dict(w=np.full(n, 0.25), wf=np.full(n, 0.75), **{key: np.concatenate(got[i][q] + [r[q]]) for q, key in enumerate(("f0", "sp", "ap"))})
        _equal(o, _whole(env, fs, fft, ln, o, False), n)
    with pytest.raises(env[0].WorldClassError):  # ended: rows are refused until the next reset
        h.push([tuple(v[:1] for v in lanes[0]["voice"])] + [tuple(v[:0] for v in lanes[0]["voice"])] * 2, [np.zeros(1), np.zeros(0), np.zeros(0)])
    with pytest.raises(env[0].WorldClassError):
        h.flush([lanes[0]["tail"], None, None])
    h.close()
    h.close()


# ---- 5. a stream reused on the other track ------------------------------------------------------------------------------------

def test_a_stream_is_reused_after_reset_onto_the_other_track(env):
    """stream 3 of a handle that has run the five is attached again, at delay 5, and takes twelve rows of NaN: every one of its ten
    ring slots holds NaN.  Reset onto slot 0 (m = 1) at delay 3 it runs 40 rows of its voice: no stale row shows, the frames are
    those of the whole call on that track"""
    w, codec, wio, torch = env
    fs, fft = 16000, 512
    bins = fft // 2 + 1
    h = _new(env, fs, fft, 5)
    first = _drive(env, fs, fft, _lanes(fs, fft), handle=h)
    _equal(first[3], [_five(env, fs, fft, False)[3][key] for key in ("f0", "sp", "ap")], "first")

    def poison(h):
        h.reset(3, 1, 5)
        nan = [torch.full((6 * wd,), np.nan, dtype=torch.float64, device="cuda") for wd in (1, bins, bins)]
        outs = [_guarded(torch, 6, wd) for wd in (1, bins, bins)]
        assert h.push_device([0, 0, 0, 6, 0], *nan, torch.zeros(6, dtype=torch.float64, device="cuda"), *outs) == [0, 0, 0, 1, 0]
        assert h.push_device([0, 0, 0, 6, 0], *nan, torch.zeros(6, dtype=torch.float64, device="cuda"), *outs) == [0, 0, 0, 6, 0]
        w.lib().wc_synchronize()
        assert h.pending(3) == 5 and bool(torch.isnan(outs[1][:6 * bins]).all())

    ln = _lane(fs, fft, 3, rows=40, slot=0, delay=3)
    o = _drive(env, fs, fft, [None, None, None, ln, None], handle=h, pre=poison)[3]
    want = _whole(env, fs, fft, ln, o, False)
    _equal(o, want, "reused")
    assert _same(np.isnan(o["sp"]).any(axis=1), ~np.isfinite(_used(ln)))


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------

def _refused(w, fn, *args):
    with pytest.raises(w.WorldClassError) as e:
        fn(*args)
    assert "error -1:" in str(e.value), str(e.value)


def test_refusals_leave_everything_as_it_was(env):
    w, codec, wio, torch = env
    from world_class_amd.stream import TrackMorph, _lib
    fs, fft = 16000, 1024
    bins = fft // 2 + 1
    nan, inf = float("nan"), float("inf")
    L = _lib()
    src = _voice(fs, fft, 1)

    def state(h):
        return [(h.frames_received(u), h.frames_formed(u), h.pending(u), h.get_delay(u)) for u in range(5)] + [h.track_length(t) for t in (0, 1)]

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
        _refused(w, push, at(0, 2), d_in, None)             # ... with positions to read (delay 0: both rows form frames) ...
        _refused(w, push, at(0, 2), d_in, d_pos, [None] * 3)  # ... and with frames to write
        _refused(w, lambda: w._check(L.wc_track_morph_push_device(h._h, None, None, None, None, None, None, None, None, (C.c_int * 5)())))
        _refused(w, lambda: w._check(L.wc_track_morph_push_device(h._h, (C.c_int * 5)(), None, None, None, None, None, None, None, None)))
        _refused(w, flush, at(0, 1))                        # no delay
        _refused(w, flush, at(4, 1))                        # not attached
        if k == 0:
            _refused(w, flush, at(2, 1))                    # no rows
            h.set_track(1, *_tracks(fs, fft)[1])            # (no stream has rows yet: allowed, and the same rows)
        else:
            _refused(w, flush, at(2, 1), None)              # NULL tail / outputs with frames to form
            _refused(w, flush, at(2, 1), d_pos, [None] * 3)
            _refused(w, h.set_track_device, 1, 40, *[_dev(torch, v) for v in _tracks(fs, fft)[1]])  # streams with rows are attached
        _refused(w, lambda: w._check(L.wc_track_morph_flush_device(h._h, None, None, None, None, None, (C.c_int * 5)())))
        d_t = [_dev(torch, v) for v in _tracks(fs, fft)[1]]
        for bad in ((-1, 1), (2, 1), (0, 0), (0, 41)):      # a bad slot, m out of range
            _refused(w, h.set_track_device, bad[0], bad[1], *d_t)
        _refused(w, h.set_track_device, 0, 1, d_t[0], None, d_t[2])
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

    h = _new(env, fs, fft, 5)
    got = _drive(env, fs, fft, _lanes(fs, fft), ratios=True, handle=h, hook=hook)
    want = _five(env, fs, fft, True)
    for u in range(4):  # (the refused setters kept the settings of the drive, the refused pushes the ring)
        for key in ("f0", "sp", "ap"):
            assert _same(got[u][key], want[u][key]), (u, key)
    # create, and a reset onto a slot that has not been set
    for bad in ((fs, 1000, 1, 1, 4, 2, 1), (0, fft, 1, 1, 4, 2, 1), (fs, fft, 0, 1, 4, 2, 1), (fs, fft, 1, 0, 4, 2, 1), (fs, fft, 1, 1, 0, 2, 1),
                (fs, fft, 1, 1, 4, 0, 1), (fs, fft, 1, 1, 4, 2, -1)):
        with pytest.raises(w.WorldClassError):
            TrackMorph(*bad)
    g = TrackMorph(fs, fft, 1, 2, 4, 2, 0)  # max_delay = 0: no ring
    _refused(w, g.reset, 0, 1, 0)
    g.set_track(1, *[v[:3] for v in _tracks(fs, fft)[1]])
    _refused(w, g.reset, 0, 0, 0)
    _refused(w, g.reset, 0, 1, 1)
    g.reset(0, 1, 0)
    a = _voice(fs, fft, 0)
    res = g.push([tuple(v[:2] for v in a)], [np.array([0.0, 1.5])])  # weight 0 after the reset: the voice's rows as they are
    assert _same(res[0][0], a[0][:2]) and _same(res[0][1], a[1][:2]) and _same(res[0][2], a[2][:2]) and g.pending(0) == 0
    g.close()


# ---- 7. ordering on the caller's stream ---------------------------------------------------------------------------------------

def test_calls_are_ordered_on_the_callers_stream(env):
    """a long torch kernel in front on a torch stream handed over by wc_set_stream, the rows and the positions written by torch
    kernels on that stream, no synchronisation before the calls: the first two pushes return while the kernel in front still runs
    (the staging is a pair), and every call reads its rows and its positions behind it; one synchronisation at the end"""
    w, codec, wio, torch = env
    fs, fft = 16000, 1024
    bins = fft // 2 + 1
    ln = _lane(fs, fft, 2, cutting="sixes", rows=24)
    h, warm = _new(env, fs, fft, 1), _new(env, fs, fft, 1)
    warm.reset(0, 1, 0)
    warm.push([tuple(v[:2] for v in ln["voice"])], [np.zeros(2)])  # (the kernel's code is on the device before the clock matters)
    h.reset(0, ln["slot"], ln["delay"])
    host = [torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64).ravel().copy()).pin_memory() for v in ln["voice"] + (ln["pos"], ln["tail"])]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert w.lib().wc_set_stream(s.cuda_stream) == 0
    sets = []
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
                    ins = [t[off * wd:(off + c) * wd] for t, wd in zip(dev[:4], (1, bins, bins, 1))]
                    assert h.push_device([c], *ins, *o) == [m]
                    sim.push(c)
                    off += c
                running.append(not done.query())
                outs.append((o, m))
                sets += [st] * m
        s.synchronize()  # once
    finally:
        assert w.lib().wc_set_stream(None) == 0
    assert running[0] and running[1], running
    got = [np.concatenate([_rows(o[q], m, wd) for o, m in outs]) for q, wd in enumerate((1, bins, bins))]
    o = dict(f0=got[0][:, 0], sp=got[1], ap=got[2], w=np.array([t[0] for t in sets]), wf=np.array([t[1] for t in sets]))
    _equal(o, _whole(env, fs, fft, ln, o, False), "side stream")


# ---- 8. the live chain --------------------------------------------------------------------------------------------------------

def test_coded_rows_through_alignment_into_the_morph_and_a_synthesis_stream(env):
    """fft 1024.  Every push: the new rows are coded on the device (wc_code_features_device), an alignment stream with lag 3 writes
    d_settled (wc_align_stream_push_settled_device), the track morph with delay 3 reads it where it lies, a synthesis stream takes
    the frames -- nothing is downloaded between the three.  At the end tail_device -> flush_device.  The frames equal
    wc_morph_parameters_device at the settled and tail values read back afterwards; the samples equal the batch Synthesis of those
    frames bit for bit (fft 1024: no FP64 atomics, the bound of tests/test_gpu_morph_stream.py for this comparison)."""
    w, codec, wio, torch = env
    from oracle.gen_golden import synth_params
    from world_class_amd.stream import AlignStream, StreamSynthesizer, TrackMorph
    fs, fft, nd, lag, n, m = 24000, 1024, 40, 3, 30, 40
    bins = fft // 2 + 1
    track = synth_params(fs, fft, m, 8101)
    at = (np.arange(n) * 1.2).astype(np.int64)  # the voice runs through the track 1.2 times as fast, a little louder and higher
    voice = (track[0][at] * 1.1, track[1][at] * 1.21, track[2][at].copy())
    d_track, d_voice = [_dev(torch, v) for v in track], [_dev(torch, v) for v in voice]
    new = lambda k, fill=np.nan: torch.full((k,), fill, dtype=torch.float64, device="cuda")
    d_ctrack, d_coded = new(m * nd), new(MAXF * nd)
    codec.code_features_device(fs, fft, m, nd, d_track[1], None, d_ctrack, None)
    al = AlignStream(nd, 1, 1, m, MAXF)
    al.reserve_lag(lag)
    al.set_track_device(0, m, d_ctrack)
    al.reset(0, 0)
    al.set_lag(0, lag)
    h = TrackMorph(fs, fft, 1, 1, m, MAXF, lag)
    h.set_track_device(0, m, *d_track)
    h.reset(0, 0, lag)
    h.set_weight(0, 0.5, 0.25)
    syn = StreamSynthesizer(fs, fft, 5.0, 1, MAXF)
    d_pos, d_cost, d_settled, d_tail = new(n + 1), new(n + 1), new(n + 1), new(lag + 2)
    frames, y, off = [], [], 0

    def synthesise(counts, o, flush):
        c = syn.push_device(counts, *o, flush=[flush])
        w.lib().wc_synchronize()
        y.append(syn._d_y.to_host()[:c[0]].copy())

    for c in _cuts(n, 1, "cycle"):
        rows = [t[off * wd:(off + c) * wd] for t, wd in zip(d_voice, (1, bins, bins))]
        if c:
            codec.code_features_device(fs, fft, c, nd, rows[1], None, d_coded, None)
        al.push_settled_device([c], d_coded, d_pos[off:], d_cost[off:], d_settled[off:])
        want = max(off + c - lag, 0) - max(off - lag, 0)
        o = [_guarded(torch, want, 1), _guarded(torch, want, bins), _guarded(torch, want, bins)]
        assert h.push_device([c], *rows, d_settled[off:], *o) == [want]
        synthesise([want], o, 0)
        frames.append((o, want))
        off += c
    al.tail_device([1], d_tail)
    o = [_guarded(torch, lag, 1), _guarded(torch, lag, bins), _guarded(torch, lag, bins)]
    assert h.flush_device([1], d_tail, *o) == [lag]
    synthesise([lag], o, 1)
    frames.append((o, lag))
    settled, tail = d_settled.cpu().numpy(), d_tail.cpu().numpy()
    assert np.isnan(settled[n]) and np.isnan(tail[lag + 1]) and np.isfinite(settled[:n]).all() and np.isfinite(tail[:lag + 1]).all()
    used = tm.consumed(settled[:n], tail[:lag + 1], lag)
    assert (used * 2 == np.floor(used * 2)).all() and used.min() >= 0 and used.max() <= m - 1 and len(set(used)) > 5
    got = [np.concatenate([_rows(f[q], c, wd) for f, c in frames]) for q, wd in enumerate((1, bins, bins))]
    d = dict(a_lengths=[n], b_lengths=[m], out_lengths=[n], a=voice, b=track, pos_a=np.arange(n, dtype=np.float64), pos_b=used, weight=np.full(n, 0.5),
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
    print("track morph chain through a synthesis stream against the batch call: %.3e" % np.abs(y - ref[:-1]).max())
    assert np.array_equal(y, ref[:-1])
