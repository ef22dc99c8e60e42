"""-m gpu: voice morphing (wc_morph_parameters_device, wc_synthesis_compute_coded_morphed_device): the rows and the contour against
the numpy restatement of the rule (tests/morph_rule.py), the weights 0 and 1 and the spectral ratios against
wc_retime_parameters_device, the independence of the frames, NULL triples and refusals, ordering on the caller's stream, the coded
Synthesis call against the four calls it stands for, and the whole chain against the reference.  Outputs are NaN-filled with a
guard row behind them that must stay NaN."""
import ctypes as C

import numpy as np
import pytest

import morph_rule as mr
import retime_rule as rr
from test_gpu_retime import ATOMIC_ABS, SIZES, Y_ABS, _coded_rows, _dev, _guarded, _retime, _rows, _same, env  # noqa: F401

pytestmark = pytest.mark.gpu
# the project's allowance for the log / exp of two math libraries (FUSED_REL, test_gpu_modify_frames.py); the numpy rule in float64
# sits 3.6e-15 from its long-double evaluation on these inputs (tests/test_morph_rule.py prints it)
LOG_EXP_REL = 1e-12


def _morph(env, fs, fft, d, ratio_a=None, ratio_b=None, parts=(True, True, True), **over):
    """wc_morph_parameters_device on the batch d (morph_rule.batch; `over` replaces entries) into NaN-filled, guarded outputs:
    (f0, sp, ap), None for a triple that was left out"""
    w, codec, wio, torch = env
    d = dict(d, **over)
    bins, m = fft // 2 + 1, int(sum(d["out_lengths"]))
    ina = [_dev(torch, a) if on else None for a, on in zip(d["a"], parts)]
    inb = [_dev(torch, a) if on else None for a, on in zip(d["b"], parts)]
    outs = [_guarded(torch, m, wd) if on else None for wd, on in zip((1, bins, bins), parts)]
    opt = lambda a: None if a is None else _dev(torch, a)
    torch.cuda.synchronize()
    wio.morph_parameters_device(fs, fft, d["a_lengths"], *ina, d["b_lengths"], *inb, d["out_lengths"], _dev(torch, d["pos_a"]), _dev(torch, d["pos_b"]),
                                _dev(torch, d["weight"]), opt(d["f0_weight"]), opt(ratio_a), opt(ratio_b), *outs)
    w.lib().wc_synchronize()
    got = [None if o is None else _rows(o, m, wd) for o, wd in zip(outs, (1, bins, bins))]
    return (None if got[0] is None else got[0][:, 0]), got[1], got[2]


def _retimed(env, fs, fft, d, side, ratio=None):
    """wc_retime_parameters_device of one source of the batch along its own positions"""
    return _retime(env, fs, fft, d[side + "_lengths"], *d[side], d["out_lengths"], d["pos_" + side], ratio=ratio)


def _rel(got, want):
    return float(np.abs(got / want - 1).max()) if got.size else 0.0


def _invalid(ratio, fft):
    with np.errstate(invalid="ignore"):
        return (ratio != 0) & ~(np.isfinite(ratio) & (ratio >= 2.0 / fft))


def _ratios_with_bad(fft, m, first, at):
    ratio = rr.cycled(fft, m, first)
    ratio[list(at)] = [-1.0, np.nan, np.inf, 1.0 / fft]
    return ratio


# ---- 1. rows and contour against the numpy restatement ----------------------------------------------------------------------

@pytest.mark.parametrize("k,fs,fft", [(k, fs, fft) for k, (fs, fft) in enumerate(SIZES)])
def test_frames_equal_the_rule(env, k, fs, fft):
    """bit for bit: the ap rows, every frame with w in {0, 1}, every F0 except between two voiced frames with wf not in {0, 1}, the
    NaN frames.  The other sp bins and F0 values go through log and exp: LOG_EXP_REL.  Every other size takes an F0 weight of its
    own, one of them not finite."""
    d = mr.batch(fs, fft, 1100 + fft, with_f0_weight=k % 2 == 1)
    o0, o1 = d["out_lengths"][0], d["out_lengths"][0] + d["out_lengths"][1]
    m = sum(d["out_lengths"])
    d["pos_a"][[4, o1 - 1]] = [np.nan, np.inf]
    d["pos_b"][40] = -np.inf
    d["weight"][[o0, o1 + 17]] = [np.inf, np.nan]
    bad = np.zeros(m, bool)
    bad[[4, o1 - 1, 40, o0, o1 + 17]] = True
    bad_f0 = bad.copy()
    if d["f0_weight"] is not None:
        d["f0_weight"][9] = np.nan
        bad_f0[9] = True
    want = mr.rule_of(d)
    got = _morph(env, fs, fft, d)
    assert bad.sum() == 5
    assert np.isnan(got[0][bad_f0]).all() and np.isfinite(got[0][~bad_f0]).all()
    for q in (1, 2):
        assert np.isnan(got[q][bad]).all() and np.isfinite(got[q][~bad]).all()
    assert _same(got[2], want[2])
    w = d["weight"]
    ends = (w == 0) | (w == 1)
    assert ends.sum() > 50 and _same(got[1][ends | bad], want[1][ends | bad])
    wf = w if d["f0_weight"] is None else d["f0_weight"]
    fa, fb = _retimed(env, fs, fft, d, "a")[0], _retimed(env, fs, fft, d, "b")[0]
    with np.errstate(invalid="ignore"):
        glide = ~bad_f0 & (fa != 0) & (fb != 0) & (wf != 0) & (wf != 1)
    assert glide.sum() > 50 and (~glide & ~bad_f0).sum() > 50
    assert _same(got[0][~glide], want[0][~glide])
    assert (got[0][~bad_f0] == 0).any() and (got[0][~bad_f0] > 0).any()
    e_sp, e_f0 = _rel(got[1][~ends & ~bad], want[1][~ends & ~bad]), _rel(got[0][glide], want[0][glide])
    print("morph against the numpy rule, fs %d fft %d: sp %.3e, F0 %.3e (relative)" % (fs, fft, e_sp, e_f0))
    assert e_sp < LOG_EXP_REL and e_f0 < LOG_EXP_REL


# ---- 2. / 3. the spectral ratios --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,fs,fft", [(k, fs, fft) for k, (fs, fft) in enumerate(SIZES)])
def test_weights_zero_and_one_with_ratios_equal_retime_bit_for_bit(env, k, fs, fft):
    """w == 0 is wc_retime_parameters_device of A with d_ratio_a, w == 1 that of B with d_ratio_b: the eight ratios of
    retime_rule.ratios_of cycled, four bad ones in each array; a bad ratio of the OTHER source makes the sp row NaN as well"""
    d = mr.batch(fs, fft, 2100 + fft)
    m = sum(d["out_lengths"])
    ra, rb = _ratios_with_bad(fft, m, 2, (3, 50, 101, m - 1)), _ratios_with_bad(fft, m, 5, (7, 50, 160, m - 2))
    inv_a, inv_b = _invalid(ra, fft), _invalid(rb, fft)
    assert inv_a.sum() == 4 and inv_b.sum() == 4
    for side, weight, ratio, other in (("a", 0.0, ra, inv_b), ("b", 1.0, rb, inv_a)):
        want = _retimed(env, fs, fft, d, side, ratio)
        got = _morph(env, fs, fft, d, ra, rb, weight=np.full(m, weight))
        assert _same(got[0], want[0]) and _same(got[2], want[2])
        assert _same(got[1][~other], want[1][~other]) and np.isnan(got[1][other]).all()
        assert np.isnan(want[1]).all(axis=1).sum() == 4 and np.isfinite(want[1][~np.isnan(want[1]).all(axis=1)]).all()
        # either array alone: the other source's rows are not stretched, and cannot spoil a frame
        alone = _morph(env, fs, fft, d, ra if side == "a" else None, rb if side == "b" else None, weight=np.full(m, weight))
        assert _same(alone[1], want[1])


@pytest.mark.parametrize("k,fs,fft", [(k, fs, fft) for k, (fs, fft) in enumerate(SIZES)])
def test_ratios_at_other_weights_equal_the_routed_composition(env, k, fs, fft):
    """retime A with d_ratio_a and B with d_ratio_b on the device, then the numpy blend of those rows: LOG_EXP_REL (beside the two
    math libraries only one exp -> log round trip per source: one rounding in the log domain, which weights in [-0.5, 1.5] amplify
    at most twice).  A frame with an invalid ratio in either array has a NaN sp row, finite ap and F0."""
    d = mr.batch(fs, fft, 3100 + fft, with_f0_weight=k % 2 == 0)
    m = sum(d["out_lengths"])
    ra, rb = _ratios_with_bad(fft, m, 1, (5, 66, 130, m - 3)), _ratios_with_bad(fft, m, 4, (2, 66, 200, m - 1))
    rb[7::16] = 0.0  # (where A's cycle holds a 0 too: frames without a ratio on either side, at the middle weight)
    inv = _invalid(ra, fft) | _invalid(rb, fft)
    assert inv.sum() == 7
    spa, spb = _retimed(env, fs, fft, d, "a", ra)[1], _retimed(env, fs, fft, d, "b", rb)[1]
    plain = _morph(env, fs, fft, d)
    got = _morph(env, fs, fft, d, ra, rb)
    assert _same(got[0], plain[0]) and _same(got[2], plain[2]) and np.isfinite(got[0]).all() and np.isfinite(got[2]).all()
    assert np.isnan(got[1][inv]).all() and np.isfinite(got[1][~inv]).all()
    w = d["weight"]
    assert _same(got[1][(w == 0) & ~inv], spa[(w == 0) & ~inv]) and _same(got[1][(w == 1) & ~inv], spb[(w == 1) & ~inv])
    mid = (w != 0) & (w != 1) & ~inv
    wm = w[mid][:, None]
    want = np.exp((1.0 - wm) * np.log(spa[mid]) + wm * np.log(spb[mid]))
    err = _rel(got[1][mid], want)
    print("morph with ratios against the routed composition, fs %d fft %d: %.3e (relative)" % (fs, fft, err))
    assert err < LOG_EXP_REL
    both0 = mid & (ra == 0) & (rb == 0)
    assert both0.any() and _same(got[1][both0], plain[1][both0])  # (a ratio of 0 on both sides: the frame without ratios)
    moved = mid & (ra == 1.2)
    assert np.abs(got[1][moved] / plain[1][moved] - 1).max() > 1e-3  # (the stretch does change rows)


# ---- 4. a frame depends on its own values and its source rows alone ---------------------------------------------------------

def _one_pair(fs, fft, seed):
    from oracle.gen_golden import synth_params
    na, nb = 97, 74
    pos_a = rr.map_of("hold_and_back", na)
    m = len(pos_a)
    return dict(a_lengths=[na], b_lengths=[nb], out_lengths=[m], a=synth_params(fs, fft, na, seed), b=synth_params(fs, fft, nb, seed + 1), pos_a=pos_a,
                pos_b=mr.to_length(rr.map_of("slow_1.37", nb), m), weight=mr.cycled_weights(m, 2), f0_weight=mr.cycled_weights(m, 6))


def _frames(d, idx):
    """the batch d (one pair) reduced to the output frames idx"""
    return dict(d, out_lengths=[len(idx)], **{k: d[k][idx] for k in ("pos_a", "pos_b", "weight", "f0_weight")})


@pytest.mark.parametrize("fs,fft", SIZES)
def test_frames_depend_on_their_own_values_alone(env, fs, fft):
    d = _one_pair(fs, fft, 4100)
    m = d["out_lengths"][0]
    d["pos_a"][7], d["weight"][60] = np.nan, np.inf
    ra, rb = _ratios_with_bad(fft, m, 0, (3, 50, 101, m - 1)), _ratios_with_bad(fft, m, 3, (9, 50, 120, m - 2))
    base = _morph(env, fs, fft, d, ra, rb)
    idx = np.arange(m)[::-1]
    rev = _morph(env, fs, fft, _frames(d, idx), ra[idx], rb[idx])
    for b, r in zip(base, rev):
        assert _same(r, b[::-1])
    for k in (0, 1, 2, 7, 29, 30, 49, 50, 60, 63, 64, m - 2, m - 1):
        one = _morph(env, fs, fft, _frames(d, np.array([k])), ra[k:k + 1], rb[k:k + 1])
        for b, o in zip(base, one):
            assert _same(o[0], b[k]), k
    # one frame's weight, position and ratio changed: that output frame changes, no other does
    for k, key, value in ((20, "weight", 0.3), (33, "pos_a", 11.5), (34, "pos_b", 2.25), (44, "f0_weight", 0.9)):
        v = d[key].copy()
        v[k] = value
        got = _morph(env, fs, fft, d, ra, rb, **{key: v})
        keep = np.arange(m) != k
        for q, (b, g) in enumerate(zip(base, got)):
            assert _same(g[keep], b[keep]), (key, q)
        changed = [not _same(g[k:k + 1], b[k:k + 1]) for b, g in zip(base, got)]
        if key == "f0_weight":  # (A voiced, B not: the contour leaves A's F0 for 0; the rows do not look at this weight)
            assert changed == [True, False, False]
        elif key == "weight":  # (the stream has an F0 weight of its own: the contour does not look at this one)
            assert changed == [False, True, True]
        else:
            assert changed[1] and changed[2], key
    r2 = rb.copy()
    r2[21] = 1.2 if rb[21] != 1.2 else 0.8
    got = _morph(env, fs, fft, d, ra, r2)
    keep = np.arange(m) != 21
    assert _same(got[1][keep], base[1][keep]) and not _same(got[1][21], base[1][21])
    assert _same(got[0], base[0]) and _same(got[2], base[2])
    # the pair embedded between two others
    from oracle.gen_golden import synth_params
    xa, xb = synth_params(fs, fft, 50, 4200), synth_params(fs, fft, 45, 4300)
    pre, post = rr.map_of("slow_1.37", 40), rr.map_of("speed_1.5", 45)
    cat = lambda *v: np.concatenate(v)
    emb = dict(a_lengths=[40, 97, 10], b_lengths=[1, 74, 44], out_lengths=[len(pre), m, len(post)],
               a=tuple(cat(x[:40], s, x[40:]) for x, s in zip(xa, d["a"])), b=tuple(cat(x[:1], s, x[1:]) for x, s in zip(xb, d["b"])),
               pos_a=cat(pre, d["pos_a"], np.minimum(post, 9)), pos_b=cat(pre, d["pos_b"], post[::-1]),
               weight=cat(mr.cycled_weights(len(pre)), d["weight"], mr.cycled_weights(len(post), 4)),
               f0_weight=cat(mr.cycled_weights(len(pre), 1), d["f0_weight"], mr.cycled_weights(len(post), 5)))
    got = _morph(env, fs, fft, emb, cat(rr.cycled(fft, len(pre)), ra, rr.cycled(fft, len(post), 5)), cat(rr.cycled(fft, len(pre), 3), rb, rr.cycled(fft, len(post), 1)))
    for b, e in zip(base, got):
        assert _same(e[len(pre):len(pre) + m], b)
    # pair 0 of the embedding has a single frame of B, held at every position: its rows are that frame's
    first = _morph(env, fs, fft, dict(emb, weight=np.ones(len(pre) + m + len(post))))
    assert all(np.array_equal(r, xb[1][0]) for r in first[1][:len(pre)]) and all(np.array_equal(r, xb[2][0]) for r in first[2][:len(pre)])


@pytest.mark.parametrize("fs,fft", SIZES)
def test_a_source_of_one_frame_is_held(env, fs, fft):
    """pairs whose A has a single frame (B has 74 frames, then one as well): that frame is held at every position.  w = 0 writes it
    into every output frame bit for bit, also stretched by a ratio as wc_retime_parameters_device stretches it; other weights
    blend against the held row as the numpy rule does"""
    from oracle.gen_golden import synth_params
    xa, xb = tuple(v[[3, 5]] for v in synth_params(fs, fft, 8, 4400)), synth_params(fs, fft, 75, 4500)  # (B's last frame, the single one of pair 1, is unvoiced)
    m0, m1 = 24, 16
    m = m0 + m1
    d = dict(a_lengths=[1, 1], b_lengths=[74, 1], out_lengths=[m0, m1], a=xa, b=xb,
             pos_a=np.concatenate([np.linspace(-2.0, 3.5, m0), np.arange(m1) * 0.25]),
             pos_b=np.concatenate([np.linspace(0.0, 73.0, m0), np.linspace(5.0, -1.0, m1)]), weight=mr.cycled_weights(m), f0_weight=None)
    held = np.repeat(np.arange(2), [m0, m1])  # the frame of A every output frame holds
    zero = _morph(env, fs, fft, d, weight=np.zeros(m))
    assert np.array_equal(zero[0], xa[0][held]) and np.array_equal(zero[1], xa[1][held]) and np.array_equal(zero[2], xa[2][held])
    ra = rr.cycled(fft, m, 1)
    stretched = _morph(env, fs, fft, d, ra, weight=np.zeros(m))
    want = _retimed(env, fs, fft, d, "a", ra)
    for g, w_ in zip(stretched, want):
        assert _same(g, w_)
    assert np.isfinite(want[1]).all() and np.abs(want[1][ra == 1.2] / zero[1][ra == 1.2] - 1).max() > 1e-3
    got, rule = _morph(env, fs, fft, d), mr.rule_of(d)
    w = d["weight"]
    ends = (w == 0) | (w == 1)
    assert _same(got[2], rule[2]) and _same(got[1][ends], rule[1][ends])
    assert np.array_equal(got[2][~ends], (1.0 - w[~ends])[:, None] * xa[2][held][~ends] + w[~ends][:, None] * rule_b_rows(d, 2)[~ends])
    e_sp = _rel(got[1][~ends], rule[1][~ends])
    both = (xa[0][held] != 0) & (rule_b_rows(d, 0) != 0) & ~ends
    assert _same(got[0][~both], rule[0][~both]) and _rel(got[0][both], rule[0][both]) < LOG_EXP_REL
    print("morph against a held single frame, fs %d fft %d: sp %.3e (relative)" % (fs, fft, e_sp))
    assert e_sp < LOG_EXP_REL
    # the last pair holds one frame on both sides: every frame with w = 1 is B's single frame
    assert all(np.array_equal(r, xb[1][74]) for r in got[1][m0:][w[m0:] == 1]) and (w[m0:] == 1).sum() == 2


def rule_b_rows(d, q):
    """what retime_rule forms from B along pos_b: F0 (q = 0), sp (1) or ap (2)"""
    return rr.retime_batch(d["b_lengths"], *d["b"], d["out_lengths"], d["pos_b"])[q]


@pytest.mark.parametrize("fs,fft", SIZES)
def test_null_triples_and_empty_calls(env, fs, fft):
    w, codec, wio, torch = env
    d = mr.batch(fs, fft, 5100, with_f0_weight=True)
    m = sum(d["out_lengths"])
    ra, rb = rr.cycled(fft, m, 1), rr.cycled(fft, m, 6)
    full = _morph(env, fs, fft, d, ra, rb)
    for parts in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        got = _morph(env, fs, fft, d, ra, rb, parts=parts)
        for on, g, f in zip(parts, got, full):
            assert (g is None) if not on else _same(g, f)
    # a pair without output frames in the middle (its sources may be empty too), and calls without any
    al, bl, ol = d["a_lengths"], d["b_lengths"], d["out_lengths"]
    ins = lambda v, at, k: tuple(np.concatenate([x[:at], np.ones((k,) + x.shape[1:]), x[at:]]) for x in v)
    holes = dict(d, a_lengths=[al[0], 0, al[1], 5, al[2]], b_lengths=[bl[0], 3, bl[1], 0, bl[2]], out_lengths=[ol[0], 0, ol[1], 0, ol[2]],
                 a=ins(d["a"], al[0] + al[1], 5), b=ins(d["b"], bl[0], 3))
    for h, f in zip(_morph(env, fs, fft, holes, ra, rb), full):
        assert _same(h, f)
    none = _morph(env, fs, fft, dict(d, out_lengths=[0, 0, 0], pos_a=np.zeros(1), pos_b=np.zeros(1), weight=np.zeros(1), f0_weight=None))
    assert all(len(a) == 0 for a in none)
    empty = _morph(env, fs, fft, dict(d, a_lengths=[], b_lengths=[], out_lengths=[], pos_a=np.zeros(1), pos_b=np.zeros(1), weight=np.zeros(1), f0_weight=None))
    assert all(len(a) == 0 for a in empty)
    # all three triples NULL: accepted, nothing to do
    wio.morph_parameters_device(fs, fft, al, None, None, None, bl, None, None, None, ol, _dev(torch, d["pos_a"]), _dev(torch, d["pos_b"]), _dev(torch, d["weight"]))


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fs,fft", SIZES)
def test_refused_calls_leave_the_outputs_untouched(env, fs, fft):
    w, codec, wio, torch = env
    from oracle.gen_golden import synth_params
    L = w.lib()
    na, nb, m = 8, 6, 11
    bins = fft // 2 + 1
    a, b = synth_params(fs, fft, na, 6200), synth_params(fs, fft, nb, 6300)
    da, db = [_dev(torch, v) for v in a], [_dev(torch, v) for v in b]
    d_pa, d_pb, d_w = _dev(torch, np.linspace(0, na - 1, m)), _dev(torch, np.linspace(nb - 1, 0, m)), _dev(torch, mr.cycled_weights(m, 2))
    d_one = _dev(torch, np.ones(m))
    o_f0, o_sp, o_ap = _guarded(torch, m, 1), _guarded(torch, m, bins), _guarded(torch, m, bins)
    torch.cuda.synchronize()
    good = dict(fs=fs, fft=fft, n=1, al=[na], f0a=da[0], spa=da[1], apa=da[2], bl=[nb], f0b=db[0], spb=db[1], apb=db[2], ol=[m], pa=d_pa, pb=d_pb, w=d_w,
                of0=o_f0, osp=o_sp, oap=o_ap)
    ints = lambda v: None if v is None else (C.c_int * max(1, len(v)))(*v)
    ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.data_ptr())

    def call(**kw):
        g = dict(good, **kw)
        return wio._io().wc_morph_parameters_device(g["fs"], g["fft"], g["n"], ints(g["al"]), ptr(g["f0a"]), ptr(g["spa"]), ptr(g["apa"]), ints(g["bl"]),
                                                    ptr(g["f0b"]), ptr(g["spb"]), ptr(g["apb"]), ints(g["ol"]), ptr(g["pa"]), ptr(g["pb"]), ptr(g["w"]),
                                                    d_one.data_ptr(), d_one.data_ptr(), d_one.data_ptr(), ptr(g["of0"]), ptr(g["osp"]), ptr(g["oap"]))

    big = 0x7fffffff
    bad = [dict(fft=3000), dict(fft=8192), dict(fft=256), dict(fs=0), dict(fs=-48000), dict(n=-1), dict(al=[0]), dict(bl=[0]), dict(al=[-1]), dict(bl=[-1]),
           dict(ol=[-1]), dict(n=2, al=[na, 0], bl=[nb, 1], ol=[m, 1]), dict(n=2, al=[na, 1], bl=[nb, 0], ol=[m, 1]),
           dict(n=3, al=[na, na, na], bl=[nb, nb, nb], ol=[big, big, 2]), dict(n=3, al=[big, big, 2], bl=[nb, nb, nb], ol=[m, 0, 0]),
           dict(n=3, al=[na, na, na], bl=[big, big, 2], ol=[m, 0, 0]), dict(al=None), dict(bl=None), dict(ol=None), dict(pa=None), dict(pb=None), dict(w=None),
           dict(f0a=None), dict(f0b=None), dict(of0=None), dict(f0a=None, f0b=None), dict(f0a=None, of0=None), dict(spa=None), dict(spb=None), dict(osp=None),
           dict(spb=None, osp=None), dict(apa=None), dict(apb=None), dict(oap=None), dict(apa=None, apb=None),
           dict(of0=da[0]), dict(of0=db[0]), dict(osp=da[1]), dict(osp=db[1]), dict(oap=da[2]), dict(oap=db[2])]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert w.last_error(), kw
    L.wc_synchronize()
    assert bool(torch.isnan(o_f0).all()) and bool(torch.isnan(o_sp).all()) and bool(torch.isnan(o_ap).all())
    assert np.array_equal(da[0].cpu().numpy(), a[0]) and np.array_equal(db[1].cpu().numpy().reshape(nb, bins), b[1])
    with pytest.raises(w.WorldClassError):
        wio.morph_parameters_device(fs, 3000, [na], *da, [nb], *db, [m], d_pa, d_pb, d_w, None, None, None, o_f0, o_sp, o_ap)
    with pytest.raises(ValueError):
        wio.morph_parameters_device(fs, fft, [na, na], *da, [nb], *db, [m], d_pa, d_pb, d_w, None, None, None, o_f0, o_sp, o_ap)
    assert call() == 0  # (the same arguments, nothing wrong: accepted)
    L.wc_synchronize()
    assert np.isfinite(_rows(o_sp, m, bins)).all()

    # the coded Synthesis call: its own refusals and those of the calls it stands for; rng_pos and d_out stay
    nd = 20
    from oracle import port_codec as pc
    ca = [_dev(torch, pc.code_spectral_envelope(a[1], fs, fft, nd)), _dev(torch, pc.code_aperiodicity(a[2], fs, fft))]
    cb = [_dev(torch, pc.code_spectral_envelope(b[1], fs, fft, nd)), _dev(torch, pc.code_aperiodicity(b[2], fs, fft))]
    syn, syn8 = w.Synthesis(fs, fft, 5.0), w.Synthesis(8000, 1024, 5.0)
    ol = [syn.out_length(m)]
    y = torch.full((ol[0],), np.nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g2 = dict(h=syn, n=1, f0a=da[0], al=[na], cspa=ca[0], capa=ca[1], f0b=db[0], bl=[nb], cspb=cb[0], capb=cb[1], nd=nd, fo=[m], pa=d_pa, pb=d_pb, w=d_w, ol=ol,
              y=y)
    for kw in (dict(nd=0), dict(nd=fft // 2 + 1), dict(h=syn8), dict(cspa=None), dict(capa=None), dict(cspb=None), dict(capb=None), dict(f0a=None),
               dict(f0b=None), dict(al=None), dict(bl=None), dict(fo=None), dict(pa=None), dict(pb=None), dict(w=None), dict(ol=None), dict(y=None), dict(n=0),
               dict(al=[1]), dict(bl=[1]), dict(fo=[1]), dict(fo=[0]), dict(fo=[-3]), dict(ol=[-1])):
        g = dict(g2, **kw)
        rng = (C.c_uint64 * 1)(5)
        rc = L.wc_synthesis_compute_coded_morphed_device(g["h"]._h, g["n"], ptr(g["f0a"]), ints(g["al"]), ptr(g["cspa"]), ptr(g["capa"]), ptr(g["f0b"]),
                                                         ints(g["bl"]), ptr(g["cspb"]), ptr(g["capb"]), g["nd"], ints(g["fo"]), ptr(g["pa"]), ptr(g["pb"]),
                                                         ptr(g["w"]), d_one.data_ptr(), d_one.data_ptr(), d_one.data_ptr(), ints(g["ol"]), ptr(g["y"]), rng)
        assert rc == -1 and w.last_error(), kw
        assert list(rng) == [5], kw
    L.wc_synchronize()
    assert bool(torch.isnan(y).all())


# ---- 6. ordering on the caller's stream -------------------------------------------------------------------------------------

def test_morph_is_ordered_on_the_callers_stream(env):
    """a long torch kernel in front on a torch stream handed over by wc_set_stream; the rows and every per-frame array written by
    torch kernels on that stream, no synchronisation before the call; four (fs, fft) combinations interleaved, twice; one
    synchronisation at the end"""
    w, codec, wio, torch = env
    combos = [(48000, 2048), (24000, 1024), (16000, 512), (96000, 4096)]
    data, want = [], []
    for k, (fs, fft) in enumerate(combos):
        d = mr.batch(fs, fft, 7100 + fft, with_f0_weight=True)
        m = sum(d["out_lengths"])
        ra, rb = rr.cycled(fft, m, k), rr.cycled(fft, m, k + 3)
        data.append((d, d["a"] + d["b"] + (d["pos_a"], d["pos_b"], d["weight"], d["f0_weight"], ra, rb)))
        want.append(_morph(env, fs, fft, d, ra, rb))
    host = [tuple(torch.from_numpy(np.ascontiguousarray(a).ravel().copy()).pin_memory() for a in arrays) for _, arrays in data]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert w.lib().wc_set_stream(s.cuda_stream) == 0
    try:
        outs = []
        with torch.cuda.stream(s):
            junk = torch.randn(2048, 2048, device="cuda")
            for _ in range(20):  # a long-running kernel in front: the call must wait for it and for the uploads behind it
                junk = junk @ junk * 1e-3
            for rnd in range(2):
                for (fs, fft), (d, _), h in zip(combos, data, host):
                    bins, m = fft // 2 + 1, sum(d["out_lengths"])
                    t = [torch.zeros(len(a), dtype=torch.float64, device="cuda") for a in h]
                    o = [_guarded(torch, m, 1), _guarded(torch, m, bins), _guarded(torch, m, bins)]
                    for dst, src in zip(t, h):
                        dst.copy_(src, non_blocking=True)
                        dst.mul_(1.0)  # torch kernels on the stream write every input
                    wio.morph_parameters_device(fs, fft, d["a_lengths"], t[0], t[1], t[2], d["b_lengths"], t[3], t[4], t[5], d["out_lengths"], *t[6:12], *o)
                    outs.append((o, t))
        s.synchronize()  # once
    finally:
        assert w.lib().wc_set_stream(None) == 0
    for i, (o, _) in enumerate(outs):
        fft, m = combos[i % 4][1], sum(data[i % 4][0]["out_lengths"])
        got = (_rows(o[0], m, 1)[:, 0], _rows(o[1], m, fft // 2 + 1), _rows(o[2], m, fft // 2 + 1))
        for g, w_ in zip(got, want[i % 4]):
            assert _same(g, w_), i


# ---- 7. batch Synthesis from the coded rows of two voices -------------------------------------------------------------------

@pytest.mark.parametrize("fs,fft", [(24000, 1024), (48000, 2048), (16000, 512), (96000, 4096)])
def test_compute_coded_morphed_equals_decode_morph_synthesis(env, fs, fft):
    """compute_coded_morphed_device == decode_features_device twice -> morph_parameters_device -> compute_device with the same noise
    positions (bit for bit at fft 1024 / 2048, within ATOMIC_ABS at 512 / 4096, where Synthesis adds with FP64 atomics), ends at
    the same noise positions, and with w = 0, the identity map for A and no ratios it is compute_coded_device of A"""
    w, codec, wio, torch = env
    nd = 40
    d = mr.batch(fs, fft, 8100, with_f0_weight=True)
    al, bl, fo = d["a_lengths"], d["b_lengths"], d["out_lengths"]
    pa = [_coded_rows(env, fs, fft, n, 8100 + 2 * u, nd) for u, n in enumerate(al)]
    pb = [_coded_rows(env, fs, fft, n, 8101 + 2 * u, nd) for u, n in enumerate(bl)]
    f0a, cspa, capa = (np.concatenate([p[q] for p in pa]) for q in range(3))
    f0b, cspb, capb = (np.concatenate([p[q] for p in pb]) for q in range(3))
    m, ta, tb, bins = sum(fo), sum(al), sum(bl), fft // 2 + 1
    # ratios near 1, F0 weights within [0, 1]: the morphed contour stays within what the sources hold
    ra, rb = np.where(np.arange(m) % 7 < 2, 0.0, 1.1), np.linspace(0.85, 1.2, m)
    wf = np.clip(d["f0_weight"], 0.0, 1.0)
    same = (lambda x, y: np.array_equal(x, y)) if fft in (1024, 2048) else (lambda x, y: len(x) == len(y) and np.abs(x - y).max() < ATOMIC_ABS)
    syn = w.Synthesis(fs, fft, 5.0)
    start = [1000 * u + 7 for u in range(3)]
    t = {k: _dev(torch, v) for k, v in dict(f0a=f0a, cspa=cspa, capa=capa, f0b=f0b, cspb=cspb, capb=capb, pa=d["pos_a"], pb=d["pos_b"], w=d["weight"], wf=wf,
                                            ra=ra, rb=rb).items()}

    def run(ol, fn):
        y = torch.full((sum(ol) + 1,), np.nan, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        end = fn(y)
        w.lib().wc_synchronize()
        y = y.cpu().numpy()
        assert np.isnan(y[-1])
        return y[:-1], end

    ol = [syn.out_length(k) for k in fo]
    spa, apa = (torch.empty(ta * bins, dtype=torch.float64, device="cuda") for _ in range(2))
    spb, apb = (torch.empty(tb * bins, dtype=torch.float64, device="cuda") for _ in range(2))
    r_f0, r_sp, r_ap = _guarded(torch, m, 1), _guarded(torch, m, bins), _guarded(torch, m, bins)
    codec.decode_features_device(fs, fft, ta, nd, t["cspa"], t["capa"], spa, apa)
    codec.decode_features_device(fs, fft, tb, nd, t["cspb"], t["capb"], spb, apb)
    wio.morph_parameters_device(fs, fft, al, t["f0a"], spa, apa, bl, t["f0b"], spb, apb, fo, t["pa"], t["pb"], t["w"], t["wf"], t["ra"], t["rb"], r_f0, r_sp, r_ap)
    y_ref, end_ref = run(ol, lambda y: syn.compute_device(r_f0, fo, r_sp, r_ap, ol, y, rng_pos=start))
    morphed = lambda y, *per_frame: syn.compute_coded_morphed_device(t["f0a"], al, t["cspa"], t["capa"], t["f0b"], bl, t["cspb"], t["capb"], nd, fo, t["pa"],
                                                                     t["pb"], *per_frame, ol, y, rng_pos=start)
    y, end = run(ol, lambda y: morphed(y, t["w"], t["wf"], t["ra"], t["rb"]))
    assert end == end_ref and end != start
    assert np.isfinite(y).all() and same(y, y_ref)
    y_none, end_none = run(ol, lambda y: morphed(y, t["w"], None, None, None))
    assert np.isfinite(y_none).all() and np.abs(y - y_none).max() > 1e-6  # (F0 weight and ratios do change the waveform)
    # w = 0 along A's identity map: A alone
    ol1 = [syn.out_length(n) for n in al]
    d_id = _dev(torch, np.concatenate([np.arange(n, dtype=np.float64) for n in al]))
    d_zero = _dev(torch, np.zeros(ta))
    y_plain, end_plain = run(ol1, lambda y: syn.compute_coded_device(t["f0a"], al, t["cspa"], nd, t["capa"], ol1, y, rng_pos=start))
    y_id, end_id = run(ol1, lambda y: syn.compute_coded_morphed_device(t["f0a"], al, t["cspa"], t["capa"], t["f0b"], bl, t["cspb"], t["capb"], nd, al, d_id,
                                                                       d_zero, d_zero, None, None, None, ol1, y, rng_pos=start))
    assert end_id == end_plain and same(y_id, y_plain)
    assert np.isfinite(y_plain).all()
    # the first pair alone: 61 frames of A, an odd count, so B's decoded rows start 8 bytes off a 16-byte boundary in the scratch
    al_, bl_, fo_, ol_, m_ = al[:1], bl[:1], fo[:1], ol[:1], fo[0]
    assert sum(al_) % 2 == 1
    q_f0, q_sp, q_ap = _guarded(torch, m_, 1), _guarded(torch, m_, bins), _guarded(torch, m_, bins)
    codec.decode_features_device(fs, fft, al_[0], nd, t["cspa"], t["capa"], spa, apa)
    codec.decode_features_device(fs, fft, bl_[0], nd, t["cspb"], t["capb"], spb, apb)
    wio.morph_parameters_device(fs, fft, al_, t["f0a"], spa, apa, bl_, t["f0b"], spb, apb, fo_, t["pa"], t["pb"], t["w"], t["wf"], t["ra"], t["rb"], q_f0, q_sp, q_ap)
    y_ref1, end_ref1 = run(ol_, lambda y: syn.compute_device(q_f0, fo_, q_sp, q_ap, ol_, y, rng_pos=start[:1]))
    y1, end1 = run(ol_, lambda y: syn.compute_coded_morphed_device(t["f0a"], al_, t["cspa"], t["capa"], t["f0b"], bl_, t["cspb"], t["capb"], nd, fo_, t["pa"],
                                                                   t["pb"], t["w"], t["wf"], t["ra"], t["rb"], ol_, y, rng_pos=start[:1]))
    assert end1 == end_ref1 and np.isfinite(y1).all() and same(y1, y_ref1)
    assert same(y1, y[:ol_[0]])  # (and the pair does not depend on the pairs behind it)


# ---- 8. against the reference -----------------------------------------------------------------------------------------------

def reference_case(fs, fft, nd=60):
    """two voices of 120 frames of synth_params, coded and decoded by oracle/port_codec, morphed by the numpy restatement onto 120
    output frames: A along its identity map, B along a map that leaves its first ten frames in place (frame 5 holds the 600 Hz that
    keep the reference's pulse capacity safe) and then runs up to eight frames ahead; the weights of the shared cycle, the F0 weights
    three places on"""
    from oracle import port_codec as pc
    from oracle.gen_golden import synth_params
    n = 120
    srcs = []
    for seed in (6000 + fs // 1000, 6500 + fs // 1000):
        f0, sp, ap = synth_params(fs, fft, n, seed)
        csp, cap = pc.code_spectral_envelope(sp, fs, fft, nd), pc.code_aperiodicity(ap, fs, fft)
        srcs.append((f0, csp, cap, pc.decode_spectral_envelope(csp, fs, fft), pc.decode_aperiodicity(cap, fs, fft)))
    k = np.arange(n, dtype=np.float64)
    pos_a = k.copy()
    pos_b = np.where(k < 10, k, k + 8.0 * np.sin(np.pi * (k - 10) / 110.0) ** 2)
    weight, f0_weight = mr.cycled_weights(n), mr.cycled_weights(n, 3)
    a, b = srcs
    f0_m, sp_m, ap_m = mr.morph((a[0], a[3], a[4]), (b[0], b[3], b[4]), pos_a, pos_b, weight, f0_weight)
    return a[:3], b[:3], pos_a, pos_b, weight, f0_weight, f0_m, sp_m, ap_m


@pytest.mark.parametrize("fs,fft", [(16000, 1024), (48000, 2048)])
def test_compute_coded_morphed_matches_the_reference_chain(env, port, checker, fs, fft):
    """the reference's chain synthesised from noise position 0 by the reference (the real one where oracle/_ref is built,
    oracle/port.py otherwise): the device call on the coded rows of both voices within 1e-8, the project's Synthesis tolerance,
    with equal length and equal final noise position"""
    w, codec, wio, torch = env
    nd = 60
    a, b, pos_a, pos_b, weight, f0_weight, f0_m, sp_m, ap_m = reference_case(fs, fft, nd)
    n, m = len(a[0]), len(pos_a)
    assert m == 120 and np.isfinite(f0_m).all() and (f0_m == 0).any() and f0_m.max() > 599.0
    port.rng_seek(0)
    y_ref = port.synthesis(f0_m, sp_m, ap_m, fs, 5.0)
    end = port.rng_position()
    if checker is not None:
        y_ref = checker.stage_at(0, "synthesis", f0_m, sp_m, ap_m, fs, 5.0)
    assert np.isfinite(y_ref).all()
    syn = w.Synthesis(fs, fft, 5.0)
    ol = syn.out_length(m)
    assert ol == len(y_ref)
    y = torch.full((ol + 1,), np.nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    got_end = syn.compute_coded_morphed_device(_dev(torch, a[0]), [n], _dev(torch, a[1]), _dev(torch, a[2]), _dev(torch, b[0]), [n], _dev(torch, b[1]),
                                               _dev(torch, b[2]), nd, [m], _dev(torch, pos_a), _dev(torch, pos_b), _dev(torch, weight), _dev(torch, f0_weight),
                                               None, None, [ol], y, rng_pos=[0])
    w.lib().wc_synchronize()
    y = y.cpu().numpy()
    assert np.isnan(y[-1]) and got_end == [end]
    err = np.abs(y[:-1] - y_ref).max()
    print("compute_coded_morphed against the reference chain, fs %d: %.3e (peak %.2f)" % (fs, err, np.abs(y_ref).max()))
    assert err < Y_ABS
    assert checker is None or not checker.fell_back


def test_numpy_front_end(env):
    """io.morph_parameters: one pair, numpy in and out, scalars broadcast over the output frames"""
    w, codec, wio, torch = env
    d = _one_pair(24000, 1024, 9100)
    m = d["out_lengths"][0]
    got = wio.morph_parameters(d["a"], d["b"], d["pos_a"], d["pos_b"], d["weight"], 24000, 1024, f0_weight=d["f0_weight"])
    for g, w_ in zip(got, _morph(env, 24000, 1024, d)):
        assert _same(g, w_)
    got = wio.morph_parameters(d["a"], d["b"], d["pos_a"], d["pos_b"], 0.25, 24000, 1024, ratio_a=1.1, ratio_b=0.9)
    want = _morph(env, 24000, 1024, d, np.full(m, 1.1), np.full(m, 0.9), weight=np.full(m, 0.25), f0_weight=None)
    for g, w_ in zip(got, want):
        assert _same(g, w_)
