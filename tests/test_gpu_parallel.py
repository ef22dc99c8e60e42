"""-m gpu: the three calls of include/world_class_parallel.h against tests/parallel_rule.py, bit for bit, on the ragged batch of
tests/parallel_cases.py: paths from the device's own alignment and written by hand, every format pair, masks, guard columns and
rows, paths a caller wrote badly, every refusal with the outputs compared byte for byte, two host threads on their own streams; the
distortion's sum against the alignment's own cost and on a staircase whose distances span 12 orders of magnitude."""
import math
import threading

import numpy as np
import pytest

import parallel_cases as pc
import parallel_rule as pr

pytestmark = pytest.mark.gpu

DT = {"f64": np.float64, "f32": np.float32}
SHAPES = [(1, 1), (5, 7), (64, 64), (192, 192), (120, 3)]          # (dx, dy)
FORMATS = [(a, b, o) for a in ("f64", "f32") for b in ("f64", "f32") for o in ("f64", "f32")]
MASKS = ("none", "a", "b", "both")


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8).ravel()


@pytest.fixture(scope="module")
def env():
    import torch
    import world_class_amd as w
    from world_class_amd import io as wio, parallel
    w.lib().wc_set_device(0)
    return w, parallel, wio, torch


def up(env, a):
    return env[3].from_numpy(np.ascontiguousarray(a).ravel().copy()).cuda()


def down(t):
    return t.cpu().numpy()


def settle(env):
    env[3].cuda.synchronize()


def done(env):
    assert env[0].lib().wc_synchronize() == 0


@pytest.fixture(scope="module")
def batch(env):
    """the batch on the device, aligned there with closed and with open ends; paths read back, the hand-written pair put in place"""
    w, par, wio, torch = env
    al_, bl = pc.lengths()
    _, _, P, fa, fb, total = pc.offsets()
    feat_a, feat_b = pc.features()
    d_fa, d_fb = up(env, feat_a), up(env, feat_b)
    out = dict(a_lengths=al_, b_lengths=bl, feat_a=feat_a, feat_b=feat_b, d_feat_a=d_fa, d_feat_b=d_fb, total=total, fa=fa, fb=fb, P=P)
    for name, flags in (("closed", 0), ("open", 3)):
        d_cost = torch.zeros(len(al_), dtype=torch.float64, device="cuda")
        d_len = torch.full((len(al_),), -5, dtype=torch.int32, device="cuda")
        d_path = torch.full((2 * total,), pc.GARBAGE, dtype=torch.int32, device="cuda")
        settle(env)
        wio.align_features_ex_device(al_, d_fa, bl, d_fb, pc.DIMS, pc.DIM_BEGIN, pc.DIMS, 0, 0, flags, d_cost, d_len, d_path)
        done(env)
        out[name] = dict(d_cost=d_cost, d_path_length=d_len, d_path=d_path, cost=down(d_cost), path_length=down(d_len), path=down(d_path).reshape(-1, 2))
    closed = out["closed"]
    assert closed["path_length"][pc.BAD] == 0 and (closed["path_length"][:pc.BAD] > 0).all()
    assert (closed["path"][P[pc.BAD]:] == pc.GARBAGE).all()          # the pair that is not finite leaves its region unwritten
    out["path_length"], out["path"] = pc.with_hand_paths(closed["path_length"], closed["path"])
    out["d_path_length"], out["d_path"] = up(env, out["path_length"]), up(env, out["path"])
    ma, mb = pc.masks()
    out.update(mask_a=ma, mask_b=mb, d_mask_a=up(env, ma), d_mask_b=up(env, mb))
    settle(env)
    return out


def run_joint(env, B, dx, dy, fmts, masks, path_length=None, path=None, with_mask=True, pads=(1, 2, 2, 1)):
    """one call on fresh NaN-filled outputs with guard columns, a guard row and a guard byte -> (got rows, got mask, want rows, want mask)"""
    w, par, wio, torch = env
    fa_, fb_, fo = fmts
    col_a, col_b, col_o, tail = pads
    xa = pc.rows(B["fa"], col_a + dx + 1, DT[fa_], 11)
    xb = pc.rows(B["fb"], col_b + dy, DT[fb_], 12)
    ld_o = col_o + dx + dy + tail
    before = np.full((B["total"] + 1, ld_o), np.nan, dtype=DT[fo])
    ma = B["mask_a"] if masks in ("a", "both") else None
    mb = B["mask_b"] if masks in ("b", "both") else None
    path_length = B["path_length"] if path_length is None else path_length
    path = B["path"] if path is None else path
    d_len, d_path = up(env, path_length), up(env, path)
    d_out, d_m = up(env, before), torch.full((B["total"] + 1,), 0xAA, dtype=torch.uint8, device="cuda")
    d_xa, d_xb = up(env, xa), up(env, xb)
    settle(env)
    par.joint_rows(B["a_lengths"], B["b_lengths"], d_xa, xa.shape[1], dx, d_xb, xb.shape[1], dy, d_len, d_path, d_out, ld_o,
                   d_m if with_mask else None, col_a, col_b, col_o, None if ma is None else B["d_mask_a"], None if mb is None else B["d_mask_b"],
                   fa_, fb_, fo)
    done(env)
    want, want_m = pr.joint_rows(B["a_lengths"], B["b_lengths"], xa, col_a, dx, xb, col_b, dy, path_length, path, ma, mb, before[:-1], col_o)
    want = np.concatenate([want, before[-1:]])
    want_m = np.concatenate([want_m, [0xAA]]).astype(np.uint8) if with_mask else np.full(B["total"] + 1, 0xAA, dtype=np.uint8)
    return down(d_out).reshape(want.shape), down(d_m), want, want_m


def same_rows(got, want, strict):
    """the bytes; where a format was converted, a NaN may be any NaN"""
    if strict:
        return np.array_equal(raw(got), raw(want))
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(raw(np.where(nan, 0, got)), raw(np.where(nan, 0, want)))


@pytest.mark.parametrize("fmts", FORMATS, ids="-".join)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_joint_rows_equal_the_rule_in_every_format_and_leave_the_rest_alone(env, batch, shape, fmts):
    masks = MASKS[(SHAPES.index(shape) + FORMATS.index(fmts)) % 4]
    got, got_m, want, want_m = run_joint(env, batch, shape[0], shape[1], fmts, masks)
    strict = fmts[0] == fmts[1] == fmts[2]
    assert same_rows(got, want, strict)          # the gathered columns, the zero rows, the NaN guard columns and the guard row
    assert np.array_equal(got_m, want_m)
    assert want_m[:-1].sum() > 100 and (want_m[:-1] == 0).sum() > 20
    again, again_m, _, _ = run_joint(env, batch, shape[0], shape[1], fmts, masks)
    assert np.array_equal(raw(again), raw(got)) and np.array_equal(again_m, got_m)          # two runs, the same bytes


@pytest.mark.parametrize("masks", MASKS)
def test_joint_rows_under_every_mask_and_without_the_output_mask(env, batch, masks):
    got, got_m, want, want_m = run_joint(env, batch, 5, 7, ("f64", "f64", "f64"), masks)
    assert same_rows(got, want, True) and np.array_equal(got_m, want_m)
    got, got_m, want, _ = run_joint(env, batch, 5, 7, ("f32", "f64", "f32"), masks, with_mask=False)
    assert same_rows(got, want, False) and (got_m == 0xAA).all()          # d_joint_mask NULL: the rows alone
    if masks == "none":          # every slot on the path is live: the hand-written pair whole, the pair without a path not at all
        P, (a, b) = batch["P"], pc.PAIRS[pc.HAND]
        assert want_m[P[pc.HAND]:P[pc.HAND] + a + b - 1].all() and not want_m[P[pc.BAD]:-1].any()


def test_a_path_written_badly_costs_nothing_but_masked_rows(env, batch):
    path_length, path = pc.spoiled(batch["path_length"], batch["path"])
    got, got_m, want, want_m = run_joint(env, batch, 5, 7, ("f64", "f64", "f64"), "both", path_length, path)
    assert same_rows(got, want, True) and np.array_equal(got_m, want_m)
    P = batch["P"]
    for u in (1, 2):          # K = -1 and K = cap + 1: the whole pair is zero rows
        s = slice(P[u], P[u] + sum(pc.PAIRS[u]) - 1)
        assert not got[s, 2:14].any() and not got_m[s].any()
    for g in (P[3] + 5, P[4] + 9, P[4] + 11):          # i = a, j = -1, both far outside
        assert not got[g, 2:14].any() and got_m[g] == 0


# ---- the speech mask ----------------------------------------------------------------------------------------------------------------
MASK_LENGTHS = [0, 1, 63, 64, 65, 1000, 5]


def mask_column(fmt):
    rng = np.random.default_rng(21)
    col = (rng.normal(size=sum(MASK_LENGTHS)) * 4.0).astype(DT[fmt]).astype(np.float64)
    o = np.cumsum([0] + MASK_LENGTHS)
    col[o[2]] = col[o[2]:o[3]].max() + 3.0                  # top in the first frame
    col[o[4] - 1] = col[o[3]:o[4]].max() + 3.0              # top in the last frame
    col[o[4] + 7], col[o[4] + 8], col[o[4] + 9] = np.nan, np.inf, -np.inf
    col[o[5] + 500], col[o[5] + 501] = np.inf, np.nan
    col[o[6]:] = [np.nan, np.inf, -np.inf, np.nan, np.inf]          # no finite value at all
    return col.astype(DT[fmt]).astype(np.float64), o          # (what the rule sees is what the format holds)


def run_mask(env, col, fmt, margin, floor):
    w, par, wio, torch = env
    rows = np.full((len(col) + 1, 3), np.nan, dtype=DT[fmt])
    rows[:-1, 1] = col.astype(DT[fmt])
    rows[-1, 1] = 1e30          # a guard row: nothing crosses the end
    d_rows, d_m = up(env, rows), torch.full((len(col) + 1,), 0xAA, dtype=torch.uint8, device="cuda")
    settle(env)
    par.speech_mask(MASK_LENGTHS, d_rows, 3, d_m, 1, margin, floor, fmt)
    done(env)
    got = down(d_m)
    assert got[-1] == 0xAA
    return got[:-1]


@pytest.mark.parametrize("fmt", ["f64", "f32"])
def test_speech_mask_equals_the_rule(env, fmt):
    col, o = mask_column(fmt)
    for margin, floor in ((2.5, -math.inf), (math.inf, 0.5), (math.inf, -math.inf), (0.0, -math.inf), (6.0, -3.0), (40.0 * pr.DB_IN_C0, -20.0)):
        got = run_mask(env, col, fmt, margin, floor)
        want = pr.speech_mask(MASK_LENGTHS, col, margin, floor)
        assert np.array_equal(got, want), (margin, floor)
        assert not got[o[6]:].any()          # the utterance without a finite value
    both_off = run_mask(env, col, fmt, math.inf, -math.inf)
    assert np.array_equal(both_off, np.isfinite(col).astype(np.uint8)) and both_off[o[1]] == 1          # the utterance of one frame
    top_alone = run_mask(env, col, fmt, 0.0, -math.inf)
    assert top_alone[o[2]] == 1 and top_alone[o[2]:o[3]].sum() == 1 and top_alone[o[4] - 1] == 1 and top_alone[o[3]:o[4]].sum() == 1


def test_speech_mask_one_ulp_on_either_side_of_the_threshold(env):
    col, o = mask_column("f64")
    margin = 2.7
    s = slice(o[5], o[6])
    top = np.nanmax(np.where(np.isfinite(col[s]), col[s], -np.inf))
    least = top - margin
    col[o[5] + 10], col[o[5] + 11], col[o[5] + 12] = least, np.nextafter(least, math.inf), np.nextafter(least, -math.inf)
    got = run_mask(env, col, "f64", margin, -math.inf)
    assert got[o[5] + 10:o[5] + 13].tolist() == [1, 1, 0]
    assert np.array_equal(got, pr.speech_mask(MASK_LENGTHS, col, margin, -math.inf))


# ---- the distortion -----------------------------------------------------------------------------------------------------------------
def run_dist(env, al_, bl, xa, xb, col_a, col_b, dims, d_len, d_path, d_ma=None, d_mb=None, outs=(True, True, True), fmts=("f64", "f64")):
    w, par, wio, torch = env
    total = sum(a + b - 1 for a, b in zip(al_, bl))
    d_xa, d_xb = up(env, xa.astype(DT[fmts[0]])), up(env, xb.astype(DT[fmts[1]]))
    d_sum = torch.full((len(al_) + 1,), -1.0, dtype=torch.float64, device="cuda")
    d_cnt = torch.full((len(al_) + 1,), -1, dtype=torch.int64, device="cuda")
    d_cell = torch.full((total + 1,), -1.0, dtype=torch.float64, device="cuda")
    settle(env)
    par.path_distortion(al_, bl, d_xa, xa.shape[1], d_xb, xb.shape[1], dims, d_len, d_path, d_sum if outs[0] else None, d_cnt if outs[1] else None,
                        d_cell if outs[2] else None, col_a, col_b, d_ma, d_mb, fmts[0], fmts[1])
    done(env)
    return down(d_sum), down(d_cnt), down(d_cell)


@pytest.mark.parametrize("ends", ["closed", "open"])
def test_the_sum_is_the_alignments_own_cost_bit_for_bit(env, batch, ends):
    r = batch[ends]
    s, n, cell = run_dist(env, batch["a_lengths"], batch["b_lengths"], batch["feat_a"], batch["feat_b"], pc.DIM_BEGIN, pc.DIM_BEGIN,
                          pc.DIMS - pc.DIM_BEGIN, r["d_path_length"], r["d_path"])
    finite = np.isfinite(r["cost"])
    assert finite.tolist() == [True] * 6 + [False]
    assert np.array_equal(raw(s[:-1][finite]), raw(r["cost"][finite]))          # at every length: (1, 1) to (257, 130)
    assert np.array_equal(n[:-1], r["path_length"]) and n[pc.BAD] == 0 and raw(s[pc.BAD:pc.BAD + 1]).sum() == 0
    assert s[-1] == -1.0 and n[-1] == -1 and cell[-1] == -1.0          # the guards
    ws, wn, wcell = pr.path_distortion(batch["a_lengths"], batch["b_lengths"], batch["feat_a"], pc.DIM_BEGIN, batch["feat_b"], pc.DIM_BEGIN,
                                       pc.DIMS - pc.DIM_BEGIN, r["path_length"], r["path"])
    assert np.array_equal(raw(s[:-1]), raw(ws)) and np.array_equal(raw(cell[:-1]), raw(wcell))


def test_the_long_staircase_is_summed_one_cell_after_the_other(env):
    a, b, xa, xb, path = pc.long_staircase()
    d_len, d_path = up(env, np.array([len(path)], dtype=np.int32)), up(env, path)
    s, n, cell = run_dist(env, [a], [b], xa, xb, 0, 0, 3, d_len, d_path)
    ws, wn, wcell = pr.path_distortion([a], [b], xa, 0, xb, 0, 3, [len(path)], path)
    assert n[0] == 1399 and np.array_equal(raw(cell[:-1]), raw(wcell))
    assert np.array_equal(raw(s[:1]), raw(ws))          # a chunked or pairwise sum lands elsewhere (tests/test_parallel_rule.py)


@pytest.mark.parametrize("fmts", [("f64", "f64"), ("f32", "f64"), ("f64", "f32"), ("f32", "f32")], ids="-".join)
def test_counts_cells_and_sums_under_masks_with_each_output_null_in_turn(env, batch, fmts):
    al_, bl = batch["a_lengths"], batch["b_lengths"]
    xa = np.concatenate([np.full((batch["fa"], 2), np.nan), batch["feat_a"]], axis=1).astype(DT[fmts[0]])          # ld wider than the vectors
    xb = np.concatenate([batch["feat_b"], np.full((batch["fb"], 1), np.nan)], axis=1).astype(DT[fmts[1]])
    path_length, path = pc.spoiled(batch["path_length"], batch["path"])
    path_length[pc.BAD] = 5          # a hand-written path through the NaN row: what is not finite travels through
    path[batch["P"][pc.BAD]:batch["P"][pc.BAD] + 5] = [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4)]
    d_len, d_path = up(env, path_length), up(env, path)
    ws, wn, wcell = pr.path_distortion(al_, bl, xa, 3, xb, 1, 4, path_length, path, batch["mask_a"], batch["mask_b"])
    assert wn[1] == 0 and wn[2] == 0 and 0 < wn[4] < sum(pc.PAIRS[4]) - 1 and np.isnan(wcell[batch["P"][pc.BAD] + 3])
    for outs in ((True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, True), (True, False, False)):
        s, n, cell = run_dist(env, al_, bl, xa, xb, 3, 1, 4, d_len, d_path, batch["d_mask_a"], batch["d_mask_b"], outs, fmts)
        assert np.array_equal(raw(s[:-1]), raw(ws)) if outs[0] else (s == -1.0).all()
        assert np.array_equal(n[:-1], wn) if outs[1] else (n == -1).all()
        assert np.array_equal(raw(cell[:-1]), raw(wcell)) if outs[2] else (cell == -1.0).all()
        assert s[-1] == -1.0 and n[-1] == -1 and cell[-1] == -1.0


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_every_output_as_it_was(env, batch):
    w, par, wio, torch = env
    L = par._L()
    al_, bl, total, fa, fb = batch["a_lengths"], batch["b_lengths"], batch["total"], batch["fa"], batch["fb"]
    n = len(al_)
    xa, xb = up(env, pc.rows(fa, 8, np.float64, 1)), up(env, pc.rows(fb, 8, np.float64, 2))
    joint = torch.full((total * 8,), 3.25, dtype=torch.float64, device="cuda")
    jmask = torch.full((total,), 0x55, dtype=torch.uint8, device="cuda")
    d_sum, d_cnt = torch.full((n,), 3.25, dtype=torch.float64, device="cuda"), torch.full((n,), 7, dtype=torch.int64, device="cuda")
    d_cell = torch.full((total,), 3.25, dtype=torch.float64, device="cuda")
    smask = torch.full((fa,), 0x55, dtype=torch.uint8, device="cuda")
    settle(env)
    outputs = (joint, jmask, d_sum, d_cnt, d_cell, smask)
    before = [down(t).copy() for t in outputs]
    ints, p = w._ints, lambda t: None if t is None else t.data_ptr()
    A, Bl = ints(al_), ints(bl)

    def J(n_pairs=n, a=A, b=Bl, fa_=0, ra=xa, lda=8, ca=1, dx=3, fb_=0, rb=xb, ldb=8, cb=2, dy=4, pl=batch["d_path_length"], pp=batch["d_path"],
          ma=None, mb=None, fo=0, out=joint, ldo=8, co=1, om=jmask):
        return L.wc_joint_rows_device(n_pairs, a, b, fa_, p(ra), lda, ca, dx, fb_, p(rb), ldb, cb, dy, p(pl), p(pp), p(ma), p(mb), fo, p(out), ldo, co, p(om))

    def D(n_pairs=n, a=A, b=Bl, fa_=0, ra=xa, lda=8, ca=1, fb_=0, rb=xb, ldb=8, cb=2, dims=4, pl=batch["d_path_length"], pp=batch["d_path"], ma=None,
          mb=None, s=d_sum, c=d_cnt, e=d_cell):
        return L.wc_path_distortion_device(n_pairs, a, b, fa_, p(ra), lda, ca, fb_, p(rb), ldb, cb, dims, p(pl), p(pp), p(ma), p(mb), p(s), p(c), p(e))

    def M(n_utt=n, lengths=A, f=0, rows=xa, ld=8, col=0, margin=1.0, floor=0.0, m=smask):
        return L.wc_speech_mask_device(n_utt, lengths, f, p(rows), ld, col, margin, floor, p(m))

    zero, long_ = ints([0] + al_[1:]), ints([2 ** 30] * n)
    refused = [
        J(n_pairs=-1), J(a=zero), J(b=ints([-1] + bl[1:])), J(fa_=2), J(fb_=-1), J(fo=3), J(ca=-1), J(cb=-1), J(co=-1), J(dx=0), J(dy=0), J(dx=200, dy=185, lda=512, ldb=512, ldo=512),
        J(lda=3), J(ldb=5), J(ldo=7), J(a=long_, b=long_), J(a=None), J(b=None), J(ra=None), J(rb=None), J(pl=None), J(pp=None), J(out=None),
        J(out=xa), J(om=batch["d_path"]), J(om=joint), J(out=batch["d_mask_a"], ma=batch["d_mask_a"]),
        D(n_pairs=-1), D(a=zero), D(fa_=2), D(fb_=2), D(ca=-1), D(cb=-2), D(dims=0), D(lda=4), D(ldb=5), D(a=long_, b=long_), D(a=None), D(ra=None), D(rb=None),
        D(pl=None), D(pp=None), D(s=None, c=None, e=None), D(s=d_cell), D(c=d_sum), D(e=xb), D(s=batch["d_path_length"]),
        M(n_utt=-1), M(lengths=ints([-1] + al_[1:])), M(f=2), M(col=-1), M(ld=0), M(col=8), M(margin=math.nan), M(floor=math.nan), M(margin=-0.5),
        M(lengths=ints([2 ** 31 - 1] * n)), M(lengths=None), M(rows=None), M(m=None), M(m=xa),
    ]
    assert refused == [-1] * len(refused), [k for k, rc in enumerate(refused) if rc != -1]          # WC_ERR_INVALID, each of them
    assert w.last_error().startswith("speech mask: ")          # the text names the call
    done(env)
    for t, b in zip(outputs, before):
        assert np.array_equal(raw(down(t)), raw(b))
    # nothing to do: no pairs, no utterances, utterances without frames -- with NULL everywhere, and nothing is written
    assert J(n_pairs=0, a=None, b=None, ra=None, rb=None, pl=None, pp=None, out=None, om=None) == 0
    assert D(n_pairs=0, a=None, b=None, ra=None, rb=None, pl=None, pp=None, s=None, c=None, e=None) == 0
    assert M(n_utt=0, lengths=None, rows=None, m=None) == 0 and M(n_utt=2, lengths=ints([0, 0]), rows=None, m=None) == 0
    # and the limits themselves pass: dx + dy = 384, margin = +inf with floor = -inf
    wide_a, wide_b = up(env, pc.rows(fa, 192, np.float32, 3)), up(env, pc.rows(fb, 192, np.float32, 4))
    wide = torch.zeros(total * 384, dtype=torch.float32, device="cuda")
    settle(env)
    assert J(fa_=1, ra=wide_a, lda=192, ca=0, dx=192, fb_=1, rb=wide_b, ldb=192, cb=0, dy=192, fo=1, out=wide, ldo=384, co=0) == 0
    assert M(margin=math.inf, floor=-math.inf) == 0
    done(env)
    for t, b in zip(outputs[2:5], before[2:5]):
        assert np.array_equal(raw(down(t)), raw(b))


def test_two_host_threads_on_their_own_streams(env, batch):
    w, par, wio, torch = env
    al_, bl, total = batch["a_lengths"], batch["b_lengths"], batch["total"]
    inputs, results, errors = {}, {}, []
    for k, (dx, dy, seed) in enumerate(((5, 7, 31), (64, 64, 32))):
        xa, xb = pc.rows(batch["fa"], dx, np.float64, seed), pc.rows(batch["fb"], dy, np.float64, seed + 10)
        inputs[k] = (dx, dy, xa, xb, up(env, xa), up(env, xb), torch.full((total * (dx + dy),), np.nan, dtype=torch.float64, device="cuda"),
                     torch.full((total,), 0xAA, dtype=torch.uint8, device="cuda"), torch.zeros(len(al_), dtype=torch.float64, device="cuda"),
                     torch.zeros(len(al_), dtype=torch.int64, device="cuda"))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    settle(env)

    def work(k):
        try:
            dx, dy, xa, xb, d_xa, d_xb, d_out, d_m, d_sum, d_cnt = inputs[k]
            assert w.lib().wc_set_stream(streams[k].cuda_stream) == 0
            for _ in range(8):
                par.joint_rows(al_, bl, d_xa, dx, dx, d_xb, dy, dy, batch["d_path_length"], batch["d_path"], d_out, dx + dy, d_m,
                               d_mask_a=batch["d_mask_a"], d_mask_b=batch["d_mask_b"])
                par.path_distortion(al_, bl, batch["d_feat_a"], pc.DIMS, batch["d_feat_b"], pc.DIMS, 4, batch["d_path_length"], batch["d_path"], d_sum,
                                    d_cnt, None, 1, 1, batch["d_mask_a"] if k else None, batch["d_mask_b"] if k else None)
            streams[k].synchronize()
            w.lib().wc_set_stream(None)
            results[k] = (down(d_out), down(d_m), down(d_sum), down(d_cnt))
        except Exception as e:          # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in (0, 1):
        dx, dy, xa, xb = inputs[k][:4]
        want, want_m = pr.joint_rows(al_, bl, xa, 0, dx, xb, 0, dy, batch["path_length"], batch["path"], batch["mask_a"], batch["mask_b"],
                                     np.full((total, dx + dy), np.nan), 0)
        ws, wn, _ = pr.path_distortion(al_, bl, batch["feat_a"], 1, batch["feat_b"], 1, 4, batch["path_length"], batch["path"],
                                       batch["mask_a"] if k else None, batch["mask_b"] if k else None)
        got, got_m, s, n = results[k]
        assert np.array_equal(raw(got), raw(want)) and np.array_equal(got_m, want_m)
        assert np.array_equal(raw(s), raw(ws)) and np.array_equal(n, wn)
