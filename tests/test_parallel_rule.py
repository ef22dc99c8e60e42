"""tests/parallel_rule.py against the mathematics it restates: the joint rows against numpy fancy indexing on a path of
tests/align_rule.py, the mask against a direct restatement, the distortion's order against the alignment's own accumulated cost, what
lengths and entries outside their range do -- and that the inputs of tests/test_gpu_parallel.py tell the rule from three one-line
mistakes."""
import math

import numpy as np
import pytest

import align_rule as al
import parallel_cases as pc
import parallel_rule as pr


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32 if a.dtype == np.float32 else a.dtype)


@pytest.fixture(scope="module")
def batch():
    feat_a, feat_b = pc.features()
    path_length, path, cost = pc.rule_paths(feat_a, feat_b)
    return dict(feat_a=feat_a, feat_b=feat_b, path_length=path_length, path=path, cost=cost)


def test_joint_rows_are_fancy_indexing_on_an_aligned_path():
    rng = np.random.default_rng(1)
    a, b, dx, dy = 23, 31, 4, 3
    xa, xb = rng.normal(size=(a, 5)), rng.normal(size=(b, 6)).astype(np.float32)
    path = al.align(xa[:, :3], xb[:, :3].astype(np.float64), 0, 3)["path"]
    K, cap = len(path), a + b - 1
    packed = np.full((cap, 2), pc.GARBAGE, dtype=np.int32)
    packed[:K] = path
    before = np.full((cap, dx + dy + 3), np.nan)
    out, mask = pr.joint_rows([a], [b], xa, 1, dx, xb, 2, dy, [K], packed, None, None, before, 2)
    assert np.array_equal(out[:K, 2:2 + dx], xa[path[:, 0], 1:1 + dx]) and np.array_equal(out[:K, 2 + dx:2 + dx + dy], xb[path[:, 1], 2:2 + dy].astype(np.float64))
    assert (bits(out[K:, 2:2 + dx + dy]) == 0).all() and np.isnan(out[:, :2]).all() and np.isnan(out[:, 2 + dx + dy:]).all()
    assert mask.tolist() == [1] * K + [0] * (cap - K)
    ma, mb = (np.arange(a) % 3 != 0).astype(np.uint8) * 9, (np.arange(b) % 4 != 1).astype(np.uint8)
    _, masked = pr.joint_rows([a], [b], xa, 1, dx, xb, 2, dy, [K], packed, ma, mb, before, 2)
    assert masked[:K].tolist() == [int(ma[i] != 0 and mb[j] != 0) for i, j in path] and not masked[K:].any()
    f32, _ = pr.joint_rows([a], [b], xa, 1, dx, xb, 2, dy, [K], packed, None, None, before.astype(np.float32), 2)
    assert np.array_equal(f32[:K, 2:2 + dx], xa[path[:, 0], 1:1 + dx].astype(np.float32))          # a float written is the (float) of the double
    assert np.array_equal(bits(f32[:K, 2 + dx:2 + dx + dy]), bits(xb[path[:, 1], 2:2 + dy]))         # same format: the bits


def test_lengths_and_entries_outside_their_range_give_masked_zero_rows(batch):
    al_, bl = pc.lengths()
    _, _, P, fa, fb, total = pc.offsets()
    path_length, path = pc.spoiled(*pc.with_hand_paths(batch["path_length"], batch["path"]))
    xa, xb = pc.rows(fa, 3, np.float64, 1), pc.rows(fb, 2, np.float64, 2)
    out, mask = pr.joint_rows(al_, bl, xa, 0, 3, xb, 0, 2, path_length, path, None, None, np.full((total, 5), np.nan), 0)
    for u in (1, 2, pc.BAD):          # K = -1, K = cap + 1, K = 0: the whole pair
        s = slice(P[u], P[u] + sum(pc.PAIRS[u]) - 1)
        assert (bits(out[s]) == 0).all() and not mask[s].any()
    for g in (P[3] + 5, P[4] + 9, P[4] + 11):          # i = a, j = -1, both far outside
        assert (bits(out[g]) == 0).all() and mask[g] == 0
    assert mask[P[3] + 4] == 1 and mask[P[3] + 6] == 1 and mask[P[4] + 10] == 1          # their neighbours are untouched
    on, _, ra, rb = pr.slot_states(al_, bl, path_length, path)
    assert (ra[on] >= 0).all() and (ra[on] < fa).all() and (rb[on] < fb).all() and (ra[~on] == -1).all()


def test_speech_mask_against_a_direct_restatement():
    rng = np.random.default_rng(2)
    lengths = [0, 1, 7, 40, 5]
    col = rng.normal(size=sum(lengths)) * 4.0
    col[3], col[9], col[12], col[20] = np.nan, np.inf, -np.inf, col[8:48].max() + 1.0
    col[48:] = [np.nan, np.inf, -np.inf, np.nan, np.nan]          # an utterance without a finite value
    for margin, floor in ((3.0, -1.0), (0.0, -math.inf), (math.inf, 0.5), (math.inf, -math.inf)):
        got = pr.speech_mask(lengths, col, margin, floor)
        f = 0
        for n in lengths:
            v = col[f:f + n]
            fin = np.isfinite(v)
            want = np.zeros(n, dtype=np.uint8) if not fin.any() else (fin & (v >= v[fin].max() - margin) & (v >= floor)).astype(np.uint8)
            assert np.array_equal(got[f:f + n], want)
            f += n
        assert not got[48:].any() and got[0] == (1 if col[0] >= floor else 0)
    every = pr.speech_mask(lengths, col, math.inf, -math.inf)
    assert np.array_equal(every[:48], np.isfinite(col[:48]).astype(np.uint8))          # both tests off: the finite frames
    assert pr.speech_mask([40], col[8:48], 0.0, -math.inf).sum() == 1          # margin 0: the top alone
    top = 5.0
    edge = np.array([top, np.nextafter(top - 0.3, math.inf), top - 0.3, np.nextafter(top - 0.3, -math.inf)])
    assert pr.speech_mask([4], edge, 0.3, -math.inf).tolist() == [1, 1, 1, 0]          # one ulp on either side of top - margin


def test_one_decibel_in_units_of_c0():
    # c0 is the mean of ln(power) over the mel axis: a gain of g dB adds g * ln(10) / 10 to every sample and to their mean
    lg = np.random.default_rng(3).normal(size=512)
    gain_db = 7.0
    louder = np.log(np.exp(lg) * 10.0 ** (gain_db / 10.0))
    assert abs((louder.mean() - lg.mean()) - gain_db * pr.DB_IN_C0) < 1e-12 and abs(pr.DB_IN_C0 - 0.23025850929940458) < 1e-17


def test_the_sum_is_the_alignments_cost_bit_for_bit_and_not_numpys():
    rng = np.random.default_rng(4)
    differs = 0
    for k in range(20):
        a, b = int(rng.integers(20, 60)), int(rng.integers(20, 60))
        xa = np.cumsum(rng.normal(size=(a, 6)), axis=0) * 10.0 ** rng.uniform(-3, 3)
        xb = xa[np.minimum((np.arange(b) * a) // b, a - 1)] + rng.normal(size=(b, 6)) * 10.0 ** rng.uniform(-4, 1, size=(b, 1))
        r = al.align(xa, xb, 1, 6)
        K = len(r["path"])
        packed = np.full((a + b - 1, 2), pc.GARBAGE, dtype=np.int32)
        packed[:K] = r["path"]
        s, n, cell = pr.path_distortion([a], [b], xa, 1, xb, 1, 5, [K], packed)
        assert n[0] == K and bits(s)[0] == bits(np.array([r["cost"]]))[0]          # D(i, j) = d(i, j) + best is this very chain
        differs += bits(s)[0] != bits(np.array([np.sum(cell[:K])]))[0]
    assert differs >= 1          # numpy's pairwise sum lands elsewhere at least once: the order is what is tested


def test_the_long_staircase_tells_a_chunked_sum_from_the_sequential_one():
    a, b, xa, xb, path = pc.long_staircase()
    s, n, cell = pr.path_distortion([a], [b], xa, 0, xb, 0, 3, [len(path)], path)
    live = cell[cell > 0]
    assert n[0] == 1399 and math.log10(live.max() / live.min()) >= 10.0
    chunked = 0.0
    for c in range(0, 1399, 64):
        part = 0.0
        for e in cell[c:c + 64]:
            part = part + float(e)
        chunked = chunked + part
    assert s[0] != chunked and s[0] != float(np.sum(cell))


def test_distortion_counts_cells_and_what_is_not_finite(batch):
    al_, bl = pc.lengths()
    _, _, P, fa, fb, total = pc.offsets()
    path_length, path = pc.with_hand_paths(batch["path_length"], batch["path"])
    ma, mb = pc.masks()
    fa_, fb_ = batch["feat_a"], batch["feat_b"]
    s, n, cell = pr.path_distortion(al_, bl, fa_, 1, fb_, 1, 4, path_length, path, ma, mb)
    on, live, _, _ = pr.slot_states(al_, bl, path_length, path, ma, mb)
    for u, (a, b) in enumerate(pc.PAIRS):
        sl = slice(P[u], P[u] + a + b - 1)
        assert n[u] == live[sl].sum() and (cell[sl][~on[sl]] == 0).all()
    assert n[pc.BAD] == 0 and bits(s)[pc.BAD] == 0 and n[pc.HAND] < sum(pc.PAIRS[pc.HAND]) - 1
    # a NaN row under a hand-written path travels through: the cell and the sum are NaN
    hand_length = path_length.copy()
    hand_length[pc.BAD] = 5
    path2 = path.copy()
    path2[P[pc.BAD]:P[pc.BAD] + 5] = [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4)]
    s2, n2, cell2 = pr.path_distortion(al_, bl, fa_, 1, fb_, 1, 4, hand_length, path2)
    assert n2[pc.BAD] == 5 and np.isnan(s2[pc.BAD]) and np.isnan(cell2[P[pc.BAD] + 3]) and np.isfinite(cell2[P[pc.BAD] + 2])


def test_mcd_db():
    assert pr.mcd_db(3.0, 2) == (10.0 / math.log(10.0)) * math.sqrt(2.0) * 3.0 / 2


def test_the_planted_speakers_give_the_chain_its_ordering_with_room_to_spare():
    """the chain of tests/test_gpu_parallel_chain.py by the rules alone: pack, mask, align, join, five iterations of EM, convert.  The
    converted rows' mean squared distance to the target is about 0.05 of the source's; the GPU test asserts 0.25"""
    import features_rule as fr
    import gmm_rule as gm
    import gmm_train_rule as tr
    from world_class_amd.gmm_train import initial_model
    S = pc.planted_speakers()
    al_, bl, nd = S["a_lengths"], S["b_lengths"], pc.ND
    rows_a = fr.pack(al_, nd, 0, pc.ORDERS, S["f0_a"], S["sp_a"], None, 0.0)
    rows_b = fr.pack(bl, nd, 0, pc.ORDERS, S["f0_b"], S["sp_b"], None, 0.0)
    ma = pr.speech_mask(al_, rows_a[:, 0], 40.0 * pr.DB_IN_C0, -math.inf)
    mb = pr.speech_mask(bl, rows_b[:, 0], 40.0 * pr.DB_IN_C0, -math.inf)
    assert (ma == 0).sum() == 36 and (mb == 0).sum() >= 30          # the planted silence: six frames at either end of every utterance
    A, B, P, caps = pr.slot_offsets(al_, bl)
    path_length, path = np.zeros(len(al_), dtype=np.int32), np.full((sum(caps), 2), pc.GARBAGE, dtype=np.int32)
    for u, (a, b) in enumerate(zip(al_, bl)):
        r = al.align(rows_a[A[u]:A[u] + a, :nd], rows_b[B[u]:B[u] + b, :nd], 1, nd)
        path_length[u] = len(r["path"])
        path[P[u]:P[u] + len(r["path"])] = r["path"]
    dx = dy = pc.ORDERS * nd
    joint, jm = pr.joint_rows(al_, bl, rows_a, 0, dx, rows_b, 0, dy, path_length, path, ma, mb, np.zeros((sum(caps), dx + dy)), 0)
    live = jm != 0
    assert live.sum() >= 150
    model, ll = tr.iterate(*initial_model(joint[live], pc.N_MIX, 0), joint, 5, jm)
    assert all(b >= a for a, b in zip(ll, ll[1:]))
    mean = gm.convert(gm.prepare(*model, dx, dy), joint[:, :dx])[0]
    source, converted = ((joint[live, :dx] - joint[live, dx:]) ** 2).mean(), ((mean[live] - joint[live, dx:]) ** 2).mean()
    assert converted < 0.1 * source, (source, converted)          # room to spare under the 0.25 the GPU test asserts


MISTAKES = {
    "i and j swapped": ("cell_of", lambda e: (int(e[1]), int(e[0]))),
    "P_u built from max(a, b)": ("slot_offsets", None),
    "the mask ORed": ("both_count", lambda ma, mb: ma != 0 or mb != 0),
}


def _wrong_offsets(a_lengths, b_lengths):
    A, B, P, caps = [], [], [], []
    fa = fb = p = 0
    for a, b in zip(a_lengths, b_lengths):
        A.append(fa), B.append(fb), P.append(p), caps.append(a + b - 1)
        fa, fb, p = fa + a, fb + b, p + max(a, b)
    return A, B, P, caps


@pytest.mark.parametrize("mistake", sorted(MISTAKES))
def test_the_gpu_tests_inputs_catch_a_one_line_mistake(batch, monkeypatch, mistake):
    al_, bl = pc.lengths()
    _, _, _, fa, fb, total = pc.offsets()
    path_length, path = pc.with_hand_paths(batch["path_length"], batch["path"])
    ma, mb = pc.masks()
    xa, xb = pc.rows(fa, 6, np.float64, 1), pc.rows(fb, 8, np.float64, 2)
    before = np.full((total, 14), np.nan)

    def everything():
        joint, mask = pr.joint_rows(al_, bl, xa, 1, 5, xb, 1, 7, path_length, path, ma, mb, before, 1)
        s, n, cell = pr.path_distortion(al_, bl, batch["feat_a"], 1, batch["feat_b"], 1, 4, path_length, path, ma, mb)
        return [bits(joint), mask, bits(s), n, bits(cell)]

    right = everything()
    name, wrong = MISTAKES[mistake]
    monkeypatch.setattr(pr, name, wrong or _wrong_offsets)
    mistaken = everything()
    caught = [not np.array_equal(r, m) for r, m in zip(right, mistaken)]
    if mistake == "the mask ORed":
        assert caught == [False, True, True, True, False]          # the rows and the cells do not read a mask
    else:
        assert caught[0] and caught[2] and caught[4]
