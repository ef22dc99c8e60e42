"""CPU: the hand-written candidate tables of tests/harvest_tail.py reach the paths they are named for.  Proven from the oracle's
trace and outputs (oracle/wc_oracle.cpp, wco_harvest_tail), table by table, before any of them is sent to a device
(tests/test_gpu_harvest_tail.py takes its tables from the same list, and a table without a check here fails here)."""
import numpy as np
import pytest

import harvest_tail as T


def moves(tr):
    """frames every section's first and last frame moved in the walks"""
    return tr["ext_before"][:, 0] - tr["ext_after"][:, 0], tr["ext_after"][:, 1] - tr["ext_before"][:, 1]


def pairs(a):
    return [tuple(int(v) for v in p) for p in a]


def check_removal(name, res):
    """removeUnreliableCandidates: support at exactly 5 % (kept) and one ulp beyond (removed), from one side only, from frame 0 /
    L-1 only (removed), across the kernel's 8-frame blocks and in its last partial block, in slots >= 64 and >= 128, a full row,
    empty rows; searchF0Base: equal top scores, the lower slot wins, and a top score that is removed does not count"""
    nc = int(name.split("_")[1])
    _, cand, score = T.table(name)
    r = res[0]
    marks, base = T.removal_marks(nc)
    want = {"frame_0_only", "frame_last_only", "block_edge", "at_5_percent_next_only", "at_5_percent_prev_only", "beyond_5_percent",
            "one_ulp_beyond_next", "one_ulp_beyond_prev", "slot_64_up", "base_tie", "top_score_removed", "partial_block"}
    if nc > 128:
        want.add("slot_128_up")
    assert set(marks) == want
    for kind, items in marks.items():
        for fr, sl, kept in items:
            assert cand[fr, sl] != 0.0
            assert (r["cand"][fr, sl] != 0.0) == kept, (kind, fr, sl)
            assert r["cand"][fr, sl] == (cand[fr, sl] if kept else 0.0) and r["score"][fr, sl] == (score[fr, sl] if kept else 0.0)
    assert any(sl >= 64 for fr, sl, _ in marks["slot_64_up"]) and (nc <= 128 or any(sl >= 128 for fr, sl, _ in marks["slot_128_up"]))
    assert (cand[30] != 0).all() and 0 < (r["cand"][30] != 0).sum() < nc   # the full row: partly kept
    assert (cand != 0).sum(axis=1).min() == 0                              # empty rows
    n_in, n_out = int((cand != 0).sum()), int((r["cand"] != 0).sum())
    assert 0 < n_out < n_in                                                # kept and removed
    for fr, f in base.items():
        top = score[fr].max()
        assert r["f0_base"][fr] == f, fr
        if fr != 47:
            slots = np.flatnonzero(score[fr] == top)
            assert len(slots) == 2 and cand[fr, slots[0]] == f and cand[fr, slots[1]] != f  # a tie; the lower slot's value is the base
    assert {int(s[1] - s[0]) for fr in (35, 39) for s in [np.flatnonzero(score[fr] == score[fr].max())]} == {32, 64}


def check_ties(name, res):
    """selectBestF0 in the walks: of two candidates at the same error (180 | 220 around 200) the later slot wins -- slots of two lanes,
    l | l+64, k | k+128 --, 18 / 100 is accepted and one ulp beyond is not"""
    nc = int(name.split("_")[1])
    _, cand, _ = T.table(name)
    r = res[0]
    chosen, mv = T.ties_marks(nc)
    for fr, v in chosen:
        live = np.flatnonzero(r["cand"][fr])
        assert r["s3"][fr] == v and r["f0_fixed"][fr] == v, fr
        if len(live) == 2:
            assert r["cand"][fr, live[1]] == v and r["cand"][fr, live[0]] != v   # the later slot's
    gaps = {int(np.diff(np.flatnonzero(cand[fr]))[0]) for fr, _ in chosen if (cand[fr] != 0).sum() == 2}
    assert 64 in gaps and (nc <= 128 or 128 in gaps) and 4 in gaps
    back, fwd = moves(r["trace"])
    got = {(u, d): int(fwd[u] if d > 0 else back[u]) for u, d, _ in mv}
    assert got == {(u, d): m for u, d, m in mv}
    n_thr = 4
    assert sorted(m for _, d, m in mv[-n_thr:] if d > 0) == [0, 2] and sorted(m for _, d, m in mv[-n_thr:] if d < 0) == [1, 3]  # both outcomes
    assert r["trace"]["count"] == len(mv)


def check_walks(name, res):
    """extendF0: 101 frames each way; clamped at 1 / 0 and at L-2 / L-1; three misses and a hit (goes on), four misses (stops);
    the first and the last section fixStep1 can leave (2 .. 8 and L-8 .. L-2); no move at all"""
    for r, expect in zip(res, (T.WALKS_EXPECT_0, T.WALKS_EXPECT_1)):
        tr = r["trace"]
        assert pairs(tr["ext_before"]) == [e[0] for e in expect]
        assert pairs(tr["ext_after"]) == [e[1] for e in expect]
    L = T.WALKS_L[0]
    back, fwd = moves(res[0]["trace"])
    assert pairs(res[0]["trace"]["sec2"])[0] == (2, 8) and pairs(res[0]["trace"]["sec2"])[-1] == (L - 8, L - 2)
    assert back[1] == 101 and fwd[1] == 101 and back[4] == 0 and fwd[4] == 0
    assert back[0] == 2 and fwd[-1] == 1                 # clamped: 2 .. 8 can only reach 1 and 0, L-2 only L-1
    assert fwd[2] == 7 and fwd[3] == 2                   # across three misses; not across four
    back1, fwd1 = moves(res[1]["trace"])
    assert back1[0] == 41 and fwd1[1] == 39              # clamped walks of some length
    assert res[1]["s3"][0] != 0 and res[1]["s3"][T.WALKS_L[1] - 1] != 0


def check_steps(name, res):
    """fixStep1: 1 / 125 = 0.008 kept, one ulp beyond dropped, a voiced frame behind two unvoiced ones dropped; fixStep2: ed - st of 5
    cleared and of 6 kept, more than 64 sections cleared; the section lists with a first and a last frame on each of 63, 64, 65,
    255, 256, 257"""
    r = res[0]
    s1, s2 = pairs(r["trace"]["sec1"]), pairs(r["trace"]["sec2"])
    assert (11, 29) in s1                                # 125 -> 126 on frame 20 kept
    assert (41, 49) in s1 and (51, 59) in s1 and r["f0_base"][50] != 0 and r["s1"][50] == 0   # 125 -> up(126) on frame 50 dropped
    assert r["f0_base"][8] == 0 and r["f0_base"][9] == 0 and r["f0_base"][10] != 0 and r["s1"][10] == 0
    assert (71, 76) in s1 and (71, 76) not in s2 and (91, 97) in s1 and (91, 97) in s2
    assert len(s1) - len(s2) > 64 and set(s2) <= set(s1)
    first, last = set(), set()
    for r, expect in zip(res[1:], T.STEPS_EDGE_SECTIONS):
        assert pairs(r["trace"]["sec1"]) == expect and pairs(r["trace"]["sec2"]) == expect
        first |= {st for st, _ in expect}
        last |= {ed for _, ed in expect}
    assert set(T.STEPS_EDGE_FRAMES) <= first and set(T.STEPS_EDGE_FRAMES) <= last


def check_many(name, res):
    """49, 97 and 148 sections after fixStep2 (the extension phase's second and third trip over its grid of 96 walks), every one of
    them moved by both of its walks; extendSub's second and third round of 64 sections decide otherwise than the first; at 148, sections of seven frames with one frame between them: as many as an utterance holds,
    and the channel windows still fit the storage of the utterance alone in its call"""
    n = int(name.split("_")[1])
    tr = res[0]["trace"]
    s2 = tr["sec2"]
    assert len(s2) == n and (n < 130 or len(s2) >= 130)
    back, fwd = moves(tr)
    assert (back >= 1).all() and (fwd >= 1).all()
    assert tr["window_sum"] <= T.channel_capacity(T.MANY_L)
    low = [k for k in T.MANY_LOW if k < n]
    assert list(np.flatnonzero(~tr["selected"])) == low and tr["count"] == n - len(low)
    for k in low:   # extendSub reloads its lanes every 64 sections: these differ from the sections 64 and 128 places before them
        assert tr["selected"][k - 64] and tr["selected"][k & 63]
    assert (len(low) > 0) == (n > 64) and (max(low, default=0) >= 128) == (n > 128)
    if n == 148:
        assert ((s2[:, 1] - s2[:, 0]) == 6).all() and ((s2[1:, 0] - s2[:-1, 1]) == 2).all()
        assert n >= T.MANY_L // 8 - 2   # (a section and its gap take eight frames)
        assert tr["s1_lt_s2"] > 128


def check_extendsub(name, res):
    """extendSub: ed - st on both sides of 2200 / mean and equal to it (not kept); the mean carried from section to section decides
    otherwise than a mean reset per section would; sums over more than 64 and 128 frames; no section kept (the row at position 0 is
    still copied); the first kept section is not the earliest"""
    _, cand, _ = T.table(name)
    r = res[0]
    tr = r["trace"]
    bounds, kept = T.py_extendsub(r["cand"], r["s2"], pairs(tr["sec2"]), reset=False)
    assert bounds == pairs(tr["ext_after"]) and kept == [bool(v) for v in tr["selected"]]
    _, kept_reset = T.py_extendsub(r["cand"], r["s2"], pairs(tr["sec2"]), reset=True)
    assert kept_reset != kept                            # the carried mean is what decides sections 1 and 3
    n = tr["ext_after"][:, 1] - tr["ext_after"][:, 0]
    assert n[0] == 22 and 2200.0 / 100.0 == 22 and not kept[0]            # equality (the first section's mean carries nothing)
    assert n[1] == 22 and kept[1] and n[2] == 23 and kept[2] and n[4] == 15 and not kept[4]
    assert n[5] > 64 and n[6] > 128 and kept[5] and kept[6]
    r = res[1]
    assert r["trace"]["count"] == 0 and len(r["trace"]["sec2"]) == 2
    assert np.array_equal(np.flatnonzero(r["s3"]), np.arange(10, 26))      # position 0's row, and only that
    r = res[2]
    tr = r["trace"]
    assert tr["count"] >= 1 and tr["selected"][0] and tr["selected"][1] and tr["ext_after"][1, 0] < tr["ext_after"][0, 0]
    assert not r["s3"][40:50].any() and r["s3"][50:58].all()              # (the section that starts first is never merged)


def check_merge(name, res):
    """mergeF0: every branch -- disjoint, contained, s1 > s2, s1 < s2, s1 == s2 -- with 26 kept sections (std::sort past its
    insertion-sort threshold of 16) of which two groups of three and more start on the same frame; s1 == s2 with both sums zero"""
    tr = res[0]["trace"]
    for k in ("disjoint", "contained", "s1_gt_s2", "s1_lt_s2", "s1_eq_s2"):
        assert tr[k] > 0, k
    assert tr["count"] >= 17 and tr["groups3"] >= 2
    starts = tr["ext_after"][tr["selected"], 0]
    assert (starts == 3).sum() >= 3 and (starts == 5).sum() >= 3         # where the two tracks begin
    r = res[1]
    a, b = pairs(r["trace"]["ext_after"])
    assert r["trace"]["s1_eq_s2"] == 1 and a[1] >= b[0] and not r["score"][b[0]:a[1] + 1].any()
    assert r["s3"][b[0]] == 160.0                        # ... and then the later section is taken from its start


def check_step4(name, res):
    """fixStep4: gaps of 8 filled, gaps of 9 left; more than 64 gaps of either kind, and then more than 64 sections for the smoothing;
    sections that reach frames 0 and L-1 through their walks, which the smoothing sees and fixStep4 does not"""
    r = res[0]
    tr = r["trace"]
    s3 = tr["sec3"]
    gaps = s3[1:, 0] - s3[:-1, 1] - 1
    if name == "step4_small":
        assert sorted(set(int(g) for g in gaps if g < 20)) == [8, 9] and tr["gaps_filled"] == 2 and tr["gaps_left"] == 3
        L = len(r["s3"])
        assert r["s3"][0] != 0 and r["s3"][L - 1] != 0 and s3[0, 0] == 1 and s3[-1, 1] == L - 2
        assert r["f0_1ms"][0] != 0 and r["f0_1ms"][L - 1] != 0
        assert r["f0_fixed"][41:49].all() and not r["f0_fixed"][81:90].any()
    else:
        gap = int(name[-1])
        assert (gaps == gap).all() and len(gaps) > 64
        assert (tr["gaps_filled"], tr["gaps_left"]) == ((69, 0) if gap == 8 else (0, 69))
        assert tr["smooth_sections"] == (1 if gap == 8 else 70)


def check_small(name, res):
    """the shortest utterance Harvest takes (three frames), one of 37 frames whose only section reaches both ends, and three sections
    in 500 frames (the call behind the many-section one in the stale-scratch test)"""
    r = res[0]
    L = len(r["f0_1ms"])
    assert L == {"tiny": 3, "short37": 37, "three_sections": 500}[name]
    assert len(r["trace"]["sec2"]) == {"tiny": 0, "short37": 1, "three_sections": 3}[name]
    if name == "tiny":
        assert not r["cand"][1].any() and r["f0_base"][0] == 100.0 and r["f0_base"][2] == 300.0
    if name == "short37":
        assert r["f0_1ms"].all()


CHECKS = {"removal": check_removal, "ties": check_ties, "walks": check_walks, "steps": check_steps, "many": check_many,
          "extendsub": check_extendsub, "merge": check_merge, "step4": check_step4, "tiny": check_small, "short37": check_small,
          "three": check_small}


@pytest.mark.parametrize("name", sorted(T.TABLES))
def test_table_reaches_its_path(port, name):
    x_lengths, cand, score = T.table(name)
    assert cand.shape == score.shape and cand.shape[1] == T.NC[T.TABLES[name][1]]
    assert cand.shape[0] == sum(T.frames_1ms(n) for n in x_lengths)
    live = cand[cand != 0]
    assert live.min() >= T.F0_FLOOR and live.max() <= T.F0_CEIL and (score >= 0).all() and not score[cand == 0].any()
    res = T.reference(port, name)
    for r, n in zip(res, x_lengths):   # whatever the table, its channel windows fit the storage of the utterance alone in its call
        assert r["trace"]["window_sum"] <= T.channel_capacity(T.frames_1ms(n))
    check = CHECKS[name.split("_")[0]]
    assert check.__doc__
    check(name, res)


def test_builders_are_deterministic():
    for name in ("ties_210", "extendsub", "merge"):
        a, b = T.TABLES[name][0](), T.TABLES[name][0]()
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("fp", [1.0, 2.5, 5.0, 10.0])
def test_output_frame_periods(port, fp):
    """the output picks f0_1ms at matlab_round(i * fp): at 2.5 ms every other index is a rounding half"""
    r = T.reference(port, "step4_small", fp)[0]
    n = len(r["f0"])
    assert n == int(1000.0 * T.table("step4_small")[0][0] / T.FS / fp) + 1
    at = np.minimum(len(r["f0_1ms"]) - 1, np.floor(np.arange(n) * fp + 0.5).astype(int))
    assert np.array_equal(r["f0"], r["f0_1ms"][at]) and np.array_equal(r["tpos"], np.arange(n) * fp / 1000.0)
    if fp == 2.5:
        assert ((np.arange(n) * fp) % 1 == 0.5).sum() >= n // 2 - 1
    assert (r["f0"] != 0).any() and (r["f0"] == 0).any()
