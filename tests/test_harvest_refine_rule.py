"""CPU: the refinement tables of tests/harvest_refine.py reach what they are named for, the CPU oracle's refinement
(wco_harvest_refine: the hv_overlap + hv_refine of every wco_harvest call) makes the rule's integer decisions and keeps the rule's
zero pattern on them, and the rule is sharp: every way of getting the refinement subtly wrong that is listed in
harvest_refine.MUTANTS leaves the device's bound by at least 100 x on the table built for it.  Also measures K_ref, the oracle's
largest error in units (harvest_refine's docstring), which tests/test_gpu_harvest_refine.py turns into the device's bound.

Measured here (x86-64, glibc): K_ref = 0.664 (crowded_32, 1 / score); per table the oracle stays below 0.7 units.
"""
from fractions import Fraction

import numpy as np
import pytest

import harvest_refine as R


def live_values(name, key):
    return np.concatenate([r[key][r["live"]] for r in R.rule(name)])


def test_k_ref(port):
    """the oracle's largest error against the long double rule, in units: a radix-2 FFT of at most 12 stages behind a window of
    exact cosines cannot be off by more than a few first-order roundings, and it is off by something"""
    k = R.k_ref(port)
    print("harvest refinement: K_ref = %.4f units" % k)
    assert 0.05 < k < 12.0


@pytest.mark.parametrize("name", sorted(R.BUILDERS))
def test_decimated_signal_is_the_signal_and_rows_have_the_handle_width(port, name):
    """what the tables assume of the handle: at decimation 1 on signals below 1 the decimated signal is the signal with one zero
    appended, and the detector's rows are S wide -- from a whole Harvest call of the oracle on the first and the shortest utterance"""
    t = R.table(name)
    port.set_harvest_options(float(t.fs), t.cio, False)
    try:
        for u in {0, int(np.argmin([len(x) for x in t.xs]))}:
            d = port.harvest_debug(t.xs[u], t.fs, f0_floor=t.floor, f0_ceil=t.ceil)
            assert np.array_equal(d["y"], t.y(u))
            assert d["cand"].shape == (t.L1(u), 7 * t.S)
    finally:
        port.set_harvest_options()


@pytest.mark.parametrize("name", R.NAMES)
def test_oracle_makes_the_rules_decisions_and_keeps_its_zero_pattern(port, name):
    t, k = R.table(name), R.k_ref(port)
    worst_f = worst_s = 0.0
    for r, (c1, s1, dec) in zip(R.rule(name), R.oracle(port, name)):
        live = r["live"]
        assert np.array_equal(dec[..., 0] != 0, live)
        for col, key in enumerate(("hw", "N", "basic", "nh")):
            assert np.array_equal(dec[..., col][live], r[key][live].astype(np.int64)), (name, key)
        assert np.array_equal(dec[..., 4:][live], r["bins"][live]), (name, "bins")
        R.same_zero_pattern(t, r, c1, s1, k)
        ef, es = R.errors(r, c1, s1)
        worst_f, worst_s = max(worst_f, float(ef.max())), max(worst_s, float(es.max()))
    print("harvest refinement %s: oracle's worst error in units: F0 %.3f, 1 / score %.3f" % (name, worst_f, worst_s))
    assert max(worst_f, worst_s) <= k


@pytest.mark.parametrize("name", R.NAMES)
def test_decisions_recomputed_in_exact_arithmetic(name):
    """the rule's float64 decisions are the correctly rounded evaluation, operation by operation, of the reference's expressions:
    every operation redone on exact rationals and rounded once"""
    t = R.table(name)
    fs = float(t.fs)

    def fl(q):
        return float(q)  # Fraction -> float rounds correctly
    seen = set()
    for r in R.rule(name):
        for i, p in np.argwhere(r["live"]):
            f = float(r["f"][i, p])
            if f in seen:
                continue
            seen.add(f)
            v = fl(Fraction(fl(Fraction(fl(Fraction(1.5) * Fraction(fs))) / Fraction(f))) + 1)
            hw = int(v)
            assert hw == r["hw"][i, p]
            n_pow = 4
            while n_pow <= 2 * hw + 1:  # 2 hw + 1 is odd: never a power of two, its logarithm never near an integer
                n_pow *= 2
            assert 2 * n_pow == r["N"][i, p]
            assert min(int(fl(Fraction(fl(Fraction(fs) / 2)) / Fraction(f))), 6) == r["nh"][i, p]
            unit = fl(Fraction(fl(Fraction(f) * int(r["N"][i, p]))) / Fraction(fs))
            for h in range(int(r["nh"][i, p])):
                assert int(fl(Fraction(fl(Fraction(unit) * (h + 1))) + Fraction(1, 2))) == r["bins"][i, p, h]
    assert seen


@pytest.mark.parametrize("name", R.NAMES)
def test_survival_and_the_near_threshold_cap(port, name):
    """at least half the live candidates survive the thresholds on the reference side, and at most 1 % lie within the comparison
    bound of floor, ceiling or score 2.5 (where the zero pattern is not compared)"""
    t, k = R.table(name), R.k_ref(port)
    live = sum(int(r["live"].sum()) for r in R.rule(name))
    near = sum(int(R.near_threshold(t, r, k).sum()) for r in R.rule(name))
    alive = sum(int((c1 != 0).sum()) for c1, _, _ in R.oracle(port, name))
    print("harvest refinement %s: %d live candidates, %d survive, %d near a threshold" % (name, live, alive, near))
    assert live > 0 and 2 * alive >= live
    assert 100 * near <= live


def adjacent_pairs(t):
    """(lower, upper) doubles one ulp apart among a table's cut candidates"""
    f = sorted({float(t.cand0[u][i, j]) for u, i, j in t.notes["cut_candidates"]})
    return [(a, b) for a, b in zip(f[:-1], f[1:]) if R.up(a) == b]


def check_cuts(name):
    t = R.table(name)
    fs = float(t.fs)
    pairs = adjacent_pairs(t)
    d = [(R.decisions(fs, 0, a), R.decisions(fs, 0, b)) for a, b in pairs]
    hw_cut = {(hi["hw"], lo["hw"]) for lo, hi in d if lo["hw"] != hi["hw"]}
    n_cut = {(hi["N"], lo["N"]) for lo, hi in d if lo["N"] != hi["N"]}
    nh_cut = {(hi["nh"], lo["nh"]) for lo, hi in d if lo["nh"] != hi["nh"]}
    bin_cut = {h for lo, hi in d for h in range(min(lo["nh"], hi["nh"])) if lo["N"] == hi["N"] and lo["bins"][h] != hi["bins"][h]}
    sizes = {int(v) for v in live_values(name, "N")}
    if "low" in name:
        assert n_cut == {(2048, 4096), (1024, 2048), (512, 1024), (256, 512)}  # every size the handle reaches: 17.5 .. 260 Hz at 8 kHz
        assert {(511, 512), (255, 256), (127, 128), (63, 64), (120, 121)} <= hw_cut
        assert sizes == {256, 512, 1024, 2048, 4096}
    else:
        assert n_cut == {(512, 1024), (256, 512), (128, 256), (64, 128)}  # 71 .. 1400 Hz at 8 kHz
        assert {(127, 128), (63, 64), (31, 32), (15, 16), (96, 97), (48, 49)} <= hw_cut
        assert nh_cut == {(5, 6), (4, 5), (3, 4), (2, 3)}
        assert {int(v) for v in live_values(name, "nh")} == {2, 3, 4, 5, 6}
    assert bin_cut == set(range(6))
    # exactly representable cuts: the quotient is the integer itself
    exact = [f for f in (100.0, 125.0, 250.0, 800.0, 1000.0) if t.floor <= f <= t.ceil]
    assert all(1.5 * fs / f == int(1.5 * fs / f) for f in exact) and len(exact) >= 2


def check_longest(name):
    t = R.table(name)
    hw = live_values(name, "hw")
    assert hw.max() >= 512 and 4096 in live_values(name, "N")
    assert (hw.astype(int) >> 3 >= 64).any()  # window-length classes 64 .. 127 of the group kernel's histogram (hw / 8)
    assert t.floor == R.lowest_floor(t.fs) == {8000: 17.1, 16000: 34.2}[t.fs]
    assert (t.S <= 16) == ("wide" not in name) and (7 * t.S > 128) == ("wide" in name)


def check_slots(name):
    t = R.table(name)
    S = int(name.split("_")[1])
    assert t.S == S and t.rows().shape[1] == S and len(t.rows().ravel()) // t.L1(0) == S
    r = R.rule(name)[0]
    assert r["live"][:, 7 * S - 1].any() and int(r["live"][50].sum()) == 3 * S  # the last position of a row; three full blocks in one row
    assert {16: 7 * S <= 112, 17: 112 < 7 * S <= 128, 18: 112 < 7 * S <= 128, 19: 7 * S > 128, 32: 7 * S == 224}[S]


def check_edges(name):
    t = R.table(name)
    rs = R.rule(name)
    assert {t.L1(u) % 4 for u in range(len(t.xs))} == {0, 1, 2, 3}
    lo = sum(int((r["clamp_lo"] & ~r["clamp_hi"]).sum()) for r in rs)
    hi = sum(int((r["clamp_hi"] & ~r["clamp_lo"]).sum()) for r in rs)
    both = [int((r["clamp_lo"] & r["clamp_hi"]).sum()) for r in rs]
    assert lo > 20 and hi > 20 and both[3] > 20 and sum(both) == both[3]  # the utterance shorter than its windows
    assert len(t.y(3)) < 2 * live_values(name, "hw").min() + 1
    for u, r in enumerate(rs):
        for i in (0, 1, 2, 3, t.L1(u) - 4, t.L1(u) - 1):
            assert r["live"][i].any()
        assert (r["survive"] & (r["clamp_lo"] | r["clamp_hi"])).any()


def check_ragged(name):
    t = R.table(name)
    assert len(t.xs) == 4 and np.abs(t.xs[1]).max() < 0.01 * min(np.abs(t.xs[k]).max() for k in (0, 2, 3))
    assert (t.cand0[0][-3:] > 0).all() and (t.cand0[2][:3] > 0).all() and (t.cand0[2][-3:] > 0).all() and (t.cand0[3][:3] > 0).all()
    r = R.rule(name)[1]
    assert r["clamp_lo"][0].any() and r["clamp_hi"][-1].any() and r["survive"][0].any() and r["survive"][-1].any()
    assert len(t.y(1)) < R.PAD and int(r["live"].sum()) < 7 * 12  # the short one's rows stay sparse: a neighbour's full rows would show


def check_one_live(name, port):
    t = R.table(name)
    for (u, i, j), r, (c1, s1, _) in zip(t.notes["live"], R.rule(name), R.oracle(port, name)):
        want = np.zeros(r["live"].shape, dtype=bool)
        for b in range(7):
            frame = {0: i, 1: i + 1, 2: i + 2, 3: i + 3, 4: i - 1, 5: i - 2, 6: i - 3}[b]  # block b of frame i + b holds frame i, ...
            if 0 <= frame < t.L1(u):
                want[frame, j + t.S * b] = True
        assert np.array_equal(r["live"], want) and np.array_equal(c1 != 0, want) and np.array_equal(s1 != 0, want)
    assert [int(r["live"].sum()) for r in R.rule(name)] == [7, 4, 4]


def check_silence(name):
    r = R.rule(name)[0]
    assert int(r["zero"].sum()) >= 20 and not r["survive"][r["zero"]].any()
    assert (r["rf"][r["zero"]] == 0.0).all() and np.allclose(r["inv"][r["zero"]], 1.0)
    partial = r["live"] & ~r["zero"]
    assert r["survive"][partial].sum() > 200  # windows that are silent in part only refine to something


def check_crowded(name):
    t = R.table(name)
    r = R.rule(name)[0]
    S = t.S
    assert r["live"][47].all() and (t.cand0[0][44:51] > 0).all()
    keys = [R.key_of(float(t.fs), float(f)) for f in r["f"][47]]
    distinct = {k for k, _ in keys}
    assert len(distinct) > 64, len(distinct)
    assert 7 * S - len(distinct) >= 24  # stretches of equal keys: four slots hold one value each through all seven frames
    entries = {}
    for k, e in keys:
        entries.setdefault(e, set()).add(k)
    assert sum(len(v) > 1 for v in entries.values()) >= 1  # distinct keys that meet in the 256-entry table
    if S == 32:
        assert 7 * S - 1 == 223 and r["live"][47, 223]
    # the packed key holds what the rule decides
    for p in range(0, 7 * S, 5):
        kk, _ = keys[p]
        assert (kk & 2047) == r["hw"][47, p] and (kk >> 32) == r["bins"][47, p, 0]


CHECKS = dict(cuts=check_cuts, longest=check_longest, slots=check_slots, edges=check_edges, ragged=check_ragged, one=check_one_live,
              silence=check_silence, crowded=check_crowded)


@pytest.mark.parametrize("name", R.NAMES)
def test_table_reaches_what_it_is_named_for(port, name):
    check = CHECKS[name.split("_")[0]]
    if check is check_one_live:
        check(name, port)
    else:
        check(name)
    assert R.table(name).cos == name.endswith("_cos")


def mutant_ratio(name, mutant, k):
    """how far a mutant of the rule leaves the device's bound, as a multiple of it, on the candidates the device test compares
    (live, surviving, not near a threshold); a candidate that appears at a position where the rule has none, or is missing
    where the rule has one, counts as infinitely far"""
    t = R.table(name)
    worst = 0.0
    for r0, rm in zip(R.rule(name), R.rule(name, mutant)):
        firm = r0["live"] & r0["survive"] & ~R.near_threshold(t, r0, k)
        if (firm & ~rm["live"]).any() or (rm["live"] & ~r0["live"]).any():
            return np.inf
        b = (R.allowed(r0, k) * r0["unit"])[firm]
        worst = max(worst, float((np.abs(rm["rf"] - r0["rf"])[firm] / b).max()),
                    float((np.abs(rm["inv"] - r0["inv"])[firm] / (b / r0["f"][firm])).max()))
    return worst


@pytest.mark.parametrize("mutant", [m for m in R.MUTANTS if m != "fused_bin"])
def test_mutant_of_the_rule_leaves_the_bound(port, mutant):
    name = R.MUTANT_TABLE[mutant]
    got = mutant_ratio(name, mutant, R.k_ref(port))
    print("harvest refinement: mutant %s on %s leaves the bound %.3g x" % (mutant, name, got))
    assert got >= 100.0
    if mutant in ("hw+1", "bin+1", "nh-1", "basic+1"):  # the same mistake behind the cosine table
        assert mutant_ratio(name + "_cos", mutant, R.k_ref(port)) >= 100.0


def test_fused_bin_is_the_same_function():
    """bin_unit * (h + 1) + 0.5 rounded once (a contracted multiply-add) instead of twice: the one mutant no table can catch,
    because it is not a mutant.  Truncation can only tell the two apart at an integer M with one result below and one at or above.
    The product is exact to a few more bits than a double holds; with P its rounding, P + 0.5 is computed exactly whenever it stays
    below M (P and M - 0.5 lie on one grid of spacing s, as does everything below M in M's binade), so the unfused result reaches M
    exactly when P = M - 0.5, that is when the exact product is within s / 2 of M - 0.5 -- which is when the fused sum is within
    s / 2 of M.  The two grids differ only where a power of two lies in [M - 0.5, M): M = 1.  Bins are f N / fs (h + 1) > 6
    (N > 4 (3 fs / f) / 2).  Checked here on every candidate of every table and on every half-integer product the cuts hold, two
    ulps to either side."""
    n = 0
    for name in sorted(R.BUILDERS):
        t = R.table(name)
        for f in {float(v) for c in t.cand0 for v in c[c > 0]}:
            assert R.decisions(float(t.fs), 0, f, "fused_bin")["bins"] == R.decisions(float(t.fs), 0, f)["bins"]
            n += 1
    for m in list(range(6, 4200, 7)) + [2 ** k - 1 for k in range(3, 13)]:
        for h in range(1, 7):
            u0 = (m + 0.5) / h
            for u in (u0, R.up(u0), R.down(u0), R.up(R.up(u0)), R.down(R.down(u0))):
                assert int(u * h + 0.5) == int(float(Fraction(u) * h + Fraction(1, 2)))
    assert n > 1000
